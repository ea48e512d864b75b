"""The dispersion gradient of the negative-binomial Laplace evidence, host side (no GPU): the float64 restatement the GPU tests
are checked against (tests/_nb_dispersion_ref.py) is itself checked -- psi(y + r) - psi(r) against mpmath, the integrands of rows
1 and 2 and the total gradient against central differences, DispersionParameter's autograd, the two float64 training runs -- and
the Python and C-ABI argument checks (docs/kernels/counts.md, "Learning the dispersion")."""
import ctypes
import inspect
import math
import os
import types
import warnings

import numpy as np
import pytest
import torch

import _nb_dispersion_ref as dr
import _nb_ref as nb
import _observed_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE, NORM, NU = "dumbbell_k10_loop", "symmetric", 2
_Q = {}


def _precision(golden):
    """The fixture's precision scaled to the prior marginal variance _nb_ref.PRIOR_VARIANCE, as test_nb_cpu.py does"""
    if CASE not in _Q:
        g = golden(CASE)
        Q1, _ = oref.precision_root(oref.oracle(g, NORM), NU, float(g["kappa"]), 1.0, NORM)
        _Q[CASE] = (np.diag(np.linalg.inv(Q1)).mean() / nb.PRIOR_VARIANCE) * Q1
    return _Q[CASE]


# ------------------------------------------------------------------------------------------------ psi(y + r) - psi(r)
PSI_Y = [0, 1, 2, 31, 32, 33, 1000, 2 ** 24]
PSI_R = [2.0 ** -10, 0.37, 1.0, 31.5, 32.0, 33.0, 1000.0, 2.0 ** 20]


def test_psi_diff_against_mpmath():
    """The device's form of psi(y + r) - psi(r) against mpmath at 50 digits on the 8 x 8 table: the worst error in units of
    2^-53 |result| is within MEASURED_PSI_ULP (measured: 3.60 at y = 32, r = 0.37, the 32-term sum); y = 0 gives exactly 0."""
    import mpmath
    mpmath.mp.dps = 50
    worst, at = 0.0, None
    for r in PSI_R:
        got = dr.psi_diff(np.array(PSI_Y, np.float64), r)
        for y, v in zip(PSI_Y, got):
            if y == 0:
                assert v == 0.0
                continue
            ref = mpmath.digamma(mpmath.mpf(y) + mpmath.mpf(r)) - mpmath.digamma(mpmath.mpf(r))
            err = float(abs((mpmath.mpf(float(v)) - ref) / ref) * mpmath.mpf(2) ** 53)
            if err > worst:
                worst, at = err, (y, r)
    print("psi_diff against mpmath: worst %.2f units of 2^-53 |result| at (y, r) = %s; the constant is %.2f" % (worst, at, dr.MEASURED_PSI_ULP))
    assert worst <= dr.MEASURED_PSI_ULP
    assert dr.DEVICE_PSI_ULP == 4 * dr.MEASURED_PSI_ULP


# ------------------------------------------------------------------------------------------------ the integrands
@pytest.mark.parametrize("r", [0.37, 2.0, 1000.0])
def test_rows_match_central_differences_in_r(golden, r):
    """At fixed f: row 0's integrand against the central difference in r of l + c(y, r) (c by mpmath-free log_const), row 1's
    against that of h, row 2's dg / dr against that of g, at the tolerances of
    test_nb_cpu.py::test_reference_site_matches_central_differences (g: 1e-6, h: 1e-8, each of max(1, |.|))."""
    c = nb.nb_counts(golden(CASE))
    d = nb.data(c, r)
    rng = np.random.default_rng(3)
    f = 0.5 * rng.standard_normal(c["y"].shape[0])
    obs = d["obs"]
    eps = 1e-5 * r
    args = (d["y"], d["aux"], obs, d["mean"])
    plus, minus = nb.site(f, *args, r + eps), nb.site(f, *args, r - eps)
    _, g, h, _, _ = nb.site(f, *args, r)
    t = dr.node_terms(f, d["y"], d["aux"], obs, d["mean"], r)
    dh = t["pq"] - t["hp"] / r
    dg = t["h"] / r - t["pi"]
    assert (np.abs((plus[2] - minus[2]) / (2 * eps) - dh) <= 1e-8 * np.maximum(1.0, h)).all()
    assert (np.abs((plus[1] - minus[1]) / (2 * eps) - dg) <= 1e-6 * np.maximum(1.0, np.abs(g))).all()
    assert (dh[~obs] == 0).all() and (dg[~obs] == 0).all()
    cp = nb.log_const(np.where(obs, d["y"], 0.0), r + eps, np.longdouble)[0]
    cm = nb.log_const(np.where(obs, d["y"], 0.0), r - eps, np.longdouble)[0]
    fd = np.where(obs, ((plus[0] - minus[0]) + np.asarray(cp - cm, np.float64)) / (2 * eps), 0.0)
    row0 = ((t["psi"] + t["lse"]) + t["pi"]) - t["ypr"]
    scale = np.abs(t["psi"]) + np.abs(t["lse"]) + np.abs(t["pi"]) + np.abs(t["ypr"])
    assert (np.abs(fd - row0) <= 1e-6 * np.maximum(1.0, scale)).all()
    # the sums are the sums of the integrands, and the rows without var / u are 0
    v, u = rng.uniform(0.01, 2.0, f.shape[0]), rng.standard_normal(f.shape[0])
    rows, sc = dr.dispersion_sums(f, d["y"], d["aux"], obs, v, u, d["mean"], r)
    eff = t["eff"]
    want = np.array([row0.sum(), (-0.5 * v * dh)[eff].sum(), (-0.5 * u * dg)[eff].sum()])
    assert (np.abs(rows - want) <= 1e-13 * sc).all() and (np.abs(rows) <= sc).all()
    none, _ = dr.dispersion_sums(f, d["y"], d["aux"], obs, None, None, d["mean"], r)
    assert none[0] == rows[0] and none[1] == 0.0 and none[2] == 0.0
    nan = np.where(obs, 1.0, np.nan)                      # NaN at the unobserved nodes is not read
    again, _ = dr.dispersion_sums(f, d["y"] * nan, d["aux"] * nan, obs, v * nan, u * nan, d["mean"], r)
    assert np.array_equal(again, rows)


@pytest.mark.parametrize("r", [0.5, 2.0, 16.0])
def test_total_gradient_matches_central_differences_of_the_dense_evidence(golden, r):
    """d log Z / dr of dispersion_gradient against the central difference of _nb_ref.mode_log_z at r (1 +- 1e-5) with the mode
    re-fitted: 1e-6 relative, the project's bar for evidence gradients (measured: 1.0e-10, 7.5e-10 and 8.2e-10)."""
    Q = _precision(golden)
    c = nb.nb_counts(golden(CASE))
    g = dr.dispersion_gradient(Q, nb.data(c, r))
    step = 1e-5 * r
    zp = nb.mode_log_z(Q, nb.data(c, r + step), f0=g["f"])[1]["value"]
    zm = nb.mode_log_z(Q, nb.data(c, r - step), f0=g["f"])[1]["value"]
    fd = (zp - zm) / (2 * step)
    rel = abs(g["total"] - fd) / abs(fd)
    print("r = %g: rows %s, analytic %.9f, central differences %.9f, relative difference %.1e" % (r, g["rows"], g["total"], fd, rel))
    assert rel <= 1e-6


# ------------------------------------------------------------------------------------------------ the parameter
def test_dispersion_parameter():
    """init comes back exactly; autograd through exp gives r G for the raw parameter within 1e-12; rho is clamped at both bounds."""
    from manifold_gp_amd.counts import DISPERSION_MAX, DISPERSION_MIN, DispersionParameter
    for init in (2.0 ** -10, 0.37, 1.0, 2.0, 16.0, 1000.0 / 3.0, 2.0 ** 20):
        p = DispersionParameter(init)
        r = p()
        assert r.dtype == torch.float64 and r.dim() == 0 and r.requires_grad and float(r.detach()) == init
        assert [tuple(q.shape) for q in p.parameters()] == [()] and float(p.raw.detach()) == math.log(init) == dr.raw_dispersion(init)
        G = -1.4956
        got, = torch.autograd.grad(G * r, list(p.parameters()))
        assert abs(float(got) - init * G) <= 1e-12 * abs(init * G)
    p = DispersionParameter(2.0)
    with torch.no_grad():
        p.raw.add_(0.75)
    assert abs(float(p()) - 2.0 * math.exp(0.75)) <= 1e-15 * 2.0 * math.exp(0.75)
    assert abs(float(p()) - float(dr.dispersion_of(p.raw.detach(), 2.0))) <= 4e-16 * float(p())
    for raw, bound in ((100.0, DISPERSION_MAX), (-100.0, DISPERSION_MIN), (math.log(DISPERSION_MAX) + 1e-9, DISPERSION_MAX)):
        with torch.no_grad():
            p.raw.fill_(raw)
        assert float(p()) == bound
        got, = torch.autograd.grad(p(), list(p.parameters()))
        assert float(got) == 0.0                           # beyond the bound the parameter no longer moves r
    for bad in (0.0, 2.0 ** -11, 2.0 ** 21, float("nan")):
        with pytest.raises(ValueError, match="dispersion must be a finite scalar"):
            DispersionParameter(bad)


# ------------------------------------------------------------------------------------------------ the float64 training runs
def test_float64_learn_from_16(golden):
    """30 steps of Adam(0.1) on rho from r = 16 with the kernel fixed: the dense log Z gains at least 40 (measured: +43.05, from
    -747.42 to -704.38) and r ends inside [1, 4] (1.375); LEARN_GAIN is what the device run is compared with."""
    Q = _precision(golden)
    c = nb.nb_counts(golden(CASE))
    t = dr.LEARN
    trace = dr.learn(Q, c, t["r0"], t["steps"], t["lr"])
    gain = trace[-1][1] - trace[0][1]
    print("float64 learn from r = %g: %d steps, r = %.4f, log Z %.3f -> %.3f, gain %+.3f (LEARN_GAIN %.2f)"
          % (t["r0"], t["steps"], trace[-1][0], trace[0][1], trace[-1][1], gain, dr.LEARN_GAIN))
    assert len(trace) == t["steps"] + 1 and trace[0][0] == 16.0
    assert gain >= 40.0 and 1.0 <= trace[-1][0] <= 4.0
    assert abs(gain - dr.LEARN_GAIN) <= 0.01


def test_float64_train_length_scale_output_scale_and_dispersion(golden):
    """10 epochs of Adam(0.1) on the raw length scale, the raw output scale and rho together from _nb_dispersion_ref.TRAIN: the
    gain of the dense log Z is TRAIN_GAIN, what the device's laplace_train is compared with; all three parameters move."""
    g = golden(CASE)
    c = nb.nb_counts(g)
    t = dr.TRAIN
    trace = dr.train(g, NORM, NU, c, t["kappa0"], t["scale0"], t["r0"], t["steps"], t["lr"])
    gain = trace[-1][3] - trace[0][3]
    print("float64 train: kappa %.4f -> %.4f, scale %.5g -> %.5g, r %.3f -> %.3f, log Z %.3f -> %.3f, gain %+.3f (TRAIN_GAIN %.2f)"
          % (trace[0][0], trace[-1][0], trace[0][1], trace[-1][1], trace[0][2], trace[-1][2], trace[0][3], trace[-1][3], gain,
             dr.TRAIN_GAIN))
    assert all(trace[0][k] != trace[-1][k] for k in range(3))
    assert gain >= 5.0 and abs(gain - dr.TRAIN_GAIN) <= 0.01


# ------------------------------------------------------------------------------------------------ host-side checks
NEW = ("mgp_nb_dispersion_sums_workspace_bytes", "mgp_nb_dispersion_sums")


def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mgp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(handle, name)


def test_entry_point_checks_its_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    nan, inf = float("nan"), float("inf")
    bytes_ = lib.mgp_nb_dispersion_sums_workspace_bytes
    assert bytes_(0) == 0 and bytes_(-1) == 0 and bytes_(1) == 32 and bytes_(1025) == 64 and bytes_(2 ** 40) == 1024 * 32
    sums = lib.mgp_nb_dispersion_sums
    ok = lambda **kw: dict(dict(f=u, y=u, n=4, r=2.0, floor=1e-30, out=d, work=d, wb=64), **kw)
    call = lambda a: sums(a["f"], a["y"], None, None, None, None, a["n"], 0.0, a["r"], a["floor"], a["out"], a["work"], a["wb"], None)
    for kw in (dict(f=None), dict(y=None), dict(out=None), dict(n=0), dict(n=-3), dict(floor=-1.0), dict(floor=nan)):
        assert call(ok(**kw)) == -1, kw
    for r in (0.0, -1.0, 2.0 ** -11, 2.0 ** 20 + 1.0, nan, inf, -inf):
        assert call(ok(r=r)) == -1, r
    assert call(ok(work=None)) == -2 and call(ok(wb=31)) == -2 and call(ok(work=d + 4)) == -2
    assert call(ok(n=1025, wb=63)) == -2                                                       # one byte short
    assert call(ok(f=None, work=None)) == -1                                                   # the arguments come first


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def _fake_fit(family, dispersion=None):
    """What laplace_evidence reads of a fit before its first device call"""
    f = torch.zeros(3)
    return types.SimpleNamespace(_pseudo=None, mean=f, desc=_fake_desc(), family=family, prior_mean=0.0, _aux=None, s_ref=1.0,
                                 dispersion=dispersion, y=torch.tensor([0.0, 3.0, 7.0]), observed=None, log_likelihood=0.0,
                                 latent_variance=lambda s: (torch.ones(3, dtype=torch.float64), None))


def test_python_argument_checks():
    from manifold_gp_amd import counts as ct, evidence as ev
    from manifold_gp_amd.models import RiemannGP
    from manifold_gp_amd.utils import laplace_train
    d = _fake_desc()
    y = torch.tensor([0.0, 3.0, 7.0])
    f = torch.zeros(3)
    v = torch.ones(3, dtype=torch.float64)
    nan = float("nan")
    # the wrapper: the checks come before the device, host tensors are refused
    for bad in (nan, 0.0, 2.0 ** -11, 2.0 ** 21):
        with pytest.raises(ValueError, match="dispersion must be a finite scalar"):
            ct.nb_dispersion_sums(f, y, None, None, v, v, 0.0, bad)
    with pytest.raises(ValueError, match="needs dispersion"):
        ct.nb_dispersion_sums(f, y, None, None, v, v, 0.0, None)
    with pytest.raises(ValueError, match="h_floor"):
        ct.nb_dispersion_sums(f, y, None, None, v, v, 0.0, 2.0, -1.0)
    with pytest.raises(ValueError, match="y must be a tensor"):
        ct.nb_dispersion_sums(f, [0.0, 3.0, 7.0], None, None, v, v, 0.0, 2.0)
    for kw in (dict(y=torch.zeros(4)), dict(aux=torch.zeros(2)), dict(variance=torch.ones(4)), dict(u=torch.ones(2)),
               dict(observed=torch.ones(4, dtype=torch.bool))):
        a = dict(dict(y=y, aux=None, observed=None, variance=v, u=v), **kw)
        with pytest.raises(ValueError, match="entries, f 3"):
            ct.nb_dispersion_sums(f, a["y"], a["aux"], a["observed"], a["variance"], a["u"], 0.0, 2.0)
    with pytest.raises(ValueError, match="observed must be a bool tensor"):
        ct.nb_dispersion_sums(f, y, None, torch.ones(3), v, v, 0.0, 2.0)
    with pytest.raises(ValueError, match="no entries"):
        ct.nb_dispersion_sums(torch.zeros(0), torch.zeros(0), None, None, None, None, 0.0, 2.0)
    for var, u in ((v, v), (None, None), (v, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ct.nb_dispersion_sums(f, y, None, None, var, u, 0.0, 2.0)
    # laplace_evidence(dispersion=): the family, the type and the value are checked before the device
    r = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    for family in ("poisson", "binomial", "bernoulli"):
        with pytest.raises(ValueError, match="dispersion belongs to a negative_binomial fit"):
            ev.laplace_evidence(_fake_fit(family), dispersion=r)
    nbfit = _fake_fit("negative_binomial", 2.0)
    for bad in (2.0, torch.tensor(2.0), torch.tensor([2.0], dtype=torch.float64), torch.tensor(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="0-dim float64 tensor"):
            ev.laplace_evidence(nbfit, dispersion=bad)
    for other in (torch.tensor(2.0 + 2.0 ** -50, dtype=torch.float64), torch.tensor(float(np.float32(0.37)), dtype=torch.float64)):
        with pytest.raises(ValueError, match="not the fit's"):
            ev.laplace_evidence(_fake_fit("negative_binomial", 0.37) if float(other) < 1 else nbfit, dispersion=other)
    for good in (r, r.detach(), None):                     # valid: the first device call refuses the host tensors
        with pytest.raises(RuntimeError, match="no CPU path"):
            ev.laplace_evidence(nbfit, dispersion=good)
    # the live dispersion of laplace_train / RiemannGP.laplace_evidence
    p = ct.DispersionParameter(16.0)
    kw, live = ct._live_dispersion(dict(dispersion=p, mean=0.5))
    assert kw == dict(dispersion=16.0, mean=0.5) and type(kw["dispersion"]) is float and live.requires_grad and float(live) == 16.0
    kw, live = ct._live_dispersion(dict(dispersion=r))
    assert kw == dict(dispersion=2.0) and live is r
    for plain in (2.0, np.float32(0.5), torch.tensor(2.0), 1):
        given = dict(dispersion=plain)
        kw, live = ct._live_dispersion(given)
        assert kw is given and live is None                # a number keeps today's path
    p.raw.requires_grad_(False)
    kw, live = ct._live_dispersion(dict(dispersion=p))
    assert live is None and float(kw["dispersion"]) == 16.0 and not isinstance(kw["dispersion"], torch.nn.Module)
    with pytest.raises(ValueError, match="real scalar"):
        ct._live_dispersion(dict(dispersion=torch.ones(2, dtype=torch.float64, requires_grad=True)))
    assert ct._live_dispersion({}) == ({}, None)
    # learn_dispersion
    for kw_, msg in ((dict(steps=0), "steps must be"), (dict(lr=0.0), "steps must be"), (dict(steps=2.5), "steps must be an int"),
                     (dict(variance=v), "callable")):
        with pytest.raises(ValueError, match=msg):
            ct.learn_dispersion(d, y, 16.0, **kw_)
    with pytest.raises(ValueError, match="dispersion must be a finite scalar"):
        ct.learn_dispersion(d, y, nan)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ct.learn_dispersion(d, y, 16.0, steps=2)
    assert list(inspect.signature(ct.learn_dispersion).parameters) == ["desc", "y", "dispersion0", "observed", "exposure", "mean", "steps",
                                                                      "lr", "var_samples", "variance", "fit_kw", "evidence_kw"]
    assert list(inspect.signature(ct.nb_dispersion_sums).parameters) == ["f", "y", "aux", "observed", "variance", "u", "mean",
                                                                        "dispersion", "h_floor"]
    assert "dispersion" in inspect.signature(ev.laplace_evidence).parameters
    assert "dispersion_grad" in inspect.signature(ev.LaplaceEvidence.__init__).parameters
    assert callable(laplace_train) and callable(RiemannGP.laplace_evidence)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ev.LaplaceEvidence(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, "dense", 1, None, None).dispersion_grad is None
