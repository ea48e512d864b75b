"""The Laplace evidence, host side (no GPU): the float64 restatement the GPU tests are checked against (tests/_evidence_ref.py) is
itself checked -- logdet B against logdet A - logdet Q, the analytic gradient against central differences of the dense log Z
with the mode re-fitted, h' against central differences of h, the float64 Lanczos quadrature on B at the GPU tests' probes against
the dense value -- and the C-ABI and Python argument checks, exports and signatures."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _observed_ref as oref

FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
_P = {}


def _unit_precision(golden, case, norm, nu, kappa=None):
    g = golden(case)
    return oref.precision_root(oref.oracle(g, norm), nu, float(g["kappa"]) if kappa is None else kappa, 1.0, norm)[0]


def _problem(golden, case, norm, nu, family):
    """The fixture's precision scaled to a prior marginal variance of about 9 (as test_laplace_cpu.py), the family's data, the
    float64 mode."""
    key = (case, norm, nu)
    if key not in _P:
        Q1 = _unit_precision(golden, case, norm, nu)
        _P[key] = dict(Q1=Q1, scale=np.diag(np.linalg.inv(Q1)).mean() / 9.0)
    base = _P[key]
    if family not in base:
        d = eref.data(golden(case), family)
        Q = base["scale"] * base["Q1"]
        base[family] = dict(Q=Q, d=d, f=eref.mode(Q, d), scale=base["scale"])
    return base[family]


@pytest.mark.parametrize("family", eref.FAMILIES)
@pytest.mark.parametrize("case", FIXTURES)
def test_logdet_b_is_logdet_a_minus_logdet_q(golden, case, family):
    p = _problem(golden, case, "symmetric", 2, family)
    _, h, _ = eref.site(family, p["f"], p["d"]["y"], p["d"]["aux"], p["d"]["obs"], p["d"]["mean"])
    eff = p["d"]["obs"] & (h >= eref.H_FLOOR)
    got = eref.logdet_b(p["Q"], h, eff)
    want = np.linalg.slogdet(p["Q"] + np.diag(h))[1] - np.linalg.slogdet(p["Q"])[1]
    z = eref.log_z(p["Q"], p["f"], p["d"])
    print("%s %s: logdet B = %.4f (logdet A - logdet Q: %.4f), m = %d, log Z = %.4f, cond B = %.2f"
          % (case, family, got, want, z["m"], z["value"], np.linalg.cond(eref.dense_b(p["Q"], h, eff))))
    assert abs(got - want) <= 1e-10 * abs(want)
    assert z["m"] == int(p["d"]["obs"].sum()) and abs(z["value"] - (z["log_likelihood"] - z["quad"] - 0.5 * got)) <= 1e-12 * abs(z["value"])


def _dq_dlogkappa(golden, case, nu, kappa, scale):
    """d (scale (tau I + L_sym)^nu) / d log kappa = -2 nu tau scale (tau I + L_sym)^(nu - 1), tau = 2 nu / kappa^2 (symmetric)"""
    lo = oref.oracle(golden(case), "symmetric")
    tau = 2.0 * nu / kappa ** 2
    A = tau * np.eye(lo.n) + lo.dense_symmetric()
    return -2.0 * nu * tau * scale * np.linalg.matrix_power(A, nu - 1)


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_analytic_gradient_matches_central_differences_of_the_refitted_log_z(golden, family):
    """theta = log scale and log kappa on k10_loop, symmetric, nu = 2: 1e-6 relative."""
    case, nu = "dumbbell_k10_loop", 2
    p = _problem(golden, case, "symmetric", nu, family)
    kappa, scale, d = float(golden(case)["kappa"]), p["scale"], p["d"]
    step = 1e-4

    def logz(ls, lk):
        Q = scale * np.exp(ls) * _unit_precision(golden, case, "symmetric", nu, kappa * np.exp(lk))
        return eref.log_z(Q, eref.mode(Q, d, f0=p["f"]), d)["value"]
    for name, dQ, at in (("log scale", p["Q"], (step, 0.0)), ("log kappa", _dq_dlogkappa(golden, case, nu, kappa, scale), (0.0, step))):
        got, terms = eref.gradient(p["Q"], dQ, p["f"], d)
        fd = (logz(*at) - logz(-at[0], -at[1])) / (2.0 * step)
        print("%s, %s: analytic %.9f (terms %.6f %.6f %.6f), central differences %.9f" % (family, name, got, *terms, fd))
        assert abs(got - fd) <= 1e-6 * abs(fd), (name, got, fd)


@pytest.mark.parametrize("family", eref.FAMILIES)
def test_curvature_derivative_matches_central_differences_and_is_finite(family):
    rng = np.random.default_rng(4)
    eta = rng.uniform(-12.0, 8.0, 400)
    y = rng.integers(0, 5, 400).astype(np.float64)
    aux = None if family == "bernoulli" else (np.zeros(400) if family == "poisson" else y + rng.integers(1, 30, 400))
    eps = 1e-6
    h_plus, h_minus = (eref.site(family, eta + s, y, aux, None, 0.0)[1] for s in (eps, -eps))
    _, h, hp = eref.site(family, eta, y, aux, None, 0.0)
    assert (np.abs((h_plus - h_minus) / (2 * eps) - hp) <= 1e-8 * np.maximum(h, 1e-300) + 1e-9 * np.abs(hp)).all()
    ext = np.array([1e4, -1e4, 0.0, 1e-9, -1e-9])
    ye = np.ones(5)
    auxe = None if family == "bernoulli" else (np.zeros(5) if family == "poisson" else np.full(5, 7.0))
    _, h, hp = eref.site(family, ext, ye, auxe, None, 0.0)
    assert np.isfinite(h).all() and np.isfinite(hp).all()
    if family != "poisson":
        N = 1.0 if family == "bernoulli" else 7.0
        assert hp[0] == 0.0 and hp[1] == 0.0 and hp[2] == 0.0                      # saturated tails, the symmetric point
        assert hp[3] == pytest.approx(-N * 0.25 * 0.5e-9, rel=1e-6) and hp[4] == -hp[3]   # no cancellation near 0
    root, corr, sums, _, eff = eref.site_outputs(family, ext.astype(np.float32), ye, auxe, None, np.ones(5), 0.0)
    assert np.isfinite(root).all() and np.isfinite(corr).all() and np.isfinite(sums).all()
    if family == "poisson":
        assert root[0] == np.float32(eref.FLT_MAX) and corr[0] == np.float32(eref.FLT_MAX) and not eff[1]
    else:
        assert not eff[0] and not eff[1] and root[0] == 0.0 and sums[1] == 3.0


@pytest.mark.parametrize("case, norm, nu", eref.SLQ_CASES)
def test_float64_quadrature_on_b_is_within_five_standard_errors(golden, case, norm, nu):
    """The float64 Lanczos quadrature on B at the probe count, step count and seed of the GPU tests against the dense value."""
    p = _problem(golden, case, norm, nu, "bernoulli")
    _, h, _ = eref.site("bernoulli", p["f"], p["d"]["y"], None, p["d"]["obs"], 0.0)
    eff = p["d"]["obs"] & (h >= eref.H_FLOOR)
    m = int(eff.sum())
    dense = eref.logdet_b(p["Q"], h, eff)
    Z = eref.probes(eff, eref.SLQ_PROBES, eref.SLQ_SEED)
    per, est, se = eref.slq_per_probe(eref.b_matmul(p["Q"], h), Z, eref.SLQ_STEPS, m)
    print("%s %s nu = %d: dense %.4f, quadrature %.4f +- %.4f (%.2f standard errors), m = %d"
          % (case, norm, nu, dense, est, se, abs(est - dense) / se, m))
    assert (np.abs(Z).sum(0) == m).all() and (Z[~eff] == 0).all()
    assert abs(est - dense) <= 5.0 * se


def test_float64_training_run_gains_what_the_gpu_test_assumes(golden):
    """The float64 restatement of the laplace_train test's optimiser with exact gradients from _evidence_ref.TRAIN: log Z rises at
    every step, by the recorded 12.906 in all (at least 5)."""
    t = eref.TRAIN
    g = golden("dumbbell_k10_loop")
    trace = eref.train_f64(g, "symmetric", 2, eref.data(g, "bernoulli"), t["kappa0"], t["scale0"], t["steps"], t["lr"])
    z = [v[2] for v in trace]
    print("log Z %s; kappa %.4f -> %.4f, scale %.5g -> %.5g" % (["%.3f" % v for v in z], trace[0][0], trace[-1][0], trace[0][1], trace[-1][1]))
    assert len(z) == t["steps"] + 1 and all(b > a for a, b in zip(z, z[1:]))
    assert z[-1] - z[0] >= 5.0 and abs(z[-1] - z[0] - t["gain_f64"]) <= 0.01


# ------------------------------------------------------------------------------------------------ host-side checks
def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgp_laplace_evidence_site_workspace_bytes", "mgp_laplace_evidence_site", "mgp_scale_rows"):
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    buf, dbl = (ctypes.c_float * 8)(), (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    assert lib.mgp_laplace_evidence_site_workspace_bytes(0) == 0 and lib.mgp_laplace_evidence_site_workspace_bytes(1025) == 64
    assert lib.mgp_laplace_evidence_site_workspace_bytes(2 ** 40) == 1024 * 32
    site = lib.mgp_laplace_evidence_site
    for fam in (0, 1, 2):
        assert site(None, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, d, 64, None) == -1
        assert site(u, None, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, d, 64, None) == -1
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, None, u, d, d, 64, None) == -1
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, None, d, 64, None) == -1
        assert site(u, u, u, None, d, 0, 0.0, fam, 1e-30, u, u, d, d, 64, None) == -1
        assert site(u, u, u, None, d, 4, 0.0, fam, -1.0, u, u, d, d, 64, None) == -1
        assert site(u, u, u, None, d, 4, 0.0, fam, float("nan"), u, u, d, d, 64, None) == -1
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, None, 64, None) == -2
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, d, 31, None) == -2
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, d + 4, 64, None) == -2
    assert site(u, u, None, None, d, 4, 0.0, 1, 1e-30, u, u, d, d, 64, None) == -1          # binomial without trials
    for fam in (3, -1, 7):
        assert site(u, u, u, None, d, 4, 0.0, fam, 1e-30, u, u, d, d, 64, None) == -3
    rows = lib.mgp_scale_rows
    assert rows(None, u, None, 2, 4, u, None) == -1 and rows(u, None, None, 2, 4, u, None) == -1
    assert rows(u, u, None, 2, 4, None, None) == -1 and rows(u, u, None, 0, 4, u, None) == -1
    assert rows(u, u, None, 2, 0, u, None) == -1 and rows(u, u, None, 2, 257, u, None) == -1


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_python_argument_checks():
    from manifold_gp_amd import evidence as ev
    from manifold_gp_amd.classification import MulticlassLaplaceFit
    f, y = torch.zeros(3), torch.tensor([0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="family"):
        ev.evidence_site(f, y, None, None, None, 0.0, "gauss")
    with pytest.raises(ValueError, match="trials"):
        ev.evidence_site(f, y, None, None, None, 0.0, "binomial")
    with pytest.raises(ValueError, match="no aux"):
        ev.evidence_site(f, y, y, None, None, 0.0, "bernoulli")
    with pytest.raises(ValueError, match="h_floor"):
        ev.evidence_site(f, y, None, None, None, 0.0, "bernoulli", h_floor=-1.0)
    with pytest.raises(ValueError, match="observed"):
        ev.evidence_site(f, y, None, torch.ones(3), None, 0.0, "bernoulli")
    with pytest.raises(ValueError, match="variance"):
        ev.evidence_site(f, y, None, None, torch.ones(4), 0.0, "bernoulli")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.evidence_site(f, y, None, None, torch.ones(3), 0.0, "bernoulli")
    V = torch.zeros(3, 4)
    for bad in (torch.zeros(3), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(4, 3).t(), torch.zeros(3, 257)):
        with pytest.raises(ValueError, match="V "):
            ev.scale_rows(torch.ones(3), bad)
    with pytest.raises(ValueError, match="row factors"):
        ev.scale_rows(torch.ones(4), V)
    with pytest.raises(ValueError, match="X must"):
        ev.scale_rows(torch.ones(3), V, torch.zeros(3, 5))
    with pytest.raises(ValueError, match="out must"):
        ev.scale_rows(torch.ones(3), V, None, torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.scale_rows(torch.ones(3), V)
    d, s = _fake_desc(), torch.ones(3)
    with pytest.raises(NotImplementedError):
        ev.logdet_b(_fake_desc(form=2), s, 3)
    for kw, match in ((dict(m=0), "m must"), (dict(m=4), "exceeds"), (dict(num_probes=0), "num_probes"), (dict(steps=True), "steps"),
                      (dict(solve_tol=0.0), "solve_tol"), (dict(method="lanczos"), "method"), (dict(probes=torch.ones(4, 2)), "probes"),
                      (dict(probes=torch.ones(3, 1)), "probes")):
        with pytest.raises(ValueError, match=match):
            ev.logdet_b(d, s, **dict(dict(m=3), **kw))
    with pytest.raises(ValueError, match="root_h"):
        ev.logdet_b(d, torch.ones(4), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.logdet_b(d, s, 3)
    with pytest.raises(NotImplementedError, match="softmax"):
        MulticlassLaplaceFit(d, None, None, torch.zeros(3, 2), None, True, 0, [], 0.0).evidence()
    with pytest.raises(NotImplementedError):
        ev.laplace_evidence(MulticlassLaplaceFit(d, None, None, torch.zeros(3, 2), None, True, 0, [], 0.0))


def test_exports_and_signatures():
    import manifold_gp_amd
    from manifold_gp_amd import evidence as ev, slq, utils
    from manifold_gp_amd.classification import LaplaceFit
    from manifold_gp_amd.counts import CountLaplaceFit
    from manifold_gp_amd.models import RiemannGP
    assert list(inspect.signature(ev.logdet_b).parameters)[:9] == ["desc", "root_h", "m", "num_probes", "steps", "seed", "solve_tol",
                                                                   "method", "probes"]
    sig = inspect.signature(ev.logdet_b).parameters
    assert (sig["num_probes"].default, sig["steps"].default, sig["solve_tol"].default, sig["method"].default) == (16, 12, 1e-6, "auto")
    assert list(inspect.signature(ev.laplace_evidence).parameters)[:4] == ["fit", "operator", "variance", "var_samples"]
    assert inspect.signature(ev.laplace_evidence).parameters["var_samples"].default == 64
    assert list(inspect.signature(RiemannGP.laplace_evidence).parameters) == ["self", "observed", "family", "kw"]
    assert inspect.signature(RiemannGP.laplace_evidence).parameters["family"].default == "bernoulli"
    assert list(inspect.signature(utils.laplace_train).parameters) == ["model", "optimizer", "observed", "family", "max_iter", "tolerance",
                                                                       "fit_kw", "evidence_kw", "verbose"]
    sig = inspect.signature(utils.laplace_train).parameters
    assert (sig["max_iter"].default, sig["tolerance"].default, sig["family"].default) == (50, 1e-2, "bernoulli")
    assert "laplace_train" in utils.__all__ and callable(slq._quadrature_log_each)
    assert callable(LaplaceFit.evidence) and CountLaplaceFit.evidence is LaplaceFit.evidence
    for name in ("value", "se", "log_likelihood", "quad", "logdet", "logdet_se", "method"):
        assert name in inspect.signature(ev.LaplaceEvidence.__init__).parameters
    assert ev.FAMILIES == {"poisson": 0, "binomial": 1, "bernoulli": 2} and ev.DENSE_MAX == 512
    assert manifold_gp_amd.evidence is ev


def test_per_probe_quadrature_adds_up_to_the_sum():
    from manifold_gp_amd import slq
    rng = np.random.default_rng(0)
    a, b = rng.uniform(1.0, 3.0, (6, 5)), rng.uniform(0.1, 0.5, (6, 5))
    b[2, 3] = 0.0                                                    # an exhausted Krylov space: the scalar routine
    each = slq._quadrature_log_each(a, b)
    assert each.shape == (5,) and abs(each.sum() - slq._quadrature_log_sum(a, b)) <= 1e-12 * np.abs(each).sum()
    assert each[3] == slq._quadrature_log(a[:, 3], b[:, 3])
