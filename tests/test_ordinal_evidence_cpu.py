"""The evidence of the ordered-category fit and the cutpoint learning, host side (no GPU): the float64 restatement the GPU tests
are checked against (tests/_ordinal_evidence_ref.py) is itself checked -- h' against central differences of h and against mpmath
at extreme arguments, the cutpoint gradient and the hyper-parameter gradient against central differences of the dense log Z with
the mode re-fitted, K = 2 against the Bernoulli evidence, logdet B against logdet A - logdet Q, the two float64 optimisers' gains
-- then CutpointParameter, the C-ABI and the Python argument checks, exports and signatures."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _ordinal_evidence_ref as oev
import _ordinal_ref as oref
from test_evidence_cpu import _dq_dlogkappa, _fake_desc, _unit_precision

INF = np.inf
CASE, NORM, NU = "dumbbell_k10_loop", "symmetric", 2
_P = {}


def _problem(golden):
    """k10_loop, symmetric, nu = 2, the precision scaled to a prior marginal variance of about 9; K = 4 categories at 10 % of the
    nodes, the frequency cutpoints, the float64 mode."""
    if not _P:
        Q1 = _unit_precision(golden, CASE, NORM, NU)
        scale = np.diag(np.linalg.inv(Q1)).mean() / 9.0
        Q = scale * Q1
        d = oev.data(golden(CASE), oev.LEARN["K"], oev.LEARN["frac"])
        _P.update(Q=Q, Qi=np.linalg.inv(Q), scale=scale, d=d, f=oev.mode(Q, d))
    return _P


# ------------------------------------------------------------------------------------------------ the site restatement
def test_curvature_derivative_matches_central_differences():
    """h' against central differences of h at |f| <= 6, cutpoints in [-4, 4] with gaps >= 0.25, the end categories included (the
    inputs of test_ordinal_cpu.py's autograd check), to its 1e-9: the difference quotient with step 1e-6 carries 2^-53 / 1e-6 =
    1e-10 of rounding and 1e-12 of truncation."""
    rng = np.random.default_rng(0)
    n = 4000
    f = rng.uniform(-6.0, 6.0, n)
    lo = rng.uniform(-4.0, 3.5, n)
    hi = lo + rng.uniform(0.25, 4.0, n)
    lo[: n // 4] = -INF
    hi[n // 4: n // 2] = INF
    eps = 1e-6
    hp = oev.site(f, lo, hi)[3]
    fd = (oev.site(f + eps, lo, hi)[2] - oev.site(f - eps, lo, hi)[2]) / (2 * eps)
    err = np.abs(fd - hp).max()
    print("h' against central differences: %.1e" % err)
    assert err <= 1e-9
    l, g, h, _ = oev.site(f, lo, hi)
    assert all(np.array_equal(a, b) for a, b in zip((l, g, h), oref.site(f, lo, hi)))


def test_curvature_derivative_matches_mpmath_at_extreme_arguments():
    """|f| up to 1e4, gaps down to 2^-20, infinite ends (the grid of test_ordinal_cpu.py) against 60-digit arithmetic:
    h' = -(t_hi (sc_hi - s_hi) + t_lo (sc_lo - s_lo)) to 1e-14 of the sum of its two absolute terms, the bar of h there (the two
    ends' terms cancel where the interval is symmetric about f, so the sum itself has no relative accuracy).  Finite everywhere,
    exactly 0 where both ends saturate."""
    import mpmath as mp
    from test_ordinal_cpu import EXTREME_F, EXTREME_INTERVALS
    worst = 0.0
    with mp.workdps(60):
        sig = lambda x: 1 / (1 + mp.exp(-x))
        for f in EXTREME_F:
            for lo, hi in EXTREME_INTERVALS:
                f32, lo32, hi32 = np.float32(f), np.float32(lo), np.float32(hi)
                hp = oev.site(np.array([f32]), np.array([lo32]), np.array([hi32]))[3][0]
                assert np.isfinite(hp), (f, lo, hi)
                F = mp.mpf(float(f32))
                want, size = mp.mpf(0), mp.mpf(0)
                for b in (hi32, lo32):
                    if np.isfinite(b):
                        s, sc = sig(mp.mpf(float(b)) - F), sig(F - mp.mpf(float(b)))
                        want -= s * sc * (sc - s)
                        size += abs(s * sc * (sc - s))
                if size > mp.mpf(10) ** -290:
                    worst = max(worst, float(abs(mp.mpf(float(hp)) - want) / size))
                else:
                    assert abs(hp) <= 1e-290
    print("h' against mpmath: %.1e of the absolute terms" % worst)
    assert worst <= 1e-14
    ext = np.array([1e4, -1e4], np.float32)
    root, corr, sums, _, eff = oev.site_outputs(ext, np.array([-INF, 0.0], np.float32), np.array([0.0, INF], np.float32), None,
                                                np.ones(2))
    assert not eff.any() and not root.any() and not corr.any() and np.isfinite(sums).all()


def test_cut_sums_restatement_edges():
    """Rows 1 and 2 are zeros without var / u; a category >= K and an unobserved node (NaN everywhere) add nothing; K = 2 has one
    column fed from both sides."""
    f = np.array([0.3, -0.2, 1.0, np.float32(0.1)])
    cat = np.array([0, 1, 7, 255])
    lo, hi = np.array([-INF, 0.0, 0.0, np.nan]), np.array([0.0, INF, INF, np.nan])
    obs = np.array([True, True, True, False])
    out, scale = oev.cut_sums(f, lo, hi, cat, obs, None, None, 2)
    assert out.shape == (3, 1) and not out[1:].any() and np.isfinite(out).all()
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    assert out[0, 0] == pytest.approx(sig(0.3) - sig(0.2), rel=1e-15)                 # sigma(-u_0) - sigma(l_1)
    assert scale[0, 0] == pytest.approx(sig(0.3) + sig(0.2), rel=1e-15)
    full, _ = oev.cut_sums(f, lo, hi, cat, obs, np.ones(4), np.ones(4), 2)
    assert full[1, 0] != 0.0 and full[2, 0] != 0.0 and full[0, 0] == out[0, 0]
    floor, _ = oev.cut_sums(f, lo, hi, cat, obs, np.ones(4), np.ones(4), 2, h_floor=0.4)
    assert not floor[1:].any() and floor[0, 0] == out[0, 0]                           # the floor masks rows 1 and 2 only


# ------------------------------------------------------------------------------------------------ the dense evidence
def test_logdet_b_is_logdet_a_minus_logdet_q(golden):
    p = _problem(golden)
    Q, f, d = p["Q"], p["f"], p["d"]
    h = oev.posterior(Q, f, d)[0]
    z = oev.log_z(Q, f, d)
    want = np.linalg.slogdet(Q + np.diag(h))[1] - np.linalg.slogdet(Q)[1]
    print("logdet B = %.6f (logdet A - logdet Q: %.6f), m = %d, log Z = %.4f" % (z["logdet"], want, z["m"], z["value"]))
    assert abs(z["logdet"] - want) <= 1e-10 * abs(want)
    assert z["m"] == int(d["obs"].sum()) and abs(oev.log_z(Q, f, d, p["Qi"])["value"] - z["value"]) <= 1e-12 * abs(z["value"])
    assert abs(z["log_likelihood"] - oref.log_likelihood(f, d["y"], d["cuts"], d["obs"])) <= 1e-12 * abs(z["log_likelihood"])


def test_two_categories_cut_at_zero_are_the_bernoulli_evidence(golden):
    """K = 2, b_1 = 0 on the labels of the Bernoulli tests: log Z, its three parts and the hyper-parameter gradient equal those of
    _evidence_ref's Bernoulli family to 1e-12 relative at the same point."""
    p = _problem(golden)
    Q = p["Q"]
    b = eref.data(golden(CASE), "bernoulli")
    d = dict(y=(b["y"] > 0.5).astype(np.int64), obs=b["obs"], cuts=np.array([0.0]), K=2)
    f = eref.mode(Q, b)
    got, want = oev.log_z(Q, f, d), eref.log_z(Q, f, b)
    for key in ("value", "log_likelihood", "quad", "logdet"):
        assert abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), key
    assert got["m"] == want["m"]
    assert np.abs(oev.mode(Q, d) - f).max() <= 1e-9 * np.abs(f).max()
    g1, g2 = oev.gradient(Q, Q, f, d, p["Qi"])[0], eref.gradient(Q, Q, f, b)[0]
    assert abs(g1 - g2) <= 1e-12 * abs(g2)


def test_cutpoint_gradient_matches_central_differences_of_the_refitted_log_z(golden):
    """d log Z / d b_k, k = 1, 2, 3, against central differences (step 1e-5) of the dense log Z with the mode re-fitted: 1e-6
    relative, the bar of test_evidence_cpu.py."""
    p = _problem(golden)
    Q, Qi, f, d = p["Q"], p["Qi"], p["f"], p["d"]
    G, rows, scale = oev.cut_gradient(Q, f, d)
    step = 1e-5
    for k in range(d["K"] - 1):
        z = []
        for s in (step, -step):
            cuts = d["cuts"].copy()
            cuts[k] += s
            dk = dict(d, cuts=cuts)
            z.append(oev.log_z(Q, oev.mode(Q, dk, f0=f), dk, Qi)["value"])
        fd = (z[0] - z[1]) / (2.0 * step)
        print("b_%d: analytic %.9f (rows %.6f %.6f %.6f), central differences %.9f" % (k + 1, G[k], *rows[:, k], fd))
        assert abs(G[k] - fd) <= 1e-6 * abs(fd), (k, G[k], fd)
    assert (scale >= np.abs(rows)).all()


def test_hyper_parameter_gradient_matches_central_differences_of_the_refitted_log_z(golden):
    """theta = log scale and log kappa: 1e-6 relative."""
    p = _problem(golden)
    kappa, scale, d = float(golden(CASE)["kappa"]), p["scale"], p["d"]
    step = 1e-4

    def logz(ls, lk):
        Q = scale * np.exp(ls) * _unit_precision(golden, CASE, NORM, NU, kappa * np.exp(lk))
        return oev.log_z(Q, oev.mode(Q, d, f0=p["f"]), d)["value"]
    for name, dQ, at in (("log scale", p["Q"], (step, 0.0)), ("log kappa", _dq_dlogkappa(golden, CASE, NU, kappa, scale), (0.0, step))):
        got, terms = oev.gradient(p["Q"], dQ, p["f"], d, p["Qi"])
        fd = (logz(*at) - logz(-at[0], -at[1])) / (2.0 * step)
        print("%s: analytic %.9f (terms %.6f %.6f %.6f), central differences %.9f" % (name, got, *terms, fd))
        assert abs(got - fd) <= 1e-6 * abs(fd), (name, got, fd)


def test_float64_cutpoint_learning_gains_what_the_gpu_test_assumes(golden):
    """learn_f64 from the frequency cutpoints: log Z rises at every one of the 10 steps, by the recorded gain in all (at least 5)."""
    p = _problem(golden)
    t = oev.LEARN
    trace = oev.learn_f64(p["Q"], p["d"], t["steps"], t["lr"])
    z = [v[1] for v in trace]
    print("log Z %s; cutpoints %s -> %s" % (["%.3f" % v for v in z], trace[0][0], trace[-1][0]))
    assert len(z) == t["steps"] + 1 and all(b > a for a, b in zip(z, z[1:]))
    assert z[-1] - z[0] >= 5.0 and abs(z[-1] - z[0] - oev.LEARN_GAIN_F64) <= 0.01
    assert abs(z[0] - oev.log_z(p["Q"], p["f"], p["d"])["value"]) <= 1e-9 * abs(z[0])


def test_float64_joint_training_gains_what_the_gpu_test_assumes(golden):
    """train_f64 on length scale, output scale and cutpoints together from _evidence_ref.TRAIN's start: the recorded gain in 10
    steps (at least 5; Adam at lr 0.1 overshoots in between, so not monotone)."""
    t = eref.TRAIN
    g = golden(CASE)
    d = oev.data(g, oev.LEARN["K"], oev.LEARN["frac"])
    trace = oev.train_f64(g, NORM, NU, d, t["kappa0"], t["scale0"], t["steps"], t["lr"])
    z = [v[3] for v in trace]
    print("log Z %s; kappa %.4f -> %.4f, scale %.5g -> %.5g, cutpoints %s -> %s"
          % (["%.3f" % v for v in z], trace[0][0], trace[-1][0], trace[0][1], trace[-1][1], trace[0][2], trace[-1][2]))
    assert z[-1] - z[0] >= 5.0 and abs(z[-1] - z[0] - oev.TRAIN_GAIN_F64) <= 0.01


# ------------------------------------------------------------------------------------------------ CutpointParameter
def test_cutpoint_parameter_round_trip_order_and_autograd():
    from manifold_gp_amd.ordinal import GAP_FLOOR, CutpointParameter, ordinal_cutpoints
    inits = [torch.tensor([-1.17364752, 0.03681397, 1.20796478], dtype=torch.float64), torch.tensor([0.25], dtype=torch.float64),
             torch.tensor([-3000.0, -2999.0 + 2.0 ** -9, 0.0, 50.0, 4000.0], dtype=torch.float64),
             ordinal_cutpoints(torch.tensor([0, 0, 1, 3, 3, 3, 5]), 6)]
    for init in inits:
        K = init.shape[0] + 1
        cut = CutpointParameter(K, init)
        b = cut()
        assert cut.raw.dtype == torch.float64 and cut.raw.shape == (K - 1,) and b.dtype == torch.float64 and b.requires_grad
        assert list(cut.parameters())[0] is cut.raw and cut.num_categories == K
        assert float((b.detach() - init).abs().max()) <= 4 * np.spacing(float(init.abs().max())) * K
        assert np.array_equal(oev.cutpoints_of(cut.raw.detach()).numpy(), b.detach().numpy())
        assert np.allclose(oev.raw_cutpoints(init.numpy()), cut.raw.detach().numpy(), rtol=1e-14, atol=0)
    # strictly increasing after the float32 rounding for |b| < 2^12, wherever the optimiser drives the raw parameters
    cut = CutpointParameter(5, torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64))
    with torch.no_grad():
        cut.raw.copy_(torch.tensor([4000.0, -800.0, -40.0, -1e6], dtype=torch.float64))
    b32 = cut().detach().float()
    assert float(cut().detach().max()) < 2.0 ** 12 and bool((b32[1:] > b32[:-1]).all())
    assert float((cut().detach()[1:] - cut().detach()[:-1]).min()) >= GAP_FLOOR == 2.0 ** -10
    # autograd of forward() against central differences
    cut = CutpointParameter(4, inits[0])
    wts = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64)
    grad, = torch.autograd.grad((wts * cut()).sum(), cut.raw)
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[j] = 1e-6
        fd = float((wts * (oev.cutpoints_of(cut.raw.detach() + e) - oev.cutpoints_of(cut.raw.detach() - e))).sum()) / 2e-6
        assert abs(float(grad[j]) - fd) <= 1e-9 * max(1.0, abs(fd))
    for bad in (torch.tensor([0.0, 2.0 ** -10]), torch.tensor([1.0, 0.5]), torch.tensor([0.0, float("inf")]), torch.zeros(2, 2)):
        with pytest.raises(ValueError):
            CutpointParameter(3, bad.double())
    with pytest.raises(ValueError):
        CutpointParameter(4, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError):
        CutpointParameter(1, torch.tensor([0.0]))


# ------------------------------------------------------------------------------------------------ host-side checks
def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgp_hip.h")).read()
    for name in ("mgp_ordinal_evidence_site_workspace_bytes", "mgp_ordinal_evidence_site", "mgp_ordinal_cut_sums_workspace_bytes",
                 "mgp_ordinal_cut_sums"):
        assert name in _lib.SIGNATURES and hasattr(handle, name) and name + "(" in header
    buf, dbl, byt = (ctypes.c_float * 8)(), (ctypes.c_double * 256)(), (ctypes.c_uint8 * 8)()
    u, d, c = ctypes.addressof(buf), ctypes.addressof(dbl), ctypes.addressof(byt)
    wb = lib.mgp_ordinal_evidence_site_workspace_bytes
    assert wb(0) == 0 and wb(1025) == 64 and wb(2 ** 40) == 1024 * 32 and wb(5) == lib.mgp_laplace_evidence_site_workspace_bytes(5)
    site = lib.mgp_ordinal_evidence_site
    assert site(None, u, u, None, d, 4, 1e-30, u, u, d, d, 64, None) == -1
    assert site(u, None, u, None, d, 4, 1e-30, u, u, d, d, 64, None) == -1
    assert site(u, u, None, None, d, 4, 1e-30, u, u, d, d, 64, None) == -1
    assert site(u, u, u, None, d, 4, 1e-30, None, u, d, d, 64, None) == -1
    assert site(u, u, u, None, d, 4, 1e-30, u, u, None, d, 64, None) == -1
    assert site(u, u, u, None, d, 0, 1e-30, u, u, d, d, 64, None) == -1
    assert site(u, u, u, None, d, 4, -1.0, u, u, d, d, 64, None) == -1
    assert site(u, u, u, None, d, 4, float("nan"), u, u, d, d, 64, None) == -1
    assert site(u, u, u, None, d, 4, 1e-30, u, u, d, None, 64, None) == -2
    assert site(u, u, u, None, d, 4, 1e-30, u, u, d, d, 31, None) == -2
    assert site(u, u, u, None, d, 4, 1e-30, u, u, d, d + 4, 64, None) == -2
    cb = lib.mgp_ordinal_cut_sums_workspace_bytes
    assert cb(0, 4) == 0 and cb(10, 1) == 0 and cb(10, 65) == 0 and cb(10, 2) == 24 and cb(257, 4) == 2 * 72
    assert cb(2 ** 40, 64) == 1024 * 3 * 63 * 8
    cuts = lib.mgp_ordinal_cut_sums
    ok = dict(f=u, lo=u, hi=u, cat=c, obs=None, var=d, u=d, n=4, K=4, floor=1e-30, out=d, work=d, wb=72)

    def call(**kw):
        a = dict(ok, **kw)
        return cuts(a["f"], a["lo"], a["hi"], a["cat"], a["obs"], a["var"], a["u"], a["n"], a["K"], a["floor"], a["out"], a["work"],
                    a["wb"], None)
    for name in ("f", "lo", "hi", "cat", "out"):
        assert call(**{name: None}) == -1, name
    assert call(n=0) == -1 and call(K=1) == -1 and call(K=65) == -1 and call(floor=-1.0) == -1 and call(floor=float("nan")) == -1
    assert call(work=None) == -2 and call(wb=71) == -2 and call(work=d + 4) == -2 and call(K=5) == -2


def test_python_argument_checks():
    from manifold_gp_amd import evidence as ev, ordinal
    f, lo, hi = torch.zeros(3), torch.tensor([-INF, 0.0, 1.0]), torch.tensor([0.0, 1.0, INF])
    cat, one = torch.tensor([0, 1, 2]), torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="h_floor"):
        ordinal.ordinal_evidence_site(f, lo, hi, None, None, -1.0)
    with pytest.raises(ValueError, match="lo must"):
        ordinal.ordinal_evidence_site(f, None, hi)
    with pytest.raises(ValueError, match="hi has"):
        ordinal.ordinal_evidence_site(f, lo, torch.ones(4))
    with pytest.raises(ValueError, match="observed"):
        ordinal.ordinal_evidence_site(f, lo, hi, torch.ones(3))
    with pytest.raises(ValueError, match="variance"):
        ordinal.ordinal_evidence_site(f, lo, hi, None, torch.ones(4))
    with pytest.raises(ValueError, match="no entries"):
        ordinal.ordinal_evidence_site(torch.zeros(0), torch.zeros(0), torch.zeros(0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ordinal.ordinal_evidence_site(f, lo, hi, None, one)
    for K in (1, 65, 2.0, True):
        with pytest.raises(ValueError, match="num_categories"):
            ordinal.ordinal_cut_sums(f, lo, hi, cat, None, one, one, K)
    for bad in (None, cat.double(), cat > 0):
        with pytest.raises(ValueError, match="cat must"):
            ordinal.ordinal_cut_sums(f, lo, hi, bad, None, one, one, 3)
    with pytest.raises(ValueError, match="cat has"):
        ordinal.ordinal_cut_sums(f, lo, hi, torch.tensor([0, 1]), None, one, one, 3)
    with pytest.raises(ValueError, match="u has"):
        ordinal.ordinal_cut_sums(f, lo, hi, cat, None, one, torch.ones(2), 3)
    with pytest.raises(ValueError, match="h_floor"):
        ordinal.ordinal_cut_sums(f, lo, hi, cat, None, one, one, 3, h_floor=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ordinal.ordinal_cut_sums(f, lo, hi, cat, None, None, None, 3)
    # learn_cutpoints: its own arguments, then the fit's, all before the device
    d, y = _fake_desc(), torch.tensor([0.0, 1.0, 2.0])
    for kw, match in ((dict(steps=0), "steps"), (dict(steps=2.5), "steps"), (dict(lr=0.0), "lr"), (dict(variance=torch.ones(3)), "variance"),
                      (dict(num_categories=1), "num_categories"), (dict(cutpoints0=torch.tensor([0.0, 2.0 ** -11])), "2\\^-10"),
                      (dict(cutpoints0=torch.tensor([1.0])), "cutpoints")):
        with pytest.raises(ValueError, match=match):
            ordinal.learn_cutpoints(d, y, **dict(dict(num_categories=3), **kw))
    with pytest.raises(ValueError, match="categories"):
        ordinal.learn_cutpoints(d, torch.tensor([0.0, 1.0, 5.0]), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ordinal.learn_cutpoints(d, y, 3)
    # laplace_evidence(cutpoints=)
    b = torch.tensor([-0.5, 0.5], dtype=torch.float64)
    fit = ordinal.OrdinalLaplaceFit(d, torch.tensor([0, 1, 2]), None, f, True, 0, [], 0.0, b, lo, hi)
    assert ev._site_of(fit) == ("ordinal", 0.0, None, 2.0, None) and ev.ORDINAL_FAMILY == "ordinal"
    for bad, match in ((b.float(), "float64"), (b[:1], "float64"), ([0.0, 1.0], "float64"), (b + 1e-3, "fit.cutpoints")):
        with pytest.raises(ValueError, match=match):
            ev.laplace_evidence(fit, cutpoints=bad)
    assert ev._check_cutpoints(fit, "ordinal", b) is False and ev._check_cutpoints(fit, "ordinal", b.clone().requires_grad_()) is True
    assert ev._check_cutpoints(fit, "ordinal", (b + 1e-12).requires_grad_()) is True      # the same float32 values
    with pytest.raises(ValueError, match="ordinal fit"):
        ev._check_cutpoints(fit, "bernoulli", b)
    with pytest.raises(NotImplementedError, match="ordinal"):
        fit.evidence()
    with pytest.raises(NotImplementedError, match="laplace_evidence"):
        fit.evidence(method="dense")
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.laplace_evidence()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.laplace_evidence(fit)
    with pytest.raises(ValueError, match="family"):
        ev.evidence_site(f, f, None, None, None, 0.0, "ordinal")                           # the (y, aux) stage has no such family
    # cutpoints given as a module or as a tensor that requires grad are split into the fit's values and the live tensor
    cut = ordinal.CutpointParameter(3, b)
    kw, live = ordinal._live_cutpoints(dict(num_categories=3, cutpoints=cut))
    assert live is not None and live.requires_grad and not kw["cutpoints"].requires_grad and torch.equal(kw["cutpoints"], live.detach())
    assert ordinal._live_cutpoints(dict(cutpoints=b))[1] is None and ordinal._live_cutpoints(dict(num_categories=3)) == (dict(num_categories=3), None)
    with torch.no_grad():
        assert ordinal._live_cutpoints(dict(cutpoints=cut))[1] is None


def test_exports_and_signatures():
    from manifold_gp_amd import evidence as ev, ordinal, utils
    from manifold_gp_amd.classification import LaplaceFit
    from manifold_gp_amd.models import RiemannGP
    P = lambda fn: list(inspect.signature(fn).parameters)
    assert P(ordinal.ordinal_evidence_site) == ["f", "lo", "hi", "observed", "variance", "h_floor"]
    assert P(ordinal.ordinal_cut_sums) == ["f", "lo", "hi", "cat", "observed", "variance", "u", "K", "h_floor"]
    assert P(ordinal.learn_cutpoints) == ["desc", "y", "num_categories", "observed", "cutpoints0", "steps", "lr", "var_samples", "variance",
                                          "fit_kw", "evidence_kw"]
    sig = inspect.signature(ordinal.learn_cutpoints).parameters
    assert (sig["steps"].default, sig["lr"].default, sig["var_samples"].default) == (30, 0.1, 64)
    assert P(ordinal.CutpointParameter.__init__) == ["self", "num_categories", "init"] and issubclass(ordinal.CutpointParameter, torch.nn.Module)
    assert P(ev.laplace_evidence)[:4] == ["fit", "operator", "variance", "var_samples"] and P(ev.laplace_evidence)[-1] == "cutpoints"
    assert inspect.signature(ev.laplace_evidence).parameters["cutpoints"].default is None
    assert P(ev.LaplaceEvidence.__init__)[-2:] == ["site_sums", "cutpoint_grad"]
    assert ev.LaplaceEvidence(0, 0, 0, 0, 0, 0, "dense", 1, None, None).cutpoint_grad is None
    assert ev.FAMILIES == {"poisson": 0, "binomial": 1, "bernoulli": 2} and ev.NB_FAMILY == "negative_binomial"
    assert P(RiemannGP.laplace_evidence) == ["self", "observed", "family", "kw"]
    assert P(utils.laplace_train) == ["model", "optimizer", "observed", "family", "max_iter", "tolerance", "fit_kw", "evidence_kw", "verbose"]
    assert P(ordinal.laplace_fit_ordinal)[:5] == ["desc", "y", "num_categories", "cutpoints", "observed"]
    assert callable(ordinal.OrdinalLaplaceFit.laplace_evidence) and ordinal.OrdinalLaplaceFit.evidence is not LaplaceFit.evidence
    assert not hasattr(LaplaceFit, "laplace_evidence")
