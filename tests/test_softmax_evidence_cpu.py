"""The Laplace evidence of the softmax fit, host side (no GPU): the float64 restatement the GPU tests are checked against
(tests/_softmax_evidence_ref.py) is itself checked -- R R^T = H and R s = 0, logdet B against logdet A - C logdet Q, the block
formula of B against the general one, the closed form of the curvature term g against brute force and against its sample form, the
analytic gradient against central differences of the dense log Z with the mode re-fitted, the float64 Lanczos quadrature on B
against the dense value -- and the C-ABI and Python argument checks, exports and signatures."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _observed_ref as oref
import _softmax_evidence_ref as sev
import _softmax_ref as sref
from test_evidence_cpu import _dq_dlogkappa, _fake_desc, _unit_precision

CASE, NU, C = "dumbbell_k10_loop", 2, sev.C_FIT
_P = {}


def _problem(golden):
    """k10_loop, symmetric, nu = 2, scaled to a prior marginal variance of about 9, C = 3, the labels of _softmax_ref.labels
    (10 % observed), the float64 mode"""
    if not _P:
        Q1 = _unit_precision(golden, CASE, "symmetric", NU)
        scale = np.diag(np.linalg.inv(Q1)).mean() / 9.0
        Q = scale * Q1
        t, obs, _ = sref.labels(golden(CASE), C)
        solver = sref.Solver(Q, obs)
        F = sref.newton(Q, t, obs, C, solver=solver)[0]
        _P.update(Q1=Q1, scale=scale, Q=Q, t=t, obs=obs, solver=solver, F=F, Pi=sref.site(F, t, obs)[2])
    return _P


def _small(seed=0, n=40, C=4, m=9):
    """a small dense problem: a random SPD Q, random softmax rows at m of the n nodes"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    Q = G @ G.T / n + 0.3 * np.eye(n)
    obs = np.zeros(n, bool)
    obs[rng.choice(n, m, replace=False)] = True
    Pi = np.where(obs[:, None], sref.softmax(rng.standard_normal((n, C)) * 2.0), 0.0)
    return Q, obs, Pi


def test_factor_is_a_root_of_the_hessian_and_annihilates_s():
    _, obs, Pi = _small()
    R, H = sref.factor_blocks(Pi), sref.hess_blocks(Pi)
    assert np.abs(np.einsum("iab,icb->iac", R, R) - H).max() <= 1e-15
    assert np.abs(np.einsum("iab,ib->ia", R, np.sqrt(Pi))).max() <= 1e-15               # R s = 0
    rng = np.random.default_rng(1)
    V = rng.standard_normal((Pi.shape[0], Pi.shape[1], 5))
    for k in range(5):
        assert np.abs(sev.root_apply(Pi, V)[0][:, :, k] - np.einsum("iab,ib->ia", R, V[:, :, k])).max() <= 1e-14
        assert np.abs(sev.root_apply_t(Pi, V)[0][:, :, k] - np.einsum("iba,ib->ia", R, V[:, :, k])).max() <= 1e-14
    sc = np.swapaxes(V, 1, 2).copy()
    assert np.array_equal(np.swapaxes(sev.root_apply(Pi, sc, "sc")[0], 1, 2), sev.root_apply(Pi, V)[0])
    assert np.array_equal(sev.root_apply_t(Pi, V, V)[0], V + sev.root_apply_t(Pi, V)[0])
    # unobserved rows: 0 forward, V transposed, whatever the entries hold
    Vn = np.where(obs[:, None, None], V, np.nan)
    assert not sev.root_apply(Pi, Vn)[0][~obs].any() and np.array_equal(sev.root_apply_t(Pi, Vn, V)[0][~obs], V[~obs])


def test_logdet_b_is_logdet_a_minus_c_logdet_q_and_the_block_formula_is_the_general_one():
    Q, obs, Pi = _small()
    n, Cs = Pi.shape
    Bg = sev.dense_b_general(Q, Pi)
    solver = sref.Solver(Q, obs)
    Bo = sev.dense_b(solver.Koo, Pi[obs])
    at = (np.flatnonzero(obs)[:, None] * Cs + np.arange(Cs)[None, :]).reshape(-1)
    off = np.setdiff1d(np.arange(n * Cs), at)
    assert np.abs(Bg[np.ix_(at, at)] - Bo).max() <= 1e-13                                  # the block formula on the observed entries
    assert np.array_equal(Bg[np.ix_(off, off)], np.eye(off.size)) and not Bg[np.ix_(off, at)].any()   # the identity elsewhere
    assert np.abs(Bg - Bg.T).max() <= 1e-14 and np.linalg.eigvalsh(Bg).min() >= 1.0 - 1e-12
    s = np.sqrt(Pi).reshape(-1)
    for i in np.flatnonzero(obs):                                                          # a unit eigenvalue along s_i
        e = np.zeros(n * Cs)
        e[i * Cs:(i + 1) * Cs] = s[i * Cs:(i + 1) * Cs]
        assert np.abs(Bg @ e - e).max() <= 1e-14
    want = np.linalg.slogdet(sref.dense_system(Q, Pi))[1] - Cs * np.linalg.slogdet(Q)[1]
    got, got_o = np.linalg.slogdet(Bg)[1], sev.logdet_b(solver, Pi)
    assert abs(got - want) <= 1e-10 * abs(want) and abs(got_o - want) <= 1e-10 * abs(want)


def test_logdet_identity_on_the_fixture(golden):
    p = _problem(golden)
    Q, Pi = p["Q"], p["Pi"]
    got = sev.logdet_b(p["solver"], Pi)
    want = np.linalg.slogdet(sref.dense_system(Q, Pi))[1] - C * np.linalg.slogdet(Q)[1]
    z = sev.log_z(Q, p["F"], p["t"], p["obs"], p["solver"])
    print("logdet B = %.6f (logdet A - C logdet Q: %.6f), m = %d, log Z = %.6f" % (got, want, z["m"], z["value"]))
    assert abs(got - want) <= 1e-10 * abs(want)
    assert z["m"] == int(p["obs"].sum()) and z["value"] == z["log_likelihood"] - z["quad"] - 0.5 * got


def test_closed_form_of_the_curvature_term_matches_brute_force(golden):
    p = _problem(golden)
    g, brute = sev.curvature(p["solver"], p["Pi"]), sev.curvature_brute(p["solver"], p["F"], p["obs"])
    print("g: largest %.4g, closed form against central differences of H: %.2e" % (np.abs(g).max(), np.abs(g - brute).max()))
    assert not g[~p["obs"]].any() and np.abs(g).max() > 0
    assert np.abs(g - brute).max() <= 1e-8 * np.abs(g).max()
    assert np.abs(g.sum(1)).max() <= 1e-12 * np.abs(g).max()                               # H 1 = 0 for every f: the rows of g sum to 0
    # the blocks of A^-1 the closed form uses, against the naive inverse on a small problem
    Q, obs, Pi = _small()
    solver = sref.Solver(Q, obs)
    Ai = np.linalg.inv(sref.dense_system(Q, Pi))
    V, _ = sev.covariance_blocks(solver, Pi)
    Cs = Pi.shape[1]
    for k, i in enumerate(np.flatnonzero(obs)):
        assert np.abs(V[k] - Ai[i * Cs:(i + 1) * Cs, i * Cs:(i + 1) * Cs]).max() <= 1e-12
    n = Q.shape[0]
    M = sum(np.kron(np.linalg.inv(Q), np.eye(Cs))[c::Cs, c::Cs] - Ai[c::Cs, c::Cs] for c in range(Cs))
    assert np.abs(sev.trace_matrix(solver, Pi) - M).max() <= 1e-12 and M.shape == (n, n)


def test_sample_form_of_the_curvature_term_converges_to_the_dense_one(golden):
    """S = 2048 deviations delta ~ N(0, A^-1) on the observed rows, through the arithmetic of mgp_softmax_curvature: every entry
    within 6 of its own standard errors."""
    p = _problem(golden)
    g = sev.curvature(p["solver"], p["Pi"])[p["obs"]]
    _, Soo = sev.covariance_blocks(p["solver"], p["Pi"])
    S, m = 2048, g.shape[0]
    L = np.linalg.cholesky(0.5 * (Soo + Soo.T))
    delta = (L @ np.random.default_rng(5).standard_normal((m * C, S))).reshape(m, C, S).transpose(0, 2, 1)
    acc, acc2, _, _ = sev.curvature_sums(p["Pi"][p["obs"]], delta)
    est = acc / S
    se = np.sqrt(np.maximum(acc2 / S - est * est, 0.0) / (S - 1))
    worst = (np.abs(est - g) / se).max()
    print("sample form of g at S = %d: worst entry %.2f standard errors from the dense one (largest |g| %.4g, largest se %.4g)"
          % (S, worst, np.abs(g).max(), se.max()))
    assert worst <= 6.0


def test_analytic_gradient_matches_central_differences_of_the_refitted_log_z(golden):
    """theta = log scale and log kappa on k10_loop, symmetric, nu = 2, C = 3: 1e-6 relative."""
    p = _problem(golden)
    kappa, scale, t, obs = float(golden(CASE)["kappa"]), p["scale"], p["t"], p["obs"]
    step = 1e-4

    def logz(ls, lk):
        Q = scale * np.exp(ls) * _unit_precision(golden, CASE, "symmetric", NU, kappa * np.exp(lk))
        solver = sref.Solver(Q, obs)
        return sev.log_z(Q, sref.newton(Q, t, obs, C, f0=p["F"], solver=solver)[0], t, obs, solver)["value"]
    for name, dQ, at in (("log scale", p["Q"], (step, 0.0)), ("log kappa", _dq_dlogkappa(golden, CASE, NU, kappa, scale), (0.0, step))):
        got, terms, _ = sev.gradient(p["Q"], dQ, p["F"], t, obs, p["solver"])
        fd = (logz(*at) - logz(-at[0], -at[1])) / (2.0 * step)
        print("%s: analytic %.9f (terms %.6f %.6f %.6f), central differences %.9f" % (name, got, *terms, fd))
        assert abs(got - fd) <= 1e-6 * abs(fd), (name, got, fd)


def test_float64_quadrature_on_b_is_within_five_standard_errors(golden):
    p = _problem(golden)
    dense = sev.logdet_b(p["solver"], p["Pi"])
    Z = sev.probes(p["obs"], C, sev.SLQ_PROBES, sev.SLQ_SEED)
    m = int(p["obs"].sum())
    per, est, se = sev.slq_per_probe(p["solver"], p["Pi"], Z, sev.SLQ_STEPS)
    print("dense %.4f, quadrature %.4f +- %.4f (%.2f standard errors), m C = %d" % (dense, est, se, abs(est - dense) / se, m * C))
    assert (np.abs(Z).sum((0, 1)) == m * C).all() and not Z[~p["obs"]].any()
    assert abs(est - dense) <= 5.0 * se
    # the probe term of the gradient at the same probes: within 5 standard errors of the dense trace
    exact = 0.5 * float((sev.trace_matrix(p["solver"], p["Pi"]) * p["Q"]).sum())
    est, se = sev.probe_trace(p["solver"], p["Q"], p["Pi"], Z)
    assert abs(est - exact) <= 5.0 * se, (exact, est, se)


def test_float64_training_run_gains_what_the_gpu_test_assumes(golden):
    """The float64 restatement of the laplace_train test's optimiser with exact gradients: log Z rises at every step, by the
    recorded gain in all (at least 5)."""
    tr = sev.TRAIN
    g = golden(CASE)
    t, obs, _ = sref.labels(g, C)
    trace = sev.train_f64(g, "symmetric", NU, t, obs, C, tr["kappa0"], tr["scale0"], tr["steps"], tr["lr"])
    z = [v[2] for v in trace]
    print("log Z %s; kappa %.4f -> %.4f, scale %.5g -> %.5g" % (["%.3f" % v for v in z], trace[0][0], trace[-1][0], trace[0][1], trace[-1][1]))
    assert len(z) == tr["steps"] + 1 and all(b > a for a, b in zip(z, z[1:]))
    assert z[-1] - z[0] >= 5.0 and abs(z[-1] - z[0] - tr["gain_f64"]) <= 0.01


# ------------------------------------------------------------------------------------------------ host-side checks
def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgp_softmax_root_apply", "mgp_softmax_curvature"):
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    buf, dbl = (ctypes.c_float * 8)(), (ctypes.c_double * 16)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    root = lib.mgp_softmax_root_apply

    def fwd(pi=u, V=u, X=None, n=2, C=3, S=1, cs=1, ss=3, tr=0, out=u):
        return root(pi, V, X, n, C, S, cs, ss, tr, out, None)
    assert fwd(pi=None) == -1 and fwd(V=None) == -1 and fwd(out=None) == -1 and fwd(X=u) == -1
    assert fwd(tr=1) == -1 and fwd(tr=1, V=None) == -1                                     # transposed without X
    assert fwd(n=0) == -1 and fwd(C=1) == -1 and fwd(C=65) == -1 and fwd(S=0) == -1
    assert fwd(C=64, S=5) == -1 and fwd(C=2, S=129) == -1                                  # C S > 256
    # strides: not positive, overlapping, beyond the row's C S floats
    for cs, ss in ((0, 1), (1, 0), (-1, 3), (1, 1), (1, 2), (2, 1), (3, 1), (5, 1), (1, 4), (2, 2), (4, 3)):
        assert fwd(C=3, S=4, cs=cs, ss=ss) == -1, (cs, ss)
    assert fwd(C=3, S=1, cs=2, ss=1) == -1
    curv = lib.mgp_softmax_curvature
    assert curv(None, u, 2, 3, 1, d, d + 64, None) == -1 and curv(u, None, 2, 3, 1, d, d + 64, None) == -1
    assert curv(u, u, 2, 3, 1, None, d + 64, None) == -1 and curv(u, u, 2, 3, 1, d, None, None) == -1
    assert curv(u, u, 2, 3, 1, d, d, None) == -1 and curv(u, u, 0, 3, 1, d, d + 64, None) == -1
    assert curv(u, u, 2, 1, 1, d, d + 64, None) == -1 and curv(u, u, 2, 65, 1, d, d + 64, None) == -1
    assert curv(u, u, 2, 3, 0, d, d + 64, None) == -1 and curv(u, u, 2, 64, 5, d, d + 64, None) == -1


def _fit(d, C=2, observed=None):
    from manifold_gp_amd.classification import MulticlassLaplaceFit
    return MulticlassLaplaceFit(d, None, observed, torch.zeros(3, C), torch.full((3, C), 1.0 / C), True, 0, [], 0.0)


def test_python_argument_checks():
    from manifold_gp_amd import evidence as ev
    pi, V = torch.full((3, 2), 0.5), torch.zeros(3, 2, 4)
    for bad in (torch.zeros(3), torch.zeros(3, 2, dtype=torch.float64), torch.zeros(2, 3).t(), torch.zeros(3, 1), torch.zeros(3, 65)):
        with pytest.raises(ValueError, match="pi "):
            ev.softmax_root_apply(bad, V)
        with pytest.raises(ValueError, match="pi "):
            ev.softmax_curvature(bad, torch.zeros(3, 4, 2))
    with pytest.raises(ValueError, match="layout"):
        ev.softmax_root_apply(pi, V, layout="ncs")
    with pytest.raises(ValueError, match="needs X"):
        ev.softmax_root_apply(pi, V, transpose=True)
    with pytest.raises(ValueError, match="takes no X"):
        ev.softmax_root_apply(pi, V, V)
    for bad in (torch.zeros(3, 2), torch.zeros(3, 3, 4), torch.zeros(4, 2, 4)):
        with pytest.raises(ValueError, match="V must be a tensor"):
            ev.softmax_root_apply(pi, bad)
    with pytest.raises(ValueError, match="V must be a tensor"):
        ev.softmax_root_apply(pi, V, layout="sc")                                          # [3, 2, 4] read as [n, S, C]: C = 4
    with pytest.raises(ValueError, match="X must be a tensor"):
        ev.softmax_root_apply(pi, None, torch.zeros(3, 3, 4), transpose=True)
    with pytest.raises(ValueError, match="columns"):
        ev.softmax_root_apply(pi, torch.zeros(3, 2, 129))
    with pytest.raises(ValueError, match="V must be a contiguous float32"):
        ev.softmax_root_apply(pi, torch.zeros(3, 2, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="V must be a contiguous float32"):
        ev.softmax_root_apply(pi, torch.zeros(3, 2, 5), torch.zeros(3, 2, 4), transpose=True)
    with pytest.raises(ValueError, match="out must be"):
        ev.softmax_root_apply(pi, V, out=torch.zeros(3, 4, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.softmax_root_apply(pi, V)
    delta = torch.zeros(3, 4, 2)
    for bad in (torch.zeros(3, 4), torch.zeros(3, 4, 3), torch.zeros(3, 4, 2, dtype=torch.float64), torch.zeros(3, 2, 4).transpose(1, 2)):
        with pytest.raises(ValueError, match="delta must"):
            ev.softmax_curvature(pi, bad)
    with pytest.raises(ValueError, match="columns"):
        ev.softmax_curvature(pi, torch.zeros(3, 129, 2))
    acc = torch.zeros(3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="come together"):
        ev.softmax_curvature(pi, delta, acc)
    with pytest.raises(ValueError, match="acc2 must"):
        ev.softmax_curvature(pi, delta, acc, torch.zeros(3, 2))
    with pytest.raises(ValueError, match="distinct"):
        ev.softmax_curvature(pi, delta, acc, acc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.softmax_curvature(pi, delta)
    d, obs = _fake_desc(), torch.tensor([True, False, True])
    with pytest.raises(NotImplementedError):
        ev.logdet_b_softmax(_fake_desc(form=2), pi, obs)
    for kw, match in ((dict(num_probes=0), "num_probes"), (dict(steps=True), "steps"), (dict(solve_tol=0.0), "solve_tol"),
                      (dict(method="lanczos"), "method"), (dict(probes=torch.ones(3, 2)), "probes"),
                      (dict(probes=torch.ones(3, 3, 4)), "probes"), (dict(probes=torch.ones(3, 2, 1)), "probes")):
        with pytest.raises(ValueError, match=match):
            ev.logdet_b_softmax(d, pi, obs, **kw)
    with pytest.raises(ValueError, match="observed"):
        ev.logdet_b_softmax(d, pi, torch.ones(3))
    with pytest.raises(ValueError, match="rows"):
        ev.logdet_b_softmax(d, torch.full((4, 2), 0.5), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.logdet_b_softmax(d, pi, obs)
    with pytest.raises(NotImplementedError, match="MulticlassLaplaceFit"):
        ev.softmax_evidence(object())
    with pytest.raises(ValueError, match="curvature"):
        ev.softmax_evidence(_fit(d), curvature=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="method"):
        _fit(d).laplace_evidence(method="exact")
    # the old names keep raising; the message names the new one
    with pytest.raises(NotImplementedError, match="softmax") as info:
        _fit(d).evidence()
    assert "laplace_evidence" in str(info.value)
    with pytest.raises(NotImplementedError):
        ev.laplace_evidence(_fit(d))
    Z = ev.softmax_probes(obs, 2, 5, 3)
    assert Z.shape == (3, 2, 5) and Z.dtype == torch.float32 and not Z[1].any() and bool((Z[obs].abs() == 1).all())
    assert torch.equal(Z, ev.softmax_probes(obs, 2, 5, 3))
    assert np.array_equal(Z.numpy(), sev.probes(obs.numpy(), 2, 5, 3))


def test_the_multiclass_family_needs_num_classes_and_unknown_families_still_raise():
    from manifold_gp_amd.models import RiemannGP
    from manifold_gp_amd.utils import laplace_train
    model = RiemannGP.__new__(RiemannGP)                       # the dispatch alone: no kernel, no data
    with pytest.raises(ValueError, match="num_classes"):
        RiemannGP._laplace_fit(model, None, "multiclass")
    with pytest.raises(ValueError, match="num_classes"):
        RiemannGP.laplace_evidence(model, family="multiclass")
    with pytest.raises(ValueError, match="family"):
        RiemannGP.laplace_evidence(model, family="softmax")
    with pytest.raises(ValueError, match="family"):
        laplace_train(model, None, family="softmax")


def test_exports_and_signatures():
    import manifold_gp_amd
    from manifold_gp_amd import evidence as ev
    from manifold_gp_amd.classification import MulticlassLaplaceFit
    sig = inspect.signature(ev.softmax_root_apply).parameters
    assert list(sig)[:5] == ["pi", "V", "X", "transpose", "out"] and sig["X"].default is None and sig["transpose"].default is False
    assert list(inspect.signature(ev.softmax_curvature).parameters)[:2] == ["pi", "delta"]
    sig = inspect.signature(ev.logdet_b_softmax).parameters
    assert list(sig) == ["desc", "pi", "observed", "num_probes", "steps", "seed", "solve_tol", "method", "probes", "max_iter"]
    assert (sig["num_probes"].default, sig["steps"].default, sig["seed"].default, sig["solve_tol"].default, sig["method"].default,
            sig["probes"].default, sig["max_iter"].default) == (16, 12, 1337, 1e-6, "auto", None, 5000)
    sig = inspect.signature(ev.softmax_evidence).parameters
    assert list(sig)[:5] == ["fit", "operator", "curvature", "var_samples", "block"]
    assert (sig["operator"].default, sig["curvature"].default, sig["var_samples"].default, sig["block"].default) == (None, None, 64, None)
    assert callable(MulticlassLaplaceFit.laplace_evidence) and callable(ev._SoftmaxBOperator)
    op = ev._SoftmaxBOperator(_fake_desc(), torch.full((3, 2), 0.5), 1e-6, 100)
    assert op.shape == (6, 6) and op.solves == 0 and op.iterations == 0
    with pytest.raises(ValueError, match="V must be"):
        op.matmul(torch.zeros(5, 2))
    assert ev.MULTICLASS_FAMILY == "multiclass" and ev.DENSE_MAX_ENTRIES == 4096 and ev.DENSE_MAX == 512
    assert ev._softmax_method("auto", 512, 8) == "dense" and ev._softmax_method("auto", 513, 2) == "slq"
    assert ev._softmax_method("auto", 400, 11) == "slq" and ev._softmax_method("slq", 3, 2) == "slq"
    assert manifold_gp_amd.evidence is ev
