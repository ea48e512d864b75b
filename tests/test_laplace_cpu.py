"""Laplace classification, host side (no GPU): the float64 restatement the GPU tests are checked against
(tests/_laplace_ref.py) is itself checked -- its mode is stationary, its gradient agrees with central differences of its
objective, its trapezoid rule agrees with 30-digit quadrature --, and the C-ABI and Python argument checks."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _laplace_ref as lref
import _observed_ref as oref


@pytest.fixture(scope="module")
def problem(golden):
    """dumbbell_k10_loop, symmetric, nu = 2, scaled to a prior marginal variance of about 9 (|f_hat| of a few units: with the
    fixture's own scale |f_hat| ~ 0.01 and the problem is linear)."""
    g = golden("dumbbell_k10_loop")
    lo = oref.oracle(g, "symmetric")
    Q1, _ = oref.precision_root(lo, 2, float(g["kappa"]), 1.0, "symmetric")
    scale = np.diag(np.linalg.inv(Q1)).mean() / 9.0
    t, obs, _ = lref.labels(g)
    return scale * Q1, t, obs


def test_reference_mode_is_stationary_and_nonlinear(problem):
    Q, t, obs = problem
    f, trace = lref.newton(Q, t, obs)
    res = np.abs(lref.gradient(Q, f, t, obs)).max()
    print("max |g - Q f| = %.2e after %d steps; max |f| = %.2f" % (res, len(trace), np.abs(f).max()))
    assert res <= 1e-10
    assert np.abs(f).max() > 1.0                                  # the regime the GPU tests are meant to run in
    assert all(b[0] >= a[0] - 1e-12 * abs(a[0]) for a, b in zip(trace, trace[1:]))


def test_reference_gradient_matches_central_differences(problem):
    Q, t, obs = problem
    rng = np.random.default_rng(3)
    f = rng.standard_normal(Q.shape[0])
    grad = lref.gradient(Q, f, t, obs)
    eps = 1e-5
    for i in list(np.flatnonzero(obs)[:5]) + list(np.flatnonzero(~obs)[:5]):
        d = np.zeros_like(f)
        d[i] = eps
        fd = (lref.psi(Q, f + d, t, obs) - lref.psi(Q, f - d, t, obs)) / (2 * eps)
        assert abs(fd - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])), (i, fd, grad[i])
    # the curvature against central differences of the gradient's likelihood part
    g_plus, g_minus = lref.site(f + eps, None, t, obs)[1], lref.site(f - eps, None, t, obs)[1]
    h = lref.site(f, None, t, obs)[2]
    assert np.abs(-(g_plus - g_minus) / (2 * eps) - h).max() <= 1e-9


def test_reference_site_is_finite_at_extreme_latents():
    f = np.array([1e4, -1e4, 1e4, -1e4, 0.0, 88.0, -90.0], np.float32)
    y = np.array([1, 1, 0, 0, 1, 0, 1], np.float32)
    w, rhs, sums, _ = lref.site_outputs(f, None, y, None, 4.0)
    assert np.isfinite(w).all() and np.isfinite(rhs).all() and np.isfinite(sums).all()
    assert w[0] == 0 and w[1] == 0 and w[4] == 1.0
    assert np.allclose(lref.site(f, None, (y > 0.5).astype(float), None)[0][:4], [0.0, -1e4, -1e4, 0.0], rtol=0, atol=0)


M_GRID = [-12.0, -7.5, -3.0, -1.0, -0.25, 0.0, 0.5, 2.0, 5.0, 12.0]


def _quad(m, v):
    import mpmath
    mpmath.mp.dps = 30
    sd = mpmath.sqrt(v)

    def fn(u):
        return mpmath.npdf(u) / (1 + mpmath.exp(-(m + sd * u)))
    return float(mpmath.quad(fn, [-mpmath.inf, -8, -2, 0, 2, 8, mpmath.inf]))


@pytest.mark.parametrize("vs, bound", [([1e-4, 0.01, 0.25, 1.0, 4.0, 9.0, 16.0, 25.0], 1e-12), ([49.0, 100.0], 1e-6)])
def test_trapezoid_rule_against_30_digit_quadrature(vs, bound):
    """K = 129 on [-8, 8]: <= 1e-12 for v <= 25, <= 1e-6 for v <= 100, m in [-12, 12] (measured: 1.9e-14 and 6.1e-8)."""
    worst = 0.0
    for v in vs:
        got = lref.trapezoid(np.array(M_GRID), np.full(len(M_GRID), v))
        want = np.array([_quad(m, v) for m in M_GRID])
        worst = max(worst, np.abs(got - want).max())
    print("v <= %g: worst %.2e" % (max(vs), worst))
    assert worst <= bound, worst


def test_trapezoid_rule_edge_cases():
    m = np.array([-3.0, 0.0, 2.5])
    from scipy.special import expit
    assert np.abs(lref.trapezoid(m, np.zeros(3)) - expit(m)).max() <= 1e-14
    assert np.array_equal(lref.trapezoid(m, -np.ones(3)), lref.trapezoid(m, np.zeros(3)))
    assert np.isnan(lref.trapezoid(np.array([np.nan]), np.array([1.0]))).all()
    assert np.isnan(lref.trapezoid(np.array([0.0]), np.array([np.nan]))).all()


# ------------------------------------------------------------------------------------------------ host-side checks
def test_signatures_name_both_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgp_bernoulli_site_workspace_bytes", "mgp_bernoulli_site", "mgp_bernoulli_predict"):
        assert name in _lib.SIGNATURES
        assert hasattr(handle, name)


def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    assert lib.mgp_bernoulli_site_workspace_bytes(0) == 0
    assert lib.mgp_bernoulli_site_workspace_bytes(1) == 32 and lib.mgp_bernoulli_site_workspace_bytes(1025) == 64
    assert lib.mgp_bernoulli_site_workspace_bytes(2 ** 40) == 1024 * 32            # the grid cap
    site = lib.mgp_bernoulli_site
    assert site(None, None, u, None, 4, 4.0, 0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, None, 4, 4.0, 0, None, u, d, d, 64, None) == -1
    assert site(u, None, u, None, 4, 4.0, 0, u, None, d, d, 64, None) == -1
    assert site(u, None, u, None, 4, 4.0, 0, u, u, None, d, 64, None) == -1
    assert site(u, None, u, None, 0, 4.0, 0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, None, 4, 4.0, 1, u, u, d, d, 64, None) == -3           # probit: not built
    assert site(u, None, u, None, 4, 4.0, 0, u, u, d, None, 64, None) == -2
    assert site(u, None, u, None, 4, 4.0, 0, u, u, d, d, 31, None) == -2
    pred = lib.mgp_bernoulli_predict
    assert pred(None, d, 4, 129, d, None) == -1 and pred(u, None, 4, 129, d, None) == -1
    assert pred(u, d, 4, 129, None, None) == -1 and pred(u, d, 0, 129, d, None) == -1
    for K in (7, 128, 1027, -1):
        assert pred(u, d, 4, K, d, None) == -1


def test_float64_apply_checks_its_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 16)()
    idx = (ctypes.c_int32 * 8)(0, 4, 4, 4, 4, 4, 4, 4)
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    op = _lib.OperatorT()
    op.L.n, op.L.rowptr, op.L.col, op.L.vals, op.L.diag = 1, ctypes.addressof(idx), ctypes.addressof(idx), u, u
    op.nu, op.kappa, op.scale, op.noise, op.form = 2, 1.0, 1.0, 0.0, 0
    fn, ref = lib.mgp_operator_apply_double, ctypes.byref(op)
    assert lib.mgp_operator_apply_double_workspace_bytes(ref, 3) == 4 * 3 * 8
    assert lib.mgp_operator_apply_double_workspace_bytes(ref, 0) == 0
    assert fn(None, d, 1, d + 8, d + 64, 32, None) == -1 and fn(ref, None, 1, d + 8, d + 64, 32, None) == -1
    assert fn(ref, d, 1, None, d + 64, 32, None) == -1 and fn(ref, d, 1, d, d + 64, 32, None) == -1      # in place
    assert fn(ref, d, 0, d + 8, d + 64, 32, None) == -1
    assert fn(ref, d, 1, d + 8, None, 32, None) == -2 and fn(ref, d, 1, d + 8, d + 64, 31, None) == -2
    op.form = 3
    assert fn(ref, d, 1, d + 8, d + 64, 32, None) == -1                                                   # form 3 without weights


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_laplace_fit_argument_checks():
    from manifold_gp_amd.classification import bernoulli_predict, laplace_fit
    d = _fake_desc()
    y = torch.tensor([0.0, 1.0, 1.0])
    some = torch.tensor([True, False, True])
    with pytest.raises(ValueError, match="0 or 1"):
        laplace_fit(d, torch.tensor([0.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="0 or 1"):
        laplace_fit(d, torch.tensor([float("nan"), 1.0, 1.0]), observed=some)       # NaN at an observed node
    with pytest.raises(ValueError, match="no node"):
        laplace_fit(d, y, observed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        laplace_fit(d, y, observed=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        laplace_fit(d, y, observed=torch.ones(3))
    with pytest.raises(ValueError):
        laplace_fit(d, torch.zeros(4))
    with pytest.raises(ValueError, match="link"):
        laplace_fit(d, y, link="probit")
    with pytest.raises(ValueError, match="f0"):
        laplace_fit(d, y, f0=torch.zeros(2))
    with pytest.raises(NotImplementedError):
        laplace_fit(_fake_desc(form=2), y)
    with pytest.raises(RuntimeError, match="no CPU path"):                          # valid arguments, host tensors
        laplace_fit(d, torch.tensor([0.0, float("nan"), 1.0]), observed=some)
    for K in (8, 7, 1027, 129.0):
        with pytest.raises(ValueError, match="points"):
            bernoulli_predict(torch.zeros(3), torch.zeros(3), points=K)


def test_model_method_exists():
    import inspect
    from manifold_gp_amd.models import RiemannGP
    sig = inspect.signature(RiemannGP.laplace_posterior)
    assert list(sig.parameters) == ["self", "observed", "kw"]
