"""C-class Laplace classification, host side (no GPU): the float64 restatement the GPU tests are checked against
(tests/_softmax_ref.py) is itself checked -- its mode is stationary with rows that sum to zero, its gradient agrees with central
differences, its factor R reproduces H, its reduced solve agrees with the naive dense system, two classes agree with the binary
restatement at half the scale --, and the C-ABI and Python argument checks of the new entry points."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _laplace_ref as lref
import _observed_ref as oref
import _softmax_ref as sref

C3 = 3


@pytest.fixture(scope="module")
def precision(golden):
    """dumbbell_k10_loop, symmetric, nu = 2, scaled to a prior marginal variance of about 9 (as test_laplace_cpu.problem)."""
    g = golden("dumbbell_k10_loop")
    lo = oref.oracle(g, "symmetric")
    Q1, _ = oref.precision_root(lo, 2, float(g["kappa"]), 1.0, "symmetric")
    return g, (np.diag(np.linalg.inv(Q1)).mean() / 9.0) * Q1


@pytest.fixture(scope="module")
def problem(precision):
    g, Q = precision
    t, obs, _ = sref.labels(g, C3)
    F, trace = sref.newton(Q, t, obs, C3)
    return Q, t, obs, F, trace


def test_labels_cover_every_class_and_flip_five_percent(precision):
    g, _ = precision
    for C in (2, 3, 10):
        t, obs, y = sref.labels(g, C)
        assert t.min() == 0 and t.max() == C - 1 and set(np.unique(t[obs])) == set(range(C))
        assert np.isnan(y[~obs]).all() and np.array_equal(y[obs], t[obs].astype(np.float32))
        assert 0.05 <= obs.mean() <= 0.15


def test_reference_mode_is_stationary_with_zero_row_sums(problem):
    Q, t, obs, F, trace = problem
    res = np.abs(sref.gradient(Q, F, t, obs)).max()
    rows = np.abs(F.sum(1)).max()
    print("max |G - Q F| = %.2e, max |row sum| = %.2e after %d steps (steps %s); max |F| = %.2f"
          % (res, rows, len(trace), [s for _, _, s in trace], np.abs(F).max()))
    assert res <= 1e-10 and rows <= 1e-10
    assert np.abs(F).max() > 1.0                                  # the regime the GPU tests are meant to run in
    assert all(b[0] >= a[0] - 1e-12 * abs(a[0]) for a, b in zip(trace, trace[1:]))


def test_reference_gradient_and_hessian_match_central_differences(problem):
    Q, t, obs = problem[:3]
    rng = np.random.default_rng(3)
    n = Q.shape[0]
    F = rng.standard_normal((n, C3))
    grad = sref.gradient(Q, F, t, obs)
    eps = 1e-5
    for i in list(np.flatnonzero(obs)[:4]) + list(np.flatnonzero(~obs)[:3]):
        for c in range(C3):
            d = np.zeros_like(F)
            d[i, c] = eps
            fd = (sref.psi(Q, F + d, t, obs) - sref.psi(Q, F - d, t, obs)) / (2 * eps)
            assert abs(fd - grad[i, c]) <= 1e-6 * max(1.0, abs(grad[i, c])), (i, c, fd, grad[i, c])
    # H X against central differences of the likelihood part of the gradient along X
    X = rng.standard_normal((n, C3))
    Pi = sref.site(F, t, obs)[2]
    fd = -(sref.site(F + eps * X, t, obs)[1] - sref.site(F - eps * X, t, obs)[1]) / (2 * eps)
    assert np.abs(fd - sref.hess_apply(Pi, X)).max() <= 1e-9


def test_factor_reproduces_the_hessian():
    rng = np.random.default_rng(5)
    for C in (2, 3, 10, 64):
        Pi = sref.softmax(rng.standard_normal((50, C)) * 3.0)
        Pi[::7] = 0.0                                              # unobserved rows
        Rm, Hm = sref.factor_blocks(Pi), sref.hess_blocks(Pi)
        err = np.abs(Rm @ Rm.transpose(0, 2, 1) - Hm).max()
        assert err <= 1e-15, (C, err)
        eps = rng.standard_normal((50, C))
        assert np.abs(sref.noise_factor(Pi, eps) - np.einsum("icd,id->ic", Rm, eps)).max() <= 1e-14
        X = rng.standard_normal((50, C))
        assert np.abs(sref.hess_apply(Pi, X) - np.einsum("icd,id->ic", Hm, X)).max() <= 1e-14
        assert np.abs(Hm.sum(2)).max() <= 1e-15                    # H_i 1 = 0


def test_reduced_solve_and_covariance_match_the_naive_dense_system():
    rng = np.random.default_rng(11)
    n, C = 40, 3
    M = rng.standard_normal((n, n))
    Q = M @ M.T + n * np.eye(n)
    obs = rng.random(n) < 0.3
    Pi = np.where(obs[:, None], sref.softmax(rng.standard_normal((n, C))), 0.0)
    A = sref.dense_system(Q, Pi)
    B = rng.standard_normal((n, C))
    solver = sref.Solver(Q, obs)
    want = np.linalg.solve(A, B.reshape(-1)).reshape(n, C)
    assert np.abs(solver.solve(Pi, B) - want).max() <= 1e-13 * np.abs(want).max()
    cov = np.diag(np.linalg.inv(A)).reshape(n, C)
    assert np.abs(solver.covariance_diag(Pi) - cov).max() <= 1e-13 * cov.max()


def test_two_classes_are_the_binary_fit_at_half_the_scale(precision):
    g, Q = precision
    t, obs, _ = lref.labels(g)
    F, _ = sref.newton(Q, t.astype(np.int64), obs, 2)
    f, _ = lref.newton(0.5 * Q, t, obs)
    err = np.abs((F[:, 1] - F[:, 0]) - f).max()
    print("max |F_1 - F_0 - f_binary| = %.2e, max |f| = %.2f" % (err, np.abs(f).max()))
    assert err <= 1e-12


def test_reference_site_is_finite_at_extreme_latents():
    f = np.array([[1e4, -1e4, 0.0], [-1e4, -1e4, -1e4], [1e4, 1e4, -1e4], [0.0, 0.0, 0.0]], np.float32)
    t = np.array([0, 1, 2, 1])
    pi, rhs, sums, _ = sref.site_outputs(f, None, t, None)
    assert np.isfinite(pi).all() and np.isfinite(rhs).all() and np.isfinite(sums).all()
    assert pi[0].tolist() == [1.0, 0.0, 0.0] and rhs[0].tolist() == [0.0, 0.0, 0.0]
    assert pi[2].tolist() == [0.5, 0.5, 0.0] and rhs[2].tolist() == [-0.5, -0.5, 1.0]
    lp = sref.site(f, t, None)[0]
    assert lp[0] == 0.0 and abs(lp[1] + np.log(3.0)) <= 1e-15 and abs(lp[2] + 2e4 + np.log(2.0)) <= 1e-11


# ------------------------------------------------------------------------------------------------ host-side checks
NEW = ("mgp_softmax_site_workspace_bytes", "mgp_softmax_site", "mgp_softmax_hessian_add", "mgp_softmax_cg_workspace_bytes",
       "mgp_softmax_cg")


def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(handle, name)


def _op(form=0):
    from manifold_gp_amd import _lib
    buf = (ctypes.c_float * 8)()
    idx = (ctypes.c_int32 * 8)(0, 4, 4, 4, 4, 4, 4, 4)
    op = _lib.OperatorT()
    op.L.n, op.L.rowptr, op.L.col, op.L.vals, op.L.diag = 1, ctypes.addressof(idx), ctypes.addressof(idx), ctypes.addressof(buf), ctypes.addressof(buf)
    op.nu, op.kappa, op.scale, op.noise, op.form = 2, 1.0, 1.0, 0.0, form
    return op, (buf, idx)


def test_site_entry_checks_its_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf, dbl, lab = (ctypes.c_float * 256)(), (ctypes.c_double * 8)(), (ctypes.c_int32 * 8)()
    u, d, t = ctypes.addressof(buf), ctypes.addressof(dbl), ctypes.addressof(lab)
    wb = lib.mgp_softmax_site_workspace_bytes
    assert wb(0, 3) == 0 and wb(4, 1) == 0 and wb(4, 65) == 0
    assert wb(1, 3) == 32 and wb(64, 3) == 32 and wb(65, 3) == 64         # 64 rows of 4 lanes per workgroup
    assert wb(4, 64) == 32 and wb(5, 64) == 64 and wb(5, 33) == 64        # 4 rows of 64 lanes
    assert wb(2 ** 40, 3) == 1024 * 32                                    # the grid cap
    site = lib.mgp_softmax_site
    ok = dict(f=u, qf=None, labels=t, obs=None, n=4, C=3, pi=u, rhs=u, sums=d, work=d, wb=64)

    def call(**kw):
        a = dict(ok, **kw)
        return site(a["f"], a["qf"], a["labels"], a["obs"], a["n"], a["C"], a["pi"], a["rhs"], a["sums"], a["work"], a["wb"], None)
    for name in ("f", "labels", "pi", "rhs", "sums"):
        assert call(**{name: None}) == -1, name
    assert call(n=0) == -1 and call(C=1) == -1 and call(C=65) == -1
    assert call(work=None) == -2 and call(wb=31) == -2 and call(work=d + 4) == -2


def test_solver_entries_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    op, keep = _op()
    ref = ctypes.byref(op)
    buf = (ctypes.c_float * 4096)()
    u = (ctypes.addressof(buf) + 15) // 16 * 16
    wb = lib.mgp_softmax_cg_workspace_bytes
    need = wb(ref, 3)
    assert need >= 4 * 3 * 4 + lib.mgp_operator_workspace_bytes(ref, 3)
    assert wb(None, 3) == 0 and wb(ref, 1) == 0 and wb(ref, 65) == 0
    cg = lib.mgp_softmax_cg
    ok = dict(op=ref, pi=u, C=3, B=u, X=u + 64, tol=1e-3, max_iter=10, check=8, work=u + 128, wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return cg(a["op"], a["pi"], a["C"], a["B"], a["X"], a["tol"], a["max_iter"], a["check"], None, None, None, a["work"],
                  a["wb"], None)
    for name in ("op", "pi", "B", "X"):
        assert call(**{name: None}) == -1, name
    assert call(X=u) == -1 and call(C=1) == -1 and call(C=65) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(max_iter=0) == -1 and call(check=-1) == -1
    assert call(work=None) == -2 and call(wb=need - 1) == -2 and call(work=u + 132) == -2
    for form in (1, 2, 3):
        bad, keep2 = _op(form)
        bad.obs_w = u
        assert wb(ctypes.byref(bad), 3) == 0
        assert call(op=ctypes.byref(bad)) == -3, form
    op.nu = 0
    assert wb(ref, 3) == 0 and call() == -1                               # an invalid operator
    hess = lib.mgp_softmax_hessian_add
    assert hess(None, u, 4, 3, u + 64, None) == -1 and hess(u, None, 4, 3, u + 64, None) == -1
    assert hess(u, u, 4, 3, None, None) == -1 and hess(u, u + 64, 4, 3, u + 64, None) == -1
    assert hess(u, u, 0, 3, u + 64, None) == -1 and hess(u, u, 4, 1, u + 64, None) == -1 and hess(u, u, 4, 65, u + 64, None) == -1


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_fit_argument_checks():
    from manifold_gp_amd.classification import laplace_fit_multiclass
    d = _fake_desc()
    y = torch.tensor([0, 2, 1])
    some = torch.tensor([True, False, True])
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(d, torch.tensor([0, 3, 1]), 3)
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(d, torch.tensor([0, -1, 1]), 3)
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(d, torch.tensor([0.0, 0.5, 1.0]), 3)
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(d, torch.tensor([float("nan"), 1.0, 1.0]), 3, observed=some)      # NaN at an observed node
    for bad in (1, 65, 3.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            laplace_fit_multiclass(d, y, bad)
    with pytest.raises(ValueError, match="no node"):
        laplace_fit_multiclass(d, y, 3, observed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        laplace_fit_multiclass(d, y, 3, observed=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        laplace_fit_multiclass(d, y, 3, observed=torch.ones(3))
    with pytest.raises(ValueError):
        laplace_fit_multiclass(d, torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError):
        laplace_fit_multiclass(d, torch.zeros(3, 1), 3)
    with pytest.raises(ValueError, match="f0"):
        laplace_fit_multiclass(d, y, 3, f0=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="f0"):
        laplace_fit_multiclass(d, y, 3, f0=torch.zeros(3))
    with pytest.raises(NotImplementedError):
        laplace_fit_multiclass(_fake_desc(form=2), y, 3)
    for good in (y, torch.tensor([0.0, float("nan"), 2.0])):                                     # valid arguments, host tensors
        with pytest.raises(RuntimeError, match="no CPU path"):
            laplace_fit_multiclass(d, good, 3, observed=some)


def test_labels_of_every_dtype_reach_the_kernel_unchanged():
    """The observed labels come out of the validation as the same int32 values whatever dtype they came in (uint8 is the
    usual one for digit labels: a clamp on the unwidened tensor would wrap its lower bound and destroy them); entries that are
    not observed may hold anything and leave as values no class index equals."""
    from manifold_gp_amd.classification import _validate_multiclass
    d = _fake_desc()
    want = torch.tensor([0, 2, 1], dtype=torch.int32)
    for dt in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.float32, torch.float64):
        got, obs = _validate_multiclass(d, torch.tensor([0, 2, 1], dtype=dt), 3, None, None)
        assert got.dtype == torch.int32 and torch.equal(got, want) and obs is None, dt
    some = torch.tensor([True, False, True])
    for junk, dt in ((200, torch.uint8), (-100, torch.int8), (2 ** 40, torch.int64), (-2 ** 40, torch.int64),
                     (float("nan"), torch.float32), (float("inf"), torch.float64), (-1e30, torch.float32)):
        got, _ = _validate_multiclass(d, torch.tensor([2, junk, 0], dtype=dt), 3, some, None)
        assert got.dtype == torch.int32 and got[0] == 2 and got[2] == 0, (junk, dt)
        assert not 0 <= int(got[1]) < 64, (junk, dt, got)
    with pytest.raises(ValueError, match="integers in"):
        _validate_multiclass(d, torch.tensor([0, 200, 1], dtype=torch.uint8), 3, None, None)
    with pytest.raises(ValueError):
        _validate_multiclass(d, torch.tensor([False, True, True]), 3, None, None)


def test_kernel_wrappers_check_their_arguments_on_host_tensors():
    from manifold_gp_amd.classification import softmax_cg_solve, softmax_hessian_add, softmax_noise_factor, softmax_site
    f = torch.zeros(3, 3)
    lab = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        softmax_site(torch.zeros(3), None, lab)
    with pytest.raises(ValueError, match="num_classes"):
        softmax_site(torch.zeros(3, 1), None, lab)
    with pytest.raises(ValueError, match="num_classes"):
        softmax_site(torch.zeros(3, 65), None, lab)
    with pytest.raises(ValueError, match="qf"):
        softmax_site(f, torch.zeros(3, 2), lab)
    with pytest.raises(ValueError, match="labels"):
        softmax_site(f, None, lab.long())
    with pytest.raises(ValueError, match="labels"):
        softmax_site(f, None, lab[:2])
    with pytest.raises(ValueError, match="observed"):
        softmax_site(f, None, lab, torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        softmax_site(f, None, lab)
    with pytest.raises(ValueError):
        softmax_hessian_add(f, f, torch.zeros(3, 2))
    with pytest.raises(ValueError):
        softmax_hessian_add(f, f.double(), f.clone())
    with pytest.raises(RuntimeError, match="no CPU path"):
        softmax_hessian_add(f, f.clone(), f.clone())
    d = _fake_desc()
    with pytest.raises(NotImplementedError):
        softmax_cg_solve(_fake_desc(form=2), f, f)
    with pytest.raises(ValueError):
        softmax_cg_solve(d, torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="rhs"):
        softmax_cg_solve(d, f, torch.zeros(3, 2))
    with pytest.raises(ValueError, match="max_iter"):
        softmax_cg_solve(d, f, f, max_iter=0)
    with pytest.raises(ValueError, match="check_every"):
        softmax_cg_solve(d, f, f, check_every=0)
    with pytest.raises(ValueError, match="tol"):
        softmax_cg_solve(d, f, f, tol=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        softmax_cg_solve(d, f, f)
    # the factor is plain tensor algebra: checked here against the restatement, in float64
    rng = np.random.default_rng(2)
    Pi = sref.softmax(rng.standard_normal((20, 5)))
    Pi[::3] = 0.0
    eps = rng.standard_normal((20, 5))
    got = softmax_noise_factor(torch.from_numpy(Pi), torch.from_numpy(eps)).numpy()
    assert np.abs(got - sref.noise_factor(Pi, eps)).max() <= 1e-15


def test_model_method_exists():
    import inspect
    from manifold_gp_amd.models import RiemannGP
    sig = inspect.signature(RiemannGP.laplace_posterior_multiclass)
    assert list(sig.parameters) == ["self", "num_classes", "observed", "kw"]
