"""C-class Laplace classification on the MI355X (csrc/laplace.hip: mgp_softmax_site; csrc/softmax_cg.hip; the multiclass part of
manifold_gp_amd/classification.py): the site kernel and the Hessian epilogue against their float64 restatement on the same
float32 inputs, the coupled CG against the float64 matrix of the device's own CSR (_observed_ref.device_q2), the Newton fit
against a dense float64 Newton iteration on that matrix, the posterior pieces rebuilt from their public parts, and the model
method (tests/_softmax_ref.py)."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import _observed_ref as oref
import _softmax_ref as sref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

RTOL = 1e-5
U32 = 2.0 ** -24
SIZES = [1, 63, 64, 65, 257, 1546]
CLASSES = [2, 3, 10, 16, 33, 64]
# the kernels' own grid caps (csrc/laplace.hip, csrc/softmax_cg.hip): workgroups x rows per workgroup at 4 lanes per row (C = 3)
SITE_SWEEP = 1024 * 64
HESS_SWEEP = 1024 * 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mgp():
    import manifold_gp_amd
    from manifold_gp_amd import _lib
    _lib.lib()
    return manifold_gp_amd


def _ulps(got, want):
    """|got - want| in units of the float32 spacing at want"""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1: the site kernel
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])


def _site_inputs(n, C, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, C)) * 2.0
    pick = rng.random((n, C)) < 0.3
    f = np.where(pick, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), (n, C)), f).astype(np.float32)
    qf = rng.standard_normal((n, C)).astype(np.float32)
    t = rng.integers(0, C, n).astype(np.int32)
    obs = rng.random(n) < 0.1
    if n < 20:
        obs[0] = True
    return f, qf, t, obs


def _check_site(dev, f, qf, t, obs, label):
    from manifold_gp_amd.classification import softmax_site
    t_in = t if obs is None else np.where(obs, t, -7).astype(np.int32)        # labels of unobserved nodes are never read
    args = (T(f, dev), None if qf is None else T(qf, dev), T(t_in, dev), None if obs is None else T(obs, dev))
    pi, rhs, sums = softmax_site(*args)
    want_pi, want_rhs, want_sums, scale = sref.site_outputs(f, qf, t, obs)
    gp, gr, gs = pi.cpu().numpy(), rhs.cpu().numpy(), sums.cpu().numpy()
    assert pi.dtype == torch.float32 and rhs.dtype == torch.float32 and sums.dtype == torch.float64
    assert pi.shape == f.shape and rhs.shape == f.shape
    assert np.isfinite(gp).all() and np.isfinite(gr).all() and np.isfinite(gs).all()
    up, ur = _ulps(gp, want_pi).max(), _ulps(gr, want_rhs).max()
    err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("%s: pi %.2f ulp, rhs %.2f ulp, sums %.1e %.1e %.1e %.1e" % (label, up, ur, *err))
    assert up <= 1.0 and ur <= 1.0, (label, up, ur)
    if obs is not None:
        q = np.zeros_like(f) if qf is None else qf
        assert (gp[~obs] == 0).all()
        assert np.array_equal(gr[~obs], -q[~obs])
    assert err[0] <= 1e-12 and err[1] <= 1e-12 and err[3] <= 1e-12, (label, err)
    assert err[2] <= 1e-14, (label, err)
    pi2, rhs2, sums2 = softmax_site(*args)
    assert torch.equal(pi, pi2) and torch.equal(rhs, rhs2) and torch.equal(sums, sums2)      # bitwise: no atomics
    assert pi2.data_ptr() != pi.data_ptr()                                                    # fresh tensors per call


@pytest.mark.parametrize("n, Cs", [(n, CLASSES) for n in SIZES] + [(SITE_SWEEP + 3 * 64 + 5, [3])])
def test_site_kernel_matches_float64(mgp, dev, n, Cs):
    """pi and rhs within 1 float32 ulp of the rounded float64 reference (both sides compute in float64), exactly 0 / -qf at
    unobserved rows, the sums within 1e-12 of the sum of their absolute terms, the max within 1e-14; everything finite at |f|
    up to 1e4; a second call bitwise equal.  The last n runs the grid-stride loop past the grid cap."""
    for C in Cs:
        f, qf, t, obs = _site_inputs(n, C, 100 * n + C)
        _check_site(dev, f, qf, t, obs, "n = %d, C = %d, 10 %% observed" % (n, C))
        _check_site(dev, f, qf, t, None, "n = %d, C = %d, every node" % (n, C))
        _check_site(dev, f, None, t, obs, "n = %d, C = %d, qf NULL" % (n, C))


def test_site_kernel_extreme_latents_and_unaligned_arrays(mgp, dev):
    from manifold_gp_amd.classification import softmax_site
    f = np.array([[1e4, -1e4, 0.0], [-1e4, -1e4, -1e4], [1e4, 1e4, -1e4], [0.0, 0.0, 0.0]], np.float32)
    t = np.array([0, 1, 2, 1], np.int32)
    pi, rhs, sums = softmax_site(T(f, dev), None, T(t, dev))
    assert pi.cpu().tolist() == [[1.0, 0.0, 0.0], [np.float32(1 / 3)] * 3, [0.5, 0.5, 0.0], [np.float32(1 / 3)] * 3]
    assert rhs[0].cpu().tolist() == [0.0, 0.0, 0.0] and rhs[2].cpu().tolist() == [-0.5, -0.5, 1.0]
    assert abs(float(sums[0]) - (-2e4 - np.log(2.0) - 2.0 * np.log(3.0))) <= 1e-11 and float(sums[2]) == 1.0
    # blocks one float off a 16-byte boundary (views into larger buffers): the same numbers
    n, C = 257, 3
    f, qf, t, obs = _site_inputs(n, C, 5)
    pad = lambda a: T(np.concatenate([a.reshape(-1)[:1], a.reshape(-1)]), dev)[1:].view(a.shape)
    fa, qa, ta, oa = pad(f), pad(qf), pad(t), pad(obs)
    assert fa.data_ptr() % 16 == 4 and qa.data_ptr() % 16 == 4 and oa.data_ptr() % 4 == 1 and fa.is_contiguous()
    got = softmax_site(fa, qa, ta, oa)
    want = softmax_site(T(f, dev), T(qf, dev), T(t, dev), T(obs, dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_site_kernel_only_compares_labels(mgp, dev):
    """Labels outside [0, C) at OBSERVED rows (the Python fit refuses them; the C entry documents what it does): the label is
    compared with the class index, never used as an address, so such a row has G = -pi, no log p term, and its neighbours are
    untouched."""
    from manifold_gp_amd.classification import softmax_site
    for C in (3, 64):
        n = 257
        f, qf, t, _ = _site_inputs(n, C, 77 + C)
        bad = np.zeros(n, bool)
        bad[[0, 5, 64, 255, 256]] = True
        t_in = t.copy()
        t_in[bad] = np.array([-1, C, 2 ** 31 - 1, -2 ** 31, 64], np.int32)
        pi, rhs, sums = softmax_site(T(f, dev), T(qf, dev), T(t_in, dev))
        good = softmax_site(T(f, dev), T(qf, dev), T(t, dev))
        assert torch.equal(pi, good[0]) and torch.equal(rhs[T(~bad, dev)], good[1][T(~bad, dev)])
        gp, gr = pi.cpu().numpy(), rhs.cpu().numpy()
        assert np.isfinite(gp).all() and np.isfinite(gr).all()
        minus = (-sref.site(f, t, None)[2][bad] - qf[bad].astype(np.float64)).astype(np.float32)
        assert _ulps(gr[bad], minus).max() <= 1.0
        lp = sref.site(f, t, None)[0]
        assert abs(float(sums[0]) - lp[~bad].sum()) <= 1e-12 * np.abs(lp).sum()


def test_site_kernel_argument_errors(mgp, dev):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n, C = 64, 3
    f = torch.zeros(n, C, device=dev)
    lab = torch.zeros(n, dtype=torch.int32, device=dev)
    pi, rhs = torch.full((n, C), 7.0, device=dev), torch.full((n, C), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    work = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(f_=f, lab_=lab, pi_=pi, rhs_=rhs, sums_=sums, n_=n, C_=C, work_=work, wb=64):
        return lib.mgp_softmax_site(p(f_), None, p(lab_), None, n_, C_, p(pi_), p(rhs_), p(sums_), p(work_), wb, st)
    assert call(f_=None) == -1 and call(lab_=None) == -1 and call(pi_=None) == -1 and call(rhs_=None) == -1
    assert call(sums_=None) == -1 and call(n_=0) == -1 and call(C_=1) == -1 and call(C_=65) == -1
    assert call(work_=None) == -2 and call(wb=8) == -2
    torch.cuda.synchronize()
    assert bool((pi == 7.0).all()) and bool((rhs == 7.0).all()) and not sums.any()        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((pi == np.float32(1 / 3)).all())


# ------------------------------------------------------------------------------------------------ 2: the Hessian epilogue
@pytest.mark.parametrize("n, Cs", [(n, CLASSES) for n in SIZES] + [(HESS_SWEEP + 3 * 64 + 5, [3])])
def test_hessian_epilogue_matches_float64(mgp, dev, n, Cs):
    """Y + H(pi) X against float64 on the same float32 inputs.  The kernel forms  fl(y + fl(fl(p x) - fl(p d))),  d the xor-tree
    sum of the fl(p_k x_k) over the TC lanes of the row (depth L = log2 TC).  With S = sum_k |p_k x_k| >= |d| and u = 2^-24:
    |d - exact| <= (L + 1) u S, so to first order the error is at most  u (|result| + 2 |p x| + 2 p S + (L + 1) p S);  the bound
    takes that with the second-order terms covered by a factor 1 + 1e-3.  A row of zeros in pi leaves its row of Y untouched."""
    from manifold_gp_amd.classification import softmax_hessian_add
    for C in Cs:
        rng = np.random.default_rng(1000 * n + C)
        pi = sref.softmax(rng.standard_normal((n, C)) * 3.0).astype(np.float32)
        zero = rng.random(n) < 0.5
        pi[zero] = 0.0
        x = (rng.standard_normal((n, C)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
        y = rng.standard_normal((n, C)).astype(np.float32)
        yd = T(y, dev)
        out = softmax_hessian_add(T(pi, dev), T(x, dev), yd)
        assert out.data_ptr() == yd.data_ptr()
        got = out.cpu().numpy()
        p64, x64 = pi.astype(np.float64), x.astype(np.float64)
        want = y.astype(np.float64) + sref.hess_apply(p64, x64)
        S = np.abs(p64 * x64).sum(1, keepdims=True)
        L = math.log2(max(2, 1 << (C - 1).bit_length()))
        bound = (1.0 + 1e-3) * U32 * (np.abs(want) + 2.0 * np.abs(p64 * x64) + (L + 3.0) * p64 * S)
        worst = (np.abs(got - want) / bound).max()
        print("n = %d, C = %d: worst error %.2f of the bound" % (n, C, worst))
        assert worst <= 1.0, (n, C, worst)
        assert np.array_equal(got[zero], y[zero])


# ------------------------------------------------------------------------------------------------ 3: the coupled CG
_SCALED = {}


def _scaled(mgp, golden, dev, case, norm, nu):
    """(descriptor, dense float64 matrix the kernels apply) per (fixture, normalisation, nu), built once: scaled to a prior
    marginal variance of about 9 as test_gpu_laplace._problem does, so that H (entries up to 1/4) matters beside Q2."""
    key = (case, norm, nu)
    if key not in _SCALED:
        d1 = _desc(mgp, golden(case), dev, norm, nu, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        _SCALED[key] = (d1.with_(scale=scale), scale * Q1)
    return _SCALED[key]


def _system(n, C, seed):
    rng = np.random.default_rng(seed)
    pi = np.where((rng.random(n) < 0.1)[:, None], sref.softmax(rng.standard_normal((n, C)) * 2.0), 0.0).astype(np.float32)
    B = rng.standard_normal((n, C)).astype(np.float32)
    return pi, B


def _true_residual(Q, pi, B, X):
    X = X.double().cpu().numpy()
    r = B.astype(np.float64) - (Q @ X + sref.hess_apply(pi.astype(np.float64), X))
    return np.linalg.norm(r) / np.linalg.norm(B.astype(np.float64))


SOLVES = [(c, nu, 1e-3) for c in ("dumbbell_k10_loop", "dumbbell_k50_noloop") for nu in (1, 2, 3)] + \
         [("dumbbell_k50_noloop", nu, 1e-5) for nu in (1, 2, 3)] + [("dumbbell_k10_loop", 1, 1e-5)]


@pytest.mark.parametrize("case, nu, tol", SOLVES)
def test_coupled_cg_against_the_float64_matrix(mgp, golden, dev, case, nu, tol):
    """C = 3, random softmax rows at 10 % of the nodes, a random right-hand side: status 1 (no warning), the reported residual
    <= tol, the float64 true relative residual on the matrix the kernels apply <= 2 tol (the library's factor for float32
    residuals).  k10_loop at nu = 2, 3 and tol = 1e-5 is left out: a float32 CPU simulation of the recurrence drifted to
    2 tol and 25 tol there."""
    from manifold_gp_amd.classification import softmax_cg_solve
    desc, Q = _scaled(mgp, golden, dev, case, "symmetric", nu)
    pi, B = _system(desc.n, 3, nu)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*CG .*")
        X, its, resid = softmax_cg_solve(desc, T(pi, dev), T(B, dev), tol=tol)
    true = _true_residual(Q, pi, B, X)
    print("%s nu = %d tol = %g: %d iterations, reported %.3g, true %.3g (%.2f tol)" % (case, nu, tol, its, resid, true, true / tol))
    assert X.dtype == torch.float32 and X.shape == B.shape and its >= 1
    assert resid <= tol and true <= 2.0 * tol


def test_coupled_cg_is_deterministic_and_reports_its_state(mgp, golden, dev):
    from manifold_gp_amd import _lib
    from manifold_gp_amd.classification import softmax_cg_solve
    desc, Q = _scaled(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    pi, B = _system(desc.n, 3, 2)
    pid, Bd = T(pi, dev), T(B, dev)
    X, its, resid = softmax_cg_solve(desc, pid, Bd, tol=1e-3)
    for every in (1, 16, 8):
        X2, its2, resid2 = softmax_cg_solve(desc, pid, Bd, tol=1e-3, check_every=every)
        assert torch.equal(X, X2) and its2 == its and resid2 == resid, every
    # the random-walk normalisation (pre = post = sqrt(D)) and another class count
    rw, Qrw = _scaled(mgp, golden, dev, "dumbbell_k10_loop", "randomwalk", 1)
    pi10, B10 = _system(rw.n, 10, 4)
    X10, _, r10 = softmax_cg_solve(rw, T(pi10, dev), T(B10, dev), tol=1e-3)
    assert r10 <= 1e-3 and _true_residual(Qrw, pi10, B10, X10) <= 2e-3
    # max_iter reached: status 2, a warning, max_iter updates made
    with pytest.warns(UserWarning, match="did not converge in 5 iterations"):
        X5, its5, resid5 = softmax_cg_solve(desc, pid, Bd, tol=1e-6, max_iter=5)
    assert its5 == 5 and resid5 > 1e-6 and bool(torch.isfinite(X5).all())
    # B = 0: X = 0, converged without an update
    X0, its0, resid0 = softmax_cg_solve(desc, pid, torch.zeros_like(Bd))
    assert not X0.any() and its0 == 0 and resid0 == 0.0
    # forms 1-3 are refused, by the library and by the wrapper, before any launch
    X7 = torch.full_like(Bd, 7.0)
    work = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    for form in (1, 2, 3):
        bad = desc.with_(form=form, noise=0.1, obs_w=torch.ones(desc.n, device=dev))
        op = bad.struct()
        assert _lib.lib().mgp_softmax_cg_workspace_bytes(ctypes.byref(op), 3) == 0
        assert _lib.lib().mgp_softmax_cg(ctypes.byref(op), _lib.ptr(pid), 3, _lib.ptr(Bd), _lib.ptr(X7), 1e-3, 10, 8, None, None,
                                         None, _lib.ptr(work), work.numel(), _lib.stream()) == -3
        with pytest.raises(NotImplementedError):
            softmax_cg_solve(bad, pid, Bd)
    torch.cuda.synchronize()
    assert bool((X7 == 7.0).all())


# ------------------------------------------------------------------------------------------------ 4: the fit
_PROBLEMS = {}
C3 = 3


def _problem(mgp, golden, dev, case, norm, nu, C=C3):
    """One classification problem per (fixture, normalisation, nu, C), built once: the scaled descriptor, the dense float64
    matrix the kernels apply, the labels and the float64 Newton iteration from F = 0."""
    key = (case, norm, nu, C)
    if key not in _PROBLEMS:
        desc, Q = _scaled(mgp, golden, dev, case, norm, nu)
        t, obs, y = sref.labels(golden(case), C)
        solver = sref.Solver(Q, obs)
        f_ref, trace = sref.newton(Q, t, obs, C, solver=solver)
        _PROBLEMS[key] = dict(desc=desc, Q=Q, t=t, obs=obs, y=T(y, dev), observed=T(obs, dev), f_ref=f_ref, trace=trace,
                              solver=solver, C=C)
    return _PROBLEMS[key]


def _psi_slack(a, b):
    """the fit's own slack: 16 * 2^-24 on |psi| at the larger of the two points"""
    return 16.0 * 2.0 ** -24 * max(abs(a), abs(b))


def _check_mode(p, fit, label):
    f = fit.mean.double().cpu().numpy()
    res = np.abs(sref.gradient(p["Q"], f, p["t"], p["obs"])).max()
    g0 = np.abs(sref.gradient(p["Q"], np.zeros_like(f), p["t"], p["obs"])).max()
    err = np.abs(f - p["f_ref"]).max()
    print("%s: %d steps (float64: %d to rtol), max |G - Q F| = %.2e (bound %.2e), max |F - F_ref| = %.2e, max |F| = %.2f, "
          "max |row sum| = %.1e, CG iterations %s" % (label, fit.iterations, sref.steps_to(p["trace"], RTOL), res, 2 * RTOL * g0,
                                                      err, np.abs(f).max(), np.abs(f.sum(1)).max(), [h[3] for h in fit.history]))
    assert res <= 2 * RTOL * g0, (label, res)
    assert err <= 1e-4, (label, err)
    psis = [h[0] for h in fit.history]
    assert all(b >= a - _psi_slack(a, b) for a, b in zip(psis, psis[1:])), psis
    return err


FITS = [("dumbbell_k10_loop", "symmetric", 2), ("dumbbell_k50_noloop", "symmetric", 2), ("dumbbell_k10_loop", "randomwalk", 1),
        ("dumbbell_k50_noloop", "randomwalk", 3)]


@pytest.mark.parametrize("case, norm, nu", FITS)
def test_fit_matches_dense_float64_newton(mgp, golden, dev, case, norm, nu):
    """(a) the mode is stationary in float64 on the matrix the kernels apply: max |G - Q F| <= 2 rtol max |G(0)|;
    (b) max |F_hat - F_ref| <= 1e-4, the project's standing posterior bar (the float64 iteration with the same CG tolerance
    measured 1.7e-7 and 6.7e-7 on the CPU; measured on the MI355X: 8.2e-6 at k10_loop random walk nu = 1, <= 6.0e-7 in the other
    three cases; the values are printed); (c) psi never decreases beyond the slack and every
    step from F = 0 is a full one; (d) at most two steps more than float64 Newton; (e) log_likelihood within 1e-12."""
    from manifold_gp_amd.classification import MulticlassLaplaceFit, laplace_fit_multiclass
    p = _problem(mgp, golden, dev, case, norm, nu)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        fit = laplace_fit_multiclass(p["desc"], p["y"], C3, p["observed"], rtol=RTOL)
    assert isinstance(fit, MulticlassLaplaceFit) and fit.converged
    assert fit.mean.dtype == torch.float32 and fit.mean.shape == (p["desc"].n, C3) and fit.num_classes == C3
    _check_mode(p, fit, "%s %s nu = %d" % (case, norm, nu))
    assert len(fit.history) == fit.iterations
    assert all(h[2] == 1.0 for h in fit.history), fit.history
    assert fit.history[-1][1] <= RTOL
    assert fit.iterations <= sref.steps_to(p["trace"], RTOL) + 2
    lp = sref.site(fit.mean.double().cpu().numpy(), p["t"], p["obs"])[0].sum()
    assert abs(fit.log_likelihood - lp) <= 1e-12 * abs(lp)
    assert torch.equal(fit.map_proba(), torch.softmax(fit.mean.double(), dim=-1))
    # integer labels give the same fit bit for bit
    ints = laplace_fit_multiclass(p["desc"], T(p["t"], dev), C3, p["observed"], rtol=RTOL)
    assert torch.equal(ints.mean, fit.mean) and ints.history == fit.history


def test_fit_takes_labels_of_every_dtype(mgp, golden, dev):
    """uint8 (the usual dtype of digit labels), int8, int16, int32 and float64 labels give the fit of int64 labels bit for bit,
    with a log likelihood that is not 0: the labels reach the kernel."""
    from manifold_gp_amd.classification import laplace_fit_multiclass
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2)
    want = laplace_fit_multiclass(p["desc"], T(p["t"], dev), C3, p["observed"], rtol=RTOL)
    assert want.converged and want.log_likelihood < -1.0
    for dt in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.float64):
        fit = laplace_fit_multiclass(p["desc"], T(p["t"], dev).to(dt), C3, p["observed"], rtol=RTOL)
        assert torch.equal(fit.mean, want.mean) and fit.history == want.history, dt
        assert fit.log_likelihood == want.log_likelihood and torch.equal(fit.labels, want.labels), dt
    # every node observed, uint8: no entry to clamp, the same path
    with pytest.warns(UserWarning, match="not converged in 2 Newton steps"):
        full = laplace_fit_multiclass(p["desc"], T(p["t"], dev).to(torch.uint8), C3, None, rtol=RTOL, max_newton=2)
        ref = laplace_fit_multiclass(p["desc"], T(p["t"], dev), C3, None, rtol=RTOL, max_newton=2)
    assert torch.equal(full.mean, ref.mean) and full.log_likelihood == ref.log_likelihood < -1.0


def test_two_classes_match_the_binary_fit_at_half_the_scale(mgp, golden, dev):
    """F_1 - F_0 of the C = 2 fit against laplace_fit on desc.with_(scale=scale / 2): <= 2e-4, both sides being within 1e-4 of
    float64 references that agree to 1e-14 (tests/test_softmax_cpu.py)."""
    import _laplace_ref as lref
    from manifold_gp_amd.classification import laplace_fit, laplace_fit_multiclass
    desc, _ = _scaled(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    t, obs, y = lref.labels(golden("dumbbell_k10_loop"))
    two = laplace_fit_multiclass(desc, T(y, dev), 2, T(obs, dev), rtol=RTOL)
    one = laplace_fit(desc.with_(scale=float(desc.scale) / 2.0), T(y, dev), T(obs, dev), rtol=RTOL)
    err = float((two.mean[:, 1].double() - two.mean[:, 0].double() - one.mean.double()).abs().max())
    print("max |F_1 - F_0 - f_binary| = %.2e, max |f| = %.2f" % (err, float(one.mean.abs().max())))
    assert two.converged and one.converged and err <= 2e-4


def test_step_control_from_a_bad_start(mgp, golden, dev):
    """F0 = -20 at the true class of every observed row: every label confidently wrong.  The fit reaches the same mode, never
    decreases psi beyond the slack, and halves at least once if the float64 iteration does."""
    from manifold_gp_amd.classification import laplace_fit_multiclass
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    n = p["desc"].n
    f0 = np.zeros((n, C3))
    f0[np.flatnonzero(p["obs"]), p["t"][p["obs"]]] = -20.0
    f64, trace = sref.newton(p["Q"], p["t"], p["obs"], C3, f0=f0, solver=p["solver"])
    print("float64: %d steps, steps %s" % (len(trace), [s for _, _, s in trace]))
    assert np.abs(f64 - p["f_ref"]).max() <= 1e-9
    fit = laplace_fit_multiclass(p["desc"], p["y"], C3, p["observed"], rtol=RTOL, f0=T(f0.astype(np.float32), dev))
    print("fit: steps %s" % [h[2] for h in fit.history])
    assert fit.converged
    _check_mode(p, fit, "from -20 at the true class")
    if any(s < 1.0 for _, _, s in trace):
        assert any(h[2] < 1.0 for h in fit.history)


# ------------------------------------------------------------------------------------------------ 5: the posterior pieces
def test_posterior_pieces_from_their_public_parts(mgp, golden, dev):
    from manifold_gp_amd import sampling
    from manifold_gp_amd.classification import laplace_fit_multiclass, softmax_cg_solve, softmax_noise_factor, softmax_site
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2)
    desc = p["desc"]
    fit = laplace_fit_multiclass(desc, p["y"], C3, p["observed"], rtol=RTOL)
    lab = T(np.where(p["obs"], p["t"], -1).astype(np.int32), dev)
    assert torch.equal(fit.pi, softmax_site(fit.mean, None, lab, p["observed"])[0])
    pi64 = fit.pi.double().cpu().numpy()
    # the factor against float64
    eps = sampling.gmrf_noise(desc.data, C3, 9, 0, tag=2)
    got = softmax_noise_factor(fit.pi, eps)
    want = sref.noise_factor(pi64, eps.double().cpu().numpy())
    assert got.dtype == torch.float32
    assert np.abs(got.cpu().numpy() - want).max() <= 8 * U32 * max(1.0, np.abs(want).max())
    # samples rebuilt from the public pieces, bit for bit; sample s depends on (seed, s) alone
    S, seed = 256, 9
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*CG .*")
        x = fit.latent_samples(S, seed=seed)
    assert x.shape == (S, desc.n, C3) and x.dtype == torch.float32
    P = sampling._check_desc(desc)
    its = []
    for s in (0, 3, 255):
        z = sampling._precision_chunk(desc, P, C3, seed, s * C3)
        e = sampling.gmrf_noise(desc.data, C3, seed, s * C3, tag=2)
        delta, k, _ = softmax_cg_solve(desc, fit.pi, z + softmax_noise_factor(fit.pi, e), tol=1e-5)
        its.append(k)
        assert torch.equal(x[s], fit.mean + delta), s
    assert torch.equal(fit.latent_samples(4, seed=seed), x[:4])
    # the samples' mean is the mode: within 5 standard errors at >= 99 % of the entries, the errors from the dense covariance
    sd = np.sqrt(p["solver"].covariance_diag(pi64) / S)
    z = np.abs(x.double().mean(0).cpu().numpy() - fit.mean.double().cpu().numpy()) / sd
    print("mean of %d samples: worst %.2f standard errors, %.4f of the entries within 5; CG iterations %s"
          % (S, z.max(), (z <= 5).mean(), its))
    assert (z <= 5.0).mean() >= 0.99
    # the spread is the dense covariance's too (a loose check that R and z carry the right scale): ratio of mean variances
    ratio = float(x.double().var(0).mean()) / (sd ** 2 * S).mean()
    assert 0.9 <= ratio <= 1.1, ratio
    prob = fit.predict_proba(32, seed=5)
    want = torch.softmax(fit.latent_samples(32, seed=5).double(), dim=-1).mean(0)     # (another summation order: 1e-12 covers it)
    assert prob.dtype == torch.float64 and prob.shape == (desc.n, C3)
    assert float((prob - want).abs().max()) <= 1e-12 and float((prob.sum(1) - 1.0).abs().max()) <= 1e-12
    assert bool((prob >= 0).all()) and bool((prob <= 1).all())
    assert torch.equal(fit.map_proba(), torch.softmax(fit.mean.double(), dim=-1))


# ------------------------------------------------------------------------------------------------ 6: model and validation
def test_model_method_and_validation(mgp, golden, dev):
    from test_gpu_laplace import _model
    from manifold_gp_amd.classification import MulticlassLaplaceFit, laplace_fit_multiclass
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    _, obs_np, y_np = sref.labels(g, C3)
    y, obs = T(y_np, dev), T(obs_np, dev)
    model = _model(mgp, g, dev, y)
    desc = model.precision(noise=False)._descriptor()
    fit = model.laplace_posterior_multiclass(C3, observed=obs, rtol=1e-4)
    want = laplace_fit_multiclass(desc, y, C3, obs, rtol=1e-4)
    assert isinstance(fit, MulticlassLaplaceFit) and fit.converged
    assert torch.equal(fit.mean, want.mean) and fit.history == want.history and fit.iterations == want.iterations
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(desc, y, C3, None)                             # NaN labels with every node observed
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(desc, torch.where(obs, y + 1.0, y), C3, obs)   # a label == C
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(desc, torch.where(obs, y + 0.5, y), C3, obs)
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_multiclass(desc, y, 2, obs)
    for bad in (1, 65):
        with pytest.raises(ValueError, match="num_classes"):
            laplace_fit_multiclass(desc, y, bad, obs)
    with pytest.raises(ValueError, match="no node"):
        laplace_fit_multiclass(desc, y, C3, torch.zeros(n, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        laplace_fit_multiclass(desc, y[:-1], C3, obs)
    with pytest.raises(ValueError):
        laplace_fit_multiclass(desc, y, C3, obs[:-1])
    with pytest.raises(ValueError, match="f0"):
        laplace_fit_multiclass(desc, y, C3, obs, f0=torch.zeros(n, 2, device=dev))
    semi = _model(mgp, g, dev, y, labeled=T(np.arange(n) < 100, dev))
    with pytest.raises(NotImplementedError):
        semi.laplace_posterior_multiclass(C3, observed=obs)
