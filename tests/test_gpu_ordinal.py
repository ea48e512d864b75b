"""Ordered-category fits on the MI355X (mgp_ordinal_site and mgp_ordinal_predict in csrc/laplace.hip, manifold_gp_amd/ordinal.py):
the site kernel against its float64 restatement on the same float32 inputs, the predict kernel against the restatement of its
rule, the Newton fit against a dense float64 Newton iteration on the matrix the kernels apply (_observed_ref.device_q2), two
categories against the Bernoulli fit, the step control from a bad start, the predictive pieces against the dense Laplace
covariance and the model method (tests/_ordinal_ref.py)."""
import warnings

import numpy as np
import pytest
import torch

import _laplace_ref as lref
import _observed_ref as obref
import _ordinal_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

S_REF = 2.0
RTOL = 1e-5
SITE_GRID_CAP, SITE_PER_STEP = 1024, 256 * 4            # the kernel's grid cap (csrc/laplace.hip): workgroups x nodes per step
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1025, 1546, SITE_GRID_CAP * SITE_PER_STEP + 3 * SITE_PER_STEP + 5]
CATEGORIES = [2, 3, 7, 64]
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])
INF = np.inf


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


def _cuts(K):
    """K - 1 cutpoints over [-3, 3.5] (not symmetric about 0: g does not vanish at f = 0), float32 values"""
    return (np.array([0.25]) if K == 2 else np.linspace(-3.0, 3.5, K - 1)).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1: the site kernel
def _site_inputs(n, K, seed):
    """f: half standard normal x 2, half the special values up to +-1e4; labels uniform over the K categories; 70 % observed"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(n) * 2.0
    f = np.where(rng.random(n) < 0.5, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), n), f).astype(np.float32)
    qf = rng.standard_normal(n).astype(np.float32)
    lo, hi = oref.intervals(rng.integers(0, K, n), _cuts(K))
    obs = rng.random(n) < 0.7
    obs[0] = True
    return f, qf, lo, hi, obs


def _ulps(got, want):
    """|got - want| in units of the float32 spacing at want"""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _nan_outside(a, obs):
    return a if obs is None else np.where(obs, a, np.float32(np.nan)).astype(np.float32)


def _check_site(dev, f, qf, lo, hi, obs, label, pad=False):
    from manifold_gp_amd.ordinal import ordinal_site
    up = (lambda a: T(np.concatenate([a[:1], a]), dev)[1:]) if pad else (lambda a: T(a, dev))
    # NaN in lo and hi wherever the node is unobserved: never read
    args = (up(f), None if qf is None else up(qf), up(_nan_outside(lo, obs)), up(_nan_outside(hi, obs)), None if obs is None else up(obs))
    if pad:
        assert args[0].data_ptr() % 16 == 4 and args[2].data_ptr() % 16 == 4 and (obs is None or args[4].data_ptr() % 4 == 1)
    w, rhs, sums = ordinal_site(*args, s_ref=S_REF)
    want_w, want_rhs, want_sums, scale = oref.site_outputs(f, qf, lo, hi, obs, S_REF)
    gw, gr, gs = w.cpu().numpy(), rhs.cpu().numpy(), sums.cpu().numpy()
    assert w.dtype == torch.float32 and rhs.dtype == torch.float32 and sums.dtype == torch.float64
    assert np.isfinite(gw).all() and np.isfinite(gr).all() and np.isfinite(gs).all()
    uw, ur = _ulps(gw, want_w).max(), _ulps(gr, want_rhs).max()
    err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("%s: w %.2f ulp, rhs %.2f ulp, sums %.1e %.1e %.1e %.1e" % (label, uw, ur, *err))
    assert uw <= 1.0 and ur <= 1.0, (label, uw, ur)
    assert (gw >= 0).all() and (gw <= 1.0).all()                                             # s_ref h <= 1
    if obs is not None:
        q = np.zeros_like(f) if qf is None else qf
        assert (gw[~obs] == 0).all()
        assert np.array_equal(gr[~obs], (-np.float32(S_REF) * q[~obs]).astype(np.float32))
    assert err[0] <= 1e-12 and err[1] <= 1e-12 and err[3] <= 1e-12, (label, err)
    assert err[2] <= 1e-14, (label, err)
    w2, rhs2, sums2 = ordinal_site(*args, s_ref=S_REF)
    assert torch.equal(w, w2) and torch.equal(rhs, rhs2) and torch.equal(sums, sums2)       # bitwise: no atomics
    assert w2.data_ptr() != w.data_ptr()                                                     # fresh tensors per call
    return w, rhs, sums


@pytest.mark.parametrize("K", CATEGORIES)
@pytest.mark.parametrize("n", SIZES)
def test_site_kernel_matches_float64(dev, mgp, n, K):
    """w and rhs within 1 float32 ulp of the rounded float64 reference (both sides compute in float64), exactly 0 / -s_ref qf at
    unobserved nodes (lo and hi are NaN there), the sums within 1e-12 of the sum of their absolute terms, the max within 1e-14;
    everything finite at |f| up to 1e4; a second call bitwise equal.  The last n runs the grid-stride loop past the grid cap.
    Measured on the MI355X: w and rhs 0 ulp in every case, the sums within 5.1e-16, the max within 1.4e-16."""
    f, qf, lo, hi, obs = _site_inputs(n, K, 1000 * K + n % 997)
    _check_site(dev, f, qf, lo, hi, obs, "n = %d, K = %d, 70 %% observed" % (n, K))
    if K == 3 or n <= 1546:
        _check_site(dev, f, qf, lo, hi, None, "n = %d, K = %d, every node" % (n, K))
        _check_site(dev, f, None, lo, hi, obs, "n = %d, K = %d, qf NULL" % (n, K))


EXTREME_F = [1e4, -1e4, 745.0, -700.0, 0.0, 5.0]
EXTREME_INTERVALS = [(-INF, 0.0), (0.0, INF), (-INF, -3.0), (2.0, INF), (0.0, 2.0 ** -20), (5.0, 5.0 + 2.0 ** -20),
                     (-12.0 - 2.0 ** -20, -12.0), (-50.0, 60.0)]


def test_site_kernel_extreme_values_and_unaligned_arrays(dev, mgp):
    """|f| = 1e4, gaps of 2^-20 and infinite ends in every combination: finite outputs within the bars of the test above.  Then
    every array one element off its alignment (views into larger buffers): the scalar path, the same bars, and w and rhs bit
    for bit those of the aligned call."""
    from manifold_gp_amd.ordinal import ordinal_site
    f = np.repeat(EXTREME_F, len(EXTREME_INTERVALS)).astype(np.float32)
    lo = np.tile([i[0] for i in EXTREME_INTERVALS], len(EXTREME_F)).astype(np.float32)
    hi = np.tile([i[1] for i in EXTREME_INTERVALS], len(EXTREME_F)).astype(np.float32)
    assert (lo < hi).all()
    qf = np.linspace(-2.0, 2.0, f.shape[0]).astype(np.float32)
    w, rhs, sums = _check_site(dev, f, qf, lo, hi, None, "extremes")
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(rhs).all()) and bool(torch.isfinite(sums).all())
    w, rhs, sums = _check_site(dev, f, None, lo, hi, None, "extremes, qf NULL")
    k = len(EXTREME_INTERVALS)
    assert rhs.cpu().tolist()[:4] == [-2.0, 0.0, -2.0, 0.0] and rhs.cpu().tolist()[k:k + 4] == [0.0, 2.0, 0.0, 2.0]   # g = -+1, 0
    assert w.cpu().tolist()[:4] == [0.0] * 4
    n = 257
    f, qf, lo, hi, obs = _site_inputs(n, 7, 5)
    got = _check_site(dev, f, qf, lo, hi, obs, "n = 257, one element off", pad=True)
    want = ordinal_site(T(f, dev), T(qf, dev), T(lo, dev), T(hi, dev), T(obs, dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert np.abs(got[2].cpu().numpy() - want[2].cpu().numpy()).max() <= 1e-12 * n


def test_site_kernel_argument_errors(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n = 64
    f = torch.zeros(n, device=dev)
    hi = torch.ones(n, device=dev)
    w, rhs = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    work = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(f_=f, lo_=f, hi_=hi, w_=w, rhs_=rhs, sums_=sums, n_=n, work_=work, wb=64):
        return lib.mgp_ordinal_site(p(f_), None, p(lo_), p(hi_), None, n_, S_REF, p(w_), p(rhs_), p(sums_), p(work_), wb, st)
    assert call(f_=None) == -1 and call(lo_=None) == -1 and call(hi_=None) == -1
    assert call(w_=None) == -1 and call(rhs_=None) == -1 and call(sums_=None) == -1 and call(n_=0) == -1
    assert call(work_=None) == -2 and call(wb=8) == -2 and call(work_=work[4:], wb=60) == -2
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and bool((rhs == 7.0).all()) and not sums.any()        # nothing was launched
    assert call() == 0


# ------------------------------------------------------------------------------------------------ 2: the predict kernel
VARIANCES = [0.0, -1.0, 1e-8, 3e-3, 0.27, 1.0, 9.0, 26.0]


def _predict_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-6.0, 6.0, n), rng.choice(VARIANCES, n)


def _log_bound(eta, var, cuts):
    return oref.DEVICE_C * 2.0 ** -53 * (1.0 + oref.reach(eta, var, cuts))[:, None]


@pytest.mark.parametrize("K", [2, 3, 5, 64])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_predict_kernel_matches_the_rule_in_numpy(dev, mgp, n, K):
    """At 9, 129 and 1025 points, eta in [-6, 6], v from {0, -1, 1e-8, .., 26}: |log p - log p_ref| <= c 2^-53 (1 + X) per node,
    X = max |b - f_j| over the cutpoints and the grid, c = 22 from the rounding of the restatement itself
    (test_ordinal_cpu.py); rows sum to 1 within 1e-13; log=True is the log of the plain output within the same bound; a
    second call is bitwise equal.  Measured on the MI355X: at most 0.10 of the bound (1.8e-15), rows within 2.2e-15, the log output
    within 0.08 of the bound."""
    from manifold_gp_amd.ordinal import ordinal_predict
    cuts = _cuts(K)
    eta, var = _predict_inputs(n, 100 * K + n)
    bound = _log_bound(eta, var, cuts)
    args = (T(eta, dev), T(var, dev), T(cuts, dev))
    for points in (9, 129, 1025):
        got = ordinal_predict(*args, points=points)
        assert got.dtype == torch.float64 and got.shape == (n, K)
        p = got.cpu().numpy()
        want = oref.trapezoid(eta, var, cuts, points)
        assert (p > 0).all() and (p <= 1).all()
        err = np.abs(np.log(p) - np.log(want))
        rows = np.abs(p.sum(1) - 1.0).max()
        logp = ordinal_predict(*args, points=points, log=True).cpu().numpy()
        lerr = np.abs(logp - np.log(p))
        print("n = %d, K = %d, %d points: log p off by %.2f of the bound (%.1e), rows sum to 1 within %.1e, log output %.2f of the "
              "bound; smallest p %.1e" % (n, K, points, (err / bound).max(), err.max(), rows, (lerr / bound).max(), p.min()))
        assert (err <= bound).all(), (points, (err / bound).max())
        assert rows <= 1e-13, (points, rows)
        assert (lerr <= bound).all(), (points, (lerr / bound).max())
        assert torch.equal(got, ordinal_predict(*args, points=points))
    assert torch.equal(ordinal_predict(*args), ordinal_predict(*args, points=129))


def test_predict_kernel_edge_values_and_argument_errors(dev, mgp):
    """var <= 2^-76, zero and negative included, is the plain probability at eta (bitwise the same for all of them); NaN in eta
    or var gives a row of NaN and leaves the other rows alone; float32 inputs are taken as float64; the entry point's checks."""
    from manifold_gp_amd import _lib
    from manifold_gp_amd.ordinal import ordinal_predict
    cuts = _cuts(5)
    eta = np.array([-3.0, 0.0, 2.5, 7.0, 1.0])
    c = T(cuts, dev)
    zero = ordinal_predict(T(eta, dev), torch.zeros(5, dtype=torch.float64, device=dev), c)
    for v in ([-1.0, -1e-30, -100.0, -0.0, 2.0 ** -76], [2.0 ** -77, 0.0, -INF, 1e-30, 2.0 ** -80]):
        assert torch.equal(zero, ordinal_predict(T(eta, dev), T(np.array(v), dev), c))
    want = oref.trapezoid(eta, np.zeros(5), cuts)
    assert (np.abs(np.log(zero.cpu().numpy()) - np.log(want)) <= _log_bound(eta, np.zeros(5), cuts)).all()
    assert float((zero.sum(1) - 1.0).abs().max()) <= 1e-15
    nan = float("nan")
    got = ordinal_predict(T(np.array([nan, 0.0, 2.5, nan, 1.0]), dev), T(np.array([1.0, nan, 1.0, 0.0, 1.0]), dev), c)
    assert torch.isnan(got).all(1).cpu().tolist() == [True, True, False, True, False]
    assert torch.isnan(got).any(1).cpu().tolist() == [True, True, False, True, False]
    both = ordinal_predict(T(eta.astype(np.float32), dev), torch.ones(5, device=dev), c.float())
    assert torch.equal(both, ordinal_predict(T(eta, dev), torch.ones(5, dtype=torch.float64, device=dev), c))
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    e, out = T(eta, dev), torch.full((5, 5), 7.0, dtype=torch.float64, device=dev)
    assert lib.mgp_ordinal_predict(None, p(e), p(c), 5, 5, 129, 0, p(out), st) == -1
    assert lib.mgp_ordinal_predict(p(e), None, p(c), 5, 5, 129, 0, p(out), st) == -1
    assert lib.mgp_ordinal_predict(p(e), p(e), None, 5, 5, 129, 0, p(out), st) == -1
    assert lib.mgp_ordinal_predict(p(e), p(e), p(c), 5, 5, 129, 0, None, st) == -1
    assert lib.mgp_ordinal_predict(p(e), p(e), p(c), 0, 5, 129, 0, p(out), st) == -1
    for K in (1, 65):
        assert lib.mgp_ordinal_predict(p(e), p(e), p(c), 5, K, 129, 0, p(out), st) == -1
    for points in (8, 7, 128, 1027):
        assert lib.mgp_ordinal_predict(p(e), p(e), p(c), 5, 5, points, 0, p(out), st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                        # nothing was launched


# ------------------------------------------------------------------------------------------------ 3-6: the fit
_PROBLEMS = {}
K_FIT = 4


def _problem(mgp, golden, dev, case, norm, nu):
    """One ordinal problem per (fixture, normalisation, nu), built once: the descriptor scaled to a prior marginal variance of
    about 9 (as test_gpu_laplace.py), the dense float64 matrix the kernels apply, the labels of _ordinal_ref.labels (K = 4, about
    half the nodes observed, NaN elsewhere), the cutpoints of their cumulative frequencies and the float64 Newton iteration."""
    key = (case, norm, nu)
    if key not in _PROBLEMS:
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = obref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        y, obs = oref.labels(g, K_FIT)
        cuts = oref.cutpoints(y, K_FIT, obs)
        lo, hi = oref.intervals(y, cuts)
        Q = scale * Q1
        f_ref, trace = oref.newton(Q, lo, hi, obs)
        _PROBLEMS[key] = dict(desc=d1.with_(scale=scale), Q=Q, labels=y, obs=obs, cuts=cuts, lo=lo, hi=hi, f_ref=f_ref, trace=trace,
                              y=T(np.where(obs, y, np.nan).astype(np.float32), dev), observed=T(obs, dev), cutpoints=T(cuts, dev))
    return _PROBLEMS[key]


def _fit(p):
    from manifold_gp_amd.ordinal import laplace_fit_ordinal
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        return laplace_fit_ordinal(p["desc"], p["y"], K_FIT, p["cutpoints"], p["observed"], rtol=RTOL)


def _fitted(p):
    if "fit" not in p:
        p["fit"] = _fit(p)
    return p["fit"]


def _check_mode(p, fit, label):
    f = fit.mean.double().cpu().numpy()
    res = np.abs(oref.gradient(p["Q"], f, p["lo"], p["hi"], p["obs"])).max()
    g0 = np.abs(oref.gradient(p["Q"], np.zeros_like(f), p["lo"], p["hi"], p["obs"])).max()
    err = np.abs(f - p["f_ref"]).max()
    print("%s: %d steps %s (float64: %d to rtol), max |g - Q f| = %.2e (relative to max |g(0)| = %.3f: %.1e), max |f - f_ref| = %.2e, "
          "max |f| = %.2f, CG iterations %s" % (label, fit.iterations, [h[2] for h in fit.history], oref.steps_to(p["trace"], RTOL), res,
                                                g0, res / g0, err, np.abs(f).max(), [h[3] for h in fit.history]))
    assert fit.converged
    assert err <= 1e-4, (label, err)
    assert fit.history[-1][1] <= RTOL
    return err


CASES = [(c, n, nu) for c in ("dumbbell_k10_loop", "dumbbell_k50_noloop") for n in ("symmetric", "randomwalk") for nu in (1, 2, 3)]


@pytest.mark.parametrize("case, norm, nu", CASES)
def test_fit_matches_dense_float64_newton(mgp, golden, dev, case, norm, nu):
    """The bars of the binary fit's test: max |f_hat - f_ref| <= 1e-4 (a float32 simulation on the CPU with exact solves gives
    1.4e-7 .. 1.5e-7), the final relative gradient <= rtol, at most two steps more than the float64 iteration takes to rtol,
    log_likelihood (with the constant sum_obs log c_k) within 1e-12 relative of the float64 value at the returned mode.
    Measured on the MI355X: 4 full steps in all 12 cases (float64: 4), max |f_hat - f_ref| 1.4e-7 .. 1.5e-7."""
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit
    p = _problem(mgp, golden, dev, case, norm, nu)
    fit = _fitted(p)
    assert isinstance(fit, OrdinalLaplaceFit) and fit.mean.dtype == torch.float32 and fit.mean.shape == (p["desc"].n,)
    _check_mode(p, fit, "%s %s nu = %d" % (case, norm, nu))
    assert len(fit.history) == fit.iterations
    assert fit.iterations <= oref.steps_to(p["trace"], RTOL) + 2
    lp = oref.log_likelihood(fit.mean.double().cpu().numpy(), p["labels"], p["cuts"], p["obs"])
    print("log-likelihood %.9f, float64 at the returned mode %.9f" % (fit.log_likelihood, lp))
    assert abs(fit.log_likelihood - lp) <= 1e-12 * abs(lp)
    assert fit.num_categories == K_FIT and fit.cutpoints.dtype == torch.float64 and fit.cutpoints.device.type == "cuda"
    assert np.array_equal(fit.cutpoints.cpu().numpy(), p["cuts"])
    want = oref.trapezoid(fit.mean.double().cpu().numpy(), np.zeros(p["desc"].n), p["cuts"])
    got = fit.map_proba().cpu().numpy()
    assert got.shape == want.shape and (np.abs(got - want) <= 8 * 2.0 ** -53 * want).all()


def test_two_categories_cut_at_zero_are_the_bernoulli_fit(mgp, golden, dev):
    """laplace_fit_ordinal with K = 2 and the cutpoint 0 against laplace_fit on the same 0/1 labels: modes within 2e-4 of each
    other, each within 1e-4 of the same dense float64 mode."""
    from manifold_gp_amd.classification import laplace_fit
    from manifold_gp_amd.ordinal import laplace_fit_ordinal
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    t, obs, y = lref.labels(golden("dumbbell_k10_loop"))
    f_ref, _ = lref.newton(p["Q"], t, obs)
    yd, od = T(y, dev), T(obs, dev)
    a = laplace_fit(p["desc"], yd, od, rtol=RTOL)
    b = laplace_fit_ordinal(p["desc"], yd, 2, torch.zeros(1, dtype=torch.float64), od, rtol=RTOL)
    fa, fb = a.mean.double().cpu().numpy(), b.mean.double().cpu().numpy()
    print("K = 2 against laplace_fit: max |difference of the modes| = %.2e; against the dense mode %.2e and %.2e; steps %d and %d"
          % (np.abs(fa - fb).max(), np.abs(fa - f_ref).max(), np.abs(fb - f_ref).max(), a.iterations, b.iterations))
    assert a.converged and b.converged
    assert np.abs(fa - fb).max() <= 2e-4
    assert np.abs(fa - f_ref).max() <= 1e-4 and np.abs(fb - f_ref).max() <= 1e-4
    assert abs(a.log_likelihood - b.log_likelihood) <= 1e-6 * abs(a.log_likelihood)


def test_step_control_from_a_bad_start(mgp, golden, dev):
    """f0 = 20 x standard normal noise: the float64 iteration halves its first steps there (the CPU simulation: 12 steps, eight
    of them halved); the fit converges to the same mode with at least one halved step."""
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    from manifold_gp_amd.ordinal import laplace_fit_ordinal
    f0 = oref.bad_start(p["desc"].n)
    fit = laplace_fit_ordinal(p["desc"], p["y"], K_FIT, p["cutpoints"], p["observed"], rtol=RTOL, f0=T(f0, dev))
    print("fit: steps %s" % [h[2] for h in fit.history])
    _check_mode(p, fit, "from 20 x noise")
    assert any(h[2] < 1.0 for h in fit.history)


def test_posterior_pieces(mgp, golden, dev):
    """With variance= the EXACT dense diagonal of (Q2 + H)^-1 at the returned mode, predict_proba is the float64 restatement of
    the rule within the predict kernel's bound: no Monte-Carlo noise enters.  predict_log_density, predict_exceedance and
    predict_category are consistent with that matrix.  latent_variance(64) lies within 5 of its own standard errors of the dense
    diagonal at >= 99 % of the nodes."""
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    fit = _fitted(p)
    n, K, cuts = p["desc"].n, K_FIT, p["cuts"]
    f = fit.mean.double().cpu().numpy()
    dense = np.diag(np.linalg.inv(p["Q"] + np.diag(oref.curvature(f, p["lo"], p["hi"], p["obs"]))))
    v = T(dense, dev)
    prob, used = fit.predict_proba(variance=v)
    assert torch.equal(used, v) and prob.dtype == torch.float64 and prob.shape == (n, K)
    got, want = prob.cpu().numpy(), oref.trapezoid(f, dense, cuts)
    err = np.abs(np.log(got) - np.log(want))
    bound = _log_bound(f, dense, cuts)
    print("predict_proba with the dense variances: log p off by %.2f of the bound (%.1e); rows sum to 1 within %.1e; variances "
          "%.3g .. %.3g" % ((err / bound).max(), err.max(), np.abs(got.sum(1) - 1).max(), dense.min(), dense.max()))
    assert (err <= bound).all() and np.abs(got.sum(1) - 1.0).max() <= 1e-13
    logp = fit.predict_proba(variance=v, log=True)[0]
    assert (np.abs(logp.cpu().numpy() - np.log(got)) <= bound).all()
    # the log density of held-out categories: the one entry per node of the log matrix, NaN outside `at`
    rng = np.random.default_rng(2)
    held = rng.integers(0, K, n)
    at = ~p["obs"]
    dens = fit.predict_log_density(T(np.where(at, held, np.nan).astype(np.float32), dev), at=T(at, dev), variance=v)
    assert dens.dtype == torch.float64 and dens.shape == (n,)
    assert torch.equal(dens[T(at, dev)], logp[torch.arange(n, device=dev), T(held, dev)][T(at, dev)])
    assert bool(torch.isnan(dens[~T(at, dev)]).all())
    assert torch.equal(fit.predict_log_density(T(held, dev), variance=v), logp[torch.arange(n, device=dev), T(held, dev)])
    with pytest.raises(ValueError, match="integers in"):
        fit.predict_log_density(T(np.full(n, K), dev), variance=v)
    # exceedance: the sum of the categories above k
    for k in range(K):
        exc = fit.predict_exceedance(k, variance=v).cpu().numpy()
        assert np.abs(exc - got[:, k + 1:].sum(1)).max() <= 1e-15
    assert not fit.predict_exceedance(K - 1, variance=v).any()
    ks = rng.integers(0, K, n)
    exc = fit.predict_exceedance(T(ks, dev), variance=v).cpu().numpy()
    assert np.abs(exc - np.array([got[i, ks[i] + 1:].sum() for i in range(n)])).max() <= 1e-15
    # categories: the mode and the median of the predictive distribution
    assert np.array_equal(fit.predict_category("mode", variance=v).cpu().numpy(), got.argmax(1))
    med = fit.predict_category("median", variance=v)
    assert med.dtype == torch.int64 and np.array_equal(med.cpu().numpy(), np.minimum((got.cumsum(1) < 0.5).sum(1), K - 1))
    agree = (med.cpu().numpy()[p["obs"]] == p["labels"][p["obs"]]).mean()
    print("the predictive median is the observed category at %.3f of the observed nodes" % agree)
    assert agree > 1.0 / K                                                                 # (better than chance: 1 / K)
    # the inherited latent variance, from the restated pseudo-observations
    var, se = fit.latent_variance(64, seed=5)
    z = np.abs(var.cpu().numpy() - dense) / se.cpu().numpy()
    print("latent_variance(64): worst %.2f standard errors, %.4f of the nodes within 5" % (z.max(), (z <= 5).mean()))
    assert (z <= 5.0).mean() >= 0.99
    prob64, var64 = fit.predict_proba(64, seed=5)
    assert torch.equal(var64, var) and float((prob64.sum(1) - 1.0).abs().max()) <= 1e-13
    x = fit.latent_samples(8, seed=9)
    assert x.dtype == torch.float32 and x.shape == (8, n)
    with pytest.raises(NotImplementedError):
        fit.evidence()


def test_model_method(mgp, golden, dev):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit, laplace_fit_ordinal, ordinal_cutpoints
    g = golden("dumbbell_k10_loop")
    labels, obs_np = oref.labels(g, K_FIT)
    x = T(g["train_x"], dev)
    y, obs = T(np.where(obs_np, labels, np.nan).astype(np.float32), dev), T(obs_np, dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev)).to(dev)
    desc = model.precision(noise=False)._descriptor()
    fit = model.laplace_posterior_ordinal(K_FIT, observed=obs, rtol=1e-4)
    want = laplace_fit_ordinal(desc, y, K_FIT, None, obs, rtol=1e-4)
    assert isinstance(fit, OrdinalLaplaceFit) and fit.converged and fit.num_categories == K_FIT
    assert torch.equal(fit.mean, want.mean) and fit.history == want.history and fit.log_likelihood == want.log_likelihood
    # the default cutpoints: ordinal_cutpoints of the observed labels, as float32 holds them
    assert torch.equal(fit.cutpoints.cpu(), ordinal_cutpoints(y, K_FIT, obs).float().double())
    assert np.abs(fit.cutpoints.cpu().numpy() - oref.cutpoints(labels, K_FIT, obs_np)).max() <= 2e-7
    given = model.laplace_posterior_ordinal(K_FIT, cutpoints=fit.cutpoints, observed=obs, rtol=1e-4)
    assert torch.equal(given.mean, fit.mean)
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_ordinal(desc, y, K_FIT, None, None)                       # NaN labels with every node observed
    with pytest.raises(ValueError, match="integers in"):
        model.laplace_posterior_ordinal(K_FIT - 1, observed=obs)              # a label beyond the categories
    semi = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev),
                     labeled=T(np.arange(x.shape[0]) < 100, dev)).to(dev)
    with pytest.raises(NotImplementedError):
        semi.laplace_posterior_ordinal(K_FIT, observed=obs)
