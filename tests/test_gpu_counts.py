"""Count fits on the MI355X (mgp_count_site in csrc/laplace.hip, manifold_gp_amd/counts.py): the site kernel against its float64
restatement on the same float32 inputs, the binomial stage at one trial against the Bernoulli stage, the Newton fit against a
dense float64 Newton iteration on the matrix the kernels apply (_observed_ref.device_q2), the step control from a low start,
the pseudo-observations against the dense Laplace covariance, the predicted counts and the model method
(tests/_counts_ref.py)."""
import warnings

import numpy as np
import pytest
import torch
from scipy.special import expit

import _counts_ref as cref
import _laplace_ref as lref
import _observed_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

FAMILIES = ["poisson", "binomial"]
SITE_GRID_CAP, SITE_PER_STEP = 1024, 256 * 4            # the kernel's grid cap (csrc/laplace.hip): workgroups x nodes per step
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1025, 1546, SITE_GRID_CAP * SITE_PER_STEP + 3 * SITE_PER_STEP + 5]
S_REF = {"poisson": 2.0 ** -9, "binomial": 2.0 ** -4}
MEAN = {"poisson": 0.75, "binomial": -0.25}
BIG = 2.0 ** 24
EXTREME = [(f, y) for f in (1e4, -1e4, 88.0, -90.0, 0.0) for y in (0.0, 1.0, BIG)]


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


# ------------------------------------------------------------------------------------------------ 1: the site kernel
def _site_inputs(family, n, seed, extremes):
    """f with eta = f + mean (+ aux) uniform in [-30, 12]; counts from a few sizes up to 2^24; 10 % observed.  extremes: the 15
    (f, y) pairs of EXTREME at random observed nodes (n >= 63)."""
    rng = np.random.default_rng(seed)
    eta = rng.uniform(-30.0, 12.0, n)
    qf = rng.standard_normal(n).astype(np.float32)
    obs = rng.random(n) < 0.1
    obs[0] = True
    if family == "poisson":
        aux = np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32)
        y = rng.choice([0.0, 1.0, 2.0, 5.0, 40.0, 1000.0, BIG], n)
        f = (eta - MEAN[family] - aux).astype(np.float32)
    else:
        aux = np.where(rng.random(n) < 0.1, BIG, rng.integers(1, 40, n)).astype(np.float32)
        y = np.floor(rng.random(n) * (aux.astype(np.float64) + 1.0)).clip(0.0, aux)
        f = (eta - MEAN[family]).astype(np.float32)
    y = y.astype(np.float32)
    if extremes and n >= 63:
        at = rng.choice(n, len(EXTREME), replace=False)
        f[at] = [e[0] for e in EXTREME]
        y[at] = [e[1] for e in EXTREME]
        obs[at] = True
        aux[at] = 0.0 if family == "poisson" else BIG
    return f, qf, y, aux, obs


def _ulps(got, want):
    """|got - want| in units of the float32 spacing at want (which is inf at FLT_MAX: 0 ulp where both are saturated)"""
    with np.errstate(over="ignore"):
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _nan_outside(a, obs):
    return a if obs is None or a is None else np.where(obs, a, np.float32(np.nan)).astype(np.float32)


def _check_site(dev, family, f, qf, y, aux, obs, label, pad=False):
    """One call against the restatement; returns the largest observed fraction of the rhs bound's float64 term."""
    from manifold_gp_amd.counts import count_site
    s_ref, mean = S_REF[family], MEAN[family]
    up = (lambda a: T(np.concatenate([a[:1], a]), dev)[1:]) if pad else (lambda a: T(a, dev))
    # NaN in y and aux wherever the node is unobserved: never read
    args = (up(f), None if qf is None else up(qf), up(_nan_outside(y, obs)), None if aux is None else up(_nan_outside(aux, obs)),
            None if obs is None else up(obs))
    if pad:
        assert args[0].data_ptr() % 16 == 4 and (obs is None or args[4].data_ptr() % 4 == 1)
    w, rhs, sums = count_site(*args, s_ref, mean, family)
    want_w, want_rhs, want_sums, scale, cancel = cref.site_outputs(family, f, qf, y, aux, obs, s_ref, mean)
    gw, gr, gs = w.cpu().numpy(), rhs.cpu().numpy(), sums.cpu().numpy()
    assert w.dtype == torch.float32 and rhs.dtype == torch.float32 and sums.dtype == torch.float64
    assert np.isfinite(gw).all() and np.isfinite(gr).all() and np.isfinite(gs[:3]).all()
    sat = np.abs(want_rhs) == cref.FLT_MAX
    assert np.array_equal(gr[sat], want_rhs[sat]) and np.array_equal(gw[want_w == cref.FLT_MAX], want_w[want_w == cref.FLT_MAX])
    uw = _ulps(gw, want_w).max()
    diff = np.abs(gr.astype(np.float64) - want_rhs.astype(np.float64))
    with np.errstate(over="ignore"):
        ulp = np.where(sat, 0.0, np.spacing(np.abs(want_rhs)).astype(np.float64))
    f64 = 4.0 * 2.0 ** -53 * cancel
    assert (diff <= ulp + f64).all(), (label, (diff - ulp - f64).max())
    frac = (np.maximum(diff - ulp, 0.0) / np.where(f64 > 0, f64, 1.0)).max()
    with np.errstate(invalid="ignore"):
        err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("%s %s: w %.2f ulp, rhs beyond 1 ulp: %.2f of the float64 term, sums %.1e %.1e %.1e %.1e, saturated %d"
          % (family, label, uw, frac, *err, int(sat.sum())))
    assert uw <= 1.0, (label, uw)
    if obs is not None:
        q = np.zeros_like(f) if qf is None else qf
        assert (gw[~obs] == 0).all()
        assert np.array_equal(gr[~obs], (-np.float32(s_ref) * q[~obs]).astype(np.float32))
    assert err[0] <= 1e-12 and err[1] <= 1e-12 and err[2] <= 1e-14, (label, err)
    if np.isinf(want_sums[3]):
        assert gs[3] == np.inf
    else:
        assert err[3] <= 1e-12, (label, err)
    w2, rhs2, sums2 = count_site(*args, s_ref, mean, family)
    assert torch.equal(w, w2) and torch.equal(rhs, rhs2) and torch.equal(sums, sums2)       # bitwise: no atomics
    assert w2.data_ptr() != w.data_ptr()                                                     # fresh tensors per call
    return frac


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_site_kernel_matches_float64(dev, mgp, n, family):
    """w within 1 float32 ulp of the rounded float64 reference; |rhs - ref| <= ulp32(ref) + 4 * 2^-53 s_ref (mu or N + y + |qf|):
    both sides round a float64 value, and g is a difference of terms of that size formed with the float64 exp of two libraries
    (measured on the MI355X: w 0 ulp and rhs within 1 ulp in every case, so the largest observed fraction of the second term is
    0; sums within 6.1e-16, the max within 1.6e-16);
    exactly 0 / -s_ref qf at unobserved nodes; sums 0, 1, 3 within 1e-12 of
    the sum of their absolute terms, the max within 1e-14; +-FLT_MAX where the restatement overflows float32 and sum 3 = +inf
    there; NaN counts and aux at unobserved nodes; a second call bitwise equal.  The last n runs the grid-stride loop past the
    grid cap."""
    f, qf, y, aux, obs = _site_inputs(family, n, n, extremes=True)
    _check_site(dev, family, f, qf, y, aux, obs, "n = %d, 10 %% observed, extremes" % n)
    f, qf, y, aux, obs = _site_inputs(family, n, n + 1, extremes=False)
    _check_site(dev, family, f, qf, y, aux, None, "n = %d, every node" % n)
    _check_site(dev, family, f, None, y, aux, obs, "n = %d, qf NULL" % n)
    if family == "poisson":
        _check_site(dev, family, f, qf, y, None, obs, "n = %d, aux NULL" % n)


@pytest.mark.parametrize("family", FAMILIES)
def test_site_kernel_unaligned_arrays_and_extreme_values(dev, mgp, family):
    """Arrays one float off a 16-byte boundary (views into larger buffers) take the scalar path: the same bounds, and the same
    w and rhs bit for bit as the aligned call.  Then the 15 extreme (f, y) pairs alone."""
    from manifold_gp_amd.counts import count_site
    n = 257
    f, qf, y, aux, obs = _site_inputs(family, n, 5, extremes=True)
    _check_site(dev, family, f, qf, y, aux, obs, "n = 257, one float off", pad=True)
    pad = lambda a: T(np.concatenate([a[:1], a]), dev)[1:]
    got = count_site(pad(f), pad(qf), pad(y), pad(aux), pad(obs), S_REF[family], MEAN[family], family)
    want = count_site(T(f, dev), T(qf, dev), T(y, dev), T(aux, dev), T(obs, dev), S_REF[family], MEAN[family], family)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    f = np.array([e[0] for e in EXTREME], np.float32)
    y = np.array([e[1] for e in EXTREME], np.float32)
    aux = None if family == "poisson" else np.full(f.shape, BIG, np.float32)
    w, rhs, sums = count_site(T(f, dev), None, T(y, dev), None if aux is None else T(aux, dev), None, 2.0 ** -24, 0.0, family)
    want_w, want_rhs, want_sums, _, _ = cref.site_outputs(family, f, None, y, aux, None, 2.0 ** -24, 0.0)
    assert np.array_equal(w.cpu().numpy(), want_w) and bool(torch.isfinite(sums[:3]).all())
    assert _ulps(rhs.cpu().numpy(), want_rhs).max() <= 1.0
    if family == "poisson":
        assert w.cpu().tolist()[:6] == [cref.FLT_MAX] * 3 + [0.0] * 3 and rhs.cpu().tolist()[:3] == [-cref.FLT_MAX] * 3
        assert float(sums[3]) == np.inf
    else:
        assert w.cpu().tolist()[:6] == [0.0] * 6 and float(w[-1]) == 0.25
        assert abs(float(sums[0]) - want_sums[0]) <= 1e-12 * abs(want_sums[0])


def test_site_kernel_argument_errors(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n = 64
    f = torch.zeros(n, device=dev)
    w, rhs = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    work = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(f_=f, aux_=f, w_=w, rhs_=rhs, sums_=sums, n_=n, family=0, work_=work, wb=64):
        return lib.mgp_count_site(p(f_), None, p(f), p(aux_), None, n_, 1.0, 0.0, family, p(w_), p(rhs_), p(sums_), p(work_), wb, st)
    assert call(f_=None) == -1 and call(w_=None) == -1 and call(rhs_=None) == -1 and call(sums_=None) == -1
    assert call(n_=0) == -1 and call(family=2) == -3 and call(work_=None) == -2 and call(wb=8) == -2
    assert call(family=1, aux_=None) == -1
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and bool((rhs == 7.0).all()) and not sums.any()        # nothing was launched
    assert call() == 0 and call(aux_=None) == 0


# ------------------------------------------------------------------------------------------------ 2: one trial is Bernoulli
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])


def test_one_trial_reproduces_the_bernoulli_stage(dev, mgp):
    """trials = 1, mean = 0, s_ref = 4: w is bitwise bernoulli_site's (the same expression), rhs within the bound of test 1
    (g = t - pi there, y (1 - pi) - (1 - y) pi without the subtraction here)."""
    from manifold_gp_amd.classification import bernoulli_site
    from manifold_gp_amd.counts import count_site
    n = 1546
    rng = np.random.default_rng(2)
    f = rng.standard_normal(n) * 2.0
    f = np.where(rng.random(n) < 0.5, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), n), f).astype(np.float32)
    qf = rng.standard_normal(n).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    obs = rng.random(n) < 0.5
    a = (T(f, dev), T(qf, dev), T(y, dev))
    wb, rb, sb = bernoulli_site(*a, T(obs, dev), s_ref=4.0)
    wc, rc, sc = count_site(*a, torch.ones(n, device=dev), T(obs, dev), 4.0, 0.0, "binomial")
    assert torch.equal(wb, wc)
    diff = (rb.double() - rc.double()).abs().cpu().numpy()
    bound = np.spacing(np.abs(rb.cpu().numpy())).astype(np.float64) + 4.0 * 2.0 ** -53 * 4.0 * (1.0 + y + np.abs(qf))
    print("rhs: %d of %d entries differ, worst %.2f of the bound" % ((diff > 0).sum(), n, (diff / bound).max()))
    assert (diff <= bound).all()
    sb, sc = sb.cpu().numpy(), sc.cpu().numpy()
    assert np.abs(sb - sc).max() <= 1e-12 * max(1.0, np.abs(sb).max())


# ------------------------------------------------------------------------------------------------ 3-6: the fit
_PROBLEMS = {}


def _problem(mgp, golden, dev, case, norm, nu, family):
    """One count problem per (fixture, normalisation, nu, family), built once: the descriptor scaled to a prior marginal variance
    of about 9, the dense float64 matrix the kernels apply, the data of _counts_ref.counts and the float64 Newton iteration."""
    key = (case, norm, nu)
    if key not in _PROBLEMS:
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        _PROBLEMS[key] = dict(desc=d1.with_(scale=scale), Q=scale * Q1, counts=cref.counts(g))
    base = _PROBLEMS[key]
    if family not in base:
        c = base["counts"]
        d = cref.poisson_data(c) if family == "poisson" else cref.binomial_data(c)
        f_ref, trace = cref.newton(base["Q"], d)
        nan = lambda a: T(np.where(c["obs"], a, np.nan).astype(np.float32), dev)
        kw = dict(exposure=T(c["E"], dev)) if family == "poisson" else dict(trials=nan(c["N"]))
        base[family] = dict(desc=base["desc"], Q=base["Q"], counts=c, d=d, f_ref=f_ref, trace=trace, y=nan(d["y"]), observed=T(c["obs"], dev),
                            kw=dict(family=family, **kw))
    return base[family]


def _fit(p, **kw):
    from manifold_gp_amd.counts import laplace_fit_counts
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        return laplace_fit_counts(p["desc"], p["y"], p["observed"], **p["kw"], **kw)


def _fitted(p):
    if "fit" not in p:
        p["fit"] = _fit(p)
    return p["fit"]


def _check_mode(p, fit, label):
    f = fit.mean.double().cpu().numpy()
    err = np.abs(f - p["f_ref"]).max()
    res = np.abs(cref.gradient(p["Q"], f, p["d"])).max()
    g0 = np.abs(cref.gradient(p["Q"], np.zeros_like(f), p["d"])).max()
    lp = cref.log_likelihood(p["f_ref"], p["d"])
    lerr = abs(fit.log_likelihood - lp) / abs(lp)
    print("%s: %d steps %s, max |f - f_ref| = %.2e, max |g - Q f| = %.2e (relative to max |g(0)| = %.0f: %.1e), max |f| = %.2f, "
          "log-likelihood %.6f (relative error %.1e), CG iterations %s"
          % (label, fit.iterations, [h[2] for h in fit.history], err, res, g0, res / g0, np.abs(f).max(), fit.log_likelihood, lerr,
             [h[3] for h in fit.history]))
    assert fit.converged
    assert err <= 1e-4, (label, err)
    assert lerr <= 1e-6, (label, lerr)
    return err


FIT_CASES = [("poisson", c, n, nu) for c in ("dumbbell_k10_loop", "dumbbell_k50_noloop")
             for n, nu in (("symmetric", 2), ("randomwalk", 1), ("symmetric", 3))] + \
            [("binomial", "dumbbell_k10_loop", "symmetric", 2), ("binomial", "dumbbell_k50_noloop", "symmetric", 2),
             ("binomial", "dumbbell_k10_loop", "randomwalk", 3)]


@pytest.mark.parametrize("family, case, norm, nu", FIT_CASES)
def test_fit_matches_dense_float64_newton(mgp, golden, dev, family, case, norm, nu):
    """converged by the step rule, every step from f0 = 0 a full one, max |f_hat - f_ref| <= 1e-4 (a float32 simulation on the
    CPU gives 1.1e-7 .. 2.5e-7 with an exact linear solve; with cg_tol = 1e-3 the last step of <= 1e-3 leaves ~1e-6), the
    log-likelihood with its constant within 1e-6 relative of the restatement's at its own mode.  Measured on the MI355X: mode
    1.7e-6 (Poisson, k10_loop, symmetric, nu = 2), 1.2e-7 .. 2.0e-7 in the other eight cases; log-likelihood <= 1.6e-9."""
    from manifold_gp_amd.counts import CountLaplaceFit
    p = _problem(mgp, golden, dev, case, norm, nu, family)
    fit = _fitted(p)
    assert isinstance(fit, CountLaplaceFit) and fit.mean.dtype == torch.float32 and fit.mean.shape == (p["desc"].n,)
    _check_mode(p, fit, "%s %s %s nu = %d" % (family, case, norm, nu))
    assert len(fit.history) == fit.iterations and all(h[2] == 1.0 for h in fit.history), fit.history
    assert fit.s_ref == p["d"]["s_ref"] and abs(fit.prior_mean - p["d"]["mean"]) <= 1e-14
    eta = fit.mean.double().cpu().numpy() + fit.prior_mean
    want = np.exp(p["d"]["aux"] + eta) if family == "poisson" else p["d"]["aux"] * expit(eta)
    got = fit.map_mean().cpu().numpy()
    obs = p["d"]["obs"]
    assert np.abs(got[obs] - want[obs]).max() <= 1e-6 * np.abs(want[obs]).max()


def test_step_control_from_a_low_start(mgp, golden, dev):
    """Poisson from f0 = -3 at every node: the first Newton steps overshoot and are halved (the CPU simulation: 1/16, 1/2, then
    full); the fit converges to the same mode."""
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2, "poisson")
    fit = _fit(p, f0=torch.full((p["desc"].n,), -3.0, device=dev))
    _check_mode(p, fit, "from f0 = -3")
    assert any(h[2] < 1.0 for h in fit.history)


@pytest.mark.parametrize("family", FAMILIES)
def test_pseudo_observations_against_the_dense_laplace_covariance(mgp, golden, dev, family):
    """latent_variance(256) within 5 of its own standard errors of diag((Q2 + H)^-1) at every node, the ratio of the means within
    2 %; the mean of 256 latent_samples within 5 dense standard errors of f_hat at every node.  The 5 caps a correct sampler's
    maximum over 1546 nodes (probability about 1e-3); it is not a measurement."""
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2, family)
    fit = _fitted(p)
    f = fit.mean.double().cpu().numpy()
    dense = np.diag(np.linalg.inv(p["Q"] + np.diag(cref.curvature(f, p["d"]))))
    var, se = fit.latent_variance(256, seed=5)
    var, se = var.cpu().numpy(), se.cpu().numpy()
    z = np.abs(var - dense) / se
    ratio = var.mean() / dense.mean()
    print("%s: latent_variance(256): worst %.2f standard errors, ratio of the means %.4f, variances %.3g .. %.3g"
          % (family, z.max(), ratio, dense.min(), dense.max()))
    x = fit.latent_samples(256, seed=9)
    assert x.dtype == torch.float32 and x.shape == (256, p["desc"].n)
    zs = np.abs(x.double().mean(0).cpu().numpy() - f) / np.sqrt(dense / 256.0)
    print("%s: mean of 256 samples: worst %.2f standard errors" % (family, zs.max()))
    assert z.max() <= 5.0 and abs(ratio - 1.0) <= 0.02
    assert zs.max() <= 5.0


def test_predicted_counts(mgp, golden, dev):
    """Poisson: the log-normal closed form from the same latent variance, 1e-12 relative at every node; binomial: N x the
    trapezoid rule of _laplace_ref at the float32 eta_hat, 1e-13 N at every node; E = 1 / N = 1 where the caller gave none at
    an unobserved node.  Measured on the MI355X: 3.6e-16 and 6.4e-16 (Poisson mean, variance), 8.9e-16 and 4.6e-16 (binomial)."""
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2, "poisson")
    fit = _fitted(p)
    m, v, lv = fit.predict_mean(16, seed=5)
    assert torch.equal(lv, fit.latent_variance(16, seed=5)[0]) and m.dtype == torch.float64
    E, lvn = p["counts"]["E"], lv.cpu().numpy()
    want = E * np.exp(fit.mean.double().cpu().numpy() + fit.prior_mean + 0.5 * lvn)
    want_v = want + want ** 2 * np.expm1(lvn)
    em, ev = np.abs(m.cpu().numpy() - want) / want, np.abs(v.cpu().numpy() - want_v) / want_v
    print("poisson predict_mean: worst relative error of the mean %.2e, of the variance %.2e; means %.3g .. %.3g, latent "
          "variances %.3g .. %.3g" % (em.max(), ev.max(), want.min(), want.max(), lvn.min(), lvn.max()))
    assert (em <= 1e-12).all() and (ev <= 1e-12).all()                       # at every node, relative to that node's value
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2, "binomial")
    fit = _fitted(p)
    m, v, lv = fit.predict_mean(16, seed=5, points=129)
    obs = p["d"]["obs"]
    N = np.where(obs, p["d"]["aux"], 1.0)                                    # the trials were NaN at the unobserved nodes
    assert np.array_equal(fit.trials.cpu().numpy(), N)
    eta32 = (fit.mean.double() + fit.prior_mean).float().double().cpu().numpy()
    prob = lref.trapezoid(eta32, lv.cpu().numpy())
    em, ev = np.abs(m.cpu().numpy() - N * prob) / N, np.abs(v.cpu().numpy() - N * prob * (1.0 - prob)) / N
    print("binomial predict_mean: worst error of the mean / N %.2e, of the variance / N %.2e" % (em.max(), ev.max()))
    assert (em <= 1e-13).all() and (ev <= 1e-13).all()                       # at every node: 1e-13 on the probability
    with pytest.raises(NotImplementedError):
        fit.predict_proba()


def test_one_trial_fit_is_the_bernoulli_fit(mgp, golden, dev):
    """laplace_fit_counts(family="binomial", trials=1) against laplace_fit on the same 0/1 labels: modes within 1e-5."""
    from manifold_gp_amd.classification import laplace_fit
    from manifold_gp_amd.counts import laplace_fit_counts
    g = golden("dumbbell_k10_loop")
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2, "poisson")
    _, obs, y = lref.labels(g)
    y, obs = T(y, dev), T(obs, dev)
    a = laplace_fit(p["desc"], y, obs)
    b = laplace_fit_counts(p["desc"], y, obs, family="binomial", trials=torch.ones(p["desc"].n, device=dev))
    err = float((a.mean.double() - b.mean.double()).abs().max())
    print("one trial against laplace_fit: max |difference of the modes| = %.2e; steps %d and %d" % (err, a.iterations, b.iterations))
    assert a.converged and b.converged and b.s_ref == 4.0 and b.prior_mean == 0.0
    assert err <= 1e-5
    assert abs(a.log_likelihood - b.log_likelihood) <= 1e-6 * abs(a.log_likelihood)


def test_model_method(mgp, golden, dev):
    from manifold_gp_amd.counts import CountLaplaceFit, laplace_fit_counts
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    g = golden("dumbbell_k10_loop")
    c = cref.counts(g)
    x = T(g["train_x"], dev)
    y, obs, E = T(np.where(c["obs"], c["y"], np.nan).astype(np.float32), dev), T(c["obs"], dev), T(c["E"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev)).to(dev)
    desc = model.precision(noise=False)._descriptor()
    fit = model.laplace_posterior_counts(observed=obs, exposure=E)
    want = laplace_fit_counts(desc, y, obs, exposure=E)
    assert isinstance(fit, CountLaplaceFit) and fit.converged and fit.family == "poisson"
    assert torch.equal(fit.mean, want.mean) and fit.history == want.history and fit.log_likelihood == want.log_likelihood
    with pytest.raises(ValueError, match="integers in"):
        laplace_fit_counts(desc, y, None, exposure=E)                         # NaN counts with every node observed
    with pytest.raises(ValueError, match="needs trials"):
        model.laplace_posterior_counts(observed=obs, family="binomial")
    semi = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev),
                     labeled=T(np.arange(x.shape[0]) < 100, dev)).to(dev)
    with pytest.raises(NotImplementedError):
        semi.laplace_posterior_counts(observed=obs)
