"""Laplace classification on the MI355X (csrc/laplace.hip, manifold_gp_amd/classification.py): the two kernels against their
float64 restatement on the same float32 inputs, the Newton fit against a dense float64 Newton iteration on the matrix the
kernels apply (_observed_ref.device_q2), the step control, the posterior pieces against the sampling functions they
delegate to, and the model method (tests/_laplace_ref.py)."""
import warnings

import numpy as np
import pytest
import torch

import _laplace_ref as lref
import _observed_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
NORMS = ["symmetric", "randomwalk"]
S_REF = 4.0
RTOL = 1e-5
# the kernels' own grid caps (csrc/laplace.hip): workgroups x 256 threads x nodes per thread and step
SITE_GRID_CAP, SITE_PER_STEP = 1024, 256 * 4
PREDICT_GRID_CAP, PREDICT_PER_STEP = 2048, 256
SIZES = [1, 63, 64, 65, 255, 257, 1546]


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
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])


def _site_inputs(n, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(n) * 2.0
    pick = rng.random(n) < 0.5
    f = np.where(pick, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), n), f).astype(np.float32)
    qf = rng.standard_normal(n).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    obs = rng.random(n) < 0.1
    if n < 20:
        obs[0] = True
    return f, qf, y, obs


def _ulps(got, want):
    """|got - want| in units of the float32 spacing at want"""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _check_site(mgp, dev, f, qf, y, obs, label):
    from manifold_gp_amd.classification import bernoulli_site
    y_in = y if obs is None else np.where(obs, y, np.float32(np.nan)).astype(np.float32)
    args = (T(f, dev), None if qf is None else T(qf, dev), T(y_in, dev), None if obs is None else T(obs, dev))
    w, rhs, sums = bernoulli_site(*args, s_ref=S_REF)
    want_w, want_rhs, want_sums, scale = lref.site_outputs(f, qf, y, obs, S_REF)
    gw, gr, gs = w.cpu().numpy(), rhs.cpu().numpy(), sums.cpu().numpy()
    assert w.dtype == torch.float32 and rhs.dtype == torch.float32 and sums.dtype == torch.float64
    assert np.isfinite(gw).all() and np.isfinite(gr).all() and np.isfinite(gs).all()
    uw, ur = _ulps(gw, want_w).max(), _ulps(gr, want_rhs).max()
    err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("%s: w %.2f ulp, rhs %.2f ulp, sums %.1e %.1e %.1e %.1e" % (label, uw, ur, *err))
    assert uw <= 1.0 and ur <= 1.0, (label, uw, ur)
    if obs is not None:
        q = np.zeros_like(f) if qf is None else qf
        assert (gw[~obs] == 0).all()
        assert np.array_equal(gr[~obs], (-np.float32(S_REF) * q[~obs]).astype(np.float32))
    assert err[0] <= 1e-12 and err[1] <= 1e-12 and err[3] <= 1e-12, (label, err)
    assert err[2] <= 1e-14, (label, err)
    w2, rhs2, sums2 = bernoulli_site(*args, s_ref=S_REF)
    assert torch.equal(w, w2) and torch.equal(rhs, rhs2) and torch.equal(sums, sums2)      # bitwise: no atomics
    assert w2.data_ptr() != w.data_ptr()                                                    # fresh tensors per call


@pytest.mark.parametrize("n", SIZES + [SITE_GRID_CAP * SITE_PER_STEP + 3 * SITE_PER_STEP + 5])
def test_site_kernel_matches_float64(mgp, dev, n):
    """w and rhs within 1 float32 ulp of the rounded float64 reference (both sides compute in float64), exactly 0 / -s_ref qf
    at unobserved nodes, the sums within 1e-12 of the sum of their absolute terms, the max within 1e-14; everything finite
    at |f| up to 1e4; a second call bitwise equal.  The last n runs the grid-stride loop past the grid cap."""
    f, qf, y, obs = _site_inputs(n, n)
    _check_site(mgp, dev, f, qf, y, obs, "n = %d, 10 %% observed" % n)
    _check_site(mgp, dev, f, qf, y, None, "n = %d, every node" % n)
    _check_site(mgp, dev, f, None, y, obs, "n = %d, qf NULL" % n)


def test_site_kernel_extreme_latents_and_unaligned_arrays(mgp, dev):
    from manifold_gp_amd.classification import bernoulli_site
    f = np.array([1e4, -1e4, 1e4, -1e4, 0.0], np.float32)
    y = np.array([1, 1, 0, 0, 1], np.float32)
    w, rhs, sums = bernoulli_site(T(f, dev), None, T(y, dev))
    assert w.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert rhs.cpu().tolist() == [0.0, 4.0, -4.0, 0.0, 2.0]
    assert abs(float(sums[0]) - (-2e4 - np.log(2.0))) <= 1e-11 and float(sums[2]) == 1.0
    # arrays one float off a 16-byte boundary (views into larger buffers): the scalar path, same numbers
    n = 257
    f, qf, y, obs = _site_inputs(n, 5)
    pad = lambda a: T(np.concatenate([a[:1], a]), dev)[1:]
    fa, qa, ya, oa = pad(f), pad(qf), pad(y), pad(obs)
    assert fa.data_ptr() % 16 == 4 and oa.data_ptr() % 4 == 1
    got = bernoulli_site(fa, qa, ya, oa)
    want = bernoulli_site(T(f, dev), T(qf, dev), T(y, dev), T(obs, dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert np.abs(got[2].cpu().numpy() - want[2].cpu().numpy()).max() <= 1e-12 * n


def test_site_kernel_argument_errors(mgp, dev):
    from manifold_gp_amd import _lib
    from manifold_gp_amd.classification import bernoulli_site
    lib = _lib.lib()
    n = 64
    f = torch.zeros(n, device=dev)
    w, rhs = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    work = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(f_=f, w_=w, rhs_=rhs, sums_=sums, n_=n, link=0, work_=work, wb=64):
        return lib.mgp_bernoulli_site(p(f_), None, p(f), None, n_, S_REF, link, p(w_), p(rhs_), p(sums_), p(work_), wb, st)
    assert call(f_=None) == -1 and call(w_=None) == -1 and call(rhs_=None) == -1 and call(sums_=None) == -1
    assert call(n_=0) == -1 and call(link=1) == -3 and call(work_=None) == -2 and call(wb=8) == -2
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and bool((rhs == 7.0).all()) and not sums.any()        # nothing was launched
    assert call() == 0
    with pytest.raises(ValueError):
        bernoulli_site(f, None, f, link="probit")


# ------------------------------------------------------------------------------------------------ 2: the predict kernel
def _predict_inputs(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-12.0, 12.0, n).astype(np.float32)
    v = rng.choice([0.0, 1e-4, 1e-2, 0.25, 1.0, 4.0, 9.0, 25.0, 100.0], n)
    return m, v


@pytest.mark.parametrize("n, Ks", [(k, (129,)) for k in SIZES[:-1]] + [(1546, (9, 129, 1025)),
                                                                      (PREDICT_GRID_CAP * PREDICT_PER_STEP + 777, (9,))])
def test_predict_kernel_matches_the_rule_in_numpy(mgp, dev, n, Ks):
    """Against the numpy restatement of the same rule at m in [-12, 12], v in {0, 1e-4, ..., 100}: <= 1e-13.  The last n runs
    the grid-stride loop past the grid cap (K = 9 keeps the numpy side small)."""
    from manifold_gp_amd.classification import bernoulli_predict
    m, v = _predict_inputs(n, n)
    for K in Ks:
        got = bernoulli_predict(T(m, dev), T(v, dev), points=K)
        assert got.dtype == torch.float64 and got.shape == (n,)
        err = np.abs(got.cpu().numpy() - lref.trapezoid(m, v, K)).max()
        print("n = %d, K = %d: %.2e" % (n, K, err))
        assert err <= 1e-13, (K, err)
        assert bool((got >= 0).all()) and bool((got <= 1).all())
    assert torch.equal(bernoulli_predict(T(m, dev), T(v, dev)), bernoulli_predict(T(m, dev), T(v, dev), points=129))


def test_predict_kernel_negative_variance_and_nan(mgp, dev):
    from manifold_gp_amd.classification import bernoulli_predict
    m = torch.tensor([-3.0, 0.0, 2.5, float("nan"), 1.0], device=dev)
    zero = bernoulli_predict(m, torch.zeros(5, dtype=torch.float64, device=dev))
    neg = bernoulli_predict(m, torch.tensor([-1.0, -1e-30, -100.0, -1.0, -0.0], dtype=torch.float64, device=dev))
    assert torch.equal(zero[[0, 1, 2, 4]], neg[[0, 1, 2, 4]])
    assert float((zero[[0, 1, 2, 4]] - torch.sigmoid(m.double()[[0, 1, 2, 4]])).abs().max()) <= 1e-14
    assert bool(torch.isnan(zero[3])) and bool(torch.isnan(neg[3]))
    got = bernoulli_predict(m, torch.tensor([1.0, float("nan"), 1.0, 1.0, 1.0], dtype=torch.float64, device=dev))
    assert torch.isnan(got).cpu().tolist() == [False, True, False, True, False]
    from manifold_gp_amd import _lib
    out = torch.zeros(5, dtype=torch.float64, device=dev)
    for K in (8, 7, 1027):
        assert _lib.lib().mgp_bernoulli_predict(_lib.ptr(m), _lib.ptr(out), 5, K, _lib.ptr(out), _lib.stream()) == -1


# ------------------------------------------------------------------------------------------------ the float64 apply
@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("norm", NORMS)
def test_float64_apply_matches_device_matrix(mgp, golden, dev, norm, nu):
    """Descriptor.apply_f64 (the fit's Q2 f) against the float64 matrix of the device's own CSR: 1e-12 of |Q2| |x| at every
    entry, one column and three, forms 0 and 3; the float32 chain on the same input is printed beside it."""
    desc = _desc(mgp, golden("dumbbell_k10_loop"), dev, norm, nu)
    Q = oref.device_q2(desc)
    rng = np.random.default_rng(nu)
    n = desc.n
    w32 = T(rng.random(n).astype(np.float32), dev)
    for C in (1, 3):
        x = rng.standard_normal((n, C))
        xd = T(x, dev)
        scale = abs(Q) @ np.abs(x) + np.abs(x)
        for d, want in ((desc, Q @ x), (desc.with_(form=3, noise=4.0, obs_w=w32), w32.double().cpu().numpy()[:, None] * x + 4.0 * (Q @ x))):
            got = d.apply_f64(xd if C > 1 else xd[:, 0])
            assert got.dtype == torch.float64 and got.shape == ((n, C) if C > 1 else (n,))
            err = (np.abs(got.cpu().numpy().reshape(n, C) - want) / scale).max()
            err32 = (np.abs(d.apply(xd.float()).double().cpu().numpy() - want) / scale).max()
            print("%s nu = %d C = %d form %d: float64 chain %.1e, float32 chain %.1e" % (norm, nu, C, d.form, err, err32))
            assert err <= 1e-12, err


# ------------------------------------------------------------------------------------------------ 3-5: the fit
_PROBLEMS = {}


def _problem(mgp, golden, dev, case, norm, nu):
    """One classification problem per (fixture, normalisation, nu), built once: the descriptor scaled to a prior marginal
    variance of about 9 (scale = float32(mean diag(Q1^-1) / 9): |f_hat| of 1.6-3.5, h over 0.03-0.25; with the fixtures'
    own scale |f_hat| ~ 0.01 and the problem is linear), the dense float64 matrix the kernels apply, the labels and the
    float64 Newton iteration from f = 0."""
    key = (case, norm, nu)
    if key not in _PROBLEMS:
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        t, obs, y = lref.labels(g)
        Q = scale * Q1
        f_ref, trace = lref.newton(Q, t, obs)
        _PROBLEMS[key] = dict(desc=d1.with_(scale=scale), Q=Q, t=t, obs=obs, y=T(y, dev), observed=T(obs, dev), f_ref=f_ref,
                              trace=trace)
    return _PROBLEMS[key]


def _psi_slack(a, b):
    """the fit's own slack: 16 * 2^-24 on |sum log p| + |f^T Q2 f| / 2, which is |psi| (the first is <= 0, the second >= 0),
    at the larger of the two points"""
    return 16.0 * 2.0 ** -24 * max(abs(a), abs(b))


def _check_mode(p, fit, label):
    f = fit.mean.double().cpu().numpy()
    res = np.abs(lref.gradient(p["Q"], f, p["t"], p["obs"])).max()
    g0 = np.abs(lref.gradient(p["Q"], np.zeros_like(f), p["t"], p["obs"])).max()
    err = np.abs(f - p["f_ref"]).max()
    print("%s: %d steps (float64: %d to rtol), max |g - Q f| = %.2e (bound %.2e), max |f - f_ref| = %.2e, max |f| = %.2f, "
          "CG iterations %s" % (label, fit.iterations, lref.steps_to(p["trace"], RTOL), res, 2 * RTOL * g0, err, np.abs(f).max(),
                                [h[3] for h in fit.history]))
    assert res <= 2 * RTOL * g0, (label, res)
    assert err <= 1e-4, (label, err)
    psis = [h[0] for h in fit.history]
    assert all(b >= a - _psi_slack(a, b) for a, b in zip(psis, psis[1:])), psis
    return err


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("case", FIXTURES)
def test_fit_matches_dense_float64_newton(mgp, golden, dev, case, norm, nu):
    """(a) the mode is stationary in float64 on the matrix the kernels apply: max |g - Q f| <= 2 rtol max |g(0)|;
    (b) max |f_hat - f_ref| <= 1e-4 (a float32 simulation on the CPU gave <= 2.2e-5 in all 12 cases; measured on the
    MI355X: 4.7e-5 at k10_loop nu = 1, <= 1.3e-5 elsewhere); (c) psi never
    decreases beyond the slack and every step from f0 = 0 is a full one; (d) at most two steps more than float64 Newton."""
    from manifold_gp_amd.classification import laplace_fit
    p = _problem(mgp, golden, dev, case, norm, nu)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        fit = laplace_fit(p["desc"], p["y"], p["observed"], rtol=RTOL)
    assert fit.converged and fit.mean.dtype == torch.float32 and fit.mean.shape == (p["desc"].n,)
    _check_mode(p, fit, "%s %s nu = %d" % (case, norm, nu))
    assert len(fit.history) == fit.iterations
    assert all(h[2] == 1.0 for h in fit.history), fit.history
    assert fit.history[-1][1] <= RTOL
    assert fit.iterations <= lref.steps_to(p["trace"], RTOL) + 2
    lp = lref.site(fit.mean.double().cpu().numpy(), None, p["t"], p["obs"])[0].sum()
    assert abs(fit.log_likelihood - lp) <= 1e-12 * abs(lp)
    assert torch.equal(fit.map_proba(), torch.sigmoid(fit.mean.double()))


def test_step_control_from_a_bad_start(mgp, golden, dev):
    """f0 = -20 (2 t - 1) on the observed nodes: every label confidently wrong.  The float64 iteration halves twice there
    and takes 8 steps; the fit reaches the same mode, never decreases psi, converges in at most 14 steps."""
    from manifold_gp_amd.classification import laplace_fit
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    f0 = np.where(p["obs"], -20.0 * (2.0 * p["t"] - 1.0), 0.0)
    f64, trace = lref.newton(p["Q"], p["t"], p["obs"], f0=f0)
    print("float64: %d steps, steps %s" % (len(trace), [s for _, _, s in trace]))
    assert np.abs(f64 - p["f_ref"]).max() <= 1e-9
    assert sum(s < 1.0 for _, _, s in trace) >= 1
    fit = laplace_fit(p["desc"], p["y"], p["observed"], rtol=RTOL, f0=T(f0.astype(np.float32), dev))
    print("fit: steps %s" % [h[2] for h in fit.history])
    assert fit.converged and fit.iterations <= 14
    _check_mode(p, fit, "from -20 (2 t - 1)")
    assert any(h[2] < 1.0 for h in fit.history)


def test_posterior_pieces_delegate_to_the_samplers(mgp, golden, dev):
    from manifold_gp_amd import sampling
    from manifold_gp_amd.classification import bernoulli_predict, laplace_fit
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    desc = p["desc"]
    fit = laplace_fit(desc, p["y"], p["observed"], rtol=RTOL)
    f = fit.mean.double()
    e = torch.exp(-f.abs())
    h = e / (1.0 + e) ** 2
    g = T(p["t"], dev) - torch.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    obs = p["observed"]
    assert bool((h[obs] >= 1e-30).all())                                      # obs_eff = observed here
    noise = torch.where(obs, 1.0 / h, torch.ones_like(h))
    var, se = fit.latent_variance(32, seed=5)
    want_var, want_se = sampling.posterior_variance(desc, noise, 32, 5, observed=obs)
    assert torch.equal(var, want_var) and torch.equal(se, want_se)
    targets = torch.where(obs, f + g * noise, torch.zeros_like(f))
    x = fit.latent_samples(256, seed=9)
    assert torch.equal(x, sampling.posterior_samples(desc, targets, noise, 256, 9, observed=obs))
    # the samples' mean is the mode: within 5 standard errors at >= 99 % of the nodes, the errors from the dense covariance
    hd = np.where(p["obs"], h.cpu().numpy(), 0.0)
    sd = np.sqrt(np.diag(np.linalg.inv(p["Q"] + np.diag(hd))) / 256.0)
    z = np.abs(x.double().mean(0).cpu().numpy() - f.cpu().numpy()) / sd
    print("mean of 256 samples: worst %.2f standard errors, %.4f of the nodes within 5" % (z.max(), (z <= 5).mean()))
    assert (z <= 5.0).mean() >= 0.99
    prob, pvar = fit.predict_proba(32, seed=5)
    assert torch.equal(pvar, var) and torch.equal(prob, bernoulli_predict(fit.mean, var))
    assert prob.dtype == torch.float64 and bool((prob >= 0).all()) and bool((prob <= 1).all())
    pulled = (prob - 0.5).abs() <= (fit.map_proba() - 0.5).abs() + 1e-15
    assert bool(pulled[var > 0].all()) and bool((var > 0).all())
    # an observed node whose curvature underflows is dropped from the pseudo-observations, not divided by
    with pytest.warns(UserWarning, match="not converged"):
        far = laplace_fit(desc, p["y"], obs, max_newton=0, f0=torch.where(obs, 200.0, 0.0).float() * (obs.cumsum(0) == 1))
    _, far_noise, eff = far._pseudo()
    assert int(obs.sum()) - int(eff.sum()) == 1 and bool(torch.isfinite(far_noise).all())


# ------------------------------------------------------------------------------------------------ 6: model and validation
def _model(mgp, g, dev, y, labeled=None):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x = T(g["train_x"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    return RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev), labeled=labeled).to(dev)


def test_model_method_and_validation(mgp, golden, dev):
    from manifold_gp_amd.classification import LaplaceFit, laplace_fit
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    _, obs_np, y_np = lref.labels(g)
    y, obs = T(y_np, dev), T(obs_np, dev)
    model = _model(mgp, g, dev, y)
    desc = model.precision(noise=False)._descriptor()
    fit = model.laplace_posterior(observed=obs, rtol=1e-4)
    want = laplace_fit(desc, y, obs, rtol=1e-4)
    assert isinstance(fit, LaplaceFit) and fit.converged
    assert torch.equal(fit.mean, want.mean) and fit.history == want.history and fit.iterations == want.iterations
    with pytest.raises(ValueError, match="0 or 1"):
        laplace_fit(desc, y, None)                                            # NaN labels with every node observed
    with pytest.raises(ValueError, match="0 or 1"):
        laplace_fit(desc, torch.where(obs, 2.0 * y, y), obs)
    with pytest.raises(ValueError, match="no node"):
        laplace_fit(desc, y, torch.zeros(n, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        laplace_fit(desc, y[:-1], obs)
    with pytest.raises(ValueError):
        laplace_fit(desc, y, obs[:-1])
    with pytest.raises(ValueError, match="f0"):
        laplace_fit(desc, y, obs, f0=torch.zeros(n - 1, device=dev))
    with pytest.raises(ValueError, match="link"):
        laplace_fit(desc, y, obs, link="probit")
    semi = _model(mgp, g, dev, y, labeled=T(np.arange(n) < 100, dev))
    with pytest.raises(NotImplementedError):
        semi.laplace_posterior(observed=obs)
