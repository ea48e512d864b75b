"""Negative-binomial count fits on the MI355X (mgp_nb_site and mgp_nb_evidence_site in csrc/laplace.hip, mgp_nb_predict_pmf /
mgp_nb_predict_logpmf in csrc/count_predict.hip, manifold_gp_amd/counts.py and evidence.py) against the float64 restatement of
tests/_nb_ref.py: the site kernel, the pmf kernels at the bar whose constants test_nb_cpu.py measures, the Newton fit against a
dense float64 iteration on the matrix the kernels apply, the posterior pieces, the evidence with its gradient, the dispersion
profile and the coincident-point fixture."""
import math
import warnings

import numpy as np
import pytest
import torch

import _count_pmf_ref as pref
import _nb_ref as nb
import _observed_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

NBF = "negative_binomial"
S_REF, MEAN = 2.0 ** -9, 0.75
BIG = 2.0 ** 24
EXTREME = [(f, y) for f in (1e4, -1e4, 88.0, -90.0, 0.0) for y in (0.0, 1.0, BIG)]      # the pairs of test_gpu_counts.py
SITE_R = [2.0 ** -10, 1.5, 2.0 ** 20]
DENSE_BAR = 10 * 1.43e-8                                  # test_gpu_evidence.py: |device - dense float64| / logdet B


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


def _off(a, dev):
    """a device copy of `a` one element off its vector boundary (a view into a larger buffer)"""
    return T(np.concatenate([a[:1], a]), dev)[1:]


def _ulps(got, want):
    with np.errstate(over="ignore"):
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _nan_outside(a, obs, dtype=np.float32):
    return a if obs is None or a is None else np.where(obs, a, np.nan).astype(dtype)


# ------------------------------------------------------------------------------------------------ 1: the site kernels
def _site_inputs(n, seed, r, extremes):
    """f with z = f + mean + aux - log r uniform in [-30, 12]; counts from a few sizes up to 2^24; 10 % observed; latent variances
    in [0.01, 9].  extremes: the 15 (f, y) pairs of EXTREME at random observed nodes (n >= 63)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-30.0, 12.0, n)
    qf = rng.standard_normal(n).astype(np.float32)
    obs = rng.random(n) < 0.1
    obs[0] = True
    var = rng.uniform(0.01, 9.0, n)
    aux = np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32)
    y = rng.choice([0.0, 1.0, 2.0, 5.0, 40.0, 1000.0, BIG], n).astype(np.float32)
    f = (z - MEAN - aux + math.log(r)).astype(np.float32)
    if extremes and n >= 63:
        at = rng.choice(n, len(EXTREME), replace=False)
        f[at] = [e[0] for e in EXTREME]
        y[at] = [e[1] for e in EXTREME]
        obs[at] = True
        aux[at] = 0.0
    return f, qf, y, aux, obs, var


def _check_site(dev, r, f, qf, y, aux, obs, label, pad=False):
    """One mgp_nb_site call against the restatement, at the bars of test_gpu_counts.py; returns (w, rhs) of the device."""
    from manifold_gp_amd.counts import count_site
    up = (lambda a: _off(a, dev)) if pad else (lambda a: T(a, dev))
    args = (up(f), None if qf is None else up(qf), up(_nan_outside(y, obs)), None if aux is None else up(_nan_outside(aux, obs)),
            None if obs is None else up(obs))
    if pad:
        assert args[0].data_ptr() % 16 == 4 and (obs is None or args[4].data_ptr() % 4 == 1)
    w, rhs, sums = count_site(*args, S_REF, MEAN, NBF, r)
    want_w, want_rhs, want_sums, scale, cancel = nb.site_outputs(f, qf, y, aux, obs, S_REF, MEAN, r)
    gw, gr, gs = w.cpu().numpy(), rhs.cpu().numpy(), sums.cpu().numpy()
    assert w.dtype == torch.float32 and rhs.dtype == torch.float32 and sums.dtype == torch.float64
    assert np.isfinite(gw).all() and np.isfinite(gr).all() and np.isfinite(gs).all()           # nothing saturates
    uw = _ulps(gw, want_w).max()
    diff = np.abs(gr.astype(np.float64) - want_rhs.astype(np.float64))
    ulp = np.spacing(np.abs(want_rhs)).astype(np.float64)
    f64 = 4.0 * 2.0 ** -53 * cancel
    assert (diff <= ulp + f64).all(), (label, (diff - ulp - f64).max())
    frac = (np.maximum(diff - ulp, 0.0) / np.where(f64 > 0, f64, 1.0)).max()
    err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("r = %g %s: w %.2f ulp, rhs beyond 1 ulp: %.2f of the float64 term, sums %.1e %.1e %.1e %.1e" % (r, label, uw, frac, *err))
    assert uw <= 1.0, (label, uw)
    if obs is not None:
        q = np.zeros_like(f) if qf is None else qf
        assert (gw[~obs] == 0).all()
        assert np.array_equal(gr[~obs], (-np.float32(S_REF) * q[~obs]).astype(np.float32))
    assert err[0] <= 1e-12 and err[1] <= 1e-12 and err[2] <= 1e-14 and err[3] <= 1e-12, (label, err)
    w2, rhs2, sums2 = count_site(*args, S_REF, MEAN, NBF, r)
    assert torch.equal(w, w2) and torch.equal(rhs, rhs2) and torch.equal(sums, sums2)           # bitwise: no atomics
    return w, rhs


@pytest.mark.parametrize("r", SITE_R)
@pytest.mark.parametrize("n", [1, 3, 257, 4099])
def test_site_kernel_matches_float64(dev, mgp, n, r):
    """mgp_nb_site at the bars of test_gpu_counts.py: w within 1 float32 ulp of the rounded float64 reference, |rhs - ref| <=
    ulp32(ref) + 4 * 2^-53 s_ref (2 y + r + |qf|), exactly 0 / -s_ref qf at unobserved nodes, sums within 1e-12 / 1e-12 / 1e-14 /
    1e-12 of the sum of their absolute terms, everything finite (h <= (y + r) / 4: no saturation), NaN counts and exposures at
    unobserved nodes, a second call bitwise equal.  n = 1: a lone node; 3: less than a quad; 257: a ragged tail past one
    workgroup's first sweep of quads; 4099: several workgroups and a ragged tail.  Variants: 10 % observed with the extreme
    latents, every node observed, qf NULL, aux NULL, arrays one float (obs one byte) off their vector boundaries -- bitwise the
    aligned call.  Measured on the MI355X: w 0 ulp and rhs within 1 ulp in every case (0 of the float64 term), sums within
    2.9e-16, 1.6e-16, 0 and 2.4e-16."""
    f, qf, y, aux, obs, _ = _site_inputs(n, n, r, extremes=True)
    _check_site(dev, r, f, qf, y, aux, obs, "n = %d, 10 %% observed, extremes" % n)
    f, qf, y, aux, obs, _ = _site_inputs(n, n + 1, r, extremes=False)
    _check_site(dev, r, f, qf, y, aux, None, "n = %d, every node" % n)
    _check_site(dev, r, f, None, y, aux, obs, "n = %d, qf NULL" % n)
    _check_site(dev, r, f, qf, y, None, obs, "n = %d, aux NULL" % n)
    aligned = _check_site(dev, r, f, qf, y, aux, obs, "n = %d, aligned" % n)
    shifted = _check_site(dev, r, f, qf, y, aux, obs, "n = %d, one float off" % n, pad=True)
    assert torch.equal(aligned[0], shifted[0]) and torch.equal(aligned[1], shifted[1])


@pytest.mark.parametrize("r", SITE_R)
def test_evidence_site_kernel_matches_float64(dev, mgp, r):
    """mgp_nb_evidence_site at the bars of test_gpu_evidence.py: root_h and corr within 1 float32 ulp, 0 off the nodes kept, m exact,
    sum l and sum corr within 1e-12 of the sum of their absolute terms, max |corr| within 1e-14; var NULL; unaligned bitwise.
    Measured on the MI355X: 0 ulp both, sums within 3.0e-16."""
    from manifold_gp_amd.evidence import evidence_site
    for n in (3, 257, 4099):
        f, _, y, aux, obs, var = _site_inputs(n, 3 * n, r, extremes=True)
        outs = []
        for pad in (False, True):
            up = (lambda a: _off(a, dev)) if pad else (lambda a: T(a, dev))
            args = (up(f), up(_nan_outside(y, obs)), up(_nan_outside(aux, obs)), up(obs), up(_nan_outside(var, obs, np.float64)))
            root, corr, sums = evidence_site(*args, MEAN, NBF, 1e-6, dispersion=r)
            outs.append((root, corr, sums))
        root, corr, sums = outs[0]
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
        want_root, want_corr, want_sums, scale, eff = nb.evidence_outputs(f, y, aux, obs, var, MEAN, r, 1e-6)
        gr, gc, gs = root.cpu().numpy(), corr.cpu().numpy(), sums.cpu().numpy()
        assert np.isfinite(gr).all() and np.isfinite(gc).all() and np.isfinite(gs).all()
        ur, uc = _ulps(gr, want_root).max(), _ulps(gc, want_corr).max()
        err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
        print("r = %g n = %d: root_h %.2f ulp, corr %.2f ulp, sums %.1e %.1e %.1e, m = %d" % (r, n, ur, uc, err[0], err[2], err[3], eff.sum()))
        assert ur <= 1.0 and uc <= 1.0 and (gr[~eff] == 0).all() and (gr[eff] > 0).all() and (gc[~eff] == 0).all()
        assert gs[1] == float(eff.sum()) and err[0] <= 1e-12 and err[2] <= 1e-12 and err[3] <= 1e-14
        root0, corr0, sums0 = evidence_site(T(f, dev), T(y, dev), T(aux, dev), T(obs, dev), None, MEAN, NBF, 1e-6, dispersion=r)
        assert corr0 is None and torch.equal(root0, root) and float(sums0[2]) == 0.0 and float(sums0[3]) == 0.0


# ------------------------------------------------------------------------------------------------ 2: the pmf kernels
NS, KCOUNTS = [1, 3, 64, 65, 257], [1, 2, 63, 64, 65, 300]
PMF_R = [0.37, 8.0, 2.0 ** 20]


@pytest.mark.parametrize("r", PMF_R)
@pytest.mark.parametrize("k0, with_aux", [(0, True), (0, False), (1000, True)])
def test_pmf_kernel_matches_the_restatement(dev, mgp, k0, with_aux, r):
    """|log pmf_dev - log pmf_ref| <= c 2^-53 T + r_129 at P = 129 for n in {1, 3, 64, 65, 257} x K in {1, 2, 63, 64, 65, 300} counts
    from k0 (the first n nodes and K counts of one reference block): T the sum of the absolute terms of g(z*) plus 1,
    c = _nb_ref.DEVICE_C and r_129 = _nb_ref.BAR_129, both from test_nb_cpu.py.  m uniform in [-6, 9], v from {0, -1, 1e-8, 3e-3,
    0.27, 1, 9, 26}, exposures in [0.5, 20] or none, r in {0.37, 8, 2^20}.  Every shape runs once with log_out on arrays one
    element off a 16-byte boundary and once without log_out on aligned ones.  Measured on the MI355X: the worst entry of the
    nine cases is at 0.013 of its bound (r = 2^20: 0.012, 0.001 without exposures, 0.013 from k0 = 1000; r = 0.37 and r = 8: 0.001
    and below)."""
    from manifold_gp_amd.counts import count_predict_pmf
    m, v, a = nb.gpu_inputs(max(NS), 300 + k0 + int(with_aux))
    a64 = a.astype(np.float64) if with_aux else np.zeros_like(m)
    k = k0 + np.arange(max(KCOUNTS), dtype=np.float64)
    want, bound_t, _, _, _ = nb.rule(m[:, None], v[:, None], a64[:, None], k[None, :], r, points=129, full=True)
    bound = nb.DEVICE_C * 2.0 ** -53 * bound_t + nb.BAR_129
    assert np.isfinite(want).all()
    worst = 0.0
    for n in NS:
        for K in KCOUNTS:
            w, b = want[:n, :K], bound[:n, :K]
            lp = count_predict_pmf(_off(m[:n], dev), _off(v[:n], dev), _off(a[:n], dev) if with_aux else None, NBF, k0, k0 + K - 1,
                                   points=129, log=True, dispersion=r)
            p = count_predict_pmf(T(m[:n], dev), T(v[:n], dev), T(a[:n], dev) if with_aux else None, NBF, k0, k0 + K - 1, points=129,
                                  dispersion=r)
            assert lp.shape == (n, K) and lp.dtype == torch.float64 and p.shape == (n, K) and p.dtype == torch.float64
            lp, p = lp.cpu().numpy(), p.cpu().numpy()
            assert np.isfinite(lp).all()
            err = np.abs(lp - w)
            assert (err <= b).all(), (n, K, (err / b).max())
            worst = max(worst, (err / b).max())
            seen = w > -700.0
            assert (p >= 0).all() and (np.abs(np.log(p[seen]) - w[seen]) <= b[seen] + 2.0 ** -52).all(), (n, K)
            assert (p[w < -750.0] == 0).all()
    print("r = %g k0 = %d aux %s: worst |log pmf - ref| is %.3f of its bound" % (r, k0, with_aux, worst))


@pytest.mark.parametrize("r", PMF_R)
def test_logpmf_is_the_matching_pmf_entry_nan_propagates_and_calls_repeat_bitwise(dev, mgp, r):
    """mgp_nb_predict_logpmf equals the entry y_i - k0 of row i of mgp_nb_predict_pmf with log_out bit for bit, with and without
    the mask; NaN outside the mask, NaN counts there tolerated; NaN in eta, var or y gives NaN; a second call of either entry is
    bitwise equal; aligned and one-element-off arrays give the same bits."""
    from manifold_gp_amd.counts import count_predict_logpmf, count_predict_pmf
    n, K = 257, 300
    rng = np.random.default_rng(3)
    kw = dict(dispersion=r)
    for k0 in (0, 1000):
        m, v, a = nb.gpu_inputs(n, 11 + k0)
        y = (k0 + rng.integers(0, K, n)).astype(np.float32)
        at = rng.random(n) < 0.5
        args = (T(m, dev), T(v, dev), T(a, dev))
        block = count_predict_pmf(*args, NBF, k0, k0 + K - 1, log=True, **kw)
        assert torch.equal(block, count_predict_pmf(*args, NBF, k0, k0 + K - 1, log=True, **kw))
        assert torch.equal(block, count_predict_pmf(_off(m, dev), _off(v, dev), _off(a, dev), NBF, k0, k0 + K - 1, log=True, **kw))
        want = block[torch.arange(n, device=dev), T((y - k0).astype(np.int64), dev)]
        every = count_predict_logpmf(*args, T(y, dev), None, NBF, **kw)
        assert every.dtype == torch.float64 and every.shape == (n,) and torch.equal(every, want)
        y_nan = np.where(at, y, np.float32(np.nan)).astype(np.float32)
        mask = T(at, dev)
        some = count_predict_logpmf(*args, T(y_nan, dev), mask, NBF, **kw)
        assert torch.equal(some[mask], want[mask]) and bool(torch.isnan(some[~mask]).all())
        off = count_predict_logpmf(_off(m, dev), _off(v, dev), _off(a, dev), _off(y_nan, dev), _off(at, dev), NBF, **kw)
        assert torch.equal(off[mask], want[mask]) and bool(torch.isnan(off[~mask]).all())
        unmasked = count_predict_logpmf(*args, T(y_nan, dev), None, NBF, **kw)               # NaN counts read: NaN out
        assert bool(torch.isnan(unmasked[~mask]).all()) and torch.equal(unmasked[mask], want[mask])
    m2, v2 = m.copy(), v.copy()
    m2[0], v2[1] = np.nan, np.nan
    block = count_predict_pmf(T(m2, dev), T(v2, dev), T(a, dev), NBF, 0, 69, **kw)
    assert bool(torch.isnan(block[:2]).all()) and bool(torch.isfinite(block[2:]).all())


# ------------------------------------------------------------------------------------------------ 3-6: the fit
_PROBLEMS = {}
CASE = "dumbbell_k10_loop"


def _problem(mgp, golden, dev, norm, nu, r=nb.R_TRUE):
    """One problem per (normalisation, nu) on dumbbell_k10_loop, built once: the descriptor scaled to the prior marginal variance
    _nb_ref.PRIOR_VARIANCE, the dense float64 matrix the kernels apply, the counts of _nb_ref.nb_counts; per dispersion the data
    and the dense float64 Newton iteration."""
    key = (norm, nu)
    if key not in _PROBLEMS:
        g = golden(CASE)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / nb.PRIOR_VARIANCE))
        c = nb.nb_counts(g)
        nan = lambda a: T(np.where(c["obs"], a, np.nan).astype(np.float32), dev)
        _PROBLEMS[key] = dict(g=g, desc=d1.with_(scale=scale), Q=scale * Q1, scale=scale, counts=c, y=nan(c["y"]), observed=T(c["obs"], dev),
                              E=T(c["E"], dev))
    base = _PROBLEMS[key]
    if r not in base:
        d = nb.data(base["counts"], r)
        f_ref, trace = nb.newton(base["Q"], d)
        base[r] = dict(base, d=d, f_ref=f_ref, trace=trace)
    return base[r]


def _fit(p, **kw):
    from manifold_gp_amd.counts import fit_counts
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        return fit_counts(p["desc"], p["y"], p["observed"], family=NBF, dispersion=p["d"]["r"], exposure=p["E"], **kw)


def _fitted(p):
    if "fit" not in p:
        p["fit"] = _fit(p)
    return p["fit"]


@pytest.mark.parametrize("norm, nu", [("symmetric", 2), ("symmetric", 1), ("randomwalk", 2), ("randomwalk", 1)])
def test_fit_matches_dense_float64_newton(mgp, golden, dev, norm, nu):
    """r = 2 on the overdispersed counts, 10 % of the nodes observed, exposures in [0.5, 20]: converged, max |f_hat - f_ref| <= 1e-4
    (the bar of the other fits), the log-likelihood with sum c(y, r) within 1e-6 relative of the restatement's at its own mode,
    s_ref and the default mean the reference's, the number of Newton steps that of the float32 simulation on the CPU +- 1.
    Measured on the MI355X: 5 steps, all full, in the four cases as in the simulation; mode 4.1e-7 .. 6.2e-7 (3.3e-7 .. 5.4e-7 for
    the random walk), log-likelihood <= 2.5e-9."""
    from manifold_gp_amd.counts import CountLaplaceFit, laplace_fit_negative_binomial
    p = _problem(mgp, golden, dev, norm, nu)
    fit = _fitted(p)
    d = p["d"]
    assert isinstance(fit, CountLaplaceFit) and fit.family == NBF and fit.dispersion == 2.0 and fit.mean.dtype == torch.float32
    f = fit.mean.double().cpu().numpy()
    err = np.abs(f - p["f_ref"]).max()
    lp = nb.log_likelihood(p["f_ref"], d)
    lerr = abs(fit.log_likelihood - lp) / abs(lp)
    _, _, steps, _ = nb.simulate(p["Q"], d)
    print("%s nu = %d: %d steps %s (simulation %d), max |f - f_ref| = %.2e, max |f| = %.2f, log-likelihood %.6f (relative error %.1e), "
          "CG iterations %s" % (norm, nu, fit.iterations, [h[2] for h in fit.history], steps, err, np.abs(f).max(), fit.log_likelihood, lerr,
                                [h[3] for h in fit.history]))
    assert fit.converged and err <= 1e-4 and lerr <= 1e-6
    assert fit.s_ref == d["s_ref"] and abs(fit.prior_mean - d["mean"]) <= 1e-14
    assert abs(fit.iterations - steps) <= 1
    obs = d["obs"]
    want = np.exp(d["aux"] + f + fit.prior_mean)
    assert np.abs(fit.map_mean().cpu().numpy()[obs] - want[obs]).max() <= 1e-6 * want[obs].max()
    if (norm, nu) == ("symmetric", 2):                    # the front with the dispersion as an argument is the same fit
        again = laplace_fit_negative_binomial(p["desc"], p["y"], 2.0, p["observed"], exposure=p["E"])
        assert torch.equal(again.mean, fit.mean) and again.log_likelihood == fit.log_likelihood


def test_posterior_pieces(mgp, golden, dev):
    """symmetric, nu = 2.  latent_variance(256) within 5 of its own standard errors of diag((Q2 + H)^-1) at every node, the ratio
    of the means within 2 % (the bar of test_gpu_counts.py); predict_mean against the closed form m = E exp(eta + v / 2),
    var = m + m^2 (e^v - 1) + m^2 e^v / r from that variance at 1e-12 relative; predict_interval and predict_exceedance against
    the quantiles and tail sums of the restatement's pmf at every 8th node (exact / 1e-12); the default kmax reaches everywhere;
    predict_log_density at the observed nodes is the pmf's entry.  Measured on the MI355X: 2.70 standard errors, ratio 1.0008;
    predict_mean 4.0e-16 and 6.9e-16; exceedance 1.2e-15."""
    p = _problem(mgp, golden, dev, "symmetric", 2)
    fit, d, r = _fitted(p), p["d"], 2.0
    f = fit.mean.double().cpu().numpy()
    n = f.shape[0]
    dense = np.diag(np.linalg.inv(p["Q"] + np.diag(nb.curvature(f, d))))
    var, se = fit.latent_variance(256, seed=5)
    z = np.abs(var.cpu().numpy() - dense) / se.cpu().numpy()
    ratio = float(var.mean()) / dense.mean()
    print("latent_variance(256): worst %.2f standard errors, ratio of the means %.4f, variances %.3g .. %.3g" % (z.max(), ratio, dense.min(), dense.max()))
    assert z.max() <= 5.0 and abs(ratio - 1.0) <= 0.02
    m, v, lv = fit.predict_mean(16, seed=5)
    assert torch.equal(lv, fit.latent_variance(16, seed=5)[0]) and m.dtype == torch.float64
    E, lvn = p["counts"]["E"], lv.cpu().numpy()
    want_m, want_v = nb.predict_mean(f + fit.prior_mean, lvn, E, r)
    em, ev = np.abs(m.cpu().numpy() - want_m) / want_m, np.abs(v.cpu().numpy() - want_v) / want_v
    print("predict_mean: worst relative error of the mean %.2e, of the variance %.2e" % (em.max(), ev.max()))
    assert (em <= 1e-12).all() and (ev <= 1e-12).all()
    sub = slice(0, None, 8)
    eta = (fit.eta() + fit.exposure.log()).cpu().numpy()                                       # as the fit hands it to the kernel
    k = np.arange(256, dtype=np.float64)
    ref = np.exp(nb.rule(eta[sub, None], lvn[sub, None], 0.0, k[None, :], r))
    cdf = np.cumsum(ref, axis=1)
    thr = np.random.default_rng(4).integers(0, 256, n)
    for threshold, want in ((10, 1.0 - cdf[:, 10]), (T(thr, dev), 1.0 - cdf[np.arange(ref.shape[0]), thr[sub]])):
        got = fit.predict_exceedance(threshold, variance=lv).cpu().numpy()
        assert (got >= 0).all() and (got <= 1).all()
        err = np.abs(got[sub] - np.maximum(want, 0.0)).max()
        print("exceedance: worst error %.2e" % err)
        assert err <= 1e-12
    for level in (0.9, 0.5):
        lo, hi, reached = fit.predict_interval(level, kmax=255, variance=lv)
        wl, wh, wr = pref.quantiles(ref, level)
        assert np.array_equal(lo.cpu().numpy()[sub], wl) and np.array_equal(hi.cpu().numpy()[sub], wh)
        assert np.array_equal(reached.cpu().numpy()[sub], wr) and bool((hi[~reached] == -1).all())
    lo, hi, reached = fit.predict_interval(0.9, variance=lv)                                   # the default block
    assert bool(reached.all()) and bool((hi >= lo).all())
    obs = d["obs"]
    ld = fit.predict_log_density(p["y"], at=p["observed"], variance=lv).cpu().numpy()
    assert np.isfinite(ld[obs]).all() and np.isnan(ld[~obs]).all()
    want = nb.rule(eta[obs], lvn[obs], 0.0, d["y"][obs], r)
    assert abs(ld[obs].sum() - want.sum()) <= 1e-9 * abs(want.sum())
    x = fit.latent_samples(64, seed=9)
    assert x.shape == (64, n) and bool(torch.isfinite(x).all())


def _q_of(p, kappa=None, scale=None, nu=2):
    """the dense matrix of the symmetric problem at another length scale or output scale: Q / scale = (tau I + L)^nu, by the
    eigendecomposition of the device's own matrix"""
    if "eig" not in p:
        w, U = np.linalg.eigh(p["Q"] / p["scale"])
        p["eig"] = (w ** (1.0 / nu) - 2.0 * nu / float(np.float32(p["g"]["kappa"])) ** 2, U)
    lam, U = p["eig"]
    kappa = float(np.float32(p["g"]["kappa"])) if kappa is None else kappa
    Q = (p["scale"] if scale is None else scale) * (U * (2.0 * nu / kappa ** 2 + lam) ** nu) @ U.T
    return 0.5 * (Q + Q.T)


def test_evidence_and_its_gradient(mgp, golden, dev):
    """symmetric, nu = 2, m = 149 observed nodes: method "dense", exact up to the solves.  The value against the dense float64
    evidence at the device's mode at the bars of test_gpu_evidence.py (log-likelihood and quad 1e-6 relative, logdet B DENSE_BAR).
    The gradient with respect to length scale and output scale, given probes and variance = the dense diag(A^-1), against central
    differences of the dense float64 evidence with the mode re-fitted: the probe term is an estimate, so the bar is 5 of its
    standard errors (from exact float64 solves with the same probes) plus the operator-level 2e-3 relative of test_gpu_evidence.py;
    the float64 analytic gradient agrees with the central differences to 1e-5 relative.  Measured on the MI355X: logdet B
    1.43e-8 relative; length scale 132.15 against 135.13 (standard error 5.88), output scale -110409 against -111918 (7.56e3)."""
    import _evidence_ref as eref
    O = mgp.operators
    p = _problem(mgp, golden, dev, "symmetric", 2)
    fit, d, g, Q, nu = _fitted(p), p["d"], p["g"], p["Q"], 2
    f = fit.mean.double().cpu().numpy()
    z = nb.log_z(Q, f, d)
    ev = fit.evidence()
    e_ld, e_ll, e_q = abs(ev.logdet - z["logdet"]) / z["logdet"], abs(ev.log_likelihood - z["log_likelihood"]) / abs(z["log_likelihood"]), \
        abs(ev.quad - z["quad"]) / z["quad"]
    print("evidence: m = %d, log Z dense %.5f, device %.5f; logdet relative %.2e, log-likelihood %.1e, quad %.1e"
          % (ev.m, z["value"], float(ev.value), e_ld, e_ll, e_q))
    assert ev.method == "dense" and ev.m == z["m"] <= 512 and ev.se == 0.0
    assert e_ld <= DENSE_BAR and e_ll <= 1e-6 and e_q <= 1e-6
    assert abs(float(ev.value) - z["value"]) <= 1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * DENSE_BAR * z["logdet"]
    # the gradient
    theta = [float(np.float32(v)) for v in (float(g["eps"]), float(g["kappa"]), p["scale"])]
    th = [torch.tensor(v, device=dev, requires_grad=True) for v in theta]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    lap = O.GraphLaplacianOperator(val, idx, p["desc"].n, th[0].view(1, 1), "symmetric", bool(g["self_loops"]))
    op = O.ScaleWrapperOperator(O.PrecisionMaternOperator(lap, nu, th[1]), th[2])
    f_ref = p["f_ref"]                                    # the float64 mode: what the central differences re-fit from
    _, _, h, hp, _ = nb.site(f_ref, d["y"], d["aux"], d["obs"], d["mean"], d["r"])
    Ai, Qi = np.linalg.inv(Q + np.diag(h)), np.linalg.inv(Q)
    eff = d["obs"] & (h >= eref.H_FLOOR)
    Z = eref.probes(eff, 16, 4321)
    evg = fit.evidence(operator=op, variance=T(np.diag(Ai), dev), probes=T(Z.astype(np.float32), dev), solve_tol=1e-6)
    assert evg.value.requires_grad
    got = [float(x) for x in torch.autograd.grad(evg.value, th)]
    u = Ai @ (np.diag(Ai) * hp)
    SZ = np.sqrt(h)[:, None] * Z
    for name, got_i, t0, make in (("kappa", got[1], theta[1], lambda t: _q_of(p, kappa=t)), ("outputscale", got[2], theta[2], lambda t: _q_of(p, scale=t))):
        step = 1e-4 * t0
        zs = [nb.mode_log_z(make(t), d, f0=f_ref)[1]["value"] for t in (t0 + step, t0 - step)]
        cd = (zs[0] - zs[1]) / (2 * step)
        dQ = (make(t0 + step) - make(t0 - step)) / (2 * step)
        analytic = -0.5 * float(f_ref @ (dQ @ f_ref)) + 0.5 * float(u @ (dQ @ f_ref)) + 0.5 * float(np.sum((Qi - Ai) * dQ))
        per = 0.5 * np.einsum("ip,ip->p", Qi @ SZ, dQ @ (Ai @ SZ))
        se = float(per.std(ddof=1) / 4.0)
        print("d log Z / d %s: device %.6g, central difference %.6g, float64 analytic %.6g, probe standard error %.3g"
              % (name, got_i, cd, analytic, se))
        assert abs(analytic - cd) <= 1e-5 * abs(cd) + 1e-4 * se
        assert abs(got_i - cd) <= 5.0 * se + 2e-3 * abs(cd), (name, got_i, cd, se)


def test_dispersion_profile_finds_the_reference_argmax(mgp, golden, dev):
    """dispersion_profile over r in {0.5, 1, 2, 4, 16, 2^20}: every value within the bar of test_gpu_evidence.py's dense comparison,
    1e-6 (|log-likelihood| + quad) + DENSE_BAR logdet / 2, of the dense float64 evidence at the device's mode; the argmax that of
    those dense values and the reference's, r = 2 (test_nb_cpu.py checks its separation from the runner-up: 5.2 against bars of
    7e-4).  Measured on the MI355X: the worst value at 0.002 of its bar; 5, 4, 3, 3, 3, 4 Newton steps from the warm starts."""
    from manifold_gp_amd.counts import dispersion_profile
    p = _problem(mgp, golden, dev, "symmetric", 2)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        results, best = dispersion_profile(p["desc"], p["y"], nb.PROFILE, observed=p["observed"], exposure=p["E"])
    vals, worst = [], 0.0
    for (r, fit, ev), want_r in zip(results, nb.PROFILE):
        d = nb.data(p["counts"], r)
        z = nb.log_z(p["Q"], fit.mean.double().cpu().numpy(), d)
        vals.append(z["value"])
        bar = 1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * DENSE_BAR * z["logdet"]
        worst = max(worst, abs(float(ev.value) - z["value"]) / bar)
        assert r == want_r and fit.dispersion == r and fit.converged and ev.method == "dense"
        assert abs(float(ev.value) - z["value"]) <= bar, (r, float(ev.value), z["value"])
    print("profile: device %s, dense %s, worst %.3f of the bar; Newton steps %s"
          % (["%.3f" % float(e.value) for _, _, e in results], ["%.3f" % v for v in vals], worst, [f.iterations for _, f, _ in results]))
    assert best == int(np.argmax(vals)) and nb.PROFILE[best] == nb.R_TRUE


def test_model_methods_pass_the_dispersion(mgp, golden, dev):
    from manifold_gp_amd.counts import fit_counts
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    g = golden(CASE)
    c = nb.nb_counts(g)
    x = T(g["train_x"], dev)
    y, obs, E = T(np.where(c["obs"], c["y"], np.nan).astype(np.float32), dev), T(c["obs"], dev), T(c["E"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev)).to(dev)
    desc = model.precision(noise=False)._descriptor()
    fit = model.laplace_posterior_counts(observed=obs, family=NBF, dispersion=2.0, exposure=E)
    want = fit_counts(desc, y, obs, family=NBF, dispersion=2.0, exposure=E)
    assert fit.converged and fit.family == NBF and torch.equal(fit.mean, want.mean) and fit.log_likelihood == want.log_likelihood
    ev = model.laplace_evidence(observed=obs, family=NBF, dispersion=2.0, exposure=E)
    assert abs(float(ev.value) - float(want.evidence().value)) <= 1e-6 * abs(float(ev.value))
    with pytest.raises(ValueError, match="needs dispersion"):
        model.laplace_posterior_counts(observed=obs, family=NBF)
    with pytest.raises(ValueError, match="dispersion belongs"):
        model.laplace_evidence(observed=obs, family="poisson", dispersion=2.0, exposure=E)


def test_coincident_points(mgp, dev):
    """On dumbbell_dup the negative-binomial fit applies and solves only: the mode is within 1e-4 of the dense float64 iteration;
    latent_variance refuses with the ValueError of the other fits.  Measured on the MI355X: 5 steps, 1.9e-6."""
    from manifold_gp_amd.counts import fit_counts
    from test_gpu_coincident import REFUSAL, _graph, _precision, _q2
    g, graph = _graph(mgp, dev, "dumbbell_dup")
    assert graph.self_edges > 0
    Q1 = _q2(g, "symmetric", 2, 1.0)
    scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / nb.PRIOR_VARIANCE))
    desc, Q = _precision(mgp, dev, "dumbbell_dup", "symmetric", 2, scale), scale * Q1
    c = nb.nb_counts(g)
    d = nb.data(c, nb.R_TRUE)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        fit = fit_counts(desc, T(np.where(c["obs"], c["y"], np.nan).astype(np.float32), dev), T(c["obs"], dev), family=NBF,
                         dispersion=nb.R_TRUE, exposure=T(c["E"], dev))
    err = np.abs(fit.mean.double().cpu().numpy() - nb.newton(Q, d)[0]).max()
    print("coincident negative-binomial fit: %d steps, max |f - f_ref| = %.2e" % (fit.iterations, err))
    assert fit.converged and err <= 1e-4
    with pytest.raises(ValueError, match=REFUSAL):
        fit.latent_variance(8, seed=1)
