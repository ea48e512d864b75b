"""The predictive count pmf on the MI355X (csrc/count_predict.hip, CountLaplaceFit.predict_pmf / predict_log_density /
predict_exceedance / predict_interval): both kernels against the float64 restatement of their rule (tests/_count_pmf_ref.py) at
edge shapes, mgp_count_predict_logpmf against the matching entries of mgp_count_predict_pmf bit for bit, repeated calls, the
grid-stride loops past the grid caps, and the fit's methods end to end on the dumbbell (docs/kernels/count_predict.md)."""
import math

import numpy as np
import pytest
import torch

import _count_pmf_ref as R
from test_gpu_counts import _fitted, _problem
from test_gpu_variance import T

pytestmark = pytest.mark.gpu

FAMILIES = ["poisson", "binomial"]
NS = [1, 3, 64, 65, 257]
KCOUNTS = [1, 2, 63, 64, 65, 300]
PMF_GRID_CAP, LOGPMF_GRID_CAP = 2048 * 4, 2048 * 256      # waves / threads of the capped grids (csrc/count_predict.hip)


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
    """a device copy of `a` one element off a 16-byte boundary (a view into a larger buffer)"""
    t = T(np.concatenate([a[:1], a]), dev)[1:]
    assert t.data_ptr() % 16 == a.itemsize
    return t


# ------------------------------------------------------------------------------------------------ 1: the kernels
CASES = [("poisson", 0, True), ("poisson", 0, False), ("poisson", 1000, True), ("binomial", 0, True), ("binomial", 1000, True)]


@pytest.mark.parametrize("family, k0, with_aux", CASES)
def test_pmf_kernel_matches_the_restatement(dev, mgp, family, k0, with_aux):
    """|log pmf_dev - log pmf_ref| <= c 2^-53 T + r at P = 129 for n in {1, 3, 64, 65, 257} x K in {1, 2, 63, 64, 65, 300} counts
    from k0 (the first n nodes and K counts of one reference block): T the sum of the absolute terms of g(eta*) plus 1, c = 44
    (4 x the 11 of the restatement against its own long-double evaluation, test_count_pmf_cpu.py), r = 6.0e-10 (4 x the rule's
    1.5e-10 at P = 129).  m uniform in [-6, 9], v from {0, -1, 1e-8, 3e-3, 0.27, 1, 9, 26}, exposures in [0.5, 20] or none,
    trials from {1, 2, 39, 1000, 65535}; -inf exactly where k > N.  Every shape runs once with log_out on arrays one element off
    a 16-byte boundary and once without log_out on aligned ones.  Measured on the MI355X: the worst entry of the five cases is at
    0.033 of its bound (Poisson 0.017, 0.001 without exposures, 0.016 from k0 = 1000; binomial 0.033 both)."""
    from manifold_gp_amd.counts import count_predict_pmf
    fam = FAMILIES.index(family)
    m, v, a = R.gpu_inputs(fam, max(NS), 100 * fam + k0 + int(with_aux))
    a64 = a.astype(np.float64) if with_aux else np.zeros_like(m)
    k = k0 + np.arange(max(KCOUNTS), dtype=np.float64)
    want, bound_t, _, _, _ = R.rule(fam, m[:, None], v[:, None], a64[:, None], k[None, :], points=129, full=True)
    bound = R.DEVICE_C * 2.0 ** -53 * bound_t + R.BAR_129
    neg = np.isneginf(want)
    assert not np.isnan(want).any() and (fam == 0 or neg.any())
    worst = 0.0
    for n in NS:
        for K in KCOUNTS:
            w, b, gone = want[:n, :K], bound[:n, :K], neg[:n, :K]
            aux_off = _off(a[:n], dev) if with_aux else None
            aux_on = T(a[:n], dev) if with_aux else None
            lp = count_predict_pmf(_off(m[:n], dev), _off(v[:n], dev), aux_off, family, k0, k0 + K - 1, points=129, log=True)
            p = count_predict_pmf(T(m[:n], dev), T(v[:n], dev), aux_on, family, k0, k0 + K - 1, points=129)
            assert lp.shape == (n, K) and lp.dtype == torch.float64 and p.shape == (n, K) and p.dtype == torch.float64
            lp, p = lp.cpu().numpy(), p.cpu().numpy()
            assert np.array_equal(np.isneginf(lp), gone) and (p[gone] == 0).all() and not np.isnan(lp).any()
            err = np.abs(lp - w)[~gone]
            assert (err <= b[~gone]).all(), (n, K, (err / b[~gone]).max())
            worst = max(worst, (err / b[~gone]).max() if err.size else 0.0)
            seen = ~gone & (w > -700.0)                                 # the pmf itself where it is a normal number
            errp = np.abs(np.log(p[seen]) - w[seen])
            assert (p >= 0).all() and (errp <= b[seen] + 2.0 ** -52).all(), (n, K)
            assert (p[~gone & (w < -750.0)] == 0).all()
    print("%s k0 = %d aux %s: worst |log pmf - ref| is %.3f of its bound" % (family, k0, with_aux, worst))


@pytest.mark.parametrize("family", FAMILIES)
def test_logpmf_is_the_matching_pmf_entry_and_calls_repeat_bitwise(dev, mgp, family):
    """mgp_count_predict_logpmf equals the entry y_i - k0 of row i of mgp_count_predict_pmf with log_out bit for bit, with and
    without the mask; NaN outside the mask, NaN counts there tolerated; a second call of either entry is bitwise equal; aligned
    and one-element-off arrays give the same bits."""
    from manifold_gp_amd.counts import count_predict_logpmf, count_predict_pmf
    fam = FAMILIES.index(family)
    n, K = 257, 300
    rng = np.random.default_rng(3)
    for k0 in (0, 1000):
        m, v, a = R.gpu_inputs(fam, n, 11 + k0)
        y = (k0 + rng.integers(0, K, n)).astype(np.float32)
        at = rng.random(n) < 0.5
        args = (T(m, dev), T(v, dev), T(a, dev))
        block = count_predict_pmf(*args, family, k0, k0 + K - 1, log=True)
        assert torch.equal(block, count_predict_pmf(*args, family, k0, k0 + K - 1, log=True))
        assert torch.equal(block, count_predict_pmf(_off(m, dev), _off(v, dev), _off(a, dev), family, k0, k0 + K - 1, log=True))
        want = block[torch.arange(n, device=dev), T((y - k0).astype(np.int64), dev)]
        every = count_predict_logpmf(*args, T(y, dev), None, family)
        assert every.dtype == torch.float64 and every.shape == (n,)
        assert torch.equal(every, want)
        y_nan = np.where(at, y, np.float32(np.nan)).astype(np.float32)
        some = count_predict_logpmf(*args, T(y_nan, dev), T(at, dev), family)
        mask = T(at, dev)
        assert torch.equal(some[mask], want[mask]) and bool(torch.isnan(some[~mask]).all())
        assert torch.equal(some[mask], count_predict_logpmf(*args, T(y_nan, dev), mask, family)[mask])
        off = count_predict_logpmf(_off(m, dev), _off(v, dev), _off(a, dev), _off(y_nan, dev), _off(at, dev), family)
        assert torch.equal(off[mask], want[mask]) and bool(torch.isnan(off[~mask]).all())


def test_grid_stride_loops_past_the_grid_caps(dev, mgp):
    """More (node, 64-count chunk) tasks than waves in the capped grid (9 nodes x 1024 chunks > 8192), and more nodes than
    threads in the capped grid of the logpmf kernel: the later sweeps give the bits of calls that fit in one sweep."""
    from manifold_gp_amd.counts import count_predict_logpmf, count_predict_pmf
    n, K = 9, 65536
    assert n * (K // 64) > PMF_GRID_CAP >= 8 * (K // 64)
    m, v, a = R.gpu_inputs(0, n, 21)
    m, v, a = T(m, dev), T(v, dev), T(a, dev)
    block = count_predict_pmf(m, v, a, "poisson", 0, K - 1, log=True)
    for i in (0, 8):
        assert torch.equal(block[i:i + 1], count_predict_pmf(m[i:i + 1], v[i:i + 1], a[i:i + 1], "poisson", 0, K - 1, log=True))
    assert bool(torch.isfinite(block).all())
    n = LOGPMF_GRID_CAP + 300
    m, v, a = R.gpu_inputs(1, n, 22)
    y = np.random.default_rng(23).integers(0, 3, n).astype(np.float32)
    m, v, a, y = T(m, dev), T(v, dev), T(a, dev), T(y, dev)
    out = count_predict_logpmf(m, v, a, y, None, "binomial")
    for s in (slice(0, 1000), slice(n - 1000, n)):
        assert torch.equal(out[s], count_predict_logpmf(m[s], v[s], a[s], y[s], None, "binomial"))
    assert not bool(torch.isnan(out).any())


# ------------------------------------------------------------------------------------------------ 2: the fit's methods
KMAX = 2048
SUBSET = slice(0, None, 8)                   # the nodes whose rows are restated on the CPU


def _normal_tail(z):
    return 0.5 * math.erfc(z / math.sqrt(2.0))


@pytest.mark.parametrize("family", FAMILIES)
def test_predictive_distribution_end_to_end(mgp, golden, dev, family):
    """dumbbell_k50_noloop, symmetric, nu = 2, with a given latent variance (latent_variance(16, seed = 5)).
    predict_pmf (P = 129) rows sum to 1 within 1e-9 at every binomial node (block 0 .. max trials) and at the Poisson nodes whose
    mass and mean beyond kmax = 2048 are negligible; there sum k pmf agrees with predict_mean's mean (E exp(eta + v / 2), the same
    latent variance) to 1e-8 relative.  The plain selection -- closed-form mean + 12 standard deviations below kmax -- is necessary
    but not sufficient: the rate is log-normal, and at v = 9 a node with mean 1.9 passes it while 7e-5 of its mass and a tenth of
    its mean lie beyond 2048 (the rule is right there: the deficit is the tail).  So a node must also have
    P(z > z0 - sqrt(v)) <= 1e-10, z0 = (log(kmax - 12 sqrt(kmax)) - eta - log E) / sqrt(v): the share of the mean carried by rates
    above kmax - 12 sqrt(kmax).  Measured on the MI355X: 156 of the 1546 nodes pass the first selection and 151 of them the
    second; there |sum - 1| <= 2.8e-14 and the mean is within 2.9e-14 (binomial: |sum - 1| <= 1.4e-14 at all 1546 nodes); over the
    156 alone the worst deficits are 6.3e-9 and 1.7e-5, under those nodes' tail bound of 4.0e-5.  At every node the sum is at
    most 1 + 1e-9.
    predict_exceedance and predict_interval (P = 65, block 0 .. 255) against numpy cumulative sums of the restatement's pmf at
    every 8th node: lo, hi, reached exactly, the exceedance to 1e-12; reached is False somewhere at kmax = 255 (Poisson).
    predict_log_density at the observed nodes with their own counts: finite, NaN elsewhere, its sum within 1e-9 relative of
    the restatement's."""
    p = _problem(mgp, golden, dev, "dumbbell_k50_noloop", "symmetric", 2, family)
    fit = _fitted(p)
    fam = FAMILIES.index(family)
    n = p["desc"].n
    var = fit.latent_variance(16, seed=5)[0]
    eta, v = fit.eta().cpu().numpy(), var.cpu().numpy()
    obs = p["d"]["obs"]
    if fam == 0:
        E = fit.exposure.cpu().numpy()
        log_e = fit.exposure.log().cpu().numpy()
        eta, a = eta + log_e, np.zeros_like(eta)      # the fit adds the log-exposure to eta in float64 and passes no aux
        kmax = KMAX
    else:
        a = fit.trials.cpu().numpy()
        kmax = int(a.max())
    # the pmf block: normalisation and mean
    pmf, used = fit.predict_pmf(kmax, points=129, variance=var)
    assert pmf.shape == (n, kmax + 1) and pmf.dtype == torch.float64 and torch.equal(used, var)
    again, _ = fit.predict_pmf(kmax, points=129, variance=var)
    assert torch.equal(pmf, again)
    logs, _ = fit.predict_pmf(kmax, points=129, variance=var, log=True)
    assert torch.equal(torch.exp(logs) > 0, pmf > 0)
    pmf = pmf.cpu().numpy()
    total = pmf.sum(1)
    assert (pmf >= 0).all() and (total <= 1.0 + 1e-9).all()
    if fam == 1:
        print("binomial: latent variances %.3g .. %.3g, worst |sum - 1| = %.2e over %d nodes" % (v.min(), v.max(), np.abs(total - 1).max(), n))
        assert (np.abs(total - 1.0) <= 1e-9).all()
        assert (pmf[np.arange(kmax + 1)[None, :] > a[:, None]] == 0).all()
    else:
        m_fit, _, v_fit = fit.predict_mean(16, seed=5)
        assert torch.equal(v_fit, var)                                               # the same latent variance
        mean = m_fit.cpu().numpy()
        assert np.abs(mean - E * np.exp(fit.eta().cpu().numpy() + 0.5 * v)).max() <= 1e-12 * mean.max()
        sd = np.sqrt(mean + mean * mean * np.expm1(v))
        plain = mean + 12.0 * sd < kmax
        z0 = (math.log(kmax - 12.0 * math.sqrt(kmax)) - eta) / np.sqrt(np.maximum(v, 1e-300))
        tail = np.array([_normal_tail(z - s) for z, s in zip(z0, np.sqrt(np.maximum(v, 0.0)))])
        sel = plain & (tail <= 1e-10)
        merr = np.abs((pmf * np.arange(kmax + 1)[None, :]).sum(1) - mean) / mean
        print("poisson: %d of %d nodes have mean + 12 sd < %d, %d of them a negligible tail; there worst |sum - 1| = %.2e, worst "
              "relative error of the mean %.2e; latent variances %.3g .. %.3g, means %.3g .. %.3g"
              % (plain.sum(), n, kmax, sel.sum(), np.abs(total - 1)[sel].max(), merr[sel].max(), v.min(), v.max(), mean.min(), mean.max()))
        print("over the %d nodes of the first selection alone: worst |sum - 1| = %.2e, worst relative error of the mean %.2e, "
              "largest tail bound %.1e" % (plain.sum(), np.abs(total - 1)[plain].max(), merr[plain].max(), tail[plain].max()))
        assert sel.sum() >= 1
        assert (np.abs(total - 1.0)[sel] <= 1e-9).all()
        assert (merr[sel] <= 1e-8).all()
    # exceedance and intervals against the restatement at every 8th node
    low = 255 if fam == 0 else kmax
    k = np.arange(low + 1, dtype=np.float64)
    ref = np.exp(R.rule(fam, eta[SUBSET, None], v[SUBSET, None], a[SUBSET, None], k[None, :]))
    thr = np.random.default_rng(4).integers(0, low + 1, n)
    cdf = np.cumsum(ref, axis=1)
    for threshold, want in ((10, 1.0 - cdf[:, 10]), (T(thr, dev), 1.0 - cdf[np.arange(ref.shape[0]), thr[SUBSET]])):
        got = fit.predict_exceedance(threshold, variance=var)
        assert got.dtype == torch.float64 and got.shape == (n,)
        got = got.cpu().numpy()
        assert (got >= 0).all() and (got <= 1).all()
        err = np.abs(got[SUBSET] - np.maximum(want, 0.0)).max()
        print("%s exceedance: worst error %.2e" % (family, err))
        assert err <= 1e-12
    for level in (0.9, 0.5):
        lo, hi, reached = fit.predict_interval(level, kmax=low, variance=var)
        assert lo.dtype == torch.int64 and hi.dtype == torch.int64 and reached.dtype == torch.bool
        wl, wh, wr = R.quantiles(ref, level)
        assert np.array_equal(lo.cpu().numpy()[SUBSET], wl) and np.array_equal(hi.cpu().numpy()[SUBSET], wh)
        assert np.array_equal(reached.cpu().numpy()[SUBSET], wr)
        assert bool((hi[reached] >= lo[reached]).all()) and bool((hi[~reached] == -1).all())
        print("%s level %g: reached at %d of %d nodes, widest interval %d" % (family, level, int(reached.sum()), n, int((hi - lo).max())))
        if fam == 0:
            assert not bool(reached.all()) and bool(reached.any())
        else:
            assert bool(reached.all())
            d_lo, d_hi, d_reached = fit.predict_interval(level, variance=var)          # the default block: 0 .. max trials
            assert torch.equal(d_lo, lo) and torch.equal(d_hi, hi) and torch.equal(d_reached, reached)
    # the log density of the observed counts
    y = p["y"]                                                                          # NaN at the unobserved nodes
    ld = fit.predict_log_density(y, at=p["observed"], variance=var)
    assert ld.dtype == torch.float64 and ld.shape == (n,)
    ld = ld.cpu().numpy()
    assert np.isfinite(ld[obs]).all() and np.isnan(ld[~obs]).all()
    want = R.rule(fam, eta[obs], v[obs], a[obs], p["d"]["y"][obs].astype(np.float64))
    rel = abs(ld[obs].sum() - want.sum()) / abs(want.sum())
    print("%s log density of the %d observed counts: %.6f, relative error %.1e" % (family, obs.sum(), ld[obs].sum(), rel))
    assert rel <= 1e-9
    pmf_at = fit.predict_pmf(kmax, variance=var, log=True)[0].cpu().numpy()
    inside = obs & (p["d"]["y"] <= kmax)
    assert np.array_equal(ld[inside], pmf_at[inside, p["d"]["y"][inside].astype(np.int64)])   # the same device function
