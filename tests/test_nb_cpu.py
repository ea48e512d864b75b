"""The negative-binomial count family, host side (no GPU): the float64 restatement the GPU tests are checked against
(tests/_nb_ref.py) is itself checked -- the site against central differences and at extreme latents, c(k, r) against mpmath, the
pmf rule against a brute-force rule and against its own long-double evaluation (the two constants of the device bar), the Poisson
limit, normalisation and mean, the dense evidence's gradient and the separation of the dispersion profile -- and the Python and
C-ABI argument checks (docs/kernels/counts.md, count_predict.md, evidence.md)."""
import ctypes
import inspect
import math
import os
import types

import numpy as np
import pytest
import torch

import _count_pmf_ref as pref
import _counts_ref as cref
import _nb_ref as nb
import _observed_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = [2.0 ** -10, 1.0, 2.0 ** 20]
_Q = {}


def _precision(golden, case, norm, nu):
    """The fixture's precision scaled to the prior marginal variance _nb_ref.PRIOR_VARIANCE, as test_counts_cpu.py does to 9."""
    key = (case, norm, nu)
    if key not in _Q:
        g = golden(case)
        Q1, _ = oref.precision_root(oref.oracle(g, norm), nu, float(g["kappa"]), 1.0, norm)
        _Q[key] = (np.diag(np.linalg.inv(Q1)).mean() / nb.PRIOR_VARIANCE) * Q1
    return _Q[key]


# ------------------------------------------------------------------------------------------------ the site
@pytest.mark.parametrize("r", [0.37, 2.0, 1000.0])
def test_reference_site_matches_central_differences(golden, r):
    """l, g, h and h' of the restatement against central differences, at the tolerances of test_counts_cpu.py (h' at that of h)."""
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    d = nb.data(nb.nb_counts(golden("dumbbell_k10_loop")), r)
    rng = np.random.default_rng(3)
    f = 0.5 * rng.standard_normal(Q.shape[0])
    grad = nb.gradient(Q, f, d)
    eps = 1e-5
    obs = d["obs"]
    for i in list(np.flatnonzero(obs)[:5]) + list(np.flatnonzero(~obs)[:5]):
        e = np.zeros_like(f)
        e[i] = eps
        fd = (nb.psi(Q, f + e, d) - nb.psi(Q, f - e, d)) / (2 * eps)
        assert abs(fd - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])) + 4 * 2.0 ** -52 * abs(nb.psi(Q, f, d)) / eps, (i, fd, grad[i])
    args = (d["y"], d["aux"], obs, d["mean"], r)
    plus, minus, mid = nb.site(f + eps, *args), nb.site(f - eps, *args), nb.site(f, *args)
    l, g, h, hp, mass = mid
    assert (np.abs((plus[0] - minus[0]) / (2 * eps) - g) <= 1e-6 * np.maximum(1.0, np.abs(g))).all()
    assert (np.abs(-(plus[1] - minus[1]) / (2 * eps) - h) <= 1e-8 * np.maximum(1.0, h)).all()
    assert (np.abs((plus[2] - minus[2]) / (2 * eps) - hp) <= 1e-8 * np.maximum(1.0, h)).all()
    assert (h[obs] > 0).all() and (h <= mass / 4).all() and (h[~obs] == 0).all()
    # pi = mu / (r + mu): the textbook gradient (y - mu) r / (r + mu)
    mu = np.exp(f + d["mean"] + d["aux"])
    assert np.abs(g - np.where(obs, (d["y"] - mu) * r / (r + mu), 0.0)).max() <= 1e-12 * (d["y"][obs].max() + r)


@pytest.mark.parametrize("r", RS)
def test_reference_site_is_finite_at_extreme_latents(r):
    fs, ys = [1e4, -1e4, 88.0, -90.0, 0.0], [0.0, 1.0, 2.0 ** 24]
    f = np.repeat(fs, len(ys)).astype(np.float32)
    y = np.tile(ys, len(fs)).astype(np.float32)
    qf = np.linspace(-2.0, 2.0, f.shape[0]).astype(np.float32)
    for aux in (None, np.full(f.shape, np.float32(math.log(20.0)))):
        w, rhs, sums, _, _ = nb.site_outputs(f, qf, y, aux, None, 2.0 ** -23, 0.0, r)
        assert np.isfinite(w).all() and np.isfinite(rhs).all() and np.isfinite(sums).all()        # no saturation: h <= (y + r) / 4
        assert (w <= 1.0).all() and (w[:6] == 0).all()
        root, corr, esums, _, eff = nb.evidence_outputs(f, y, aux, None, np.full(f.shape, 9.0), 0.0, r)
        assert np.isfinite(root).all() and np.isfinite(corr).all() and np.isfinite(esums).all()
    l = nb.site(f, y, None, None, 0.0, r)[0]
    assert l[0] == -r * (1e4 - math.log(r))                                                    # y = 0 at z = 1e4 - log r: -r z


# ------------------------------------------------------------------------------------------------ c(k, r)
CONST_R = [2.0 ** -10, 0.37, 1.0, 8.0, 1000.0, 2.0 ** 20]
CONST_K = [0, 1, 3, 31, 32, 1000, 2 ** 24]


def test_log_constant_against_mpmath():
    """|c - c_mpmath| <= 8 * 2^-53 (1 + |c| + k |log r| + k) on r in {2^-10, 0.37, 1, 8, 1000, 2^20} x k in {0, 1, 3, 31, 32, 1000,
    2^24}, mpmath at 30 digits.  Measured: the worst entry is at 0.771 of 2^-53 (1 + |c| + k |log r| + k), a tenth of the bar
    (r = 1000, k = 32); c(k, 1) is exactly 0 for k < 32 and c(0, r) exactly 0.  The torch form of counts.nb_log_constant agrees
    with the restatement to 1e-14 of the same scale."""
    import mpmath
    from manifold_gp_amd.counts import nb_log_constant
    mpmath.mp.dps = 30
    worst, where = 0.0, None
    for r in CONST_R:
        got, _ = nb.log_const(np.array(CONST_K, np.float64), r)
        tor = nb_log_constant(torch.tensor(CONST_K, dtype=torch.float64), r).numpy()
        for k, c, ct in zip(CONST_K, got, tor):
            want = mpmath.loggamma(mpmath.mpf(k) + mpmath.mpf(r)) - mpmath.loggamma(mpmath.mpf(r)) - mpmath.loggamma(k + 1)
            scale = 1.0 + abs(float(want)) + k * abs(math.log(r)) + k
            err = abs(float(mpmath.mpf(float(c)) - want)) / (2.0 ** -53 * scale)
            if err > worst:
                worst, where = err, (r, k)
            assert abs(ct - c) <= 1e-14 * scale, (r, k, ct, c)
        assert got[0] == 0.0
    assert (nb.log_const(np.arange(32.0), 1.0)[0] == 0.0).all()
    print("c(k, r): worst error %.3f x 2^-53 (1 + |c| + k |log r| + k) at (r, k) = %s" % (worst, where))
    assert worst <= 8.0
    assert worst <= nb.MEASURED_CONST <= 8.0


def test_log_constant_long_double_agrees():
    """the long-double evaluation of the same form (what the rounding constant of the device bar is measured against) agrees
    with the float64 one to 8 * 2^-53 of the same scale"""
    for r in CONST_R:
        k = np.array(CONST_K, np.float64)
        a, _ = nb.log_const(k, r)
        b, _ = nb.log_const(k, r, np.longdouble)
        scale = 1.0 + np.abs(a) + k * abs(math.log(r)) + k
        assert (np.abs(a - b.astype(np.float64)) <= 8 * 2.0 ** -53 * scale).all(), r


# ------------------------------------------------------------------------------------------------ the pmf rule
KS = [0, 1, 40, 1000, 60000]
VS = [1e-8, 3e-3, 0.27, 1.0, 9.0, 26.0]                 # the v values of test_count_pmf_cpu.py
PMF_R = [0.37, 1.0, 8.0, 2.0 ** 20]
CONFIGS = [(1.7, 0.0), (-2.3, math.log(7.5)), (6.0, math.log(0.3))]      # (m, log E): E = 1, 7.5, 0.3; a negative m
_TABLE = {}


def _table():
    """The brute-force values of the case table, computed once; an entry whose integrand has not decayed at u = +-14, or is
    below 1e-200 there, is taken on u in [-38, 38] (test_count_pmf_cpu.py::_table)."""
    if not _TABLE:
        for r in PMF_R:
            for m, a in CONFIGS:
                for v in VS:
                    vals = [nb.brute(m, v, a, k, r) for k in KS]
                    for i, (val, end) in enumerate(vals):
                        if end > pref.BRUTE_END or val < 1e-200:
                            vals[i] = nb.brute(m, v, a, KS[i], r, pref.BRUTE_WIDE)
                            assert vals[i][1] <= pref.BRUTE_END
                    _TABLE[(r, m, a, v)] = np.array([x[0] for x in vals])
    return _TABLE


def test_rule_against_brute_force():
    """Relative error of the pmf at P = 129 on the case table: r in {0.37, 1, 8, 2^20} x v in {1e-8, 3e-3, 0.27, 1, 9, 26} x
    (m, E) in {(1.7, 1), (-2.3, 7.5), (6, 0.3)} x k in {0, 1, 40, 1000, 60000}, entries whose brute-force value is below 1e-200
    skipped.  Measured: 2.16e-10 (r = 2^20, m = -2.3, E = 7.5, v = 0.27, k = 60000: the conditioning of g(z*) at a large count, as for the
    Poisson family; 33 of 360 entries skipped); r_129 of the device bar
    is 4 x that."""
    worst, where, gone, total = 0.0, None, 0, 0
    ks = np.array(KS, np.float64)
    for (r, m, a, v), want in _table().items():
        got = np.exp(nb.rule(m, v, a, ks, r, points=129))
        keep = want >= 1e-200
        gone, total = gone + int((~keep).sum()), total + len(KS)
        assert (got[~keep] < 1e-150).all()
        if keep.any():
            err = np.abs(got - want)[keep] / want[keep]
            if err.max() > worst:
                worst, where = err.max(), (r, m, a, v, ks[keep][err.argmax()])
    print("P = 129: worst relative error %.3e at (r, m, a, v, k) = %s; %d of %d entries skipped" % (worst, where, gone, total))
    assert 2 * gone <= total
    assert worst <= nb.MEASURED_129 and nb.BAR_129 == 4 * nb.MEASURED_129 and nb.BAR_129 <= 1e-9


def test_rounding_constant_of_the_device_bar():
    """c of |log pmf_dev - log pmf_ref| <= c 2^-53 T + r_129: the restatement in float64 against the same evaluation (g(z*) and the
    sum at the float64 run's centre and window, P = 129) in numpy.longdouble, in units of 2^-53 T, on inputs drawn as the GPU test
    draws them, r in {0.37, 8, 2^20}, counts from 0 and from 1000.  Measured: 9.09 (r = 0.37, counts from 0), 7.19 at r = 2^20, 5.22 at r = 8; the recorded constant
    is 9.1 and the device gets 4 x that, 36.4."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    worst = 0.0
    for r in (0.37, 8.0, 2.0 ** 20):
        for k0 in (0, 1000):
            m, v, a = nb.gpu_inputs(129, 7 + k0)
            k = k0 + np.arange(150, dtype=np.float64)
            args = (m[:, None], v[:, None], a.astype(np.float64)[:, None], k[None, :], r)
            lp, T, z, tl, tr = nb.rule(*args, points=129, full=True)
            ext = nb.rule(*args, points=129, dtype=np.longdouble, at=(z, tl, tr))
            ok = np.isfinite(lp)
            assert np.array_equal(ok, np.isfinite(ext)) and ok.all()
            c = float((np.abs(lp[ok] - ext[ok]) / (2.0 ** -53 * T[ok])).max())
            print("r = %g, k0 = %d: c = %.2f (largest T %.3g)" % (r, k0, c, T[ok].max()))
            worst = max(worst, c)
    assert worst <= nb.MEASURED_C
    assert nb.DEVICE_C == max(8.0, 4 * nb.MEASURED_C)


def test_mode_iteration_ends_at_a_stationary_point():
    for r in (0.37, 8.0, 2.0 ** 20):
        m, v, a = nb.gpu_inputs(257, 31)
        k = np.concatenate([np.arange(300.0), 1000.0 + np.arange(300.0)])
        m, v, a, k = (t.ravel() for t in np.broadcast_arrays(m[:, None], v[:, None], a.astype(np.float64)[:, None], k[None, :]))
        go = v > pref.V_MIN
        m, v, k = (m + a - math.log(r))[go], v[go], k[go]
        z, its = nb.mode(m, v, k, r)
        l1, l2, _ = nb._site_z(z, k + r, k, r)
        g1, g2 = l1 - (z - m) / v, l2 - 1 / v
        left = np.abs(g1 / g2) * np.sqrt(-g2)
        print("r = %g: %d entries, %d steps at most, largest step left %.1e sigma_hat" % (r, go.sum(), its, left.max()))
        assert its <= 60 and left.max() <= 1e-6


@pytest.mark.parametrize("m, a, k, r", [(1.7, 0.0, 0, 0.37), (1.7, 0.0, 17, 8.0), (-2.3, math.log(7.5), 3, 1.0),
                                        (4.0, math.log(0.3), 30, 2.0 ** 20), (0.4, 0.0, 40, 2.0 ** -10)])
def test_degenerate_branch_and_the_switch(m, a, k, r):
    """v <= V_MIN: the plain log pmf at eta = m, against the closed form from math alone; just above V_MIN the quadrature runs and
    agrees to 1e-12; NaN in m, v or k gives NaN."""
    want = nb.plain(m, a, k, r)
    for v in (0.0, -1.0, -np.inf, 1e-30, pref.V_MIN):
        lp, T, z, _, _ = nb.rule(m, v, a, float(k), r, full=True)
        assert np.isnan(z) and abs(lp - want) <= 1e-13 * T, (v, lp, want)
    lp, _, z, tl, tr = nb.rule(m, np.nextafter(pref.V_MIN, 1.0), a, float(k), r, full=True)
    assert np.isfinite(z) and tl > 0 and tr > 0
    assert abs(lp - want) <= 1e-12 * max(1.0, abs(want))
    assert np.isnan(nb.rule(np.nan, 1.0, a, float(k), r)) and np.isnan(nb.rule(m, np.nan, a, float(k), r))
    assert np.isnan(nb.rule(m, 1.0, a, np.nan, r))


def test_poisson_limit():
    """|log pmf_NB(r) - log pmf_Poisson| of the two restatements halves per doubling of r over r = 2^16 .. 2^20, within 10 %: the
    leading term is ((k - mu)^2 - k) / 2r averaged over the latent.  k = 40, m = 3, v = 0.27: measured 3.211e-6, 1.605e-6, 8.027e-7, 4.014e-7, 2.007e-7."""
    diffs = []
    for e in range(16, 21):
        d = abs(float(nb.rule(3.0, 0.27, 0.0, 40.0, 2.0 ** e, points=129)) - float(pref.rule(0, 3.0, 0.27, 0.0, 40.0, points=129)))
        diffs.append(d)
    print("Poisson limit: |difference| at r = 2^16 .. 2^20: %s" % ["%.3e" % d for d in diffs])
    assert min(diffs) > 1e-9
    for a, b in zip(diffs, diffs[1:]):
        assert abs(a / b - 2.0) <= 0.2, (a, b)


@pytest.mark.parametrize("m, v, E, r", [(1.7, 0.27, 1.0, 1.0), (4.0, 1.0, 1.0, 8.0), (-2.3, 1.0, 7.5, 2.0), (3.0, 3e-3, 0.3, 2.0 ** 20)])
def test_rows_sum_to_one_and_have_the_closed_form_mean(m, v, E, r):
    """On the block 0 .. 65535: sum pmf = 1 and sum k pmf = E exp(m + v / 2), the mean of predict_mean, to 1e-8 -- for inputs
    (r >= 1, v <= 1, m <= 5) whose mass beyond the block is below 1e-9, which is checked first: by Cantelli's inequality with the
    closed-form variance the tail beyond 65535 is at most var / (var + (65535 - mean)^2), and for the mean's share a bound from
    the fourth moment is not needed at these sizes: the test asserts the sum itself."""
    assert r >= 1 and v <= 1 and m <= 5
    k = np.arange(65536, dtype=np.float64)
    mean, var = nb.predict_mean(m, v, E, r)
    pmf = np.exp(nb.rule(m, v, math.log(E), k, r, points=129))
    total = pmf.sum()
    print("m = %g v = %g E = %g r = %g: sum - 1 = %.2e, mean error %.2e, variance error %.2e"
          % (m, v, E, r, total - 1.0, (k * pmf).sum() / mean - 1.0, ((k - mean) ** 2 * pmf).sum() / var - 1.0))
    assert total >= 1.0 - 1e-9                           # the block holds 1 - 1e-9 of the mass
    assert abs(total - 1.0) <= 1e-9
    assert abs((k * pmf).sum() / mean - 1.0) <= 1e-8
    assert abs(((k - mean) ** 2 * pmf).sum() / var - 1.0) <= 1e-5          # the variance of predict_mean (a heavier tail)


# ------------------------------------------------------------------------------------------------ fit, evidence, profile
def test_reference_mode_and_float32_step_rule(golden):
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    d = nb.data(nb.nb_counts(golden("dumbbell_k10_loop")), nb.R_TRUE)
    f, trace = nb.newton(Q, d)
    assert np.abs(nb.gradient(Q, f, d)).max() <= 1e-10 and np.abs(f).max() > 1.0
    f32, converged, its, history = nb.simulate(Q, d)
    err = np.abs(f32.astype(np.float64) - f).max()
    print("r = 2: %d steps %s, max |f - f64| = %.2e; s_ref %g, mean %.4f, largest count %d"
          % (its, [h[2] for h in history], err, d["s_ref"], d["mean"], d["y"][d["obs"]].max()))
    assert converged and its <= 10 and err <= 1e-5
    assert d["s_ref"] == 4.0 * 2.0 ** -cref.ceil_log2(math.ceil(d["y"][d["obs"]].max() + 2.0))


def test_dispersion_profile_of_the_reference_is_separated(golden):
    """The dense evidence over r in {0.5, 1, 2, 4, 16, 2^20} on the fixture's data (drawn at r = 2): the argmax is r = 2, separated
    from the runner-up by more than 10 x the bar of the GPU comparison, 1e-6 (|log-likelihood| + quad) + DENSE_BAR logdet / 2, and
    the Poisson-like end r = 2^20 is far below.  Measured: -730.1, -708.7, -703.4, -711.6, -747.4, -789.8; bars of 1.2e-3."""
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    c = nb.nb_counts(golden("dumbbell_k10_loop"))
    vals, bars, f = [], [], None
    for r in nb.PROFILE:
        d = nb.data(c, r)
        f, z = nb.mode_log_z(Q, d, f0=f)
        vals.append(z["value"])
        bars.append(1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * 1.43e-7 * z["logdet"])
    order = np.argsort(vals)[::-1]
    print("dense evidence over r = %s: %s; bars up to %.2e" % (nb.PROFILE, ["%.3f" % v for v in vals], max(bars)))
    assert vals[order[0]] - vals[order[1]] > 10 * max(bars)
    assert nb.PROFILE[order[0]] == nb.R_TRUE and vals[order[0]] - vals[-1] > 10.0


def test_interval_coverage_poisson_against_negative_binomial(golden):
    """The worked number of docs/kernels/counts.md: on the overdispersed fixture (drawn at r = 2, 10 % of the nodes observed) the
    90 % predictive interval of a Poisson fit covers far fewer of the held-out counts (every 8th unobserved node) than that of the
    negative-binomial fit at r = 2: dense float64 fits, the latent variance from the dense Laplace covariance, the pmf by the
    restatements.  Measured: 0.954 against 0.632."""
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    c = nb.nb_counts(golden("dumbbell_k10_loop"))
    obs = c["obs"]
    d = nb.data(c, nb.R_TRUE)
    f, _ = nb.newton(Q, d)
    v = np.diag(np.linalg.inv(Q + np.diag(nb.curvature(f, d))))
    dp = dict(cref.poisson_data(c), y=c["y"])
    fp, _ = cref.newton(Q, dp)
    vp = np.diag(np.linalg.inv(Q + np.diag(cref.curvature(fp, dp))))
    k = np.arange(8192, dtype=np.float64)
    obs = np.flatnonzero(~obs)[::8]                       # held-out nodes from here on
    cover = {}
    for name, eta, var, pmf in (("nb", f + d["mean"], v, lambda e, s: nb.rule(e, s, d["aux"][obs, None], k[None, :], nb.R_TRUE)),
                                ("poisson", fp + dp["mean"], vp, lambda e, s: pref.rule(0, e, s, dp["aux"][obs, None], k[None, :]))):
        lo, hi, reached = pref.quantiles(np.exp(pmf(eta[obs, None], var[obs, None])), 0.9)
        assert reached.all()
        cover[name] = float(((c["y"][obs] >= lo) & (c["y"][obs] <= hi)).mean())
    print("coverage of the 90 %% interval at %d held-out nodes: negative binomial %.3f, Poisson %.3f" % (len(obs), cover["nb"], cover["poisson"]))
    assert cover["nb"] >= 0.85 and cover["poisson"] <= cover["nb"] - 0.2


# ------------------------------------------------------------------------------------------------ host-side checks
NEW = ("mgp_nb_site_workspace_bytes", "mgp_nb_site", "mgp_nb_predict_pmf", "mgp_nb_predict_logpmf",
       "mgp_nb_evidence_site_workspace_bytes", "mgp_nb_evidence_site")


def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mgp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(handle, name)


def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    nan, inf = float("nan"), float("inf")
    bad_r = (0.0, -1.0, 2.0 ** -11, 2.0 ** 20 + 1.0, nan, inf)
    for bytes_ in (lib.mgp_nb_site_workspace_bytes, lib.mgp_nb_evidence_site_workspace_bytes):
        assert bytes_(0) == 0 and bytes_(1) == 32 and bytes_(1025) == 64 and bytes_(2 ** 40) == 1024 * 32
    site = lib.mgp_nb_site
    ok = lambda **kw: dict(dict(f=u, y=u, aux=u, n=4, r=2.0, w=u, rhs=u, sums=d, work=d, wb=64), **kw)
    call = lambda a: site(a["f"], None, a["y"], a["aux"], None, a["n"], 1.0, 0.0, a["r"], a["w"], a["rhs"], a["sums"], a["work"], a["wb"], None)
    for kw in (dict(f=None), dict(y=None), dict(w=None), dict(rhs=None), dict(sums=None), dict(n=0), dict(n=-3)):
        assert call(ok(**kw)) == -1, kw
    for r in bad_r:
        assert call(ok(r=r)) == -1, r
    assert call(ok(work=None)) == -2 and call(ok(wb=31)) == -2 and call(ok(work=d + 4)) == -2
    ev = lib.mgp_nb_evidence_site
    ok = lambda **kw: dict(dict(f=u, y=u, n=4, r=2.0, floor=1e-30, root=u, sums=d, work=d, wb=64), **kw)
    call = lambda a: ev(a["f"], a["y"], None, None, None, a["n"], 0.0, a["r"], a["floor"], a["root"], None, a["sums"], a["work"], a["wb"], None)
    for kw in (dict(f=None), dict(y=None), dict(root=None), dict(sums=None), dict(n=0), dict(floor=-1.0), dict(floor=nan)):
        assert call(ok(**kw)) == -1, kw
    for r in bad_r:
        assert call(ok(r=r)) == -1, r
    assert call(ok(work=None)) == -2 and call(ok(wb=31)) == -2 and call(ok(work=d + 4)) == -2
    pmf, logpmf = lib.mgp_nb_predict_pmf, lib.mgp_nb_predict_logpmf
    ok = lambda **kw: dict(dict(eta=d, var=d, n=4, r=2.0, k0=0, K=3, points=65, out=d, y=u), **kw)
    cp = lambda a: pmf(a["eta"], a["var"], None, a["n"], a["r"], a["k0"], a["K"], a["points"], 0, a["out"], None)
    cl = lambda a: logpmf(a["eta"], a["var"], None, a["y"], None, a["n"], a["r"], a["points"], a["out"], None)
    for kw in (dict(eta=None), dict(var=None), dict(out=None), dict(n=0), dict(points=64), dict(points=15), dict(points=259)):
        assert cp(ok(**kw)) == -1 and cl(ok(**kw)) == -1, kw
    for kw in (dict(K=0), dict(K=65537), dict(k0=-1), dict(k0=2 ** 24, K=2)):
        assert cp(ok(**kw)) == -1, kw
    assert cl(ok(y=None)) == -1
    for r in bad_r:
        assert cp(ok(r=r)) == -1 and cl(ok(r=r)) == -1, r
    # the siblings still refuse the family codes they refused
    assert lib.mgp_count_site(u, None, u, u, None, 4, 1.0, 0.0, 2, u, u, d, d, 64, None) == -3
    assert lib.mgp_count_predict_pmf(d, d, None, 4, 2, 0, 3, 65, 0, d, None) == -3
    assert lib.mgp_laplace_evidence_site(u, u, None, None, None, 4, 0.0, 3, 1e-30, u, None, d, d, 64, None) == -3


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_python_argument_checks():
    from manifold_gp_amd import counts as ct, evidence as ev
    d = _fake_desc()
    y = torch.tensor([0.0, 3.0, 7.0])
    nan, inf = float("nan"), float("inf")
    NBF = "negative_binomial"
    with pytest.raises(ValueError, match="needs dispersion"):
        ct.fit_counts(d, y, family=NBF)
    with pytest.raises(ValueError, match="needs dispersion"):
        ct.laplace_fit_counts(d, y, family=NBF)
    for bad in (nan, inf, 0.0, -2.0, 2.0 ** -11, 2.0 ** 21):
        with pytest.raises(ValueError, match="dispersion must be a finite scalar"):
            ct.fit_counts(d, y, family=NBF, dispersion=bad)
        with pytest.raises(ValueError, match="dispersion must be a finite scalar"):
            ct.laplace_fit_negative_binomial(d, y, bad)
    for bad in ("2", [2.0], torch.ones(2), True):
        with pytest.raises(ValueError, match="dispersion must be a real scalar"):
            ct.fit_counts(d, y, family=NBF, dispersion=bad)
    for family, kw in (("poisson", {}), ("binomial", dict(trials=torch.tensor([1.0, 3.0, 9.0])))):
        with pytest.raises(ValueError, match="dispersion belongs"):
            ct.fit_counts(d, y, family=family, dispersion=2.0, **kw)
    with pytest.raises(ValueError, match="trials"):
        ct.fit_counts(d, y, family=NBF, dispersion=2.0, trials=torch.tensor([1.0, 3.0, 9.0]))
    with pytest.raises(ValueError, match="family"):
        ct.fit_counts(d, y, family="negative-binomial", dispersion=2.0)
    with pytest.raises(ValueError, match="family"):
        ct.laplace_fit_counts(d, y, family="negative-binomial")
    with pytest.raises(ValueError, match="exposure"):
        ct.fit_counts(d, y, family=NBF, dispersion=2.0, exposure=torch.tensor([1.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="integers in"):
        ct.fit_counts(d, torch.tensor([0.0, 0.5, 1.0]), family=NBF, dispersion=2.0)
    with pytest.raises(ValueError, match="every observed count is 0"):
        ct.fit_counts(d, torch.zeros(3), family=NBF, dispersion=2.0)
    # valid arguments on host tensors: the checks pass, the first device call refuses
    for r in (2.0, np.float32(0.5), torch.tensor(2.0 ** 20), 2.0 ** -10, 1):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ct.fit_counts(d, y, family=NBF, dispersion=r, exposure=torch.tensor([2.0, 1.0, 0.5]))
    # the defaults: the Poisson mean, s_ref from ceil(max y + r)
    some = torch.tensor([True, False, True])
    *_, mean, s_ref = ct._validate(d, torch.tensor([2.0, 900.0, 6.0]), some, NBF, torch.tensor([1.0, 5.0, 3.0]), None, None, 1e-3, None, 2.0)
    assert mean == pytest.approx(np.log(8.0 / 4.0), abs=1e-15) and s_ref == 4.0 / 8.0           # ceil(6 + 2) = 8
    *_, s_ref = ct._validate(d, torch.tensor([2.0, 900.0, 6.0]), some, NBF, None, None, 0.0, 1e-3, None, 2.5)
    assert s_ref == 4.0 / 16.0                                                                  # ceil(8.5) = 9 -> 16
    *_, s_ref = ct._validate(d, y, None, NBF, None, None, 0.0, 1e-3, None, 2.0 ** -10)
    assert s_ref == 4.0 / 8.0                                                                   # ceil(7 + 2^-10) = 8
    # the kernels' wrappers
    f = torch.zeros(3)
    with pytest.raises(ValueError, match="needs dispersion"):
        ct.count_site(f, None, y, None, None, 1.0, 0.0, NBF)
    with pytest.raises(ValueError, match="dispersion belongs"):
        ct.count_site(f, None, y, None, None, 1.0, 0.0, "poisson", dispersion=2.0)
    with pytest.raises(ValueError, match="finite scalar"):
        ct.count_predict_pmf(f, f, None, NBF, 0, 3, dispersion=nan)
    with pytest.raises(ValueError, match="needs dispersion"):
        ct.count_predict_logpmf(f, f, None, y, None, NBF)
    with pytest.raises(ValueError, match="needs dispersion"):
        ev.evidence_site(f, y, None, None, None, 0.0, NBF)
    with pytest.raises(ValueError, match="dispersion belongs"):
        ev.evidence_site(f, y, None, None, None, 0.0, "bernoulli", dispersion=2.0)
    for call in (lambda: ct.count_site(f, None, y, None, None, 1.0, 0.0, NBF, 2.0),
                 lambda: ct.count_predict_pmf(f, f, None, NBF, 0, 3, dispersion=2.0),
                 lambda: ct.count_predict_logpmf(f, f, None, y, None, NBF, dispersion=2.0),
                 lambda: ev.evidence_site(f, y, None, None, None, 0.0, NBF, dispersion=2.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="empty"):
        ct.dispersion_profile(d, y, [])
    with pytest.raises(ValueError, match="finite scalar"):
        ct.dispersion_profile(d, y, [1.0, nan])
    with pytest.raises(ValueError, match="takes no family"):
        ct.dispersion_profile(d, y, [1.0], family="poisson")


def test_exports_and_the_site_formulas_of_the_fit():
    """The family's float64 (g, h) of families.py (the pseudo-observations of latent_variance / latent_samples) is the restatement's
    g and h; the public names exist; dispersion= goes wherever family= is public."""
    from manifold_gp_amd import counts as ct, evidence as ev, families
    from manifold_gp_amd.models import RiemannGP
    rng = np.random.default_rng(0)
    f, y = rng.uniform(-8, 8, 50), rng.integers(0, 50, 50).astype(np.float64)
    for r in (0.37, 2.0, 2.0 ** 20):
        _, g, h, _, _ = nb.site(f, y, None, None, 0.25, r)
        tg, th = families.TABLE["negative_binomial"].gh(torch.from_numpy(f + 0.25), torch.from_numpy(y), None, r)
        assert np.abs(tg.numpy() - g).max() <= 1e-13 * (y.max() + r) and np.abs(th.numpy() - h).max() <= 1e-13 * (y.max() + r)
    assert ct.FAMILIES["negative_binomial"] == 2 and families._family("negative_binomial", "evidence").code("evidence") == 3
    assert "dispersion" in inspect.signature(ct.fit_counts).parameters
    assert list(inspect.signature(ct.laplace_fit_negative_binomial).parameters)[:3] == ["desc", "y", "dispersion"]
    assert "dispersion" in inspect.signature(ct.CountLaplaceFit.__init__).parameters
    assert list(inspect.signature(ct.dispersion_profile).parameters)[:3] == ["desc", "y", "dispersions"]
    assert "kw" in inspect.signature(RiemannGP.laplace_posterior_counts).parameters
