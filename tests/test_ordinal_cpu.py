"""Ordered-category fits, host side (no GPU): the float64 restatement the GPU tests are checked against (tests/_ordinal_ref.py)
is itself checked -- the site formulas against autograd of the naive form and against mpmath at extreme arguments, the
predictive rule against a 30-digit quadrature, its own rounding against the same rule summed in mpmath (which gives the
constant of the device test's bound) --, then ordinal_cutpoints, the C-ABI and the Python argument checks."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import _ordinal_ref as oref

INF = np.inf


# ------------------------------------------------------------------------------------------------ the site restatement
def test_site_restatement_matches_autograd_of_the_naive_form():
    """log p, g and h against float64 autograd of log(sigma(hi - f) - sigma(lo - f)) at |f| <= 6, cutpoints in [-4, 4] with
    gaps >= 0.25, the end categories included.  The naive difference is >= 0.25 sigma'(10) = 1e-5 there and carries 2^-53 of
    rounding per term: 1e-11 relative on log p's argument; two derivatives of it are asked to 1e-9."""
    rng = np.random.default_rng(0)
    n = 4000
    f = rng.uniform(-6.0, 6.0, n)
    lo = rng.uniform(-4.0, 3.5, n)
    hi = lo + rng.uniform(0.25, 4.0, n)
    lo[: n // 4] = -INF
    hi[n // 4: n // 2] = INF
    lp, g, h = oref.site(f, lo, hi)
    with np.errstate(invalid="ignore"):
        logc = np.where(np.isfinite(hi - lo), np.log(-np.expm1(-(hi - lo))), 0.0)
    ft = torch.tensor(f, requires_grad=True)
    naive = oref.naive_log_p(ft, torch.tensor(lo), torch.tensor(hi))
    g_auto, = torch.autograd.grad(naive.sum(), ft, create_graph=True)
    h_auto, = torch.autograd.grad(g_auto.sum(), ft)
    e_lp = np.abs(lp + logc - naive.detach().numpy()).max()
    e_g = np.abs(g - g_auto.detach().numpy()).max()
    e_h = np.abs(h + h_auto.numpy()).max()
    print("against autograd of the naive form: log p %.1e, g %.1e, h %.1e" % (e_lp, e_g, e_h))
    assert e_lp <= 1e-11 and e_g <= 1e-9 and e_h <= 1e-9
    assert (h > 0).all() and (h <= 0.5).all()


EXTREME_F = [0.0, 1.0, -1.0, 37.5, -37.5, 700.0, -745.0, 1e4, -1e4]
EXTREME_INTERVALS = [(-INF, 0.0), (0.0, INF), (-INF, -3.0), (2.0, INF), (-1.0, 0.5), (0.0, 2.0 ** -20), (5.0, 5.0 + 2.0 ** -20),
                     (-12.0 - 2.0 ** -20, -12.0), (-50.0, 60.0)]


def test_site_restatement_matches_mpmath_at_extreme_arguments():
    """|f| up to 1e4, gaps down to 2^-20, infinite ends, against 60-digit arithmetic on the naive difference: log p with its
    constant to 1e-14 relative, h to 1e-14 relative (where float64 holds it: it underflows at |f| > 745), g to 2^-51 absolute
    (|g| <= 1 is a difference of two numbers in [0, 1], each within 2^-53 relative).  Everything is finite; 0 <= h <= 1/2."""
    import mpmath as mp
    worst = [0.0, 0.0, 0.0]
    with mp.workdps(60):
        sig = lambda x: 1 / (1 + mp.exp(-x))
        for f in EXTREME_F:
            for lo, hi in EXTREME_INTERVALS:
                f32, lo32, hi32 = np.float32(f), np.float32(lo), np.float32(hi)
                lp, g, h = oref.site(np.array([f32]), np.array([lo32]), np.array([hi32]))
                logc = 0.0 if not np.isfinite(hi - lo) else np.log(-np.expm1(-(float(hi32) - float(lo32))))
                assert np.isfinite(lp[0]) and np.isfinite(g[0]) and 0.0 <= h[0] <= 0.5, (f, lo, hi)
                # s = sigma(b - f) and its complement sc = sigma(f - b) per end; the difference p from the smaller pair
                F = mp.mpf(float(f32))
                s_hi, sc_hi = (mp.mpf(1), mp.mpf(0)) if hi == INF else (sig(mp.mpf(float(hi32)) - F), sig(F - mp.mpf(float(hi32))))
                s_lo, sc_lo = (mp.mpf(0), mp.mpf(1)) if lo == -INF else (sig(mp.mpf(float(lo32)) - F), sig(F - mp.mpf(float(lo32))))
                p = s_hi - s_lo if s_hi < sc_lo else sc_lo - sc_hi
                t_hi, t_lo = s_hi * sc_hi, s_lo * sc_lo                               # d sigma / dx at the two ends
                rest = sc_hi + s_lo                                                   # 1 - p, a sum of positive terms
                want_lp = mp.log1p(-rest) if rest < 0.5 else mp.log(p)
                want_g = (t_lo - t_hi) / p
                want_h = t_hi + t_lo            # (the identity -d2 log p = t_hi + t_lo is the autograd test's: -p'' / p + g^2 cancels here)
                worst[0] = max(worst[0], float(abs(mp.mpf(float(lp[0])) + mp.mpf(float(logc)) - want_lp)
                                               / (abs(want_lp) + mp.mpf(10) ** -300)))
                worst[1] = max(worst[1], float(abs(mp.mpf(float(g[0])) - want_g)))
                if want_h > mp.mpf(10) ** -290:
                    assert h[0] > 0
                    worst[2] = max(worst[2], float(abs(mp.mpf(float(h[0])) - want_h) / want_h))
    print("against mpmath: log p %.1e relative, g %.1e absolute, h %.1e relative" % tuple(worst))
    assert worst[0] <= 1e-14 and worst[1] <= 2.0 ** -51 and worst[2] <= 1e-14


def test_two_categories_cut_at_zero_are_the_bernoulli_formulas():
    """K = 2, b_1 = 0: label 1 is the interval (0, inf), label 0 (-inf, 0).  Against the expressions of mgp_bernoulli_site
    (log p = min(a, 0) - log1p(e), pi = f >= 0 ? 1 / d : e / d, g = t - pi, h = e / d^2): log p and h bit for bit, g bit for bit
    at label 0 (-pi); at label 1 the ordinal form is sigma(-f) taken from e directly, the Bernoulli one 1 - pi with a rounded
    subtraction: 1 / d, e / d, 1 - e / d and the two sides' difference round by at most 2^-54 each, 2^-52 in all."""
    rng = np.random.default_rng(1)
    f = np.concatenate([rng.standard_normal(2000) * 3.0, [0.0, 1e-8, -1e-8, 20.0, -20.0, 40.0, -40.0, 90.0, -90.0, 1e4, -1e4]])
    f = f.astype(np.float32).astype(np.float64)
    t = rng.random(f.shape[0]) < 0.5
    lo, hi = oref.intervals(t.astype(np.int64), [0.0])
    lp, g, h = oref.site(f, lo, hi)
    e = np.exp(-np.abs(f))
    d = 1.0 + e
    a = np.where(t, f, -f)
    want_lp = np.where(a < 0.0, a, 0.0) - np.log1p(e)
    pi = np.where(f >= 0.0, 1.0 / d, e / d)
    want_g = np.where(t, 1.0, 0.0) - pi
    want_h = e / (d * d)
    assert np.array_equal(lp, want_lp) and np.array_equal(h, want_h)
    assert np.array_equal(g[~t], want_g[~t])
    assert np.abs(g[t] - want_g[t]).max() <= 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the predictive rule
_MP = {}


def _mp_table():
    if not _MP:
        for v in oref.TABLE_V:
            for m in oref.TABLE_M:
                for lo, hi in oref.TABLE_INTERVALS:
                    _MP[(v, m, lo, hi)] = oref.mp_probability(m, v, lo, hi)
    return _MP


def test_rule_matches_30_digit_quadrature():
    """The 129-point rule against mpmath's quadrature on the table of docs/kernels/ordinal.md (6 variances x 3 means x 7
    intervals, tails of 1e-9 and a width of 1e-3 among them): relative error <= 1e-10.  Measured: 5.3e-12 (v = 26, the interval
    (-3, -2.999)); 4.4e-6 at 65 points, printed beside it."""
    want = _mp_table()
    worst = {65: 0.0, 129: 0.0}
    for points in worst:
        for v in oref.TABLE_V:
            row = []
            for m in oref.TABLE_M:
                err = max(float(abs(oref.interval_probability(m, v, lo, hi, points) - want[(v, m, lo, hi)]) / want[(v, m, lo, hi)])
                          for lo, hi in oref.TABLE_INTERVALS)
                row.append(err)
            worst[points] = max(worst[points], max(row))
            print("%4d points, v = %-6g: %s" % (points, v, "  ".join("m = %4g: %.1e" % (m, e) for m, e in zip(oref.TABLE_M, row))))
    print("worst relative error: %.2e at 129 points, %.2e at 65" % (worst[129], worst[65]))
    assert worst[129] <= 1e-10


def test_rounding_of_the_restatement_gives_the_device_constant():
    """The float64 restatement against the SAME rule summed in 30-digit arithmetic, on the same table at 129 points:
    |log p_64 - log p_mp| in units of 2^-53 (1 + X), X = max |b - f_j| over the grid (exp(-|b - f|) carries the rounding of its
    argument).  Measured worst ratio: 5.19 (v = 1e-8, m = 2.5, (2, inf): 129 terms of the same size added in order).  The device
    test's bound is c 2^-53 (1 + X) with c = 4 x 5.19 = 20.8, rounded up to 22."""
    import mpmath as mp
    worst = 0.0
    for v in oref.TABLE_V:
        for m in oref.TABLE_M:
            for lo, hi in oref.TABLE_INTERVALS:
                p = oref.interval_probability(m, v, lo, hi, 129)
                q = oref.mp_rule(m, v, lo, hi, 129)
                X = oref.reach([m], [v], [b for b in (lo, hi) if abs(b) != INF])[0]
                with mp.workdps(30):
                    ratio = float(abs(mp.log(mp.mpf(float(p))) - mp.log(q))) / (2.0 ** -53 * (1.0 + X))
                worst = max(worst, ratio)
    print("worst ratio to 2^-53 (1 + X): %.2f; c = %g" % (worst, oref.DEVICE_C))
    assert oref.DEVICE_C == 22.0 and 4.0 * worst <= oref.DEVICE_C


def test_rule_rows_sum_to_one_and_edge_values():
    """rows sum to 1 at every rule (the sum is divided by the sum of the weights: 1.0144 at 9 points), var <= 2^-76 is the plain
    probability, NaN propagates, log is the log."""
    cuts = np.array([-2.0, -0.5, 0.25, 3.0])
    eta = np.array([-4.0, 0.0, 0.3, 2.5, 7.0])
    for points in (9, 65, 129):
        for v in (0.0, -1.0, 1e-8, 0.27, 9.0, 26.0):
            p = oref.trapezoid(eta, np.full(5, v), cuts, points)
            assert np.abs(p.sum(1) - 1.0).max() <= 1e-14 and (p > 0).all()
    assert abs(oref.rule(9)[1].sum() - 1.0144) <= 1e-4 and abs(oref.rule(65)[1].sum() - 1.0) <= 2e-15
    plain = oref.trapezoid(eta, np.array([0.0, -3.0, 2.0 ** -76, -0.0, 2.0 ** -77]), cuts)
    f = eta[:, None]
    want = np.diff(np.concatenate([np.zeros((5, 1)), 1.0 / (1.0 + np.exp(-(cuts[None, :] - f))), np.ones((5, 1))], 1), axis=1)
    assert np.abs(plain - want).max() <= 1e-15
    bad = oref.trapezoid(np.array([np.nan, 0.0, 0.0]), np.array([1.0, np.nan, 1.0]), cuts)
    assert np.isnan(bad[:2]).all() and np.isfinite(bad[2]).all()
    assert np.array_equal(oref.trapezoid(eta, np.ones(5), cuts, log=True), np.log(oref.trapezoid(eta, np.ones(5), cuts)))


# ------------------------------------------------------------------------------------------------ ordinal_cutpoints
def test_cutpoints_from_labels():
    from manifold_gp_amd.ordinal import MAX_CATEGORIES, S_REF, ordinal_cutpoints
    assert MAX_CATEGORIES == 64 and S_REF == 2.0
    # empty categories: strictly increasing all the same
    y = torch.tensor([0, 0, 5, 5, 5, 2])
    b = ordinal_cutpoints(y, 7)
    assert b.dtype == torch.float64 and b.shape == (6,) and bool((b[1:] > b[:-1]).all()) and bool(torch.isfinite(b).all())
    mass = np.array([2, 0, 1, 0, 0, 3, 0]) + 0.5
    want = np.log(np.cumsum(mass)[:-1] / (mass.sum() - np.cumsum(mass)[:-1]))
    assert np.abs(b.numpy() - want).max() <= 1e-14
    b64 = ordinal_cutpoints(torch.zeros(10), 64)                                  # one category of 64 holds every label
    assert b64.shape == (63,) and bool((b64[1:] > b64[:-1]).all())
    # large and balanced: the plain cumulative logits (the smoothing cancels: (k N / K + k / 2) / (N + K / 2) = k / K)
    K, per = 5, 200000
    yb = torch.arange(K).repeat_interleave(per)
    plain = np.log(np.arange(1, K) / (K - np.arange(1, K)))
    assert np.abs(ordinal_cutpoints(yb, K).numpy() - plain).max() <= 1e-12
    # observed picks the labels; NaN elsewhere; float labels of whole numbers
    yf = torch.tensor([0.0, float("nan"), 2.0, 1.0, float("nan")])
    obs = torch.tensor([True, False, True, True, False])
    assert torch.equal(ordinal_cutpoints(yf, 3, obs), ordinal_cutpoints(torch.tensor([0, 2, 1]), 3))
    assert np.abs(oref.cutpoints(np.array([0, 2, 1]), 3) - ordinal_cutpoints(yf, 3, obs).numpy()).max() <= 2e-7   # (float32 there)
    for bad_y, K_ in ((torch.tensor([0, 3]), 3), (torch.tensor([0.5, 1.0]), 3), (torch.tensor([-1, 1]), 3), (yf, 3)):
        with pytest.raises(ValueError, match="integers in"):
            ordinal_cutpoints(bad_y, K_)
    for bad_K in (1, 65, 3.0, True):
        with pytest.raises(ValueError, match="num_categories"):
            ordinal_cutpoints(y, bad_K)
    with pytest.raises(ValueError, match="no node"):
        ordinal_cutpoints(yf, 3, torch.zeros(5, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ host-side checks
def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgp_ordinal_site_workspace_bytes", "mgp_ordinal_site", "mgp_ordinal_predict"):
        assert name in _lib.SIGNATURES
        assert hasattr(handle, name)


def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    assert lib.mgp_ordinal_site_workspace_bytes(0) == 0
    assert lib.mgp_ordinal_site_workspace_bytes(1) == 32 and lib.mgp_ordinal_site_workspace_bytes(1025) == 64
    assert lib.mgp_ordinal_site_workspace_bytes(2 ** 40) == 1024 * 32               # the grid cap of the other site kernels
    assert lib.mgp_ordinal_site_workspace_bytes(1546) == lib.mgp_bernoulli_site_workspace_bytes(1546)
    site = lib.mgp_ordinal_site
    assert site(None, None, u, u, None, 4, 2.0, u, u, d, d, 64, None) == -1
    assert site(u, None, None, u, None, 4, 2.0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, None, None, 4, 2.0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, u, None, 4, 2.0, None, u, d, d, 64, None) == -1
    assert site(u, None, u, u, None, 4, 2.0, u, None, d, d, 64, None) == -1
    assert site(u, None, u, u, None, 4, 2.0, u, u, None, d, 64, None) == -1
    assert site(u, None, u, u, None, 0, 2.0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, u, None, -3, 2.0, u, u, d, d, 64, None) == -1
    assert site(u, None, u, u, None, 4, 2.0, u, u, d, None, 64, None) == -2
    assert site(u, None, u, u, None, 4, 2.0, u, u, d, d, 31, None) == -2
    assert site(u, None, u, u, None, 4, 2.0, u, u, d, d + 4, 64, None) == -2        # misaligned
    predict = lib.mgp_ordinal_predict
    assert predict(None, d, d, 2, 3, 129, 0, d, None) == -1
    assert predict(d, None, d, 2, 3, 129, 0, d, None) == -1
    assert predict(d, d, None, 2, 3, 129, 0, d, None) == -1
    assert predict(d, d, d, 2, 3, 129, 0, None, None) == -1
    assert predict(d, d, d, 0, 3, 129, 0, d, None) == -1
    for K in (1, 65, 0, -2):
        assert predict(d, d, d, 2, K, 129, 0, d, None) == -1
    for points in (128, 7, 8, 1026, 1027, 0):
        assert predict(d, d, d, 2, 3, points, 0, d, None) == -1


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_laplace_fit_ordinal_argument_checks():
    from manifold_gp_amd.ordinal import laplace_fit_ordinal as fit, ordinal_predict, ordinal_site
    d = _fake_desc()
    y = torch.tensor([0, 2, 1])
    some = torch.tensor([True, False, True])
    nan = float("nan")
    for bad in ([0.0, 0.5, 1.0], [0.0, -1.0, 1.0], [0.0, 3.0, 1.0], [nan, 1.0, 1.0]):
        with pytest.raises(ValueError, match="integers in"):
            fit(d, torch.tensor(bad), 3)
    with pytest.raises(ValueError, match="integers in"):
        fit(d, torch.tensor([nan, 1.0, 1.0]), 3, observed=some)                     # NaN at an observed node
    with pytest.raises(ValueError, match="integers in"):
        fit(d, y, 2)                                                                # a label beyond K
    for bad in (torch.zeros(4), [0, 1, 2], torch.tensor([True, False, True])):
        with pytest.raises(ValueError, match="y must be"):
            fit(d, bad, 3)
    with pytest.raises(ValueError, match="no node"):
        fit(d, y, 3, observed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        fit(d, y, 3, observed=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        fit(d, y, 3, observed=torch.ones(3))
    for bad in (1, 65, 3.0, True, None):
        with pytest.raises(ValueError, match="num_categories"):
            fit(d, y, bad)
    for bad in (torch.tensor([0.0]), torch.tensor([0.0, 1.0, 2.0]), [0.0, 1.0], torch.tensor([[0.0, 1.0]]),
                torch.tensor([True, False])):
        with pytest.raises(ValueError, match="cutpoints must be a real tensor"):
            fit(d, y, 3, cutpoints=bad)
    for bad in ([0.0, nan], [0.0, float("inf")], [-float("inf"), 0.0]):
        with pytest.raises(ValueError, match="finite"):
            fit(d, y, 3, cutpoints=torch.tensor(bad))
    for bad in ([1.0, 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            fit(d, y, 3, cutpoints=torch.tensor(bad))
    with pytest.raises(ValueError, match="2\\^-20 apart"):
        fit(d, y, 3, cutpoints=torch.tensor([0.0, 2.0 ** -21], dtype=torch.float64))
    with pytest.raises(ValueError, match="rounded to float32"):
        fit(d, y, 3, cutpoints=torch.tensor([64.0, 64.0 + 2.0 ** -20], dtype=torch.float64))
    with pytest.raises(ValueError, match="f0"):
        fit(d, y, 3, f0=torch.zeros(2))
    with pytest.raises(NotImplementedError):
        fit(_fake_desc(form=2), y, 3)
    # valid arguments on host tensors: the checks pass, the first device call refuses
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, y, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, torch.tensor([0.0, nan, 2.0]), 3, cutpoints=torch.tensor([0.0, 2.0 ** -20], dtype=torch.float64), observed=some)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, y, 64, cutpoints=torch.linspace(-3.0, 3.0, 63), f0=torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ordinal_site(torch.zeros(3), None, torch.zeros(3), torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ordinal_predict(torch.zeros(3), torch.ones(3), torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="strictly increasing"):
        ordinal_predict(torch.zeros(3), torch.ones(3), torch.tensor([1.0, 1.0]))
    with pytest.raises(ValueError, match="cutpoints must be a real tensor"):
        ordinal_predict(torch.zeros(3), torch.ones(3), torch.linspace(0.0, 1.0, 64))
    for bad in (128, 7, 1027, 129.0, True):
        with pytest.raises(ValueError, match="points"):
            ordinal_predict(torch.zeros(3), torch.ones(3), torch.tensor([0.0, 1.0]), points=bad)


def _host_fit(f, y, cuts, obs=None):
    """An OrdinalLaplaceFit on host tensors: what the pure-torch parts of the class compute needs no device"""
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit
    lo, hi = oref.intervals(y, cuts)
    return OrdinalLaplaceFit(_fake_desc(), torch.tensor(y), None if obs is None else torch.tensor(obs), torch.tensor(f, dtype=torch.float32),
                             True, 0, [], 0.0, torch.tensor(cuts, dtype=torch.float64), torch.tensor(lo), torch.tensor(hi))


def test_fit_object_on_the_host():
    """evidence() raises; map_proba is the product form of the restatement (rows sum to 1, relative accuracy in the tails);
    _pseudo() restates g and h of the site formulas; the predict_* argument checks precede the device."""
    from manifold_gp_amd.classification import LaplaceFit
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit
    cuts = np.array([-1.5, 0.25, 2.0])
    f = np.array([0.3, -2.0, 40.0], np.float32)
    y = np.array([1, 0, 3])
    obs = np.array([True, True, False])
    fit = _host_fit(f, y, cuts, obs)
    assert isinstance(fit, LaplaceFit) and fit.num_categories == 4
    with pytest.raises(NotImplementedError, match="ordinal"):
        fit.evidence()
    assert OrdinalLaplaceFit.evidence is not LaplaceFit.evidence
    p = fit.map_proba().numpy()
    want = oref.trapezoid(f.astype(np.float64), np.zeros(3), cuts)
    assert p.shape == (3, 4) and np.abs(p.sum(1) - 1.0).max() <= 1e-15
    assert (np.abs(p - want) <= 4 * 2.0 ** -53 * want).all() and p[2, 0] < 1e-17
    targets, noise, eff = fit._pseudo()
    lo, hi = oref.intervals(y, cuts)
    _, g, h = oref.site(f, lo, hi, obs)
    assert eff.tolist() == [True, True, False]
    assert np.abs(noise.numpy()[:2] - 1.0 / h[:2]).max() <= 1e-15 / h[:2].min() and float(noise[2]) == 1.0
    assert np.abs(targets.numpy()[:2] - (f[:2] + g[:2] / h[:2])).max() <= 1e-14 and float(targets[2]) == 0.0
    with pytest.raises(ValueError, match="kind"):
        fit.predict_category("mean")
    with pytest.raises(ValueError, match="points"):
        fit.predict_proba(points=128)
    with pytest.raises(ValueError, match="variance"):
        fit.predict_proba(variance=torch.ones(2))
    for bad in (-1, 4, 1.0, True, torch.tensor([0.0, 1.0, 2.0]), torch.tensor([0, 1]), torch.tensor([0, 1, 4])):
        with pytest.raises(ValueError, match="k must"):
            fit.predict_exceedance(bad, variance=torch.ones(3))
    with pytest.raises(ValueError, match="integers in"):
        fit.predict_log_density(torch.tensor([0, 4, 1]), variance=torch.ones(3))
    with pytest.raises(ValueError, match="at "):
        fit.predict_log_density(torch.tensor([0, 3, 1]), at=torch.ones(3), variance=torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.predict_proba(variance=torch.ones(3))


def test_model_method_and_exports():
    import manifold_gp_amd
    from manifold_gp_amd.models import RiemannGP
    sig = inspect.signature(RiemannGP.laplace_posterior_ordinal)
    assert list(sig.parameters) == ["self", "num_categories", "cutpoints", "observed", "kw"]
    sig = inspect.signature(manifold_gp_amd.ordinal.laplace_fit_ordinal)
    assert list(sig.parameters) == ["desc", "y", "num_categories", "cutpoints", "observed", "rtol", "max_newton", "cg_tol",
                                    "max_iter", "f0"]
    assert sig.parameters["rtol"].default == 1e-5 and sig.parameters["cutpoints"].default is None
    sig = inspect.signature(manifold_gp_amd.ordinal.OrdinalLaplaceFit.predict_proba)
    assert list(sig.parameters) == ["self", "S", "seed", "points", "variance", "log"]


# ------------------------------------------------------------------------------------------------ the dense iteration
def _dense_problem(golden, case="dumbbell_k10_loop", norm="symmetric", nu=2):
    """The fixture's precision scaled to a prior marginal variance of about 9 (as test_counts_cpu.py), the labels of
    _ordinal_ref.labels (K = 4, about half the nodes observed) and their intervals"""
    import _observed_ref as obref
    g = golden(case)
    Q1, _ = obref.precision_root(obref.oracle(g, norm), nu, float(g["kappa"]), 1.0, norm)
    Q = (np.diag(np.linalg.inv(Q1)).mean() / 9.0) * Q1
    y, obs = oref.labels(g)
    lo, hi = oref.intervals(y, oref.cutpoints(y, 4, obs))
    return Q, lo, hi, obs


def test_reference_mode_is_stationary_and_the_float32_iteration_reaches_it(golden):
    """The dense float64 Newton iteration ends at a stationary point in a non-linear regime with psi monotone; the fit's own
    loop on float32-rounded dense stand-ins (exact solves) converges by the gradient rule at rtol = 1e-5 with full steps, no
    more than the float64 iteration needs, within 1e-5 of the mode (measured: 4 steps, 1.4e-7).  From 20 x noise both halve
    steps and arrive at the same mode (measured: 12 steps, the first eight halved)."""
    Q, lo, hi, obs = _dense_problem(golden)
    f64, trace = oref.newton(Q, lo, hi, obs)
    g0 = np.abs(oref.gradient(Q, np.zeros_like(f64), lo, hi, obs)).max()
    assert np.abs(oref.gradient(Q, f64, lo, hi, obs)).max() <= 1e-11 * g0 and g0 <= 1.0
    assert np.abs(f64).max() > 1.0
    psis = [oref.psi(Q, np.zeros_like(f64), lo, hi, obs)] + [t[0] for t in trace]
    assert all(b >= a - 1e-12 * abs(a) for a, b in zip(psis, psis[1:]))
    f, converged, its, history = oref.simulate(Q, lo, hi, obs)
    err = np.abs(f.astype(np.float64) - f64).max()
    print("from 0: %d steps %s, max |f - f64| = %.2e, relative gradient %.1e" % (its, [h[2] for h in history], err, history[-1][1]))
    assert converged and its <= oref.steps_to(trace, 1e-5) and all(h[2] == 1.0 for h in history) and err <= 1e-5
    f0 = oref.bad_start(Q.shape[0])
    fb, tb = oref.newton(Q, lo, hi, obs, f0=f0)
    f, converged, its, history = oref.simulate(Q, lo, hi, obs, f0=f0)
    print("from 20 x noise: float64 steps %s; float32 %d steps %s" % ([t[2] for t in tb], its, [h[2] for h in history]))
    assert np.abs(fb - f64).max() <= 1e-9 and sum(t[2] < 1.0 for t in tb) >= 1
    assert converged and any(h[2] < 1.0 for h in history) and np.abs(f.astype(np.float64) - f64).max() <= 1e-5
