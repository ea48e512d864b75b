"""The predictive count pmf, host side (no GPU): the float64 restatement of the rule of csrc/count_predict.hip
(tests/_count_pmf_ref.py) against a brute-force rule on a table of cases, its normalisation and mean, the fixed-grid shortcut
that fails, the degenerate branch and the switch to it, the rounding constant of the GPU test's bar, and the C-ABI and Python
argument checks (docs/kernels/count_predict.md)."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import _count_pmf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [0, 1, 2, 5, 17, 100, 331, 1000, 5000, 65535]
VS = [1e-8, 3e-3, 0.27, 1.0, 9.0, 26.0]
# (m, a): Poisson a = log E with E = 1, 7.5, 0.3; binomial a = N
CONFIGS = {0: [(1.7, 0.0), (-2.3, math.log(7.5)), (6.0, math.log(0.3))],
           1: [(1.7, 1.0), (1.7, 39.0), (1.7, 1000.0), (1.7, 65535.0), (-2.3, 39.0), (-2.3, 65535.0)]}
_TABLE = {}


def _table():
    """The brute-force values of the case table, computed once: {(fam, m, a, v): (ks, pmf)}.  An entry whose integrand has not
    decayed at u = +-14, or is below 1e-200 on all of that grid (the mode of a binomial integrand with thousands of trials lies
    up to 30 prior standard deviations out), is taken on u in [-38, 38] with the same number of nodes instead: there the rule on
    [-14, 14] is a truncated integral."""
    if not _TABLE:
        wide = 0
        for fam, cfgs in CONFIGS.items():
            for m, a in cfgs:
                for v in VS:
                    ks = [k for k in KS if fam == 0 or k <= a]
                    if fam == 1 and int(a) not in ks:
                        ks.append(int(a))
                    vals = [R.brute(fam, m, v, a, k) for k in ks]
                    for i, (val, end) in enumerate(vals):
                        if end > R.BRUTE_END or val < 1e-200:
                            vals[i] = R.brute(fam, m, v, a, ks[i], R.BRUTE_WIDE)
                            assert vals[i][1] <= R.BRUTE_END
                            wide += 1
                    _TABLE[(fam, m, a, v)] = (np.array(ks, np.float64), np.array([x[0] for x in vals]))
        print("brute force: %d cases, %d entries on the wide grid" % (len(_TABLE), wide))
    return _TABLE


@pytest.mark.parametrize("points", [65, 129])
def test_rule_against_brute_force(points):
    """Relative error of the pmf on the case table: both families, v in {1e-8, 3e-3, 0.27, 1, 9, 26}, negative m, E != 1,
    k in {0, 1, 2, 5, 17, 100, 331, 1000, 5000, 65535} (and k = N).  Measured (the brute-force rule's own floor is 1.3e-11):
    P = 65: 2.65e-10 at v <= 9 (Poisson, m = -2.3, E = 7.5, k = 0, v = 9), 7.5e-7 at v = 26 (Poisson, m = 1.7, k = 0);
    P = 129: 1.47e-10 (Poisson, m = -2.3, E = 7.5, k = 65535, v = 0.27: the conditioning of g(eta*), not the rule).  The bars are 4 x those, under
    the caps 1e-8 (P = 65, v <= 9) and 1e-9 (P = 129).  Entries whose brute-force value is below 1e-200 are skipped: 22 of 150
    (Poisson) and 50 of 210 (binomial) at v <= 9 -- nearly all at v = 1e-8 and 3e-3, where a count far from the mean has no
    mass --, none at v = 26; at most a quarter per family and column of the table."""
    assert R.BAR_65_V9 <= 1e-8 and R.BAR_129 <= 1e-9
    worst, where, skipped = {}, {}, {}
    for (fam, m, a, v), (ks, want) in _table().items():
        got = np.exp(R.rule(fam, m, v, a, ks, points=points))
        keep = want >= 1e-200
        col = (fam, "v <= 9" if v <= 9 else "v = 26")
        c = skipped.setdefault(col, [0, 0])
        c[0] += int((~keep).sum())
        c[1] += len(ks)
        assert (got[~keep] < 1e-150).all()                           # the rule has no mass there either
        if keep.any():
            err = np.abs(got - want)[keep] / want[keep]
            if err.max() > worst.get(col[1], 0.0):
                worst[col[1]], where[col[1]] = err.max(), (fam, m, a, v, ks[keep][err.argmax()])
    print("P = %d: worst relative error %s at %s; skipped %s" % (points, worst, where, skipped))
    for col, (gone, total) in skipped.items():
        assert 4 * gone <= total, (col, gone, total)
    if points == 65:
        assert worst["v <= 9"] <= R.BAR_65_V9 and worst["v = 26"] <= R.BAR_65_V26
    else:
        assert max(worst.values()) <= R.BAR_129


@pytest.mark.parametrize("N", [1, 39, 1000])
def test_binomial_pmf_sums_to_one(N):
    """sum_{k = 0}^{N} pmf(k) = 1 to 1e-9: P = 65 at v <= 9, P = 129 at v = 26 (the rule's error at P = 65 there is 7.5e-7)."""
    k = np.arange(N + 1, dtype=np.float64)
    for m, v, points in ((1.7, 0.27, 65), (-2.3, 1.0, 65), (0.4, 9.0, 65), (-6.0, 3e-3, 65), (1.7, 26.0, 129)):
        total = np.exp(R.rule(1, m, v, float(N), k, points=points)).sum()
        print("N = %d, m = %g, v = %g, P = %d: sum - 1 = %.2e" % (N, m, v, points, total - 1.0))
        assert abs(total - 1.0) <= 1e-9
    assert R.rule(1, 0.0, 1.0, float(N), float(N + 1)) == -np.inf                 # k > N: pmf 0


def test_poisson_pmf_sums_to_one_and_has_the_log_normal_mean():
    """m = 1.7, v = 0.27: the rate's 9-sigma point is 600, so the mass beyond k = 1024 is negligible; sum pmf = 1 and
    sum k pmf = E exp(m + v / 2) (relative) to 1e-9."""
    k = np.arange(1025, dtype=np.float64)
    for E in (1.0, 2.5):
        pmf = np.exp(R.rule(0, 1.7, 0.27, math.log(E), k))
        mean = E * math.exp(1.7 + 0.27 / 2)
        print("E = %g: sum - 1 = %.2e, mean error %.2e" % (E, pmf.sum() - 1.0, (k * pmf).sum() / mean - 1.0))
        assert abs(pmf.sum() - 1.0) <= 1e-9
        assert abs((k * pmf).sum() / mean - 1.0) <= 1e-9


def test_fixed_grid_fails_where_the_rule_holds():
    """The reason for a rule of its own: the 129-point grid of mgp_bernoulli_predict with the Poisson pmf as integrand is off by
    more than 10 % at k = 1000, v = 1 (measured: 41 %), where the rule is within its bar."""
    want, end = R.brute(0, 1.7, 1.0, 0.0, 1000)
    assert end <= R.BRUTE_END
    fixed = R.fixed_grid(1.7, 1.0, 0.0, 1000)
    rule = math.exp(R.rule(0, 1.7, 1.0, 0.0, 1000.0))
    print("k = 1000, v = 1: fixed grid off by %.2f, the rule by %.1e" % (abs(fixed - want) / want, abs(rule - want) / want))
    assert abs(fixed - want) / want > 0.1
    assert abs(rule - want) / want <= R.BAR_65_V9
    assert abs(R.fixed_grid(1.7, 1.0, 0.0, 17) - R.brute(0, 1.7, 1.0, 0.0, 17)[0]) <= 1e-9      # and fine at a small count


def _closed_form(fam, m, a, k):
    if fam == 0:
        mu = math.exp(m + a)
        return k * math.log(mu) - mu - math.lgamma(k + 1)
    pi = 1.0 / (1.0 + math.exp(-m))
    return (math.lgamma(a + 1) - math.lgamma(k + 1) - math.lgamma(a - k + 1)) + k * math.log(pi) + (a - k) * math.log1p(-pi)


DEGENERATE = [(0, 1.7, 0.0, 0), (0, 1.7, 0.0, 17), (0, -2.3, math.log(7.5), 3), (0, 4.0, math.log(0.3), 30),
              (1, 1.7, 1.0, 0), (1, 1.7, 1.0, 1), (1, -2.3, 39.0, 5), (1, 0.4, 39.0, 39), (1, 0.4, 39.0, 0)]


@pytest.mark.parametrize("fam, m, a, k", DEGENERATE)
def test_degenerate_branch_and_the_switch(fam, m, a, k):
    """v <= V_MIN = 2^-76, zero and negative variances included: the plain log pmf at eta = m, against the closed form from
    math alone (1e-13 of the sum of the absolute terms).  At the switch the rule and the plain form differ by about
    v (l'^2 + l'') / 2 <= 2^-77 D^2 (D the larger of count and mean): within 1e-12 here, where D <= 40."""
    want = _closed_form(fam, m, a, k)
    for v in (0.0, -1.0, -np.inf, 1e-30, R.V_MIN):
        lp, T, eta, _, _ = R.rule(fam, m, v, a, float(k), full=True)
        assert np.isnan(eta) and abs(lp - want) <= 1e-13 * T, (v, lp, want)
    above = np.nextafter(R.V_MIN, 1.0)
    lp, _, eta, tl, tr = R.rule(fam, m, above, a, float(k), full=True)
    assert np.isfinite(eta) and tl > 0 and tr > 0                                  # the quadrature ran
    print("fam %d m %g k %d: rule just above V_MIN - plain form = %.2e" % (fam, m, k, lp - want))
    assert abs(lp - want) <= 1e-12
    assert np.isnan(R.rule(fam, np.nan, 1.0, a, float(k))) and np.isnan(R.rule(fam, m, np.nan, a, float(k)))


@pytest.mark.parametrize("fam", [0, 1])
def test_mode_iteration_ends_at_a_stationary_point(fam):
    """On inputs drawn as the GPU test draws them the iteration ends by its step rule well inside its 100 steps, and the Newton
    step left at eta* is below 1e-6 sigma_hat.  (Binomial, k = 0 of 65535 trials, m = 3.1, v = 9: Newton's method with the
    bracket alone cycles between m and m - 24; the rule that a step must halve the last one ends that.)"""
    for k0 in (0, 1000):
        m, v, a = R.gpu_inputs(fam, 257, 100 * fam + k0 + 1)
        k = k0 + np.arange(300, dtype=np.float64)
        m, v, a, k = (z.ravel() for z in np.broadcast_arrays(m[:, None], v[:, None], a.astype(np.float64)[:, None], k[None, :]))
        go = (v > R.V_MIN) & ((fam == 0) | (k <= a))
        m, v, a, k = m[go], v[go], a[go], k[go]
        eta, its = R.mode(fam, m, v, a, k)
        l1, l2, _ = R._site(fam, eta, a, k)
        g1, g2 = l1 - (eta - m) / v, l2 - 1 / v
        left = np.abs(g1 / g2) * np.sqrt(-g2)
        print("family %d, k0 = %d: %d entries, %d steps at most, largest step left %.1e sigma_hat" % (fam, k0, go.sum(), its, left.max()))
        assert its <= 60 and left.max() <= 1e-6


@pytest.mark.parametrize("fam", [0, 1])
def test_rounding_constant_of_the_device_bar(fam):
    """c of |log pmf_dev - log pmf_ref| <= c 2^-53 T + r: the restatement in float64 against the same evaluation (g(eta*) and the
    sum at the float64 run's centre and window, P = 129) in numpy.longdouble, in units of 2^-53 T, on inputs drawn as the GPU test
    draws them.  Measured: 10.7 (Poisson: mu* = exp(eta* + a) near 3e4 carries the rounding of eta* + a, about 10 ulp of
    mu*), 11.0 (binomial: N softplus(eta*) likewise).  The recorded constant is 11; the device gets 4 x that, 44."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    worst = 0.0
    for k0 in (0, 1000):
        m, v, a = R.gpu_inputs(fam, 129, 7 + k0)
        k = k0 + np.arange(150, dtype=np.float64)
        args = (fam, m[:, None], v[:, None], a.astype(np.float64)[:, None], k[None, :])
        lp, T, eta, tl, tr = R.rule(*args, points=129, full=True)
        ext = R.rule(*args, points=129, dtype=np.longdouble, at=(eta, tl, tr))
        ok = np.isfinite(lp)
        assert np.array_equal(ok, np.isfinite(ext)) and ok.any()
        c = float((np.abs(lp[ok] - ext[ok]) / (2.0 ** -53 * T[ok])).max())
        print("family %d, k0 = %d: c = %.2f (largest T %.3g)" % (fam, k0, c, T[ok].max()))
        worst = max(worst, c)
    assert worst <= R.MEASURED_C
    assert R.DEVICE_C == max(8.0, 4 * R.MEASURED_C)


# ------------------------------------------------------------------------------------------------ host-side checks
NEW = ("mgp_count_predict_pmf", "mgp_count_predict_logpmf")


def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mgp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert name + "(" in header
        assert hasattr(handle, name)


def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    dbl, flt, byt = (ctypes.c_double * 8)(), (ctypes.c_float * 8)(), (ctypes.c_uint8 * 8)()
    d, f, b = ctypes.addressof(dbl), ctypes.addressof(flt), ctypes.addressof(byt)
    pmf, logpmf = lib.mgp_count_predict_pmf, lib.mgp_count_predict_logpmf
    for fam in (0, 1):
        assert pmf(None, d, f, 4, fam, 0, 2, 65, 0, d, None) == -1
        assert pmf(d, None, f, 4, fam, 0, 2, 65, 0, d, None) == -1
        assert pmf(d, d, f, 4, fam, 0, 2, 65, 0, None, None) == -1
        assert pmf(d, d, f, 0, fam, 0, 2, 65, 0, d, None) == -1
        for K in (0, -1, 65537):
            assert pmf(d, d, f, 4, fam, 0, K, 65, 0, d, None) == -1
        assert pmf(d, d, f, 4, fam, -1, 2, 65, 0, d, None) == -1
        assert pmf(d, d, f, 4, fam, 2 ** 24, 2, 65, 0, d, None) == -1                # k0 + K - 1 = 2^24 + 1
        for points in (15, 16, 64, 259, 258, -65):
            assert pmf(d, d, f, 4, fam, 0, 2, points, 0, d, None) == -1
            assert logpmf(d, d, f, f, None, 4, fam, points, d, None) == -1
        assert logpmf(None, d, f, f, b, 4, fam, 65, d, None) == -1
        assert logpmf(d, None, f, f, b, 4, fam, 65, d, None) == -1
        assert logpmf(d, d, f, None, b, 4, fam, 65, d, None) == -1
        assert logpmf(d, d, f, f, b, 4, fam, 65, None, None) == -1
        assert logpmf(d, d, f, f, b, 0, fam, 65, d, None) == -1
    assert pmf(d, d, None, 4, 1, 0, 2, 65, 0, d, None) == -1                         # binomial without trials
    assert logpmf(d, d, None, f, None, 4, 1, 65, d, None) == -1
    for fam in (2, -1, 7):
        assert pmf(d, d, f, 4, fam, 0, 2, 65, 0, d, None) == -3
        assert logpmf(d, d, f, f, None, 4, fam, 65, d, None) == -3


def _host_fit(family):
    """A CountLaplaceFit of three nodes on host tensors: enough for every check that precedes the first device call"""
    from manifold_gp_amd.counts import CountLaplaceFit
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    desc = Descriptor(data=data, nu=2, kappa=1.0, form=0, noise=0.0)
    extra = torch.tensor([1.0, 3.0, 9.0], dtype=torch.float64)
    aux = extra.log().float() if family == "poisson" else extra.float()
    return CountLaplaceFit(desc, torch.tensor([0.0, 3.0, 7.0]), None, torch.zeros(3), True, 1, [], 0.0, family, 0.5, 1.0, aux, extra)


@pytest.mark.parametrize("family", ["poisson", "binomial"])
def test_python_argument_checks(family):
    from manifold_gp_amd import counts as ct
    fit = _host_fit(family)
    var = torch.full((3,), 0.5, dtype=torch.float64)
    y = torch.tensor([0.0, 3.0, 7.0])
    for bad in (64, 15, 259, 65.0, True, "65"):
        with pytest.raises(ValueError, match="points"):
            fit.predict_pmf(10, points=bad, variance=var)
        with pytest.raises(ValueError, match="points"):
            fit.predict_log_density(y, points=bad, variance=var)
        with pytest.raises(ValueError, match="points"):
            fit.predict_exceedance(3, points=bad, variance=var)
        with pytest.raises(ValueError, match="points"):
            fit.predict_interval(points=bad, variance=var)
        with pytest.raises(ValueError, match="points"):
            ct.count_predict_pmf(var, var, var, family, 0, 3, points=bad)
        with pytest.raises(ValueError, match="points"):
            ct.count_predict_logpmf(var, var, var, y, None, family, points=bad)
    for kmin, kmax in ((0, -1), (5, 4), (-1, 3), (0, 65536), (0, 2 ** 24 + 1), (0, 2.0), (0.0, 2), (True, 2)):
        with pytest.raises(ValueError, match="kmin|kmax"):
            fit.predict_pmf(kmax, kmin=kmin, variance=var)
        with pytest.raises(ValueError, match="kmin|kmax"):
            ct.count_predict_pmf(var, var, var, family, kmin, kmax)
    for bad in (-1, 65536, 2.5, True, torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1, 2]), torch.tensor([1, -2, 3]),
                torch.tensor([1, 2, 65536])):
        with pytest.raises(ValueError, match="threshold"):
            fit.predict_exceedance(bad, variance=var)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="level"):
            fit.predict_interval(level=bad, variance=var)
    with pytest.raises(ValueError, match="kmax"):
        fit.predict_interval(kmax=65536, variance=var)
    nan = float("nan")
    for bad in ([0.0, 0.5, 1.0], [0.0, -1.0, 1.0], [0.0, 2.0 ** 24 + 2, 1.0], [nan, 1.0, 1.0]):
        with pytest.raises(ValueError, match="integers in"):
            fit.predict_log_density(torch.tensor(bad), variance=var)
    with pytest.raises(ValueError, match="integers in"):
        fit.predict_log_density(torch.tensor([nan, 1.0, 1.0]), at=torch.tensor([True, False, True]), variance=var)
    with pytest.raises(ValueError, match="at must be"):
        fit.predict_log_density(y, at=torch.ones(3), variance=var)
    with pytest.raises(ValueError, match="at must be"):
        fit.predict_log_density(y, at=torch.ones(4, dtype=torch.bool), variance=var)
    with pytest.raises(ValueError, match="no node"):
        fit.predict_log_density(y, at=torch.zeros(3, dtype=torch.bool), variance=var)
    with pytest.raises(ValueError):
        fit.predict_log_density(torch.zeros(4), variance=var)
    for bad in (torch.zeros(4, dtype=torch.float64), [0.5, 0.5, 0.5], torch.ones(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="variance"):
            fit.predict_pmf(10, variance=bad)
    if family == "binomial":
        with pytest.raises(ValueError, match="trials"):
            fit.predict_log_density(torch.tensor([2.0, 3.0, 7.0]), variance=var)            # 2 of 1 trial
        with pytest.raises(RuntimeError, match="no CPU path"):                               # the same count outside `at`
            fit.predict_log_density(torch.tensor([2.0, 3.0, 7.0]), at=torch.tensor([False, True, True]), variance=var)
        with pytest.raises(ValueError, match="trials"):
            ct.count_predict_pmf(var, var, None, family, 0, 3)
        with pytest.raises(ValueError, match="trials"):
            ct.count_predict_logpmf(var, var, None, y, None, family)
    with pytest.raises(ValueError, match="family"):
        ct.count_predict_pmf(var, var, var, "negative-binomial", 0, 3)
    # valid arguments on host tensors: the checks pass, the first device call refuses
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.predict_pmf(10, variance=var)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.predict_log_density(y, at=torch.tensor([True, False, True]), variance=var)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.predict_exceedance(torch.tensor([1, 2, 3]), variance=var)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.predict_interval(level=0.5, kmax=20, variance=var)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ct.count_predict_pmf(var, var, var.float(), family, 0, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ct.count_predict_logpmf(var, var, var.float(), y, None, family)
