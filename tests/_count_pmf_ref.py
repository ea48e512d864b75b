"""The predictive count pmf of a count fit (docs/kernels/count_predict.md) in numpy: a restatement of the rule of
csrc/count_predict.hip, operation by operation, and the brute-force rule it is measured against.

With m the linear predictor at the mode (without the exposure), v the latent marginal variance, a = log E (Poisson) or N trials
(binomial), the log-integrand in eta is

    poisson:   g = k (eta + a) - exp(eta + a) - lgamma(k + 1) - (eta - m)^2 / 2v
    binomial:  g = log C(N, k) - k softplus(-eta) - (N - k) softplus(eta) - (eta - m)^2 / 2v

and pmf(k) = (2 pi v)^-1/2 int exp(g) d eta.  The rule: a safeguarded Newton iteration to the mode eta* of g, a window
[eta* - t_L, eta* + t_R] on whose ends g has dropped by 40, and the P-point trapezoid rule on exp(g(eta* + t) - g(eta*)) with the
difference formed without cancellation.  v <= V_MIN (zero and negative variances included) is the plain log pmf at eta = m.

`rule(..., dtype=numpy.longdouble, at=...)` evaluates g(eta*) and the sum in extended precision at a given centre and window: the
rounding of the float64 evaluation alone, which is what the constant c of the GPU test's bar measures."""
import math

import numpy as np

V_MIN = 2.0 ** -76          # v D^2 / 2 <= 2^-53 D for counts and means D <= 2^24: the two forms agree to rounding (count_predict.md)
DROP = 40.0                 # the window ends where g has dropped by this much
NEWTON_MAX = 100
DOUBLE_MAX = 40
BISECT = 6
STEP_TOL = 1e-8             # a Newton step below STEP_TOL sigma_hat (+ 4 ulp of eta) ends the iteration
ETA_MAX = 700.0
POINTS = 65

# worst relative errors of the rule against the brute-force rule on the case table of test_count_pmf_cpu.py (measured there,
# printed by it), and the bars at 4 x the measured value
MEASURED_65_V9, MEASURED_65_V26, MEASURED_129 = 2.7e-10, 7.5e-7, 1.5e-10
BAR_65_V9, BAR_65_V26, BAR_129 = 4 * MEASURED_65_V9, 4 * MEASURED_65_V26, 4 * MEASURED_129
# c of the GPU bar: the largest |float64 - longdouble| / (2^-53 T) of the restatement at one centre and window (measured in
# test_count_pmf_cpu.py); the device gets 4 x that and no less than 8
MEASURED_C = 11.0
DEVICE_C = max(8.0, 4 * MEASURED_C)

_lgamma64 = np.vectorize(math.lgamma, otypes=[np.float64])
_STIRLING = [1.0 / 12, -1.0 / 360, 1.0 / 1260, -1.0 / 1680, 1.0 / 1188, -691.0 / 360360, 1.0 / 156]


def lgamma(x, dtype=np.float64):
    """log Gamma(x) for x >= 1; float64: libm's, longdouble: the recurrence up to x >= 32 and Stirling's series there"""
    x = np.asarray(x, dtype)
    if dtype == np.float64:
        return _lgamma64(x)
    shift = np.zeros_like(x)
    z = x.copy()
    for _ in range(32):
        low = z < 32
        if not low.any():
            break
        shift = np.where(low, shift + np.log(np.where(low, z, 1)), shift)
        z = np.where(low, z + 1, z)
    half_log_2pi = np.log(2 * np.arccos(dtype(-1))) / 2
    s = (z - dtype(0.5)) * np.log(z) - z + half_log_2pi
    zi, z2 = 1 / z, 1 / (z * z)
    for num in _STIRLING:
        s = s + np.asarray(num, dtype) * zi
        zi = zi * z2
    return s - shift


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _site(fam, eta, a, k):
    """(l', l'', q): the derivatives of the log-likelihood in eta and mu (Poisson) or (pi, 1 - pi) (binomial)"""
    if fam == 0:
        mu = np.exp(np.minimum(eta + a, ETA_MAX))
        return k - mu, -mu, mu
    e = np.exp(-np.abs(eta))
    d = 1 + e
    pi = np.where(eta >= 0, 1 / d, e / d)
    pib = np.where(eta >= 0, e / d, 1 / d)
    return k * pib - (a - k) * pi, -(a * e / (d * d)), (pi, pib)


def _const(fam, a, k, dtype):
    """(-lgamma(k + 1) or log C(N, k), the sum of the absolute values of its terms)"""
    if fam == 0:
        lg = lgamma(k + 1, dtype)
        return -lg, lg
    t = [lgamma(a + 1, dtype), lgamma(k + 1, dtype), lgamma(a - k + 1, dtype)]
    return t[0] - t[1] - t[2], t[0] + t[1] + t[2]


def _loglik(fam, eta, a, k, dtype):
    """(log p(k | eta), the sum of the absolute values of its terms)"""
    c, ac = _const(fam, a, k, dtype)
    if fam == 0:
        mu = np.exp(np.minimum(eta + a, ETA_MAX))
        return k * (eta + a) - mu + c, np.abs(k * (eta + a)) + mu + ac
    t1, t2 = k * _softplus(-eta), (a - k) * _softplus(eta)
    return c - t1 - t2, ac + t1 + t2


def _drop(fam, t, k, a, q, eta, dm, v):
    """g(eta* + t) - g(eta*) without cancellation"""
    quad = t * (2 * dm + t) / (2 * v)
    with np.errstate(over="ignore", invalid="ignore"):
        if fam == 0:
            return k * t - q * np.expm1(t) - quad
        pos = eta >= 0                      # softplus(eta + t) - softplus(eta) = log1p(pi expm1(t)) = t + log1p((1 - pi) expm1(-t))
        lg = np.log1p(np.where(pos, q[1], q[0]) * np.expm1(np.where(pos, -t, t)))
        return np.where(pos, -(a - k) * t, k * t) - a * lg - quad


def mode(fam, m, v, a, k):
    """(eta*, the Newton steps taken): the root of g' by Newton's method inside a bracket, bisection where a step leaves it (and,
    binomial, where it is more than half the previous one: from eta = m with k = 0 of 65535 trials a plain Newton iteration
    cycles between m and m - v N pi inside the bracket)"""
    eps = np.finfo(np.float64).eps
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if fam == 0:
            lk = np.log(k) - a
            x = np.where(k > 0, np.maximum(m, lk), m)
            lo = np.where(k > 0, np.minimum(m, lk), m - v * np.exp(np.minimum(m + a, ETA_MAX)))
            hi = x.copy()
        else:
            inner = (k > 0) & (k < a)
            lg = np.log(k) - np.log(a - k)
            x = np.where(inner, lg, m)
            lo = np.where(inner, np.minimum(m, lg), np.where(k > 0, m, m - v * a))
            hi = np.where(inner, np.maximum(m, lg), np.where(k > 0, m + v * a, m))
        done = np.zeros(x.shape, bool)
        dxold = hi - lo
        its = 0
        for its in range(NEWTON_MAX):
            if done.all():
                break
            l1, l2, _ = _site(fam, x, a, k)
            g1 = l1 - (x - m) / v
            g2 = l2 - 1 / v
            lo = np.where(g1 > 0, x, lo)
            hi = np.where(g1 < 0, x, hi)
            step = g1 / g2
            conv = np.abs(step) <= STEP_TOL / np.sqrt(-g2) + 4 * eps * np.abs(x)
            xn = x - step
            ok = (xn > lo) & (xn < hi)
            if fam == 1:                      # g' is not concave: a step that does not halve the last one is not trusted either
                ok = ok & (np.abs(step) <= 0.5 * dxold)
            xn = np.where(conv | ok, xn, 0.5 * (lo + hi))
            dxold = np.where(done, dxold, np.abs(xn - x))
            x = np.where(done, x, xn)
            done = done | conv
    return x, its


def window(fam, m, v, a, k, eta):
    """(t_L, t_R, q, dm) at the centre eta"""
    l1, l2, q = _site(fam, eta, a, k)
    dm = eta - m
    sig = 1 / np.sqrt(-(l2 - 1 / v))
    out = []
    for sign in (-1.0, 1.0):
        lo, hi = np.zeros_like(sig), sig.copy()
        for _ in range(DOUBLE_MAX):
            need = _drop(fam, sign * hi, k, a, q, eta, dm, v) > -DROP
            if not need.any():
                break
            lo = np.where(need, hi, lo)
            hi = np.where(need, 2 * hi, hi)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            reached = _drop(fam, sign * mid, k, a, q, eta, dm, v) <= -DROP
            hi = np.where(reached, mid, hi)
            lo = np.where(reached, lo, mid)
        out.append(hi)
    return out[0], out[1]


def _sum(fam, m, v, a, k, eta, tl, tr, points, dtype):
    """(log pmf, T) of the trapezoid sum at a given centre and window, in dtype"""
    m, v, a, k, eta, tl, tr = (np.asarray(z, dtype) for z in (m, v, a, k, eta, tl, tr))
    _, _, q = _site(fam, eta, a, k)
    dm = eta - m
    h = (tl + tr) / dtype(points - 1)
    s = np.zeros_like(eta)
    for j in range(points):
        t = -tl + dtype(j) * h
        w = dtype(0.5) if j in (0, points - 1) else dtype(1)
        s = s + w * np.exp(_drop(fam, t, k, a, q, eta, dm, v))
    ll, al = _loglik(fam, eta, a, k, dtype)
    quad = dm * dm / (2 * v)
    two_pi = 2 * np.arccos(dtype(-1))
    return ll - quad + np.log(h * s / np.sqrt(two_pi * v)), al + quad + 1


def rule(fam, m, v, a, k, points=POINTS, dtype=np.float64, at=None, full=False):
    """log pmf(k) by the rule, float64 arrays broadcast against each other; fam 0: a = log-exposure, fam 1: a = trials.
    k > N gives -inf; v <= V_MIN the plain log pmf at eta = m; NaN in m or v gives NaN.
    at = (eta*, t_L, t_R): evaluate at this centre and window (from a float64 call with full=True) instead of searching.
    full: returns (log pmf, T, eta*, t_L, t_R), T the sum of the absolute terms of g(eta*) plus 1."""
    m, v, a, k = np.broadcast_arrays(*(np.asarray(z, np.float64) for z in (m, v, a, k)))
    shape = m.shape
    m, v, a, k = (z.reshape(-1).copy() for z in (m, v, a, k))
    out = np.full(m.shape, np.nan, dtype)
    T = np.ones(m.shape, dtype)
    eta, tl, tr = (np.full(m.shape, np.nan) for _ in range(3))
    nan = np.isnan(m) | np.isnan(v)
    over = (k > a) & ~nan if fam == 1 else np.zeros(m.shape, bool)
    out[over] = -np.inf
    deg = ~nan & ~over & (v <= V_MIN)
    if deg.any():
        out[deg], T[deg] = _loglik(fam, np.asarray(m[deg], dtype), np.asarray(a[deg], dtype), np.asarray(k[deg], dtype), dtype)
        T[deg] += 1
    go = ~nan & ~over & ~deg
    if go.any():
        mm, vv, aa, kk = m[go], v[go], a[go], k[go]
        if at is None:
            e, _ = mode(fam, mm, vv, aa, kk)
            l, r = window(fam, mm, vv, aa, kk, e)
        else:
            e, l, r = (np.asarray(z, np.float64).reshape(-1)[go] for z in at)
        out[go], T[go] = _sum(fam, mm, vv, aa, kk, e, l, r, points, dtype)
        eta[go], tl[go], tr[go] = e, l, r
    if full:
        return tuple(z.reshape(shape) for z in (out, T, eta, tl, tr))
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------------ brute force
BRUTE_POINTS = 2_000_001
BRUTE_WIDE = 38.0
BRUTE_END = 1e-25             # an end value above this fraction of the maximum: the grid [-14, 14] truncates the integrand
_GRID = {}


def _grid(fam, m, v, a, half):
    """the quantities of the brute-force rule that do not depend on k: the nodes, log phi(u) and the likelihood's pieces"""
    key = (fam, float(m), float(v), float(a), half)
    if key not in _GRID:
        _GRID.clear()                                   # one grid at a time: 2M doubles each
        u = np.linspace(-half, half, BRUTE_POINTS)
        eta = m + math.sqrt(v) * u
        lphi = -0.5 * u * u - 0.5 * math.log(2 * math.pi)
        if fam == 0:
            _GRID[key] = (u, lphi, eta + a, np.exp(eta + a))
        else:
            _GRID[key] = (u, lphi, _softplus(-eta), _softplus(eta))
    return _GRID[key]


def brute(fam, m, v, a, k, half=14.0):
    """(pmf(k), end) by the 2 000 001-point trapezoid rule on u in [-half, half], eta = m + sqrt(v) u; scalars.  end: the larger
    of the integrand's two end values over its maximum -- where that is not negligible the integrand reaches past the grid and
    the value is a truncated integral (BRUTE_WIDE covers every count up to 2^24 at v <= 26: phi(38) = 1e-314)."""
    u, lphi, p, q = _grid(fam, m, v, a, half)
    if fam == 0:
        e = k * p - q - math.lgamma(k + 1) + lphi
    else:
        e = (math.lgamma(a + 1) - math.lgamma(k + 1) - math.lgamma(a - k + 1)) - k * p - (a - k) * q + lphi
    f = np.exp(e)
    top = f.max()
    return float((f.sum() - 0.5 * (f[0] + f[-1])) * (u[1] - u[0])), (max(f[0], f[-1]) / top if top > 0 else 0.0)


def fixed_grid(m, v, a, k, points=129):
    """The Poisson pmf by the fixed trapezoid grid of mgp_bernoulli_predict (u in [-8, 8]): the shortcut that fails"""
    u = np.linspace(-8.0, 8.0, points)
    eta = m + math.sqrt(v) * u + a
    f = np.exp(k * eta - np.exp(eta) - math.lgamma(k + 1) - 0.5 * u * u) / math.sqrt(2 * math.pi)
    return float(f.sum() * (u[1] - u[0]))


def gpu_inputs(fam, n, seed):
    """(m, v, a) of the device tests: m uniform in [-6, 9], v from the eight values (0 and -1: the degenerate branch), float32
    log-exposures of E in [0.5, 20] or trials from {1, 2, 39, 1000, 65535}"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-6.0, 9.0, n)
    v = rng.choice([0.0, -1.0, 1e-8, 3e-3, 0.27, 1.0, 9.0, 26.0], n)
    if fam == 0:
        a = np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32)
    else:
        a = rng.choice([1.0, 2.0, 39.0, 1000.0, 65535.0], n).astype(np.float32)
    return m, v, a


def quantiles(pmf, level):
    """(lo, hi, reached) of predict_interval from a pmf block [n, K] whose first column is the count 0"""
    cdf = np.cumsum(pmf, axis=1)
    ql, qh = (1.0 - level) / 2.0, (1.0 + level) / 2.0
    lo = (cdf < ql).sum(1)
    hi = (cdf < qh).sum(1)
    reached = hi < pmf.shape[1]
    return np.where(lo < pmf.shape[1], lo, -1), np.where(reached, hi, -1), reached
