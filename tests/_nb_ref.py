"""float64 restatement of the negative-binomial family of manifold_gp_amd/counts.py (docs/kernels/counts.md, count_predict.md,
evidence.md): the per-node formulas of mgp_nb_site and mgp_nb_evidence_site, a dense Newton iteration, the fit's own loop on
dense stand-ins, the constant c(k, r) and the quadrature of mgp_nb_predict_pmf operation by operation, a brute-force rule, and
the dense Laplace evidence with its gradient.  Test infrastructure, sized for the dumbbell fixtures.

    y ~ NB(mean mu = E exp(f + mean), dispersion r),   z = f + mean + log E - log r,   pi = sigma(z) = mu / (r + mu)
    l = -y softplus(-z) - r softplus(z) (+ c(y, r)),   g = y (1 - pi) - r pi,   h = (y + r) pi (1 - pi),   h' = h ((1 - pi) - pi)

the binomial arithmetic with y + r trials and r failures at the shifted predictor z."""
import math

import numpy as np

import _count_pmf_ref as pref
import _counts_ref as cref
import _evidence_ref as eref

FAMILY = "negative_binomial"
R_MIN, R_MAX = 2.0 ** -10, 2.0 ** 20
SEED, R_TRUE = 23, 2.0          # the redraw of _counts_ref.counts as negative binomial (nb_counts)
# the prior marginal variance the fixture's precision is scaled to in the tests of this family: the truth's is 1.44.  At the 9 of
# the other fits' tests the latent field absorbs the overdispersion and the evidence grows all the way to r = 2^20
PRIOR_VARIANCE = 1.0
PROFILE = [0.5, 1.0, 2.0, 4.0, 16.0, 2.0 ** 20]     # the candidates of the dispersion_profile test
SMALL_K = 32                    # c(k, r): the sum of logarithms below, Stirling differences from here (csrc/count_predict.hip)

# The figures the tests of the negative-binomial pmf rest on, each measured by the test named and printed by it.
# c(k, r) of log_const against mpmath at 30 digits on the table of test_nb_cpu.py::test_log_constant_against_mpmath, in units of
# 2^-53 (1 + |c| + k |log r| + k); the bar of the issue is 8
MEASURED_CONST = 0.78
# worst relative error of rule() against brute() on the case table of test_nb_cpu.py::test_rule_against_brute_force at P = 129
# (2.16e-10 at r = 2^20, m = -2.3, E = 7.5, v = 0.27, k = 60000: the conditioning of g(z*), not the rule; the brute-force
# rule's own floor is about 1e-11), and r_129 of the device bar at 4 x that
MEASURED_129 = 2.2e-10
BAR_129 = 4 * MEASURED_129
# c of the device bar: the largest |float64 - longdouble| / (2^-53 T) of rule() at one centre and window
# (test_nb_cpu.py::test_rounding_constant_of_the_device_bar); the device gets 4 x that and no less than 8
MEASURED_C = 9.1                # (9.09 at r = 0.37, counts from 0)
DEVICE_C = max(8.0, 4 * MEASURED_C)


def log_r(r):
    """log r as the C entry points form it: libm's log of the double"""
    return math.log(r)


# ------------------------------------------------------------------------------------------------ the site
def site(f, y, aux, obs, mean, r):
    """(l, g, h, h', mass) per node in float64, all 0 at unobserved nodes; l without c(y, r).  mass = y + r: the size of the terms
    g is the difference of.  aux: the log-exposure (None: zeros)."""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else obs
    y = np.where(obs, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    a = np.zeros_like(f) if aux is None else np.where(obs, np.nan_to_num(np.asarray(aux, np.float64)), 0.0)
    z = f + mean + a - log_r(r)
    N = y + r
    e = np.exp(-np.abs(z))
    d = 1.0 + e
    l1 = np.log1p(e)
    pi = np.where(z >= 0, 1.0 / d, e / d)
    pib = np.where(z >= 0, e / d, 1.0 / d)
    l = -r * (np.maximum(z, 0.0) + l1) - y * (np.maximum(-z, 0.0) + l1)
    g = y * pib - r * pi
    h = N * e / (d * d)
    gap = -np.expm1(-np.abs(z)) / d
    hp = h * np.where(z >= 0, -gap, gap)
    zero = np.zeros_like(f)
    return tuple(np.where(obs, t, zero) for t in (l, g, h, hp, N))


def site_outputs(f, qf, y, aux, obs, s_ref, mean, r):
    """What mgp_nb_site leaves, as _counts_ref.site_outputs states it for mgp_count_site"""
    f = np.asarray(f, np.float64)
    qf = np.zeros_like(f) if qf is None else np.asarray(qf, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    l, g, h, _, mass = site(f, y, aux, seen, mean, r)
    res = g - qf
    with np.errstate(over="ignore"):
        sq = (res * res).sum()
    sums = np.array([l.sum(), (f * qf).sum(), np.abs(res).max(), sq])
    scale = np.array([np.abs(l).sum(), np.abs(f * qf).sum(), np.abs(res).max(), sq])
    yy = np.where(seen, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    return cref.to_f32(s_ref * h), cref.to_f32(s_ref * res), sums, scale, s_ref * (mass + yy + np.abs(qf))


def evidence_outputs(f, y, aux, obs, var, mean, r, h_floor=eref.H_FLOOR):
    """What mgp_nb_evidence_site leaves, as _evidence_ref.site_outputs states it for mgp_laplace_evidence_site"""
    f = np.asarray(f, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    l, _, h, hp, _ = site(f, y, aux, seen, mean, r)
    eff = seen & (h >= h_floor)
    root = np.where(eff, cref.to_f32(np.sqrt(h)), np.float32(0.0)).astype(np.float32)
    if var is None:
        corr, c = None, np.zeros_like(f)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.where(eff, np.clip(np.where(eff, np.asarray(var, np.float64), 0.0) * hp, -cref.FLT_MAX, cref.FLT_MAX), 0.0)
        corr = c.astype(np.float32)
    sums = np.array([l.sum(), float(eff.sum()), c.sum(), np.abs(c).max()])
    scale = np.array([np.abs(l).sum(), float(eff.sum()), np.abs(c).sum(), np.abs(c).max()])
    return root, corr, sums, scale, eff


# ------------------------------------------------------------------------------------------------ c(k, r)
_STIRLING = (1.0 / 12, -1.0 / 360, 1.0 / 1260, -1.0 / 1680, 1.0 / 1188, -691.0 / 360360)


def _stirling_s(x, dtype):
    """lgamma(x) - ((x - 1/2) log x - x + log(2 pi) / 2) for x >= 32, the Horner form of the device"""
    zi = 1 / x
    z2 = zi * zi
    s = np.asarray(_STIRLING[5], dtype)
    for c in _STIRLING[4::-1]:
        s = np.asarray(c, dtype) + z2 * s
    return zi * s


def log_const(k, r, dtype=np.float64):
    """(c(k, r) = lgamma(k + r) - lgamma(r) - lgamma(k + 1), the sum of the absolute values of its terms) with the operations of
    nb_const (csrc/count_predict.hip): k < 32 the sum of log((r + j) / (j + 1)), j ascending; beyond it lgamma(k + r) paired with
    the larger of the two other arguments through Stirling's formula.  k an array of integers >= 0, r a scalar."""
    k = np.asarray(k, dtype)
    r = dtype(r)
    lr, lgr = (dtype(log_r(float(r))), dtype(math.lgamma(float(r)))) if dtype == np.float64 else (np.log(r), pref.lgamma(r, dtype))
    c, ac = np.zeros(k.shape, dtype), np.zeros(k.shape, dtype)
    for j in range(SMALL_K - 1):
        t = np.log((r + dtype(j)) / dtype(j + 1))
        c = np.where(k > j, c + t, c)
        ac = np.where(k > j, ac + abs(t), ac)
    kk = np.maximum(k, dtype(SMALL_K))                  # (the branch not taken stays finite)
    x = kk + r
    with np.errstate(invalid="ignore", divide="ignore"):
        rr = np.maximum(r, dtype(SMALL_K))
        tb = [(x - dtype(0.5)) * np.log1p(kk / r), kk * lr, -kk, _stirling_s(x, dtype) - _stirling_s(rr, dtype), -pref.lgamma(kk + 1, dtype)]
        y, d = kk + 1, r - 1
        ta = [(x - dtype(0.5)) * np.log1p(d / y), d * np.log(y), -d * np.ones_like(kk), _stirling_s(x, dtype) - _stirling_s(y, dtype),
              -lgr * np.ones_like(kk)]
    big_r = tb[0] + tb[1] + tb[2] + tb[3] + tb[4]
    big_k = ta[0] + ta[1] + ta[2] + ta[3] + ta[4]
    abs_r, abs_k = sum(np.abs(t) for t in tb), sum(np.abs(t) for t in ta)
    pair_r = r >= kk + 1
    return (np.where(k < SMALL_K, c, np.where(pair_r, big_r, big_k)),
            np.where(k < SMALL_K, ac, np.where(pair_r, abs_r, abs_k)))


def constant(y, obs, r):
    """sum_obs c(y, r)"""
    obs = np.ones(np.shape(y), bool) if obs is None else obs
    return float(log_const(np.asarray(y, np.float64)[obs], r)[0].sum())


# ------------------------------------------------------------------------------------------------ the data and the dense fit
def nb_counts(g, seed=SEED, r=R_TRUE):
    """The counts of _counts_ref.counts on a fixture (ftrue, exposures in [0.5, 20], 10 % observed) redrawn as negative binomial
    with mean E exp(1 + ftrue) and dispersion r, from a seed of their own"""
    c = cref.counts(g)
    rng = np.random.default_rng(seed)
    mu = c["E"] * np.exp(1.0 + c["ftrue"])
    return dict(c, y=rng.negative_binomial(r, r / (r + mu)).astype(np.float64))


def data(c, r):
    """The negative-binomial problem of nb_counts() at the dispersion r: what the device reads (aux = float32 log-exposure), the
    default mean, s_ref and the constant of the likelihood"""
    obs = c["obs"]
    mean = float(np.log(c["y"][obs].sum() / c["E"][obs].sum()))
    s_ref = 4.0 * 2.0 ** -cref.ceil_log2(math.ceil(c["y"][obs].max() + r))
    return dict(family=FAMILY, y=c["y"], aux=np.log(c["E"]).astype(np.float32).astype(np.float64), obs=obs, mean=mean, s_ref=s_ref,
                r=float(r), const=constant(c["y"], obs, r))


def _s(f, d):
    return site(f, d["y"], d["aux"], d["obs"], d["mean"], d["r"])


def psi(Q, f, d):
    return _s(f, d)[0].sum() - 0.5 * f @ (Q @ f)


def gradient(Q, f, d):
    return _s(f, d)[1] - Q @ f


def curvature(f, d):
    return _s(f, d)[2]


def log_likelihood(f, d):
    return _s(f, d)[0].sum() + d["const"]


def newton(Q, d, f0=None, gtol=1e-11, max_steps=100):
    """_counts_ref.newton for this family: dense float64 Newton with step halving on psi until max |g - Q f| <= gtol"""
    f = np.zeros(Q.shape[0]) if f0 is None else np.array(f0, np.float64)
    trace = []
    for _ in range(max_steps):
        res = gradient(Q, f, d)
        if np.abs(res).max() <= gtol:
            break
        delta = np.linalg.solve(Q + np.diag(curvature(f, d)), res)
        cur, step = psi(Q, f, d), 1.0
        while psi(Q, f + step * delta, d) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        f = f + step * delta
        trace.append((psi(Q, f, d), np.abs(gradient(Q, f, d)).max(), step))
        if np.abs(step * delta).max() <= 1e-15 * max(1.0, np.abs(f).max()):
            break
    return f, trace


def simulate(Q, d, f0=None, step_tol=1e-3, max_newton=30):
    """_counts_ref.simulate for this family: the fit's own loop on dense stand-ins rounded to float32 where the device's are, the
    linear solve exact.  Returns (f float32, converged, steps, history)."""
    from manifold_gp_amd.classification import _newton
    n, s_ref = Q.shape[0], d["s_ref"]

    def site_(f, qf):
        w, rhs, sums, _, _ = site_outputs(f, qf, d["y"], d["aux"], d["obs"], s_ref, d["mean"], d["r"])
        return w, rhs, sums.tolist()

    def q2(f):
        return (Q @ f.astype(np.float64)).astype(np.float32)

    def solve(w, rhs):
        return np.linalg.solve(np.diag(w.astype(np.float64)) + s_ref * Q, rhs.astype(np.float64)).astype(np.float32), 0

    start = None if f0 is None else np.asarray(f0, np.float32)
    f, _, _, converged, its, history = _newton("simulate", site_, q2, solve, np.zeros(n, np.float32), start, 0.0, max_newton,
                                               step_tol=step_tol)
    return f, converged, its, history


# ------------------------------------------------------------------------------------------------ the dense evidence
def log_z(Q, f, d):
    """dict(value, log_likelihood, quad, logdet, m) of the dense Laplace evidence at the point f (_evidence_ref.log_z)"""
    l, _, h, _, _ = _s(f, d)
    eff = d["obs"] & (h >= eref.H_FLOOR)
    ll, quad, ld = float(l.sum()) + d["const"], 0.5 * float(f @ (Q @ f)), eref.logdet_b(Q, h, eff)
    return dict(value=ll - quad - 0.5 * ld, log_likelihood=ll, quad=quad, logdet=ld, m=int(eff.sum()))


def mode_log_z(Q, d, f0=None):
    """(mode, log_z at it)"""
    f = newton(Q, d, f0=f0)[0]
    return f, log_z(Q, f, d)


def predict_mean(eta, v, E, r):
    """(mean, variance) of a new count in closed form: m = E exp(eta + v / 2), var = m + m^2 (e^v - 1) + m^2 e^v / r"""
    m = E * np.exp(eta + 0.5 * v)
    return m, m + m * m * np.expm1(v) + m * m * np.exp(v) / r


# ------------------------------------------------------------------------------------------------ the pmf rule
def _site_z(z, A, k, r):
    """(l', l'', (pi, 1 - pi)) in the variable z with A = k + r trials and r failures"""
    e = np.exp(-np.abs(z))
    d = 1 + e
    pi = np.where(z >= 0, 1 / d, e / d)
    pib = np.where(z >= 0, e / d, 1 / d)
    return k * pib - r * pi, -(A * e / (d * d)), (pi, pib)


def _loglik(z, k, r, dtype):
    """(log p(k | z) with c(k, r), the sum of the absolute values of its terms)"""
    c, ac = log_const(k, r, dtype)
    t1, t2 = k * pref._softplus(-z), r * pref._softplus(z)
    return c - t1 - t2, ac + t1 + t2


def _drop(t, k, A, r, q, z, dm, v):
    """g(z* + t) - g(z*) without cancellation: _count_pmf_ref._drop with r in the place of N - k"""
    quad = t * (2 * dm + t) / (2 * v)
    with np.errstate(over="ignore", invalid="ignore"):
        pos = z >= 0
        lg = np.log1p(np.where(pos, q[1], q[0]) * np.expm1(np.where(pos, -t, t)))
        return np.where(pos, -r * t, k * t) - A * lg - quad


def mode(m, v, k, r):
    """(z*, the Newton steps taken) for the shifted mean m = eta + a - log r: the bracket is m and log k - log r for k > 0,
    m - v r and m for k = 0; a step that leaves it or does not halve the last one is a bisection"""
    eps = np.finfo(np.float64).eps
    A = k + r
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inner = k > 0
        lg = np.log(k) - log_r(r)
        x = np.where(inner, lg, m)
        lo = np.where(inner, np.minimum(m, lg), m - v * A)
        hi = np.where(inner, np.maximum(m, lg), m)
        done = np.zeros(x.shape, bool)
        dxold = hi - lo
        its = 0
        for its in range(pref.NEWTON_MAX):
            if done.all():
                break
            l1, l2, _ = _site_z(x, A, k, r)
            g1 = l1 - (x - m) / v
            g2 = l2 - 1 / v
            lo = np.where(g1 > 0, x, lo)
            hi = np.where(g1 < 0, x, hi)
            step = g1 / g2
            conv = np.abs(step) <= pref.STEP_TOL / np.sqrt(-g2) + 4 * eps * np.abs(x)
            xn = x - step
            ok = (xn > lo) & (xn < hi) & (np.abs(step) <= 0.5 * dxold)
            xn = np.where(conv | ok, xn, 0.5 * (lo + hi))
            dxold = np.where(done, dxold, np.abs(xn - x))
            x = np.where(done, x, xn)
            done = done | conv
    return x, its


def window(m, v, k, r, z):
    """(t_L, t_R) at the centre z"""
    A = k + r
    _, l2, q = _site_z(z, A, k, r)
    dm = z - m
    sig = 1 / np.sqrt(-(l2 - 1 / v))
    out = []
    for sign in (-1.0, 1.0):
        lo, hi = np.zeros_like(sig), sig.copy()
        for _ in range(pref.DOUBLE_MAX):
            need = _drop(sign * hi, k, A, r, q, z, dm, v) > -pref.DROP
            if not need.any():
                break
            lo = np.where(need, hi, lo)
            hi = np.where(need, 2 * hi, hi)
        for _ in range(pref.BISECT):
            mid = 0.5 * (lo + hi)
            reached = _drop(sign * mid, k, A, r, q, z, dm, v) <= -pref.DROP
            hi = np.where(reached, mid, hi)
            lo = np.where(reached, lo, mid)
        out.append(hi)
    return out[0], out[1]


def _sum(m, v, k, r, z, tl, tr, points, dtype):
    """(log pmf, T) of the trapezoid sum at a given centre and window, in dtype"""
    m, v, k, z, tl, tr = (np.asarray(t, dtype) for t in (m, v, k, z, tl, tr))
    rr = dtype(r)
    A = k + rr
    _, _, q = _site_z(z, A, k, rr)
    dm = z - m
    h = (tl + tr) / dtype(points - 1)
    s = np.zeros_like(z)
    for j in range(points):
        t = -tl + dtype(j) * h
        w = dtype(0.5) if j in (0, points - 1) else dtype(1)
        s = s + w * np.exp(_drop(t, k, A, rr, q, z, dm, v))
    ll, al = _loglik(z, k, r, dtype)
    quad = dm * dm / (2 * v)
    two_pi = 2 * np.arccos(dtype(-1))
    return ll - quad + np.log(h * s / np.sqrt(two_pi * v)), al + quad + 1


def rule(m, v, a, k, r, points=pref.POINTS, dtype=np.float64, at=None, full=False):
    """log pmf(k) by the rule of mgp_nb_predict_pmf, float64 arrays broadcast against each other; a the log-exposure, r the scalar
    dispersion.  v <= V_MIN gives the plain log pmf at eta = m; NaN in m, v or k gives NaN.  at = (z*, t_L, t_R): evaluate at this
    centre and window (from a float64 call with full=True).  full: returns (log pmf, T, z*, t_L, t_R), T the sum of the absolute
    terms of g(z*) plus 1."""
    m, v, a, k = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (m, v, a, k)))
    shape = m.shape
    m, v, a, k = (t.reshape(-1).copy() for t in (m, v, a, k))
    nan = np.isnan(m) | np.isnan(v) | np.isnan(k)
    m = m + a - log_r(r)                                # the binomial problem in z = eta + a - log r
    out = np.full(m.shape, np.nan, dtype)
    T = np.ones(m.shape, dtype)
    zs, tl, tr = (np.full(m.shape, np.nan) for _ in range(3))
    deg = ~nan & (v <= pref.V_MIN)
    if deg.any():
        out[deg], T[deg] = _loglik(np.asarray(m[deg], dtype), np.asarray(k[deg], dtype), r, dtype)
        T[deg] += 1
    go = ~nan & ~deg
    if go.any():
        mm, vv, kk = m[go], v[go], k[go]
        if at is None:
            e, _ = mode(mm, vv, kk, r)
            lft, rgt = window(mm, vv, kk, r, e)
        else:
            e, lft, rgt = (np.asarray(t, np.float64).reshape(-1)[go] for t in at)
        out[go], T[go] = _sum(mm, vv, kk, r, e, lft, rgt, points, dtype)
        zs[go], tl[go], tr[go] = e, lft, rgt
    if full:
        return tuple(t.reshape(shape) for t in (out, T, zs, tl, tr))
    return out.reshape(shape)


def plain(m, a, k, r):
    """log NB(k; mean exp(m + a), r) by mpmath at 30 digits (lgamma's plain difference loses 1e-9 at r = 2^20)"""
    import mpmath
    mpmath.mp.dps = 30
    mu, r = mpmath.exp(mpmath.mpf(m) + mpmath.mpf(a)), mpmath.mpf(r)
    return float(mpmath.loggamma(k + r) - mpmath.loggamma(r) - mpmath.loggamma(k + 1) + k * mpmath.log(mu / (r + mu))
                 + r * mpmath.log(r / (r + mu)))


_GRID = {}


def brute(m, v, a, k, r, half=14.0):
    """(pmf(k), end) by the 2 000 001-point trapezoid rule of _count_pmf_ref.brute on u in [-half, half], eta = m + sqrt(v) u,
    the constant by mpmath-free means: log_const in long double, rounded.  Scalars."""
    key = (float(m), float(v), float(a), float(r), half)
    if key not in _GRID:
        _GRID.clear()
        u = np.linspace(-half, half, pref.BRUTE_POINTS)
        z = m + math.sqrt(v) * u + a - math.log(r)
        _GRID[key] = (u, -0.5 * u * u - 0.5 * math.log(2 * math.pi), pref._softplus(-z), pref._softplus(z))
    u, lphi, p, q = _GRID[key]
    c = float(log_const(np.array([float(k)]), r, np.longdouble)[0][0])
    f = np.exp(c - k * p - r * q + lphi)
    top = f.max()
    return float((f.sum() - 0.5 * (f[0] + f[-1])) * (u[1] - u[0])), (max(f[0], f[-1]) / top if top > 0 else 0.0)


def gpu_inputs(n, seed):
    """(m, v, a) of the device tests: m uniform in [-6, 9], v from the eight values of _count_pmf_ref.gpu_inputs (0 and -1: the
    degenerate branch), float32 log-exposures of E in [0.5, 20]"""
    m, v, a = pref.gpu_inputs(0, n, seed)
    return m, v, a
