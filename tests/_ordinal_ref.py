"""float64 restatement of manifold_gp_amd/ordinal.py (Laplace approximation, cumulative-logit likelihood): the per-node site
formulas of mgp_ordinal_site, the trapezoid rule of mgp_ordinal_predict operation by operation, a dense Newton iteration with
step halving, and a 30-digit quadrature of the predictive probabilities (mpmath).  Test infrastructure, sized for the dumbbell
fixtures."""
import numpy as np

LO, HI = -8.0, 8.0
V_MIN = 2.0 ** -76
INF = np.inf


def labels(g, K=4, seed=13, frac=0.5, noise=0.6):
    """(y, obs): K ordered categories cut at the quantiles of a smooth function of the node coordinates (1.5 x the standardised
    first coordinate plus a sine of it) plus logistic noise; about half the nodes observed."""
    rng = np.random.default_rng(seed)
    x0 = g["train_x"][:, 0].astype(np.float64)
    z = (x0 - x0.mean()) / x0.std()
    s = 1.5 * z + 0.5 * np.sin(3.0 * z) + noise * rng.logistic(size=z.shape[0])
    y = np.searchsorted(np.quantile(s, np.arange(1, K) / K), s).astype(np.int64)
    return y, rng.random(z.shape[0]) < frac


def cutpoints(y, K, obs=None):
    """logit of the smoothed cumulative frequencies, as ordinal.ordinal_cutpoints, rounded to float32 as the fit holds them"""
    y = y if obs is None else y[obs]
    mass = np.bincount(y, minlength=K).astype(np.float64) + 0.5
    b = np.log(np.cumsum(mass)[:-1]) - np.log(np.cumsum(mass[::-1])[::-1][1:])
    return b.astype(np.float32).astype(np.float64)


def intervals(y, cuts):
    """(lo, hi) float32 [n]: the ends of every node's interval of cutpoints as the kernel reads them"""
    cuts = np.asarray(cuts, np.float64)
    lo = np.concatenate([[-INF], cuts])[y].astype(np.float32)
    hi = np.concatenate([cuts, [INF]])[y].astype(np.float32)
    return lo, hi


def log_widths(cuts):
    """log c_k = log(1 - exp(-(b_{k+1} - b_k))) per category, 0 at the two ends"""
    cuts = np.asarray(cuts, np.float64)
    return np.concatenate([[0.0], np.log(-np.expm1(-np.diff(cuts))), [0.0]])


def _sig(x):
    """(sigma(x), sigma(-x), sigma(x) sigma(-x), log sigma(x)) from one e = exp(-|x|), the kernel's expressions"""
    e = np.exp(-np.abs(x))
    d = 1.0 + e
    up = x >= 0.0
    return np.where(up, 1.0 / d, e / d), np.where(up, e / d, 1.0 / d), e / (d * d), -(np.where(x < 0.0, -x, 0.0) + np.log1p(e))


def site(f, lo, hi, obs=None):
    """(log p without log c, g, h) per node in float64; all three are 0 at unobserved nodes"""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else obs
    lo = np.where(obs, np.nan_to_num(np.asarray(lo, np.float64), nan=0.0, posinf=INF, neginf=-INF), 0.0)
    hi = np.where(obs, np.nan_to_num(np.asarray(hi, np.float64), nan=0.0, posinf=INF, neginf=-INF), 1.0)
    with np.errstate(invalid="ignore"):
        _, sig_mu, hu, ls_u = _sig(hi - f)
        sig_l, _, hl, _ = _sig(lo - f)
        ls_ml = _sig(f - lo)[3]
    z = np.zeros_like(f)
    return np.where(obs, ls_u + ls_ml, z), np.where(obs, sig_l - sig_mu, z), np.where(obs, hu + hl, z)


def site_outputs(f, qf, lo, hi, obs, s_ref):
    """What mgp_ordinal_site leaves, from its float32 inputs: w and rhs rounded to float32, the four sums, and the sum of the
    absolute terms of each sum (the scale of their rounding)."""
    f = np.asarray(f, np.float64)
    qf = np.zeros_like(f) if qf is None else np.asarray(qf, np.float64)
    lp, g, h = site(f, lo, hi, obs)
    r = g - qf
    sums = np.array([lp.sum(), (f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    scale = np.array([np.abs(lp).sum(), np.abs(f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    return (s_ref * h).astype(np.float32), (s_ref * r).astype(np.float32), sums, scale


def naive_log_p(f, lo, hi):
    """log(sigma(hi - f) - sigma(lo - f)) on torch float64 tensors: the form with the cancellation, for autograd on moderate
    arguments"""
    import torch
    return torch.log(torch.sigmoid(hi - f) - torch.sigmoid(lo - f))


# ------------------------------------------------------------------------------------------------ the predictive rule
def rule(points):
    step = (HI - LO) / (points - 1)
    u = LO + np.arange(points) * step
    return u, step * (0.3989422804014327 * np.exp(-0.5 * u * u))


def trapezoid(eta, var, cuts, points=129, log=False):
    """The rule of mgp_ordinal_predict operation by operation: [n, K] float64.  Per point j ascending
    p_k += wt_j sigma(b_{k+1} - f_j) sigma(f_j - b_k), then c_k (p_k / sum_j wt_j); var <= 2^-76 the plain probability at eta."""
    eta, var = np.atleast_1d(np.asarray(eta, np.float64)), np.atleast_1d(np.asarray(var, np.float64))
    cuts = np.asarray(cuts, np.float64)
    u, wt = rule(points)
    total = 0.0
    for j in range(points):
        total = total + wt[j]
    up = np.concatenate([cuts, [INF]])[None, :]
    c = np.concatenate([[1.0], -np.expm1(-np.diff(cuts)), [1.0]])[None, :]

    def term(f):
        with np.errstate(invalid="ignore"):
            below, above, _, _ = _sig(up - f[:, None])
        lower = np.concatenate([np.ones((f.shape[0], 1)), above[:, :-1]], axis=1)
        return np.concatenate([below[:, :1], below[:, 1:] * lower[:, 1:]], axis=1)

    plain = var <= V_MIN
    with np.errstate(invalid="ignore"):
        sd = np.where(plain, 0.0, np.sqrt(var))
    p = np.zeros((eta.shape[0], cuts.shape[0] + 1))
    for j in range(points):
        p = p + wt[j] * term(eta + sd * u[j])
    r = c * np.where(plain[:, None], term(eta), p / total)
    with np.errstate(divide="ignore"):
        return np.log(r) if log else r


def reach(eta, var, cuts):
    """X = max |b - f_j| over the cutpoints and the grid of the rule, per node"""
    eta, var = np.atleast_1d(np.asarray(eta, np.float64)), np.atleast_1d(np.asarray(var, np.float64))
    cuts = np.asarray(cuts, np.float64)
    sd = np.sqrt(np.where(var <= V_MIN, 0.0, var))
    ends = np.stack([eta + LO * sd, eta + HI * sd], 1)
    return np.abs(cuts[None, :, None] - ends[:, None, :]).max((1, 2))


# the table of docs/kernels/ordinal.md: variances x means x intervals of cutpoints
TABLE_V = [1e-8, 3e-3, 0.27, 1.0, 9.0, 26.0]
TABLE_M = [-4.0, 0.0, 2.5]
TABLE_INTERVALS = [(-INF, -1.0), (-1.0, 0.5), (0.5, 2.0), (2.0, INF), (6.0, 8.0), (12.0, 14.0), (-3.0, -2.999)]
DEVICE_C = 22.0          # the constant of the device test's bound c 2^-53 (1 + X): test_ordinal_cpu.py derives it


def interval_probability(m, v, lo, hi, points=129):
    """the rule for the one interval (lo, hi): the middle category of the cutpoints (lo, hi), or an end category"""
    if lo == -INF:
        return trapezoid([m], [v], [hi], points)[0, 0]
    if hi == INF:
        return trapezoid([m], [v], [lo], points)[0, 1]
    return trapezoid([m], [v], [lo, hi], points)[0, 1]


def _mp_integrand(mp, m, v, lo, hi):
    sig = lambda x: 1 / (1 + mp.exp(-x)) if x >= 0 else mp.exp(x) / (1 + mp.exp(x))
    c = mp.mpf(1) if lo == -INF or hi == INF else -mp.expm1(-(mp.mpf(hi) - mp.mpf(lo)))

    def like(f):
        r = c
        if hi != INF:
            r = r * sig(mp.mpf(hi) - f)
        if lo != -INF:
            r = r * sig(f - mp.mpf(lo))
        return r
    return like


def mp_probability(m, v, lo, hi, dps=30):
    """int P(lo < . <= hi | f) N(f; m, v) df by mpmath's quadrature at `dps` digits, the integrand in the product form"""
    import mpmath as mp
    with mp.workdps(dps):
        like = _mp_integrand(mp, m, v, lo, hi)
        m_, sd = mp.mpf(m), mp.sqrt(mp.mpf(v))
        brk = sorted(set([m_ + sd * t for t in (-40, -10, -3, 0, 3, 10, 40)]
                         + [mp.mpf(b) for b in (lo, hi) if abs(b) != INF and abs(b - m) < 40 * float(sd)]))
        val = mp.quad(lambda f: like(f) * mp.exp(-(f - m_) ** 2 / (2 * mp.mpf(v))), brk) / mp.sqrt(2 * mp.pi * mp.mpf(v))
        return val


def mp_rule(m, v, lo, hi, points=129, dps=30):
    """the rule of trapezoid() summed in mpmath from the same float64 grid and cutpoints: what the float64 restatement would
    give without rounding"""
    import mpmath as mp
    with mp.workdps(dps):
        like = _mp_integrand(mp, m, v, lo, hi)
        step = mp.mpf(16) / (points - 1)
        sd = mp.sqrt(mp.mpf(v))
        tot, acc = mp.mpf(0), mp.mpf(0)
        for j in range(points):
            u = -8 + j * step
            w = step * mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)
            tot += w
            acc += w * like(mp.mpf(m) + sd * u)
        return acc / tot


# ------------------------------------------------------------------------------------------------ the dense Newton iteration
def psi(Q, f, lo, hi, obs):
    return site(f, lo, hi, obs)[0].sum() - 0.5 * f @ (Q @ f)


def gradient(Q, f, lo, hi, obs):
    return site(f, lo, hi, obs)[1] - Q @ f


def curvature(f, lo, hi, obs):
    return site(f, lo, hi, obs)[2]


def log_likelihood(f, y, cuts, obs):
    lo, hi = intervals(y, cuts)
    return site(f, lo, hi, obs)[0].sum() + log_widths(cuts)[y][obs].sum()


def newton(Q, lo, hi, obs, f0=None, rtol=1e-12, max_steps=100):
    """Dense float64 Newton with step halving on psi.  Returns (f, trace): one (psi, relative gradient, step) per Newton step;
    the gradient max |g - Q f| is relative to its value at f = 0."""
    n = Q.shape[0]
    f = np.zeros(n) if f0 is None else np.array(f0, np.float64)
    grad0 = np.abs(gradient(Q, np.zeros(n), lo, hi, obs)).max()
    trace = []
    for _ in range(max_steps):
        r = gradient(Q, f, lo, hi, obs)
        if np.abs(r).max() <= rtol * grad0:
            break
        delta = np.linalg.solve(Q + np.diag(curvature(f, lo, hi, obs)), r)
        cur, step = psi(Q, f, lo, hi, obs), 1.0
        while psi(Q, f + step * delta, lo, hi, obs) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        f = f + step * delta
        trace.append((psi(Q, f, lo, hi, obs), np.abs(gradient(Q, f, lo, hi, obs)).max() / grad0, step))
    return f, trace


def steps_to(trace, rtol):
    """Newton steps the float64 iteration takes until its relative gradient is <= rtol."""
    for k, (_, rel, _) in enumerate(trace):
        if rel <= rtol:
            return k + 1
    return len(trace)


def simulate(Q, lo, hi, obs, f0=None, rtol=1e-5, max_newton=30, s_ref=2.0):
    """The fit's own loop (classification._newton with the gradient rule) on dense stand-ins of the device stages: the iterate,
    Q f, w, the right-hand side and the step are rounded to float32 where the device holds float32; the linear solve is exact.
    Returns (f float32, converged, steps, history)."""
    from manifold_gp_amd.classification import _newton
    n = Q.shape[0]

    def site_(f, qf):
        w, rhs, sums, _ = site_outputs(f, qf, lo, hi, obs, s_ref)
        return w, rhs, sums.tolist()

    def q2(f):
        return (Q @ f.astype(np.float64)).astype(np.float32)

    def solve(w, rhs):
        return np.linalg.solve(np.diag(w.astype(np.float64)) + s_ref * Q, rhs.astype(np.float64)).astype(np.float32), 0

    start = None if f0 is None else np.asarray(f0, np.float32)
    f, _, _, converged, its, history = _newton("simulate", site_, q2, solve, np.zeros(n, np.float32), start, rtol, max_newton)
    return f, converged, its, history


def bad_start(n, seed=3):
    """f0 = 20 x standard normal noise: far from any mode, the first Newton steps overshoot"""
    return (20.0 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
