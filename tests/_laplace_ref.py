"""float64 restatement of manifold_gp_amd/classification.py (Laplace approximation, Bernoulli-logit likelihood): the per-node
site formulas of mgp_bernoulli_site, the trapezoid rule of mgp_bernoulli_predict and a dense Newton iteration with step
halving.  Test infrastructure, sized for the dumbbell fixtures."""
import numpy as np
from scipy.special import expit

LO, HI = -8.0, 8.0


def labels(g, seed=7, flip=0.05, frac=0.10):
    """(t, obs, y): t = x_0 > median with 5 % flipped, 10 % of the nodes observed, y float32 with NaN where unobserved."""
    rng = np.random.default_rng(seed)
    x0 = g["train_x"][:, 0]
    t = x0 > np.median(x0)
    t = np.where(rng.random(t.shape[0]) < flip, ~t, t)
    obs = rng.random(t.shape[0]) < frac
    y = np.where(obs, t.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return t.astype(np.float64), obs, y


def site(f, qf, t, obs):
    """(log p, g, h) per node in float64; all three are 0 at unobserved nodes.  t in {0, 1}."""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else obs
    a = (2.0 * t - 1.0) * f
    lp = np.where(obs, -np.logaddexp(0.0, -a), 0.0)
    g = np.where(obs, t - expit(f), 0.0)
    e = np.exp(-np.abs(f))
    h = np.where(obs, e / (1.0 + e) ** 2, 0.0)
    return lp, g, h


def site_outputs(f, qf, y, obs, s_ref):
    """What mgp_bernoulli_site leaves, from its float32 inputs: w and rhs rounded to float32, the four sums, and the sum of
    the absolute terms of each of the three sums (the scale of their rounding)."""
    f = np.asarray(f, np.float64)
    qf = np.zeros_like(f) if qf is None else np.asarray(qf, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    t = np.where(seen, np.nan_to_num(np.asarray(y, np.float64)) > 0.5, False).astype(np.float64)
    lp, g, h = site(f, qf, t, seen)
    r = g - qf
    sums = np.array([lp.sum(), (f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    scale = np.array([np.abs(lp).sum(), np.abs(f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    return (s_ref * h).astype(np.float32), (s_ref * r).astype(np.float32), sums, scale


def trapezoid(m, v, K=129):
    """sum_k D phi(u_k) sigma(m + sqrt(max(v, 0)) u_k), u_k = -8 + k D, D = 16 / (K - 1), capped at 1."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    step = (HI - LO) / (K - 1)
    u = LO + np.arange(K) * step
    wt = step * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
    sd = np.sqrt(np.where(v < 0.0, 0.0, v))
    p = (expit(m[..., None] + sd[..., None] * u) * wt).sum(-1)
    return np.where(p > 1.0, 1.0, p)


def psi(Q, f, t, obs):
    return site(f, None, t, obs)[0].sum() - 0.5 * f @ (Q @ f)


def gradient(Q, f, t, obs):
    return site(f, None, t, obs)[1] - Q @ f


def newton(Q, t, obs, f0=None, rtol=1e-12, max_steps=100):
    """Dense float64 Newton with step halving on psi.  Returns (f, trace): trace holds one (psi, relative gradient, step)
    per Newton step; the gradient max |g - Q f| is relative to its value at f = 0."""
    n = Q.shape[0]
    f = np.zeros(n) if f0 is None else np.array(f0, np.float64)
    grad0 = np.abs(gradient(Q, np.zeros(n), t, obs)).max()
    trace = []
    for _ in range(max_steps):
        r = gradient(Q, f, t, obs)
        if np.abs(r).max() <= rtol * grad0:
            break
        h = site(f, None, t, obs)[2]
        delta = np.linalg.solve(Q + np.diag(h), r)
        cur, step = psi(Q, f, t, obs), 1.0
        while psi(Q, f + step * delta, t, obs) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        f = f + step * delta
        trace.append((psi(Q, f, t, obs), np.abs(gradient(Q, f, t, obs)).max() / grad0, step))
    return f, trace


def steps_to(trace, rtol):
    """Newton steps the float64 iteration takes until its relative gradient is <= rtol."""
    for k, (_, rel, _) in enumerate(trace):
        if rel <= rtol:
            return k + 1
    return len(trace)
