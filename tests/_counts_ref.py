"""float64 restatement of manifold_gp_amd/counts.py (Laplace approximation, Poisson and binomial likelihoods): the per-node
site formulas of mgp_count_site, a dense Newton iteration with step halving, and the fit's own Newton loop
(classification._newton) driven by dense numpy stand-ins whose vectors are rounded to float32 where the device's are.  Test
infrastructure, sized for the dumbbell fixtures."""
import numpy as np
from scipy.special import expit, gammaln

FLT_MAX = float(np.finfo(np.float32).max)
ETA_MAX = 700.0


def counts(g, seed=11):
    """Count data on a fixture: ftrue = 1.2 x the standardised first coordinate, exposures E ~ U(0.5, 20), 10 % of the nodes
    observed, y ~ Poisson(E exp(1 + ftrue)), trials N in 1 .. 39, k ~ Binomial(N, sigma(ftrue)), drawn in that order."""
    rng = np.random.default_rng(seed)
    x0 = g["train_x"][:, 0].astype(np.float64)
    n = x0.shape[0]
    ftrue = 1.2 * (x0 - x0.mean()) / x0.std()
    E = rng.uniform(0.5, 20.0, n)
    obs = rng.random(n) < 0.10
    y = rng.poisson(E * np.exp(1.0 + ftrue))
    N = rng.integers(1, 40, n)
    k = rng.binomial(N, expit(ftrue))
    return dict(ftrue=ftrue, E=E, obs=obs, y=y.astype(np.float64), N=N.astype(np.float64), k=k.astype(np.float64))


def ceil_log2(m):
    return int(np.ceil(np.log2(m)))


def poisson_data(c):
    """The Poisson problem of counts(): what the device reads (aux = float32 log-exposure), the default mean and s_ref."""
    obs = c["obs"]
    mean = float(np.log(c["y"][obs].sum() / c["E"][obs].sum()))
    s_ref = 2.0 ** -ceil_log2(max(1.0, c["y"][obs].max()))
    return dict(family="poisson", y=c["y"], aux=np.log(c["E"]).astype(np.float32).astype(np.float64), obs=obs, mean=mean, s_ref=s_ref)


def binomial_data(c):
    obs = c["obs"]
    return dict(family="binomial", y=c["k"], aux=c["N"], obs=obs, mean=0.0, s_ref=4.0 * 2.0 ** -ceil_log2(c["N"][obs].max()))


def site(family, f, y, aux, obs, mean):
    """(l, g, h, mass) per node in float64, all 0 at unobserved nodes; l without the f-independent constant.  mass is mu
    (Poisson) or N (binomial): the size of the terms g is the difference of."""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else obs
    y = np.where(obs, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    if family == "poisson":
        a = np.zeros_like(f) if aux is None else np.where(obs, np.nan_to_num(np.asarray(aux, np.float64)), 0.0)
        eta = f + mean + a
        mu = np.exp(np.minimum(eta, ETA_MAX))
        l, g, h, mass = y * eta - mu, y - mu, mu, mu
    else:
        N = np.where(obs, np.nan_to_num(np.asarray(aux, np.float64)), 0.0)
        eta = f + mean
        e = np.exp(-np.abs(eta))
        l = -(N - y) * np.logaddexp(0.0, eta) - y * np.logaddexp(0.0, -eta)
        g = y * expit(-eta) - (N - y) * expit(eta)
        h, mass = N * e / (1.0 + e) ** 2, N
    z = np.zeros_like(f)
    return np.where(obs, l, z), np.where(obs, g, z), np.where(obs, h, z), np.where(obs, mass, z)


def constant(family, y, aux, obs):
    """sum_obs of the f-independent part of the log-likelihood: -lgamma(y + 1) or log C(N, y)"""
    obs = np.ones(np.shape(y), bool) if obs is None else obs
    y = np.asarray(y, np.float64)[obs]
    if family == "poisson":
        return float(-gammaln(y + 1.0).sum())
    N = np.asarray(aux, np.float64)[obs]
    return float((gammaln(N + 1.0) - gammaln(y + 1.0) - gammaln(N - y + 1.0)).sum())


def to_f32(v):
    with np.errstate(over="ignore"):
        return np.clip(v, -FLT_MAX, FLT_MAX).astype(np.float32)


def site_outputs(family, f, qf, y, aux, obs, s_ref, mean):
    """What mgp_count_site leaves, from its float32 inputs: w and rhs rounded to float32 (saturated at +-FLT_MAX), the four sums,
    the sum of the absolute terms of each sum (the scale of their rounding), and per node s_ref (mass + y + |qf|): the size of
    the terms rhs is the difference of."""
    f = np.asarray(f, np.float64)
    qf = np.zeros_like(f) if qf is None else np.asarray(qf, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    l, g, h, mass = site(family, f, y, aux, seen, mean)
    r = g - qf
    with np.errstate(over="ignore"):
        sq = (r * r).sum()
    sums = np.array([l.sum(), (f * qf).sum(), np.abs(r).max(), sq])
    scale = np.array([np.abs(l).sum(), np.abs(f * qf).sum(), np.abs(r).max(), sq])
    yy = np.where(seen, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    return to_f32(s_ref * h), to_f32(s_ref * r), sums, scale, s_ref * (mass + yy + np.abs(qf))


def psi(Q, f, d):
    return site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])[0].sum() - 0.5 * f @ (Q @ f)


def gradient(Q, f, d):
    return site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])[1] - Q @ f


def curvature(f, d):
    return site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])[2]


def log_likelihood(f, d):
    return site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])[0].sum() + constant(d["family"], d["y"], d["aux"], d["obs"])


def newton(Q, d, f0=None, gtol=1e-11, max_steps=100):
    """Dense float64 Newton with step halving on psi, until max |g - Q f| <= gtol (absolute).  Returns (f, trace): one
    (psi, max |g - Q f|, step) per Newton step."""
    n = Q.shape[0]
    f = np.zeros(n) if f0 is None else np.array(f0, np.float64)
    trace = []
    for _ in range(max_steps):
        r = gradient(Q, f, d)
        if np.abs(r).max() <= gtol:
            break
        delta = np.linalg.solve(Q + np.diag(curvature(f, d)), r)
        cur, step = psi(Q, f, d), 1.0
        while psi(Q, f + step * delta, d) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        f = f + step * delta
        trace.append((psi(Q, f, d), np.abs(gradient(Q, f, d)).max(), step))
        if np.abs(step * delta).max() <= 1e-15 * max(1.0, np.abs(f).max()):          # the float64 floor of the iterate
            break
    return f, trace


def simulate(Q, d, f0=None, step_tol=1e-3, max_newton=30):
    """The fit's own loop (classification._newton with rtol = 0 and step_tol) on dense stand-ins of the device stages: the
    iterate, Q f, w, the right-hand side and the step are rounded to float32 where the device holds float32; the linear solve
    is exact.  Returns (f float32, converged, steps, history)."""
    from manifold_gp_amd.classification import _newton
    n, s_ref = Q.shape[0], d["s_ref"]

    def site_(f, qf):
        w, rhs, sums, _, _ = site_outputs(d["family"], f, qf, d["y"], d["aux"], d["obs"], s_ref, d["mean"])
        return w, rhs, sums.tolist()

    def q2(f):
        return (Q @ f.astype(np.float64)).astype(np.float32)

    def solve(w, rhs):
        return np.linalg.solve(np.diag(w.astype(np.float64)) + s_ref * Q, rhs.astype(np.float64)).astype(np.float32), 0

    start = None if f0 is None else np.asarray(f0, np.float32)
    f, _, _, converged, its, history = _newton("simulate", site_, q2, solve, np.zeros(n, np.float32), start, 0.0, max_newton,
                                               step_tol=step_tol)
    return f, converged, its, history
