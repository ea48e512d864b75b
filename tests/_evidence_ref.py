"""float64 restatement of manifold_gp_amd/evidence.py: the per-node formulas of mgp_laplace_evidence_site, the dense Laplace
evidence log Z = sum_obs l - f^T Q f / 2 - logdet B / 2 with B = I + S Q^-1 S, its analytic hyper-parameter gradient, and the
Lanczos quadrature on B with given probes.  Test infrastructure, sized for the dumbbell fixtures."""
import numpy as np
import torch

import _counts_ref as cref
import _laplace_ref as lref
from oracle.solvers import slq_logdet_same_probes

FLT_MAX = cref.FLT_MAX
H_FLOOR = 1e-30
FAMILIES = ["poisson", "binomial", "bernoulli"]
# the Lanczos cases of the GPU tests (fixture, normalisation, nu) and their estimator settings
SLQ_CASES = [("dumbbell_k10_loop", "symmetric", 2), ("dumbbell_k10_loop", "randomwalk", 3), ("dumbbell_k50_noloop", "symmetric", 1),
             ("dumbbell_k50_noloop", "symmetric", 3)]
SLQ_PROBES, SLQ_STEPS, SLQ_SEED = 16, 12, 1337


def site(family, f, y, aux, obs, mean):
    """(l, h, h') per node in float64, all 0 at unobserved nodes; l without the f-independent constant.  bernoulli: y the
    labels (class 1 where y > 0.5), one trial."""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else obs
    y = np.where(obs, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    if family == "bernoulli":
        y, aux, fam = (y > 0.5).astype(np.float64), np.ones_like(f), "binomial"
    else:
        fam = family
    l, _, h, _ = cref.site(fam, f, y, aux, obs, mean)
    if fam == "poisson":
        hp = h
    else:
        eta = f + mean
        e = np.exp(-np.abs(eta))
        gap = -np.expm1(-np.abs(eta)) / (1.0 + e)
        hp = h * np.where(eta >= 0, -gap, gap)
    return l, h, np.where(obs, hp, 0.0)


def to_f32(v):
    return cref.to_f32(v)


def site_outputs(family, f, y, aux, obs, var, mean, h_floor=H_FLOOR):
    """What mgp_laplace_evidence_site leaves, from its float32 inputs: root_h and corr (None without var) rounded to float32,
    the four sums, the sum of the absolute terms of each (the scale of their rounding) and the mask of the nodes kept."""
    f = np.asarray(f, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    l, h, hp = site(family, f, y, aux, seen, mean)
    eff = seen & (h >= h_floor)
    with np.errstate(over="ignore"):
        root = np.where(eff, to_f32(np.sqrt(h)), np.float32(0.0)).astype(np.float32)
    if var is None:
        corr, c = None, np.zeros_like(f)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.where(eff, np.clip(np.where(eff, np.asarray(var, np.float64), 0.0) * hp, -FLT_MAX, FLT_MAX), 0.0)
        corr = c.astype(np.float32)
    sums = np.array([l.sum(), float(eff.sum()), c.sum(), np.abs(c).max()])
    scale = np.array([np.abs(l).sum(), float(eff.sum()), np.abs(c).sum(), np.abs(c).max()])
    return root, corr, sums, scale, eff


# ------------------------------------------------------------------------------------------------ problems on a fixture
def data(g, family):
    """The observations of a family on a fixture, as the Laplace and count tests draw them: dict(family, y, aux, obs, mean,
    const) with const the f-independent part of the log-likelihood."""
    if family == "bernoulli":
        t, obs, _ = lref.labels(g)
        return dict(family=family, y=t, aux=None, obs=obs, mean=0.0, const=0.0)
    c = cref.counts(g)
    d = cref.poisson_data(c) if family == "poisson" else cref.binomial_data(c)
    return dict(d, const=cref.constant(family, d["y"], d["aux"], d["obs"]))


def _count_view(d):
    if d["family"] == "bernoulli":
        return dict(d, family="binomial", aux=np.ones_like(d["y"]))
    return d


def mode(Q, d, f0=None):
    """The mode of psi by the dense float64 Newton iteration of _counts_ref (bernoulli as one trial)."""
    return cref.newton(Q, _count_view(d), f0=f0)[0]


def dense_b(Q, h, eff):
    """B restricted to the effective nodes: I + S (Q^-1)_ee S"""
    s = np.sqrt(h[eff])
    Qi = np.linalg.inv(Q)
    return np.eye(int(eff.sum())) + s[:, None] * Qi[np.ix_(eff, eff)] * s[None, :]


def logdet_b(Q, h, eff):
    return float(np.linalg.slogdet(dense_b(Q, h, eff))[1])


def log_z(Q, f, d):
    """dict(value, log_likelihood, quad, logdet, m) of the dense Laplace evidence at the point f"""
    l, h, _ = site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])
    eff = d["obs"] & (h >= H_FLOOR)
    ll, quad, ld = float(l.sum()) + d["const"], 0.5 * float(f @ (Q @ f)), logdet_b(Q, h, eff)
    return dict(value=ll - quad - 0.5 * ld, log_likelihood=ll, quad=quad, logdet=ld, m=int(eff.sum()))


def gradient(Q, dQ, f, d):
    """d log Z / d theta at the mode f for Q' = dQ, dense: -1/2 f^T Q' f + 1/2 u^T Q' f + 1/2 tr((Q^-1 - A^-1) Q'),
    u = A^-1 (diag(A^-1) o h').  Returns (total, the three terms)."""
    _, h, hp = site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])
    Ai, Qi = np.linalg.inv(Q + np.diag(h)), np.linalg.inv(Q)
    u = Ai @ (np.diag(Ai) * hp)
    terms = (-0.5 * float(f @ (dQ @ f)), 0.5 * float(u @ (dQ @ f)), 0.5 * float(np.sum((Qi - Ai) * dQ)))
    return sum(terms), terms


def probes(eff, P, seed):
    """effective_probes of evidence.py from the mask: +-1 of the seeded CPU generator on the effective nodes, 0 elsewhere"""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    Z = (torch.randint(0, 2, (eff.shape[0], int(P)), generator=gen).double() * 2 - 1).numpy()
    return Z * eff[:, None]


def b_matmul(Q, h):
    """v -> B v on all n nodes with an exact solve (a Cholesky factor of Q made once)"""
    import scipy.linalg as sla
    s = np.sqrt(h)
    cho = sla.cho_factor(Q)
    return lambda v: v + s * sla.cho_solve(cho, s * v)


def slq_per_probe(matmul, Z, steps, m):
    """m e_1^T log(T_p) e_1 of every probe in float64 (oracle.solvers.slq_logdet_same_probes, which scales by the length of the
    probe vector, one column at a time): (per_probe [P], mean, standard error)"""
    n, P = Z.shape
    per = np.array([slq_logdet_same_probes(matmul, Z[:, p:p + 1], min(int(steps), int(m))) * m / n for p in range(P)])
    return per, float(per.mean()), float(per.std(ddof=1) / np.sqrt(P))


def dense_q(g, norm, nu, eps, kappa, scale):
    """The dense float64 Q = scale (2 nu / kappa^2 I + L)^nu (x D for the random walk) of oracle/grad_ref.py on the fixture's edge
    list, as a torch tensor differentiable in the 0-d float64 tensors eps, kappa, scale."""
    from oracle.grad_ref import model_apply_f64
    n = g["train_x"].shape[0]
    val, idx = torch.from_numpy(g["edge_value"].astype(np.float64)), torch.from_numpy(g["edge_index"].astype(np.int64))
    zero = torch.zeros((), dtype=torch.float64)
    as0 = lambda v: v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
    return model_apply_f64(val, idx, n, as0(eps), as0(kappa), as0(scale), zero, nu, norm, bool(g["self_loops"]),
                           torch.eye(n, dtype=torch.float64), stop="Q2")


# the start of the laplace_train test (k10_loop, symmetric, nu = 2, Bernoulli): the fixture's length scale at the output scale
# of a prior marginal variance of 9; gain_f64: what train_f64 gains from it (test_evidence_cpu.py reruns it)
TRAIN = dict(kappa0=0.5, scale0=1.0885e-05, steps=10, lr=0.1, gain_f64=12.906)


def softplus_inverse(v):
    return float(np.log(np.expm1(v)))


def train_f64(g, norm, nu, d, kappa0, scale0, steps, lr):
    """The optimiser of the laplace_train test in float64 with exact gradients: Adam(lr) on the raw (inverse-softplus) length
    scale and output scale, the graph bandwidth fixed, loss = -log Z / m with the mode re-fitted (warm-started) every step and
    the gradient the analytic formula through autograd on the dense Q.  Returns the list of (kappa, scale, dense log Z), one
    per step and one for the final hyper-parameters."""
    raw = [torch.tensor(softplus_inverse(v), dtype=torch.float64, requires_grad=True) for v in (kappa0, scale0)]
    opt = torch.optim.Adam(raw, lr=lr)
    eps, f, trace = float(g["eps"]), None, []
    for step in range(steps + 1):
        kappa, scale = (torch.nn.functional.softplus(r) for r in raw)
        Qt = dense_q(g, norm, nu, eps, kappa, scale)
        Q = Qt.detach().numpy()
        Q = 0.5 * (Q + Q.T)
        f = mode(Q, d, f0=f)
        z = log_z(Q, f, d)
        trace.append((kappa.item(), scale.item(), z["value"]))
        if step == steps:
            break
        _, h, hp = site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])
        Ai, Qi = np.linalg.inv(Q + np.diag(h)), np.linalg.inv(Q)
        u = Ai @ (np.diag(Ai) * hp)
        ft, ut, M = torch.from_numpy(f), torch.from_numpy(u), torch.from_numpy(Qi - Ai)
        sur = 0.5 * ((ut - ft) @ (Qt @ ft)) + 0.5 * (M * Qt).sum()
        opt.zero_grad()
        (-sur / z["m"]).backward()
        opt.step()
    return trace


def probe_gradient(Q, dQ, f, d, Z):
    """The surrogate's gradient with exact float64 solves: (value, standard error of the probe term)"""
    _, h, hp = site(d["family"], f, d["y"], d["aux"], d["obs"], d["mean"])
    Ai, Qi = np.linalg.inv(Q + np.diag(h)), np.linalg.inv(Q)
    u = Ai @ (np.diag(Ai) * hp)
    SZ = np.sqrt(h)[:, None] * Z
    per = 0.5 * np.einsum("ip,ip->p", Qi @ SZ, dQ @ (Ai @ SZ))
    val = -0.5 * float(f @ (dQ @ f)) + 0.5 * float(u @ (dQ @ f)) + float(per.mean())
    return val, float(per.std(ddof=1) / np.sqrt(Z.shape[1]))
