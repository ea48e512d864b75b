"""float64 restatement of the ordinal family of manifold_gp_amd/evidence.py and of the cutpoint learning of ordinal.py: the
per-node formulas of mgp_ordinal_evidence_site (l, g, h, h'), the three rows of mgp_ordinal_cut_sums, the dense Laplace evidence
log Z = sum_obs log p - f^T Q f / 2 - logdet B / 2, its analytic gradients with respect to the cutpoints and to a kernel
hyper-parameter, and the two optimisers of the GPU tests with exact gradients.  Test infrastructure, sized for the dumbbell
fixtures."""
import numpy as np
import torch

import _evidence_ref as eref
import _ordinal_ref as oref

H_FLOOR = eref.H_FLOOR
INF = np.inf
GAP_FLOOR = 2.0 ** -10


def _end(x):
    """(sigma(x), sigma(-x), a = sigma(x) sigma(-x), gap = sigma(-x) - sigma(x)) from one e = exp(-|x|); the gap as
    -+(-expm1(-|x|)) / (1 + e), - for x >= 0"""
    ax = np.abs(x)
    e = np.exp(-ax)
    d = 1.0 + e
    gap = -np.expm1(-ax) / d
    up = x >= 0.0
    return np.where(up, 1.0 / d, e / d), np.where(up, e / d, 1.0 / d), e / (d * d), np.where(up, -gap, gap)


def _clean(f, lo, hi, obs):
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else np.asarray(obs, bool)
    lo = np.where(obs, np.nan_to_num(np.asarray(lo, np.float64), nan=0.0, posinf=INF, neginf=-INF), 0.0)
    hi = np.where(obs, np.nan_to_num(np.asarray(hi, np.float64), nan=0.0, posinf=INF, neginf=-INF), 1.0)
    return f, lo, hi, obs


def site(f, lo, hi, obs=None):
    """(l, g, h, h') per node in float64, all 0 at unobserved nodes; l = log sigma(hi - f) + log sigma(f - lo), without the
    f-independent log(1 - exp(-(hi - lo)))"""
    l, g, h = oref.site(f, lo, hi, obs)
    f, lo, hi, obs = _clean(f, lo, hi, obs)
    _, _, au, gu = _end(hi - f)
    _, _, al, gl = _end(lo - f)
    return l, g, h, np.where(obs, -(au * gu + al * gl), 0.0)


def site_outputs(f, lo, hi, obs, var, h_floor=H_FLOOR):
    """What mgp_ordinal_evidence_site leaves, from its float32 inputs: root_h and corr (None without var) rounded to float32, the
    four sums, the sum of the absolute terms of each and the mask of the nodes kept."""
    f = np.asarray(f, np.float64)
    seen = np.ones(f.shape, bool) if obs is None else obs
    l, _, h, hp = site(f, lo, hi, seen)
    eff = seen & (h >= h_floor)
    root = np.where(eff, np.sqrt(h), 0.0).astype(np.float32)
    if var is None:
        corr, c = None, np.zeros_like(f)
    else:
        with np.errstate(invalid="ignore"):
            c = np.where(eff, np.where(eff, np.asarray(var, np.float64), 0.0) * hp, 0.0)
        corr = c.astype(np.float32)
    sums = np.array([l.sum(), float(eff.sum()), c.sum(), np.abs(c).max()])
    scale = np.array([np.abs(l).sum(), float(eff.sum()), np.abs(c).sum(), np.abs(c).max()])
    return root, corr, sums, scale, eff


def cut_sums(f, lo, hi, cat, obs, var, u, K, h_floor=H_FLOOR):
    """(out, scale) [3, K - 1] each: the three rows of d log Z / d b_k of mgp_ordinal_cut_sums and the sums of their absolute
    terms.  A node of category c adds (sigma(-u) + 1 / expm1(w), -1/2 var a_u gap_u, -1/2 u a_u) to column c and
    (-(sigma(l) + 1 / expm1(w)), -1/2 var a_l gap_l, -1/2 u a_l) to column c - 1; rows 1 and 2 only where h >= h_floor, zeros
    without var / u; a category >= K adds nothing."""
    f, lo, hi, obs = _clean(f, lo, hi, obs)
    cat = np.where(obs, np.asarray(cat).astype(np.int64), K)
    ok = obs & (cat < K)
    with np.errstate(over="ignore", invalid="ignore"):
        _, sig_mu, au, gu = _end(hi - f)
        sig_l, _, al, gl = _end(lo - f)
        width = 1.0 / np.expm1(hi - lo)
    deep = ok & (au + al >= h_floor)
    zero = np.zeros_like(f)
    with np.errstate(invalid="ignore"):
        v = zero if var is None else np.where(deep, np.where(deep, np.asarray(var, np.float64), 0.0), 0.0)
        w = zero if u is None else np.where(deep, np.where(deep, np.asarray(u, np.float64), 0.0), 0.0)
    upper = [np.where(ok, sig_mu + width, 0.0), np.where(deep, -0.5 * (v * (au * gu)), 0.0), np.where(deep, -0.5 * (w * au), 0.0)]
    lower = [np.where(ok, -(sig_l + width), 0.0), np.where(deep, -0.5 * (v * (al * gl)), 0.0), np.where(deep, -0.5 * (w * al), 0.0)]
    out, scale = np.zeros((3, K - 1)), np.zeros((3, K - 1))
    for k in range(1, K):
        above, below = ok & (cat == k - 1), ok & (cat == k)
        for r in range(3):
            terms = np.concatenate([upper[r][above], lower[r][below]])
            out[r, k - 1], scale[r, k - 1] = terms.sum(), np.abs(terms).sum()
    return out, scale


# ------------------------------------------------------------------------------------------------ problems on a fixture
def intervals64(y, cuts):
    """(lo, hi) in float64: the cutpoints as given, not rounded (the differences of the finite-difference tests need them)"""
    cuts = np.asarray(cuts, np.float64)
    return np.concatenate([[-INF], cuts])[y], np.concatenate([cuts, [INF]])[y]


def data(g, K, frac=0.1, cuts=None):
    """dict(y, obs, cuts, K): the labels of _ordinal_ref.labels on a fixture and the frequency cutpoints as float32 holds them"""
    y, obs = oref.labels(g, K, frac=frac)
    return dict(y=y, obs=obs, K=K, cuts=oref.cutpoints(y, K, obs) if cuts is None else np.asarray(cuts, np.float64))


def mode(Q, d, f0=None):
    lo, hi = intervals64(d["y"], d["cuts"])
    return oref.newton(Q, lo, hi, d["obs"], f0=f0)[0]


def log_z(Q, f, d, Qi=None):
    """dict(value, log_likelihood, quad, logdet, m) of the dense Laplace evidence at the point f; Qi: inv(Q) when the caller has it"""
    lo, hi = intervals64(d["y"], d["cuts"])
    l, _, h, _ = site(f, lo, hi, d["obs"])
    eff = d["obs"] & (h >= H_FLOOR)
    const = float(oref.log_widths(d["cuts"])[d["y"]][d["obs"]].sum())
    if Qi is None:
        ld = eref.logdet_b(Q, h, eff)
    else:
        s = np.sqrt(h[eff])
        ld = float(np.linalg.slogdet(np.eye(int(eff.sum())) + s[:, None] * Qi[np.ix_(eff, eff)] * s[None, :])[1])
    ll, quad = float(l.sum()) + const, 0.5 * float(f @ (Q @ f))
    return dict(value=ll - quad - 0.5 * ld, log_likelihood=ll, quad=quad, logdet=ld, m=int(eff.sum()))


def posterior(Q, f, d):
    """(h, h', v = diag(A^-1), u = A^-1 (v o h'), A^-1) at the point f, dense"""
    lo, hi = intervals64(d["y"], d["cuts"])
    _, _, h, hp = site(f, lo, hi, d["obs"])
    Ai = np.linalg.inv(Q + np.diag(h))
    v = np.diag(Ai).copy()
    return h, hp, v, Ai @ (v * hp), Ai


def cut_gradient(Q, f, d):
    """(d log Z / d b [K - 1], its three rows [3, K - 1], the sums of their absolute terms) at the mode f, dense"""
    lo, hi = intervals64(d["y"], d["cuts"])
    _, _, v, u, _ = posterior(Q, f, d)
    rows, scale = cut_sums(f, lo, hi, d["y"], d["obs"], v, u, d["K"])
    return rows.sum(0), rows, scale


def gradient(Q, dQ, f, d, Qi=None):
    """d log Z / d theta at the mode f for Q' = dQ (_evidence_ref.gradient with the ordinal h and h'): (total, the three terms)"""
    _, _, _, u, Ai = posterior(Q, f, d)
    Qi = np.linalg.inv(Q) if Qi is None else Qi
    terms = (-0.5 * float(f @ (dQ @ f)), 0.5 * float(u @ (dQ @ f)), 0.5 * float(np.sum((Qi - Ai) * dQ)))
    return sum(terms), terms


# ------------------------------------------------------------------------------------------------ the optimisers in float64
def raw_cutpoints(cuts):
    """the unconstrained parameters (b_1, rho_2 .. rho_{K-1}) of ordinal.CutpointParameter for the cutpoints `cuts`"""
    cuts = np.asarray(cuts, np.float64)
    x = np.diff(cuts) - GAP_FLOOR
    return np.concatenate([cuts[:1], x + np.log(-np.expm1(-x))])


def cutpoints_of(raw):
    """b_1, b_1 + sum (2^-10 + softplus(rho)) on a torch float64 tensor, differentiable"""
    gaps = GAP_FLOOR + torch.nn.functional.softplus(raw[1:])
    return raw[0] + torch.cat([torch.zeros_like(raw[:1]), gaps.cumsum(0)])


# the learn_cutpoints test (k10_loop, symmetric, nu = 2, K = 4, frac = 0.1, the precision scaled to a prior variance of 9) and the
# laplace_train test (the same labels from _evidence_ref.TRAIN's start): gain_f64 is what learn_f64 / train_f64 gain
# (test_ordinal_evidence_cpu.py reruns both)
LEARN = dict(K=4, frac=0.1, steps=10, lr=0.1)
LEARN_GAIN_F64, TRAIN_GAIN_F64 = 22.085, 22.457


def learn_f64(Q, d, steps, lr):
    """learn_cutpoints in float64 with exact gradients: Adam(lr) on the raw cutpoint parameters from d["cuts"], Q fixed, loss
    -log Z / m, the mode re-fitted (warm-started) every step.  Returns the list of (cutpoints, dense log Z), one per step and one
    for the final cutpoints."""
    raw = torch.tensor(raw_cutpoints(d["cuts"]), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([raw], lr=lr)
    Qi, f, trace = np.linalg.inv(Q), None, []
    for step in range(steps + 1):
        cuts = cutpoints_of(raw)
        dk = dict(d, cuts=cuts.detach().numpy().copy())
        f = mode(Q, dk, f0=f)
        z = log_z(Q, f, dk, Qi)
        trace.append((dk["cuts"], z["value"]))
        if step == steps:
            break
        G = cut_gradient(Q, f, dk)[0]
        opt.zero_grad()
        (-(torch.from_numpy(G) * cuts).sum() / z["m"]).backward()
        opt.step()
    return trace


def train_f64(g, norm, nu, d, kappa0, scale0, steps, lr):
    """_evidence_ref.train_f64 with the cutpoints trained along: Adam(lr) on the raw length scale, output scale and cutpoint
    parameters together.  Returns the list of (kappa, scale, cutpoints, dense log Z)."""
    raw = [torch.tensor(eref.softplus_inverse(v), dtype=torch.float64, requires_grad=True) for v in (kappa0, scale0)]
    raw_c = torch.tensor(raw_cutpoints(d["cuts"]), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam(raw + [raw_c], lr=lr)
    eps, f, trace = float(g["eps"]), None, []
    for step in range(steps + 1):
        kappa, scale = (torch.nn.functional.softplus(r) for r in raw)
        cuts = cutpoints_of(raw_c)
        dk = dict(d, cuts=cuts.detach().numpy().copy())
        Qt = eref.dense_q(g, norm, nu, eps, kappa, scale)
        Q = Qt.detach().numpy()
        Q = 0.5 * (Q + Q.T)
        f = mode(Q, dk, f0=f)
        Qi = np.linalg.inv(Q)
        z = log_z(Q, f, dk, Qi)
        trace.append((kappa.item(), scale.item(), dk["cuts"], z["value"]))
        if step == steps:
            break
        lo, hi = intervals64(dk["y"], dk["cuts"])
        _, _, v, u, Ai = posterior(Q, f, dk)
        G = cut_sums(f, lo, hi, dk["y"], dk["obs"], v, u, dk["K"])[0].sum(0)
        ft, ut, M = torch.from_numpy(f), torch.from_numpy(u), torch.from_numpy(Qi - Ai)
        sur = 0.5 * ((ut - ft) @ (Qt @ ft)) + 0.5 * (M * Qt).sum() + (torch.from_numpy(G) * cuts).sum()
        opt.zero_grad()
        (-sur / z["m"]).backward()
        opt.step()
    return trace
