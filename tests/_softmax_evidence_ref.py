"""float64 restatement of the softmax family of manifold_gp_amd/evidence.py, on top of _softmax_ref.py: the factor R of the softmax
Hessian and what mgp_softmax_root_apply and mgp_softmax_curvature leave from their float32 inputs, the dense B = I + R^T K R (the
general form on all n C entries and the block formula on the m C observed ones), log Z, the curvature term g in its closed form,
by brute force and from samples, the analytic hyper-parameter gradient, and the Lanczos quadrature on B with given probes.  Test
infrastructure, sized for the dumbbell fixtures.  Blocks are [n, C]; vec order is row-major (i C + c)."""
import numpy as np
import torch
from scipy.linalg import cho_solve

import _evidence_ref as eref
import _softmax_ref as sref

C_FIT = 3
SLQ_PROBES, SLQ_STEPS, SLQ_SEED = eref.SLQ_PROBES, eref.SLQ_STEPS, eref.SLQ_SEED


# ------------------------------------------------------------------------------------------------ the two kernels
def _move(a, layout):
    """[n, C, S] from either layout, and back"""
    return a if layout == "cs" else np.swapaxes(a, 1, 2)


def root_apply(pi, V, layout="cs"):
    """(want, scale) of the forward product R V in float64 from float32 inputs pi [n, C], V [n, C, S] ("cs") or [n, S, C] ("sc"):
    (R v)_c = s_c v_c - pi_c sum_k s_k v_k and the row's term scale |s_c v_c| + pi_c sum_k |s_k v_k|; a lane with pi = 0 holds 0
    whatever v is."""
    p = np.asarray(pi, np.float64)[:, :, None]
    v = _move(np.asarray(V, np.float64), layout)
    with np.errstate(invalid="ignore"):
        t = np.where(p > 0, np.sqrt(p) * v, 0.0)
    want = t - p * t.sum(1, keepdims=True)
    scale = np.abs(t) + p * np.abs(t).sum(1, keepdims=True)
    return _move(want, layout), _move(scale, layout)


def root_apply_t(pi, X, V=None, layout="cs"):
    """(want, scale) of V + R^T X (V None: R^T X): (R^T x)_c = s_c (x_c - sum_k pi_k x_k), scale |v_c| + s_c (|x_c| + sum_k pi_k |x_k|)"""
    p = np.asarray(pi, np.float64)[:, :, None]
    x = _move(np.asarray(X, np.float64), layout)
    v = np.zeros_like(x) if V is None else _move(np.asarray(V, np.float64), layout)
    with np.errstate(invalid="ignore"):
        x = np.where(p > 0, x, 0.0)
    s = np.sqrt(p)
    want = v + s * (x - (p * x).sum(1, keepdims=True))
    scale = np.abs(v) + s * (np.abs(x) + (p * np.abs(x)).sum(1, keepdims=True))
    return _move(want, layout), _move(scale, layout)


def curvature_samples(pi, delta):
    """g_s [n, S, C] and the scale of its rounding, from pi [n, C] and delta [n, S, C]: d = delta - (pi . delta),
    g_s = pi_c (d_c^2 - sum_a pi_a d_a^2); the scale repeats the formula on absolute terms."""
    p = np.asarray(pi, np.float64)[:, None, :]
    with np.errstate(invalid="ignore"):
        x = np.where(p > 0, np.asarray(delta, np.float64), 0.0)
    d = x - (p * x).sum(-1, keepdims=True)
    g = p * (d * d - (p * d * d).sum(-1, keepdims=True))
    da = np.abs(x) + (p * np.abs(x)).sum(-1, keepdims=True)
    return g, p * (da * da + (p * da * da).sum(-1, keepdims=True))


def curvature_sums(pi, delta):
    """(acc, acc2, scale of acc, scale of acc2) [n, C] of one block: what mgp_softmax_curvature adds"""
    g, sc = curvature_samples(pi, delta)
    return g.sum(1), (g * g).sum(1), sc.sum(1), (sc * sc).sum(1)


# ------------------------------------------------------------------------------------------------ dense algebra
def pi_of(F, obs):
    return sref.site(F, np.zeros(F.shape[0], np.int64), obs)[2]


def root_dense(Pi):
    """blockdiag(R_i) [n C, n C]"""
    n, C = Pi.shape
    R = np.zeros((n * C, n * C))
    blocks = sref.factor_blocks(Pi)
    for i in range(n):
        R[i * C:(i + 1) * C, i * C:(i + 1) * C] = blocks[i]
    return R


def dense_b_general(Q, Pi):
    """I + R^T (Q^-1 (x) I_C) R on all n C entries: the naive form, for small n"""
    C = Pi.shape[1]
    R = root_dense(Pi)
    return np.eye(R.shape[0]) + R.T @ np.kron(np.linalg.inv(Q), np.eye(C)) @ R


def dense_b(Koo, Pi_o):
    """B on the m C observed entries by the block formula: delta + (Q^-1)_ij (R_i^T R_j)_ab, Koo = (Q^-1)_oo"""
    m, C = Pi_o.shape
    R = sref.factor_blocks(Pi_o)                                                    # [m, c, a]
    B = np.einsum("ica,jcb->iajb", R, R) * Koo[:, None, :, None]
    return np.eye(m * C) + B.reshape(m * C, m * C)


def logdet_b(solver, Pi):
    return float(np.linalg.slogdet(dense_b(solver.Koo, Pi[solver.idx]))[1])


def log_z(Q, F, t, obs, solver=None):
    """dict(value, log_likelihood, quad, logdet, m) of the dense Laplace evidence of the softmax fit at the point F"""
    solver = sref.Solver(Q, obs) if solver is None else solver
    lp, _, Pi = sref.site(F, t, obs)
    ll, quad, ld = float(lp.sum()), 0.5 * float((F * (Q @ F)).sum()), logdet_b(solver, Pi)
    return dict(value=ll - quad - 0.5 * ld, log_likelihood=ll, quad=quad, logdet=ld, m=int(solver.idx.size))


def _woodbury(solver, Pi):
    """(T [m, C, m, C], Kk) with A^-1 = K (x) I - (K_:o (x) I) T (K_o: (x) I), T = H_o (I + (K_oo (x) I) H_o)^-1"""
    Hm, M = solver._small(Pi)
    m, C = Hm.shape[0], Hm.shape[1]
    Hd = np.zeros((m, C, m, C))
    Hd[np.arange(m), :, np.arange(m), :] = Hm
    T = np.linalg.solve(M.T, Hd.reshape(m * C, m * C)).T
    return T.reshape(m, C, m, C), np.kron(solver.Koo, np.eye(C))


def covariance_blocks(solver, Pi):
    """V_i [m, C, C]: the C x C diagonal blocks of A^-1 at the observed rows"""
    T, Kk = _woodbury(solver, Pi)
    m, C = T.shape[0], T.shape[1]
    S = Kk - Kk @ T.reshape(m * C, m * C) @ Kk
    S = S.reshape(m, C, m, C)
    return S[np.arange(m), :, np.arange(m), :], S.reshape(m * C, m * C)


def curvature(solver, Pi):
    """g [n, C] in closed form: pi_c [V_cc - sum_a pi_a V_aa - 2 (V pi)_c + 2 pi^T V pi], 0 off the observed rows"""
    V, _ = covariance_blocks(solver, Pi)
    p = Pi[solver.idx]
    dv = np.einsum("icc->ic", V)
    Vp = np.einsum("icd,id->ic", V, p)
    g = np.zeros_like(Pi)
    g[solver.idx] = p * (dv - (p * dv).sum(1, keepdims=True) - 2.0 * Vp + 2.0 * (p * Vp).sum(1, keepdims=True))
    return g


def curvature_brute(solver, F, obs, step=1e-5):
    """g_ic = tr(V_i dH_i / df_ic) with dH_i / df_ic by central differences of H(softmax(f_i)) in f_ic"""
    Pi = pi_of(F, obs)
    V, _ = covariance_blocks(solver, Pi)
    Fo = F[solver.idx]
    m, C = Fo.shape
    g = np.zeros_like(F)
    for c in range(C):
        e = np.zeros(C)
        e[c] = step
        dH = (sref.hess_blocks(sref.softmax(Fo + e)) - sref.hess_blocks(sref.softmax(Fo - e))) / (2.0 * step)
        g[solver.idx, c] = np.einsum("iab,iba->i", V, dH)
    return g


def gradient(Q, dQ, F, t, obs, solver=None, g=None):
    """d log Z / d theta at the mode F for Q' = dQ, dense: -1/2 sum_c F_c^T Q' F_c + 1/2 sum_c u_c^T Q' F_c + 1/2 tr((K - A^-1)
    (Q' (x) I)), u = A^-1 g.  Returns (total, the three terms, u)."""
    solver = sref.Solver(Q, obs) if solver is None else solver
    Pi = sref.site(F, t, obs)[2]
    g = curvature(solver, Pi) if g is None else g
    u = solver.solve(Pi, g)
    dQF = dQ @ F
    terms = (-0.5 * float((F * dQF).sum()), 0.5 * float((u * dQF).sum()), 0.5 * float((trace_matrix(solver, Pi) * dQ).sum()))
    return sum(terms), terms, u


def trace_matrix(solver, Pi):
    """sum_c of the (c, c) blocks of K (x) I - A^-1 as an n x n matrix: K_:o (sum_c T[:, c, :, c]) K_o:"""
    T, _ = _woodbury(solver, Pi)
    return solver.Ko @ np.einsum("jclc->jl", T) @ solver.Ko.T


# ------------------------------------------------------------------------------------------------ probes and quadrature
def probes(obs, C, P, seed):
    """softmax_probes of evidence.py from the mask: [n, C, P], +-1 of the seeded CPU generator on the observed rows, 0 elsewhere"""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    Z = (torch.randint(0, 2, (obs.shape[0], int(C), int(P)), generator=gen).double() * 2 - 1).numpy()
    return Z * obs[:, None, None]


def b_matmul(solver, Pi):
    """v [n C] -> B v with exact solves (the Cholesky factor of Q the solver holds)"""
    n, C = Pi.shape

    def matmul(v):
        V = v.reshape(n, C)
        X = cho_solve(solver.cf, sref.noise_factor(Pi, V))
        s = np.sqrt(Pi)
        return (V + s * (X - (Pi * X).sum(1, keepdims=True))).reshape(v.shape)
    return matmul


def slq_per_probe(solver, Pi, Z, steps):
    """m C e_1^T log(T_p) e_1 of every probe in float64: (per_probe [P], mean, standard error)"""
    n, C, P = Z.shape
    return eref.slq_per_probe(b_matmul(solver, Pi), Z.reshape(n * C, P), steps, solver.idx.size * C)


def probe_trace(solver, dQ, Pi, Z):
    """The probe term of the gradient with exact float64 solves: (value, standard error) of 1/(2 P) sum_p sum_c x_pc^T Q' y_pc"""
    n, C, P = Z.shape
    per = np.empty(P)
    for p in range(P):
        rz = sref.noise_factor(Pi, Z[:, :, p])
        per[p] = 0.5 * float((cho_solve(solver.cf, rz) * (dQ @ solver.solve(Pi, rz))).sum())
    return float(per.mean()), float(per.std(ddof=1) / np.sqrt(P))


# the start of the laplace_train test (k10_loop, symmetric, nu = 2, C = 3, the labels of _softmax_ref.labels): _evidence_ref.TRAIN's;
# gain_f64: what train_f64 gains from it in 10 steps (test_softmax_evidence_cpu.py reruns it)
TRAIN = dict(eref.TRAIN, gain_f64=16.177)


def train_f64(g, norm, nu, t, obs, C, kappa0, scale0, steps, lr):
    """The optimiser of the laplace_train test in float64 with exact gradients: Adam(lr) on the raw (inverse-softplus) length scale
    and output scale, the graph bandwidth fixed, loss = -log Z / m with the mode re-fitted (warm-started) every step and the
    gradient the analytic formula through autograd on the dense Q.  Returns the list of (kappa, scale, dense log Z)."""
    raw = [torch.tensor(eref.softplus_inverse(v), dtype=torch.float64, requires_grad=True) for v in (kappa0, scale0)]
    opt = torch.optim.Adam(raw, lr=lr)
    eps, F, trace = float(g["eps"]), None, []
    for step in range(steps + 1):
        kappa, scale = (torch.nn.functional.softplus(r) for r in raw)
        Qt = eref.dense_q(g, norm, nu, eps, kappa, scale)
        Q = Qt.detach().numpy()
        Q = 0.5 * (Q + Q.T)
        solver = sref.Solver(Q, obs)
        F = sref.newton(Q, t, obs, C, f0=F, solver=solver)[0]
        z = log_z(Q, F, t, obs, solver)
        trace.append((kappa.item(), scale.item(), z["value"]))
        if step == steps:
            break
        Pi = sref.site(F, t, obs)[2]
        u = solver.solve(Pi, curvature(solver, Pi))
        Ft, ut, M = torch.from_numpy(F), torch.from_numpy(u), torch.from_numpy(trace_matrix(solver, Pi))
        sur = 0.5 * ((ut - Ft) * (Qt @ Ft)).sum() + 0.5 * (M * Qt).sum()
        opt.zero_grad()
        (-sur / z["m"]).backward()
        opt.step()
    return trace
