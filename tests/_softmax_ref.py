"""float64 restatement of the C-class part of manifold_gp_amd/classification.py (Laplace approximation, softmax likelihood): the
per-row site formulas of mgp_softmax_site, the Hessian apply and its factor R, and a dense Newton iteration with step halving.
Blocks are [n, C], row-major as in the library.  Test infrastructure, sized for the dumbbell fixtures.

The Newton system (Q (x) I_C + H) D = B has size n C (4638 for the fixtures at C = 3), but H is zero outside the m observed
rows: with K = Q^-1 (one Cholesky factorisation per problem),  D = K (B - E H D_o)  and the observed rows solve the small system
(I + (K_oo (x) I_C) H_o) D_o = (K B)_o  of size m C.  Exact algebra, no iteration; a fit from F = 0 takes well under a second."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import logsumexp


def labels(g, C, seed=7, flip=0.05, frac=0.10):
    """(t, obs, y): t = the C-quantile bin of x_0 with 5 % moved to another class, 10 % of the nodes observed, y float32 with
    NaN where unobserved."""
    rng = np.random.default_rng(seed)
    x0 = g["train_x"][:, 0]
    n = x0.shape[0]
    t = np.searchsorted(np.quantile(x0, np.arange(1, C) / C), x0, side="right")
    moved = rng.random(n) < flip
    t = np.where(moved, (t + rng.integers(1, C, n)) % C, t).astype(np.int64)
    obs = rng.random(n) < frac
    y = np.where(obs, t.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return t, obs, y


def site(F, t, obs):
    """(log p [n], G [n, C], Pi [n, C]) in float64; all three are 0 at unobserved rows."""
    F = np.asarray(F, np.float64)
    n, C = F.shape
    seen = np.ones(n, bool) if obs is None else obs
    m = F.max(1, keepdims=True)
    e = np.exp(F - m)
    Z = e.sum(1, keepdims=True)
    Pi = np.where(seen[:, None], e / Z, 0.0)
    tt = np.where(seen, t, 0).astype(np.int64)
    lp = np.where(seen, F[np.arange(n), tt] - m[:, 0] - np.log(Z[:, 0]), 0.0)
    onehot = (np.arange(C)[None, :] == tt[:, None]) & seen[:, None]
    rest = np.where(onehot, 0.0, e).sum(1, keepdims=True)               # 1 - pi_t = sum_{c != t} e_c / Z: no cancellation
    return lp, np.where(onehot, rest / Z, -Pi), Pi


def site_outputs(f, qf, t, obs):
    """What mgp_softmax_site leaves, from its float32 inputs: pi and rhs rounded to float32, the four sums, and the sum of the
    absolute terms of each of the three sums (the scale of their rounding)."""
    f = np.asarray(f, np.float64)
    qf = np.zeros_like(f) if qf is None else np.asarray(qf, np.float64)
    lp, G, Pi = site(f, t, obs)
    r = G - qf
    sums = np.array([lp.sum(), (f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    scale = np.array([np.abs(lp).sum(), np.abs(f * qf).sum(), np.abs(r).max(), (r * r).sum()])
    return Pi.astype(np.float32), r.astype(np.float32), sums, scale


def hess_apply(Pi, X):
    """(H X)_i = pi_i o x_i - pi_i (pi_i . x_i)"""
    return Pi * X - Pi * (Pi * X).sum(1, keepdims=True)


def hess_blocks(Pi):
    """H_i = diag(pi_i) - pi_i pi_i^T as [n, C, C]"""
    C = Pi.shape[1]
    return Pi[:, :, None] * np.eye(C)[None] - Pi[:, :, None] * Pi[:, None, :]


def noise_factor(Pi, eps):
    """R eps, R_i = diag(sqrt(pi_i)) - pi_i sqrt(pi_i)^T: R_i R_i^T = H_i where sum pi_i = 1 (or pi_i = 0)."""
    root = np.sqrt(Pi)
    return root * eps - Pi * (root * eps).sum(1, keepdims=True)


def factor_blocks(Pi):
    """R_i as [n, C, C]"""
    C = Pi.shape[1]
    root = np.sqrt(Pi)
    return root[:, :, None] * np.eye(C)[None] - Pi[:, :, None] * root[:, None, :]


def psi(Q, F, t, obs):
    return site(F, t, obs)[0].sum() - 0.5 * (F * (Q @ F)).sum()


def gradient(Q, F, t, obs):
    return site(F, t, obs)[1] - Q @ F


class Solver:
    """(Q (x) I_C + H(Pi))^-1 for Pi supported on the observed rows `obs` (module docstring)."""

    def __init__(self, Q, obs):
        n = Q.shape[0]
        self.cf = cho_factor(Q)
        self.idx = np.flatnonzero(np.ones(n, bool) if obs is None else obs)
        self.Ko = cho_solve(self.cf, np.eye(n)[:, self.idx])            # K[:, o]
        self.Koo = self.Ko[self.idx]

    def _small(self, Pi):
        Hm = hess_blocks(Pi[self.idx])
        m, C = Hm.shape[0], Hm.shape[1]
        M = np.eye(m * C) + np.einsum("ij,jcd->icjd", self.Koo, Hm).reshape(m * C, m * C)
        return Hm, M

    def solve(self, Pi, B):
        Hm, M = self._small(Pi)
        m, C = Hm.shape[0], Hm.shape[1]
        KB = cho_solve(self.cf, B)
        Do = np.linalg.solve(M, KB[self.idx].reshape(-1)).reshape(m, C)
        return KB - self.Ko @ np.einsum("jcd,jd->jc", Hm, Do)

    def covariance_diag(self, Pi):
        """diag((Q (x) I_C + H)^-1) as [n, C]: K_ii - sum_jl K_ij T[j, c, l, c] K_il, T = H_o M^-1 (Woodbury)."""
        Hm, M = self._small(Pi)
        m, C = Hm.shape[0], Hm.shape[1]
        Hd = np.zeros((m, C, m, C))
        Hd[np.arange(m), :, np.arange(m), :] = Hm
        T = np.linalg.solve(M.T, Hd.reshape(m * C, m * C)).T.reshape(m, C, m, C)      # (H and K_oo are symmetric)
        Tcc = np.stack([T[:, c, :, c] for c in range(C)], -1)           # [m, m, C]
        kdiag = np.diag(cho_solve(self.cf, np.eye(self.Ko.shape[0])))
        return kdiag[:, None] - np.einsum("ij,jlc,il->ic", self.Ko, Tcc, self.Ko)


def dense_system(Q, Pi):
    """Q (x) I_C + blockdiag(H_i) in the row-major vec order (i C + c): the naive form, for small checks."""
    n, C = Pi.shape
    A = np.kron(Q, np.eye(C))
    Hm = hess_blocks(Pi)
    for i in range(n):
        A[i * C:(i + 1) * C, i * C:(i + 1) * C] += Hm[i]
    return A


def newton(Q, t, obs, C, f0=None, rtol=1e-12, max_steps=100, solver=None):
    """Dense float64 Newton with step halving on psi.  Returns (F, trace): trace holds one (psi, relative gradient, step) per
    Newton step; the gradient max |G - Q F| is relative to its value at F = 0."""
    n = Q.shape[0]
    solver = Solver(Q, obs) if solver is None else solver
    F = np.zeros((n, C)) if f0 is None else np.array(f0, np.float64)
    grad0 = np.abs(gradient(Q, np.zeros((n, C)), t, obs)).max()
    trace = []
    for _ in range(max_steps):
        R = gradient(Q, F, t, obs)
        if np.abs(R).max() <= rtol * grad0:
            break
        delta = solver.solve(site(F, t, obs)[2], R)
        cur, step = psi(Q, F, t, obs), 1.0
        while psi(Q, F + step * delta, t, obs) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        F = F + step * delta
        trace.append((psi(Q, F, t, obs), np.abs(gradient(Q, F, t, obs)).max() / grad0, step))
    return F, trace


def steps_to(trace, rtol):
    """Newton steps the float64 iteration takes until its relative gradient is <= rtol."""
    for k, (_, rel, _) in enumerate(trace):
        if rel <= rtol:
            return k + 1
    return len(trace)


def softmax(F):
    F = np.asarray(F, np.float64)
    return np.exp(F - logsumexp(F, axis=-1, keepdims=True))
