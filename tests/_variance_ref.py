"""float64 restatement of the marginal-variance estimator of manifold_gp_amd/sampling.py::posterior_variance
(docs/kernels/sampling.md, "Marginal variances"): the diagonal formulas of csrc/variance.hip on dense matrices, the
perturbation p = s z + sqrt(s) W^1/2 w2 from the Philox restatement of _sampling_ref, dense solves, the single-site
Rao-Blackwell and the plain estimator with their standard errors, and the truth diag((Q2 + W / s)^-1).  Test
infrastructure, sized for the dumbbell fixtures; no device code."""
import math

import numpy as np

import _observed_ref as oref
from _sampling_ref import edge_factor, edge_noise, node_noise


def diag_power(a, S, nu):
    """diag((diag(a) - S)^nu), nu = 1, 2, 3, for a dense S with zero diagonal, by the formulas of csrc/variance.hip:
    a, a^2 + sum_j S_ij S_ji, a^3 + 2 a sum_j S_ij S_ji + sum_j a_j S_ij S_ji - sum_j S_ij sum_k S_jk S_ki."""
    if nu == 1:
        return a.copy()
    s2 = (S * S.T).sum(1)
    if nu == 2:
        return a * a + s2
    if nu == 3:
        return a ** 3 + 2.0 * a * s2 + (S * S.T) @ a - ((S @ S) * S.T).sum(1)
    raise ValueError("nu must be 1, 2 or 3")


def split(A):
    """(a, S) with A = diag(a) - S, S with zero diagonal."""
    a = np.diag(A).copy()
    return a, np.diag(a) - A


def q2_diag(lo, nu, kappa, scale, norm):
    """diag(Q2) = scale P_i^2 diag((tau I + L_sym)^nu)_i through diag_power (P = sqrt(degree) for the random walk)."""
    a, S = split(2.0 * nu / kappa ** 2 * np.eye(lo.n) + lo.dense_symmetric())
    p2 = lo.degree if norm == "randomwalk" else np.ones(lo.n)
    return scale * p2 * diag_power(a, S, nu)


def system_diag(q, form, s=0.0, w=None):
    """The diagonal of operator form 0 (Q2), 2 (I + s Q2), 3 (W + s Q2) from q = diag(Q2)."""
    return {0: q, 2: 1.0 + s * q, 3: (0.0 if w is None else w) + s * q}[form]


class Dense:
    """The dense float64 pieces of one (fixture, normalisation, nu, scale, kappa): Q2 and the map of the noise to z."""

    def __init__(self, g, norm, nu, scale, kappa=None):
        self.lo = lo = oref.oracle(g, norm)
        self.n, self.nu, self.scale, self.norm = lo.n, nu, scale, norm
        self.kappa = float(g["kappa"]) if kappa is None else float(kappa)
        self.tau = 2.0 * nu / self.kappa ** 2
        A = self.tau * np.eye(lo.n) + lo.dense_symmetric()
        self.P = np.sqrt(lo.degree) if norm == "randomwalk" else np.ones(lo.n)
        self.Ak = np.linalg.matrix_power(A, (nu - 1) // 2 if nu % 2 else nu // 2)
        self.Q2 = scale * self.P[:, None] * np.linalg.matrix_power(A, nu) * self.P[None, :]
        self.r, self.c = lo.idx[0], lo.idx[1]
        self.E = edge_factor(lo.n, self.r, self.c, lo.triu, np.sqrt(lo.degree)) if nu % 2 else None

    def z(self, seed, S, offset=0, cache=None):
        """z = sqrt(scale) P A^k noise for the global samples offset .. offset + S - 1 (sampling._precision_chunk);
        cache: a dict that keeps the node and edge normals, which depend on (seed, S, offset) and the edge list alone."""
        cache = {} if cache is None else cache
        key = ("w0", seed, S, offset)
        if key not in cache:
            cache[key] = node_noise(self.n, 0, seed, offset, S)
        noise = cache[key]
        if self.nu % 2:
            key = ("we", seed, S, offset)
            if key not in cache:
                cache[key] = edge_noise(self.r, self.c, seed, offset, S)
            noise = math.sqrt(self.tau) * noise + self.E @ cache[key]
        return math.sqrt(self.scale) * self.P[:, None] * (self.Ak @ noise)

    def w2(self, seed, S, offset=0, cache=None):
        cache = {} if cache is None else cache
        key = ("w2", seed, S, offset)
        if key not in cache:
            cache[key] = node_noise(self.n, 2, seed, offset, S)
        return cache[key]


def perturbation(z, w2, s, w):
    """p = s z + sqrt(s) W^1/2 w2 (sampling._perturbation): Cov p = s A3."""
    return s * z + np.sqrt(s * w)[:, None] * w2


def truth(Q2, w, s):
    """diag((Q2 + W / s)^-1) = s diag(A3^-1)."""
    return s * np.diag(np.linalg.inv(oref.system(Q2, w, s)))


def estimate(delta, p, d, s, method="rao-blackwell"):
    """(var, se) from the draws delta = A3^-1 p [n, S]: e = delta - p / d and the floor s / d (rao-blackwell), e = delta and no
    floor (samples); var = floor + mean e^2, se = sqrt((mean e^4 - (mean e^2)^2) / S)."""
    S = delta.shape[1]
    if method == "rao-blackwell":
        e, floor = delta - p / d[:, None], s / d
    else:
        e, floor = delta, 0.0
    m2, m4 = (e ** 2).mean(1), (e ** 4).mean(1)
    return floor + m2, np.sqrt(np.maximum(m4 - m2 * m2, 0.0) / S)


def draws(dense, var, obs, seed, S, cache=None):
    """(delta, p, d, s): the S draws delta = A3^-1 p [n, S] of global sample indices 0 .. S - 1 from the Philox streams of
    `seed`, for per-node noise variances var [n] and the observed mask obs [n]; d = diag(A3), s = s_ref."""
    s, w = oref.weights(var, obs)
    A3 = oref.system(dense.Q2, w, s)
    p = perturbation(dense.z(seed, S, 0, cache), dense.w2(seed, S, 0, cache), s, w)
    return np.linalg.solve(A3, p), p, np.diag(A3).copy(), s


def reference(dense, var, obs, seed, S, method="rao-blackwell", cache=None):
    """(var, se) of the float64 estimator on draws(...)."""
    delta, p, d, s = draws(dense, var, obs, seed, S, cache)
    return estimate(delta, p, d, s, method)
