"""float64 restatement of the block recurrence of mgp_softmax_cg_block (manifold_gp_amd/csrc/softmax_cg_block.hip): S systems
A X_s = B_s with the shared matrix A = Q (x) I_C + H(Pi), blocks [n, S, C] as in the library, one Chronopoulos-Gear scalar set
per sample and the freeze rule (a sample whose relative residual is <= tol takes no further update).  Test infrastructure,
dense Q."""
import numpy as np

import _softmax_ref as sref


def apply_block(Q, Pi, X):
    """A X_s for every sample: [n, S, C] -> [n, S, C]"""
    n, S, C = X.shape
    W = (Q @ X.reshape(n, S * C)).reshape(n, S, C)
    P = Pi[:, None, :]
    return W + P * X - P * (P * X).sum(-1, keepdims=True)


def block_cg(Q, Pi, B, tol, max_iter=5000):
    """(X [n, S, C], iters [S], resid [S], status, frozen_at): frozen_at[s] = (step, copy of X_s) when sample s froze, or None.
    Step k decides on r_{k-1}; status 1 when every sample is frozen, 2 when step > max_iter, 3 on a non-finite residual."""
    Pi, B = np.asarray(Pi, np.float64), np.asarray(B, np.float64)
    n, S, C = B.shape
    X, R = np.zeros_like(B), B.copy()
    P, Sv = np.zeros_like(B), np.zeros_like(B)
    bb = np.zeros(S)
    gamma_old, alpha_old = np.zeros(S), np.zeros(S)
    iters, rel = np.zeros(S, np.int64), np.zeros(S)
    frozen_at = [None] * S
    status = 0
    for step in range(1, max_iter + 2):
        W = apply_block(Q, Pi, R)
        gamma = np.einsum("isc,isc->s", R, R)
        delta = np.einsum("isc,isc->s", R, W)
        if step == 1:
            bb = gamma.copy()
        rel = np.where(bb != 0.0, np.sqrt(gamma / np.where(bb != 0.0, bb, 1.0)), 0.0)
        frozen = rel <= tol
        for s in np.flatnonzero(frozen):
            if frozen_at[s] is None:
                frozen_at[s] = (step, X[:, s].copy())
        if not np.isfinite(rel).all():
            status = 3
        elif frozen.all():
            status = 1
        elif step > max_iter:
            status = 2
        if status:
            break
        for s in np.flatnonzero(~frozen):
            if step == 1:
                beta, alpha = 0.0, gamma[s] / delta[s]
            else:
                beta = gamma[s] / gamma_old[s]
                alpha = gamma[s] / (delta[s] - beta * gamma[s] / alpha_old[s])
            P[:, s] = R[:, s] + beta * P[:, s]
            Sv[:, s] = W[:, s] + beta * Sv[:, s]
            X[:, s] += alpha * P[:, s]
            R[:, s] -= alpha * Sv[:, s]
            gamma_old[s], alpha_old[s] = gamma[s], alpha
            iters[s] += 1
    return X, iters, rel, status, frozen_at


def plain_cg(A, b, tol, max_iter=5000):
    """Textbook CG on a dense SPD system in float64: (x, iterations to ||r|| <= tol ||b||)."""
    x, r = np.zeros_like(b), b.copy()
    p = r.copy()
    rr, bb = r @ r, b @ b
    for k in range(max_iter):
        if np.sqrt(rr / bb) <= tol:
            return x, k
        Ap = A @ p
        a = rr / (p @ Ap)
        x += a * p
        r -= a * Ap
        rr, old = r @ r, rr
        p = r + (rr / old) * p
    return x, max_iter


def hess_block_outputs(pi, x, y):
    """What mgp_softmax_hessian_add_block leaves on float32 inputs pi [n, C], x, y [n, S, C]: (want [n, S, C] float64, the error
    bound of test_gpu_softmax.test_hessian_epilogue_matches_float64 entry by entry)."""
    p64, x64 = pi.astype(np.float64)[:, None, :], x.astype(np.float64)
    C = pi.shape[1]
    want = y.astype(np.float64) + (p64 * x64 - p64 * (p64 * x64).sum(-1, keepdims=True))
    Sabs = np.abs(p64 * x64).sum(-1, keepdims=True)
    L = np.log2(max(2, 1 << (C - 1).bit_length()))
    bound = (1.0 + 1e-3) * 2.0 ** -24 * (np.abs(want) + 2.0 * np.abs(p64 * x64) + (L + 3.0) * p64 * Sabs)
    return want, bound


__all__ = ["apply_block", "block_cg", "plain_cg", "hess_block_outputs", "sref"]
