"""float64 restatement of the form-3 posterior of manifold_gp_amd/sampling.py (observed subsets, per-node noise) and of the
dense pieces it is checked with.  Test infrastructure, sized for the dumbbell fixtures."""
import numpy as np

from _sampling_ref import edge_factor
from oracle.laplacian import LaplacianOracle
from oracle.precision import dense_matern_precision


def oracle(g, norm):
    return LaplacianOracle(g["edge_value"], g["edge_index"], g["train_x"].shape[0], float(g["eps"]), norm,
                           bool(g["self_loops"]), dtype=np.float64)


def precision_root(lo, nu, kappa, scale, norm):
    """(Q2, R) with R R^T = Q2 the map precision_samples applies: sqrt(scale) P A^((nu-1)/2) G (odd nu), sqrt(scale) P A^(nu/2)
    (even nu), A = tau I + L_sym, G = [sqrt(tau) I | E]."""
    n = lo.n
    tau = 2.0 * nu / kappa ** 2
    A = tau * np.eye(n) + lo.dense_symmetric()
    P = np.sqrt(lo.degree) if norm == "randomwalk" else np.ones(n)
    Q2 = scale * dense_matern_precision(lo.dense(), nu, kappa, lo.degree if norm == "randomwalk" else None)
    if nu % 2:
        r, c = lo.idx[0], lo.idx[1]
        G = np.hstack([np.sqrt(tau) * np.eye(n), edge_factor(n, r, c, lo.triu, np.sqrt(lo.degree))])
        R = np.linalg.matrix_power(A, (nu - 1) // 2) @ G
    else:
        R = np.linalg.matrix_power(A, nu // 2)
    return Q2, np.sqrt(scale) * P[:, None] * R


def weights(var, obs):
    """(s_ref, w): s_ref = min over observed sigma_i^2, w_i = obs_i s_ref / sigma_i^2."""
    var = np.asarray(var, np.float64)
    s_ref = float(var[obs].min())
    return s_ref, np.where(obs, s_ref / var, 0.0)


def system(Q2, w, s_ref):
    """A3 = W + s_ref Q2 (operator form 3)."""
    return np.diag(w) + s_ref * Q2


def mean(Q2, y, var, obs):
    """A3^-1 W y, the targets of unobserved nodes never read."""
    s_ref, w = weights(var, obs)
    return np.linalg.solve(system(Q2, w, s_ref), w * np.where(obs, y, 0.0))


def perturbed_rhs(y, var, obs, z, w2):
    """W y + s_ref z + sqrt(s_ref) W^1/2 w2 for z [n, S], w2 [n, S]."""
    s_ref, w = weights(var, obs)
    return (w * np.where(obs, y, 0.0))[:, None] + s_ref * z + np.sqrt(s_ref * w)[:, None] * w2


def samples(Q2, y, var, obs, z, w2):
    s_ref, w = weights(var, obs)
    return np.linalg.solve(system(Q2, w, s_ref), perturbed_rhs(y, var, obs, z, w2))


def device_q2(desc):
    """scipy float64 Q2 = scale P (tau I + L_sym)^nu P from the descriptor's own (device) CSR: the matrix the kernels apply."""
    import scipy.sparse as sp
    data = desc.data
    gr = data.graph
    n = gr.n
    rowptr, col = gr.rowptr.cpu().numpy(), gr.col.cpu().numpy()
    L = sp.csr_matrix((-data.vals.double().cpu().numpy(), col, rowptr), shape=(n, n)) + sp.diags(data.diag.double().cpu().numpy())
    A = (2.0 * int(desc.nu) / float(desc.kappa) ** 2) * sp.identity(n, format="csr") + L
    Q = sp.identity(n, format="csr")
    for _ in range(int(desc.nu)):
        Q = (A @ Q).tocsr()
    if desc.pre is not None:
        P = sp.diags(desc.pre.double().cpu().numpy())
        Q = (P @ Q @ P).tocsr()
    return float(desc.scale) * Q
