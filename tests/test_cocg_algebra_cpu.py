"""CPU test (no GPU) of the algebra behind the complex-shift solve's stopping rule (cg.hip cx_update_kernel), restated in
numpy float64 on the oracle operator of the committed dumbbell fixture.

A = I + sigma^2 B^2 (form 2, nu = 2, symmetric normalisation, sigma^2 = noise * scale, B = tau I + L_sym) is solved as
x = Re z with (I + i sigma B) z = y by COCG.  The complex residual r = y - (I + i sigma B) z does NOT bound the residual of
the real system: y - A Re z = r_re + sigma B r_im, up to |I - i sigma B| ~ sqrt(cond A) larger.  The kernel therefore stops
on ||r_re + sigma B r_im||; these tests keep the identity and the iteration saving under the CPU suite."""
import numpy as np
import pytest

from oracle.laplacian import LaplacianOracle
from oracle.sparse import SparsePrecision


def _system(golden, noise=1e-2, scale=0.7):
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    lo = LaplacianOracle(g["edge_value"], g["edge_index"], n, float(g["eps"]), "symmetric", bool(g["self_loops"]),
                         dtype=np.float64)
    sp_ = SparsePrecision(lo, 1, float(g["kappa"]) / np.sqrt(2.0))     # B = tau I + L_sym, tau = 2 nu / kappa^2 at nu = 2
    sigma = np.sqrt(noise * scale)
    Bm = lambda v: sp_.matmul(v)
    A = lambda v: v + sigma * sigma * Bm(Bm(v))
    return Bm, A, sigma, g["train_y"].astype(np.float64)


def _cocg(Bm, sigma, y, tol, rule, max_iter=2000):
    """COCG on (I + i sigma B) z = y; rule 'complex' stops on ||r||, 'real' on ||r_re + sigma B r_im||.  Returns
    (Re z, iterations, identity defect per step)."""
    M = lambda v: v + 1j * sigma * (Bm(v.real) + 1j * Bm(v.imag))
    z = np.zeros(y.shape, np.complex128)
    r = y.astype(np.complex128)
    p = r.copy()
    gamma = r @ r                                  # unconjugated bilinear form
    yn = np.linalg.norm(y)
    defects = []
    for it in range(max_iter + 1):
        e = r.real + sigma * Bm(r.imag)            # the real system's residual of Re z
        defects.append(np.linalg.norm((y - (z.real + sigma * sigma * Bm(Bm(z.real)))) - e) / yn)
        rel = np.linalg.norm(e if rule == "real" else r) / yn
        if rel <= tol:
            return z.real, it, defects
        w = M(p)
        alpha = gamma / (p @ w)
        z = z + alpha * p
        r = r - alpha * w
        gamma_new = r @ r
        p = r + (gamma_new / gamma) * p
        gamma = gamma_new
    raise AssertionError("COCG did not converge")


def _cg(A, y, tol, max_iter=5000):
    x = np.zeros_like(y)
    r = y.copy()
    p = r.copy()
    rr = r @ r
    yn = np.linalg.norm(y)
    for it in range(max_iter + 1):
        if np.sqrt(rr) <= tol * yn:
            return x, it
        w = A(p)
        alpha = rr / (p @ w)
        x = x + alpha * p
        r = r - alpha * w
        rr_new = r @ r
        p = r + (rr_new / rr) * p
        rr = rr_new
    raise AssertionError("CG did not converge")


@pytest.mark.parametrize("tol", [1e-2, 1e-4, 1e-6])
def test_cocg_real_residual_identity_and_stop(golden, tol):
    Bm, A, sigma, y = _system(golden)
    yn = np.linalg.norm(y)
    true_rel = lambda x: np.linalg.norm(y - A(x)) / yn
    # the identity y - A Re z == r_re + sigma B r_im at every step of the recurrence
    x_re, its_re, defects = _cocg(Bm, sigma, y, tol, "real")
    assert max(defects) < 1e-12, max(defects)
    # stopping on that residual meets tol on the real system, in fewer iterations than CG on A
    assert true_rel(x_re) <= tol * (1 + 1e-9)
    x_cg, its_cg = _cg(A, y, tol)
    assert true_rel(x_cg) <= 1.01 * tol
    assert its_re < its_cg, (its_re, its_cg)
    # stopping on the complex residual does not: it reports tol while the real system misses it
    x_cx, its_cx, _ = _cocg(Bm, sigma, y, tol, "complex")
    assert its_cx < its_re and true_rel(x_cx) > 2 * tol, (its_cx, true_rel(x_cx) / tol)


def test_cocg_real_stop_on_a_near_identity_system():
    """The 20k swiss roll of the GPU tests (16 nearest neighbours by scipy here, eps 0.35, kappa 1, c = 1e-2): cond(A) ~ 2.5,
    where COCG stopped on the real residual needs as many steps as CG on A (each of one product instead of two) and
    the complex residual's earlier stop leaves the real system above the tolerance."""
    from scipy.spatial import cKDTree
    import scipy.sparse as sp
    from oracle.sparse import laplacian_sym_csr
    from tools import synth
    x, _ = synth.swiss_roll(20000, seed=5, order="morton")
    n = x.shape[0]
    d, i = cKDTree(x).query(x, 17)
    r, c, v = np.repeat(np.arange(n), 16), i[:, 1:].reshape(-1), (d[:, 1:] ** 2).reshape(-1)
    a, b = np.minimum(r, c), np.maximum(r, c)
    _, first = np.unique(a * n + b, return_index=True)
    lo = LaplacianOracle(v[first].astype(np.float32), np.stack([a[first], b[first]]), n, 0.35, "symmetric", True,
                         dtype=np.float64)
    Bs = (4.0 * sp.eye(n) + laplacian_sym_csr(lo)).tocsr()          # tau = 2 nu / kappa^2 = 4
    sigma = 0.1
    Bm = lambda v: Bs @ v
    A = lambda v: v + sigma * sigma * Bm(Bm(v))
    y = np.random.default_rng(31).normal(size=n)
    tol = 1e-6
    true_rel = lambda xx: np.linalg.norm(y - A(xx)) / np.linalg.norm(y)
    x_re, its_re, _ = _cocg(Bm, sigma, y, tol, "real")
    _, its_cg = _cg(A, y, tol)
    x_cx, its_cx, _ = _cocg(Bm, sigma, y, tol, "complex")
    assert true_rel(x_re) <= tol and its_re <= its_cg, (its_re, its_cg)
    assert its_cx < its_re and true_rel(x_cx) > tol, (its_cx, its_re, true_rel(x_cx) / tol)
