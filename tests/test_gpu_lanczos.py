"""The Lanczos kernels of the stochastic log-determinant (csrc/eigen.hip: lz_dots / lz_update / lz_normalize, blz_dots / blz_reduce /
blz_update / blz_normalize) against float64, at the sizes and widths where their launch geometry changes.

Every run is checked through the three invariants of tests/_lanczos_ref.py, column by column, in float64 (torch.float64 on the
device: oracle/grad_ref.py's Laplacian over the graph's own edge list, the Gram and residual algebra with one column's basis at a
time): I0 the start vector, I1 orthonormality of all steps + 1 vectors, I2 the three-term relation against ||A|| -- with the bounds
that file derives (I0) or fixes from its float32 restatement (I1: 256 u, I2: 64 u ||A||), never from a run of the kernels.  The
block form is run as mgp_blz_begin / desc.apply on mgp_blz_q(j) / mgp_blz_step / mgp_blz_end so that the basis can be read, and
mgp_lanczos_tridiag_block on the same inputs must return the same alpha and beta bit for bit.  Start blocks are Gaussian columns
scaled by 2^(p - 8): a norm or a start vector taken from the wrong column is O(1) in I0.

  a  every width P = 1 ... 16 on tiny and ragged rings (n = 2 ... 8 RL + 3);
  b  a 20,011-node swiss roll: rows per workgroup that are no multiple of 2 RL (the clamped second row of blz_dots_kernel),
     the deepest basis (48 vectors, 47 KB of LDS at P = 13), one random-walk operator;
  c  a 525,319-node swiss roll: 256 workgroups (the cap of blz_layout) and 8 trips of blz_reduce_kernel's loop, element grids at
     their 2048 cap, 48 KB of LDS at (16, 47); the single-vector form at its 512-workgroup cap;
  d  columns are independent (bit for bit), a zero column stays zero;
  e  a start vector whose Krylov space is exhausted after 5 steps: the quadrature truncates and is exact;
  f  slq_logdet at 525,319 nodes against the same estimator in float64 with the same probes;
  g  refusals.
Every case asserts, through the helper's formulas, that the geometry it targets ran.  The precondition of I1 (min beta >= 2^-6
normA) is asserted on the device's own beta: I2 pins every beta to 64 u ||A||, five orders below that threshold.
The measured worst ratios are in each docstring and in docs/kernels/eigen.md ("The Lanczos kernels against float64").
"""
import ctypes

import numpy as np
import pytest
import torch

import _lanczos_ref as lr
from oracle.grad_ref import laplacian_apply_f64, laplacian_f64

pytestmark = pytest.mark.gpu

U = lr.U
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3
BIG_N = 525_319
MID_N = 20_011
SCALE = 0.7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mgp():
    import manifold_gp_amd
    from manifold_gp_amd import _lib
    _lib.lib()
    return manifold_gp_amd


# ================================================================================ graphs, operators, float64 reference
class Graph:
    """A KnnGraph, its Laplacian data on the device, and the float64 Laplacian of the same edge list (on the device too)."""

    def __init__(self, mgp, graph, eps, dev):
        from manifold_gp_amd.graph import LaplacianData
        self.graph, self.n, self.dev = graph, graph.n, dev
        self.eps = float(np.float32(eps))
        self.data = LaplacianData(graph, self.eps, True)
        idx = graph.edge_index.cpu()
        lap = laplacian_f64(graph.edge_value.double().cpu(), idx, self.n, torch.tensor(self.eps, dtype=torch.float64), True)
        g = lap["diag"].abs().index_add(0, idx[0], lap["triu"].abs()).index_add(0, idx[1], lap["triu"].abs())
        self.gersh = float(g.max())                          # max_i sum_j |L_ij|: Gershgorin bound of ||L_sym||
        self.dmax = float(lap["degree"].max())
        self.lap = {k: v.to(dev) for k, v in lap.items()}
        self.idx = idx.to(dev)

    def operator(self, nu, kappa_over_eps, randomwalk=False):
        """(descriptor of A = SCALE (tau I + L)^nu [x D for the random walk], its float64 product, normA)."""
        from manifold_gp_amd.operators._descriptor import Descriptor
        kappa = float(np.float32(kappa_over_eps * self.eps))
        scale = float(np.float32(SCALE))
        sq = self.data.dsqrt if randomwalk else None
        desc = Descriptor(self.data, int(nu), kappa, pre=sq, post=sq, scale=scale)
        tau = 2.0 * nu / (kappa * kappa)
        d = self.lap["dsqrt"].view(-1, 1)

        def matmul64(V):
            out = V * d if randomwalk else V
            for _ in range(nu):
                out = tau * out + laplacian_apply_f64(self.lap, self.idx, out)
            return scale * (out * d if randomwalk else out)
        return desc, matmul64, lr.gershgorin_norm(self.gersh, tau, nu, scale, self.dmax if randomwalk else None)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _coo_graph(mgp, dev, idx, val, n, tiles="auto"):
    return Graph(mgp, mgp.graph.KnnGraph.from_coo(T(idx, dev), T(val, dev), int(n), tiles=tiles), lr.RING_EPS, dev)


def _swiss(mgp, dev, n, seed):
    from tools import synth
    x_np, _ = synth.swiss_roll(n, seed=seed, order="random")
    x = T(x_np, dev)
    knn = mgp.utils.NearestNeighbors(x)
    D, _ = knn.search(x, 10)
    knn.graph(10)
    eps = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 0.0)[0]
    return Graph(mgp, knn.knn_graph, eps, dev)


@pytest.fixture(scope="module")
def roll20k(mgp, dev):
    return _swiss(mgp, dev, MID_N, 3)


@pytest.fixture(scope="module")
def roll525k(mgp, dev):
    return _swiss(mgp, dev, BIG_N, 3)


def start_block(n, P, seed, dev):
    """Gaussian columns, column p scaled by 2^(p - 8)."""
    return T(lr.start_block(n, P, seed), dev)


# ================================================================================ running the kernels
def run_block(desc, Z, steps, compare=True):
    """P Lanczos runs through mgp_blz_begin / desc.apply / mgp_blz_step / mgp_blz_end on a workspace of its own: alpha, beta
    [steps, P] (float64 numpy) and the basis [steps + 1, n, P] (a view of the workspace).  compare: mgp_lanczos_tridiag_block on
    the same inputs returns the same alpha and beta bit for bit."""
    from manifold_gp_amd import _lib, slq
    lib = _lib.lib()
    n, P = Z.shape
    Z = _lib.f32c(Z)
    wb = lib.mgp_blz_workspace_bytes(n, P, steps)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=Z.device)
    wp, st = _lib.ptr(work), _lib.stream()
    _lib.check(lib.mgp_blz_begin(_lib.ptr(Z), n, P, steps, wp, wb, st), "mgp_blz_begin")
    off = int(lib.mgp_blz_q(n, P, steps, 0, wp, wb)) - work.data_ptr()
    Qall = work[off:off + (steps + 1) * n * P * 4].view(torch.float32).view(steps + 1, n, P)
    for j in range(steps):
        assert int(lib.mgp_blz_q(n, P, steps, j, wp, wb)) == Qall[j].data_ptr()
        W = _lib.f32c(desc.apply(Qall[j]))
        assert W.data_ptr() != Qall[j].data_ptr()
        _lib.check(lib.mgp_blz_step(_lib.ptr(W), n, P, steps, j, wp, wb, st), "mgp_blz_step")
    alpha = (ctypes.c_float * (steps * P))()
    beta = (ctypes.c_float * (steps * P))()
    _lib.check(lib.mgp_blz_end(n, P, steps, alpha, beta, wp, wb, st), "mgp_blz_end")
    A = np.array(alpha, dtype=np.float64).reshape(steps, P)
    B = np.array(beta, dtype=np.float64).reshape(steps, P)
    if compare:
        A1, B1 = slq.lanczos_tridiag_block(desc, Z, steps)
        assert np.array_equal(A, A1) and np.array_equal(B, B1), "descriptor form and begin / step / end differ"
    return A, B, Qall


def run_single(desc, z, steps):
    """mgp_lanczos_tridiag with Q_out: alpha, beta [steps], Q [steps, n]."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    op = desc.struct()
    n = desc.n
    wb = lib.mgp_lanczos_tridiag_workspace_bytes(ctypes.byref(op), steps)
    work = torch.empty(wb, dtype=torch.uint8, device=z.device)
    alpha = (ctypes.c_float * steps)()
    beta = (ctypes.c_float * steps)()
    Qm = torch.full((steps, n), float("nan"), device=z.device)
    _lib.check(lib.mgp_lanczos_tridiag(ctypes.byref(op), _lib.ptr(_lib.f32c(z)), steps, alpha, beta, _lib.ptr(Qm), _lib.ptr(work),
                                       work.numel(), _lib.stream()), "mgp_lanczos_tridiag")
    return np.array(alpha, dtype=np.float64), np.array(beta, dtype=np.float64), Qm


def check_block(A, B, Qall, Z, matmul64, normA, L, cols=None, upto=None, where=""):
    """Asserts I0, I1, I2 and the precondition for the given columns; returns the worst (I0 / bound, I1, I2)."""
    worst = [0.0, 0.0, 0.0]
    steps = A.shape[0] if upto is None else upto - 1
    for p in (range(Z.shape[1]) if cols is None else cols):
        assert np.isfinite(A[:, p]).all() and np.isfinite(B[:, p]).all(), (where, p)
        assert B[:steps, p].min() >= lr.PRECONDITION * normA, (where, p, B[:steps, p].min() / normA)
        i0, i1, i2 = lr.invariants(Z[:, p], A[:, p], B[:, p], Qall[:, :, p], matmul64, normA, upto=upto)
        assert i0 <= lr.i0_bound(L), (where, "I0", p, i0, lr.i0_bound(L))
        assert i1 <= lr.I1_BOUND, (where, "I1", p, i1)
        assert i2 <= lr.I2_BOUND, (where, "I2", p, i2)
        worst = [max(worst[0], i0 / lr.i0_bound(L)), max(worst[1], i1), max(worst[2], i2)]
    return worst


# ================================================================================ a. every width, tiny and ragged
@pytest.mark.parametrize("P", list(range(1, 17)))
def test_every_width_on_tiny_and_ragged_rings(mgp, dev, P):
    """For RL = 256 / P row lanes: rings of n = 2, 3, RL - 1, RL + 1, 4 RL - 1, 4 RL, 4 RL + 1, 8 RL + 3 nodes with random squared
    distances (one, two and three workgroups; chunks shorter than the row lanes, one row past them, one row short of and past
    four passes), steps = min(n - 1, 6), A = 0.7 (tau I + L_sym)^2; inputs from _lanczos_ref.ring_cases (start columns redrawn until
    the float64 run has the precondition).  For P that does not divide 256, 256 - RL P threads idle.
    Measured worst over all widths and sizes: I0 0.20 of its bound (P = 15), I1 12.0 u of 256 (P = 1), I2 4.5 u ||A|| of 64 (P = 7); the
    float32 restatement on the same inputs: 0.20, 15.5 u, 3.1 u ||A||."""
    RL = 256 // P
    worst = [0.0, 0.0, 0.0]
    sizes = []
    for case in lr.ring_cases(P):
        n, steps = case["n"], case["steps"]
        sizes.append(n)
        G = _coo_graph(mgp, dev, case["idx"], case["val"], n, tiles=None)
        desc, matmul64, normA = G.operator(lr.RING_NU, lr.RING_KAPPA_OVER_EPS)
        assert abs(normA - case["normA"]) <= 1e-9 * normA and steps == min(n - 1, 6)
        RLg, nblk, rpb, egrid = lr.blz_geometry(n, P)
        assert RLg == RL and nblk == -(-n // (4 * RL)) and nblk <= 3 and rpb * nblk >= n and (256 - RL * P > 0) == (256 % P != 0)
        Z = T(case["Z"], dev)
        A, B, Qall = run_block(desc, Z, steps)
        w = check_block(A, B, Qall, Z, matmul64, normA, lr.blz_chain(n, P), where=("rings", P, n))
        worst = [max(a, b) for a, b in zip(worst, w)]
    assert sizes == sorted({2, 3, RL - 1, RL + 1, 4 * RL - 1, 4 * RL, 4 * RL + 1, 8 * RL + 3} - {0, 1})
    print("rings P=%2d: worst I0 %.2f of its bound, I1 %.1f u, I2 %.2f u||A||" % (P, worst[0], worst[1], worst[2]))


# ================================================================================ b. mid size
@pytest.mark.parametrize("P,steps,norm", [(5, 20, "symmetric"), (12, 20, "symmetric"), (13, 47, "symmetric"), (12, 20, "randomwalk")])
def test_mid_size_ragged_passes(mgp, dev, roll20k, P, steps, norm):
    """20,011-node swiss roll, k = 10: 99 ... 254 workgroups whose rows are no multiple of 2 RL (the second row of a pass of
    blz_dots_kernel is clamped and masked in the last pass; at P = 12 the ragged last workgroup only), a ragged last workgroup; (13, 47): 48 basis vectors, 47,424 bytes of
    dynamic LDS, 9 idle threads.  Symmetric nu = 2 (kappa = 3 eps); random walk nu = 1 (pre = post = sqrt(D), kappa = eps).
    Measured worst: I0 0.06 of its bound, I1 6.0 u of 256 and I2 0.95 u ||A|| of 64 (both at (13, 47)); random walk 4.4 u and 0.91 u ||A||."""
    G = roll20k
    rw = norm == "randomwalk"
    desc, matmul64, normA = G.operator(1 if rw else 2, 1.0 if rw else 3.0, randomwalk=rw)
    RL, nblk, rpb, egrid = lr.blz_geometry(G.n, P)
    last = G.n - (nblk - 1) * rpb
    # a workgroup whose row count is no multiple of 2 RL ends on a pass with a clamped second row: every workgroup at P = 5 and
    # 13 (203 and 79 rows), the ragged last one at P = 12 (19 of 84 rows, fewer than the 21 row lanes)
    assert G.n == MID_N and nblk > 32 and 0 < last < rpb and egrid < lr.MAX_EGRID
    assert last % (2 * RL) != 0 and (rpb % (2 * RL) != 0 or P == 12)
    if steps == 47:
        assert steps + 1 == lr.BLZ_MAX_NQ and lr.blz_dots_lds_bytes(P, steps + 1) == 47424
    Z = start_block(G.n, P, 7 * P + steps, dev)
    A, B, Qall = run_block(desc, Z, steps)
    w = check_block(A, B, Qall, Z, matmul64, normA, lr.blz_chain(G.n, P), where=("20k", P, steps, norm))
    print("20k %s P=%d steps=%d: worst I0 %.2f of its bound, I1 %.1f u, I2 %.2f u||A||" % (norm, P, steps, w[0], w[1], w[2]))


# ================================================================================ c. past the caps
@pytest.mark.parametrize("P,steps", [(16, 47), (12, 20), (7, 9), (1, 6)])
def test_block_form_past_the_caps(mgp, dev, roll525k, P, steps):
    """525,319 nodes: nblk = 256 (the cap of blz_layout; 2,053 rows per workgroup), 8 trips of blz_reduce_kernel's block loop, element
    grids at the 2048 cap, and at (16, 47) 48 x 16 x 16 x 4 = 49,152 bytes of dynamic LDS in blz_dots_kernel.
    Measured worst: I0 0.03 of its bound, I1 5.4 u of 256, I2 0.96 u ||A|| of 64 (both at (16, 47)); (1, 6): 2.1 u, 0.60 u ||A||."""
    G = roll525k
    desc, matmul64, normA = G.operator(2, 3.0)
    RL, nblk, rpb, egrid = lr.blz_geometry(G.n, P)
    assert G.n == BIG_N and nblk == lr.BLZ_MAX_BLOCKS == 256 and -(-G.n // (4 * RL)) > 256
    assert lr.blz_reduce_trips(nblk) >= 2
    assert egrid == lr.MAX_EGRID and -(-G.n * P // 256) > 2048
    if P >= 2:
        assert G.n * P / 256 > 2048
    if (P, steps) == (16, 47):
        assert lr.blz_dots_lds_bytes(P, steps + 1) == 48 * RL * P * 4 == 49152
    Z = start_block(G.n, P, 11 * P + steps, dev)
    A, B, Qall = run_block(desc, Z, steps)
    w = check_block(A, B, Qall, Z, matmul64, normA, lr.blz_chain(G.n, P), where=("525k", P, steps))
    print("525k P=%d steps=%d: worst I0 %.2f of its bound, I1 %.1f u, I2 %.2f u||A||" % (P, steps, w[0], w[1], w[2]))


@pytest.mark.parametrize("steps", [6, 50])
def test_single_vector_form_past_the_caps(mgp, dev, roll525k, steps):
    """mgp_lanczos_tridiag at 525,319 > 512 x 1024 rows: 512 workgroups of 1,027 rows (the last one ragged), one thread adds the 512
    partials; 50 steps is the depth at which slq_logdet leaves the block form.  Q_out holds q_0 .. q_{steps-1}: I1 over those,
    I2 over the first steps - 1 relations.
    Measured: 6 steps I0 0.98 u (bound 266), I1 5.4 u, I2 0.89 u ||A||; 50 steps I0 2.75 u, I1 13.8 u of 256, I2 1.74 u ||A|| of 64."""
    G = roll525k
    desc, matmul64, normA = G.operator(2, 3.0)
    nblk, rpb, egrid = lr.lz_geometry(G.n)
    assert G.n > 512 * 1024 and nblk == lr.LZ_MAX_BLOCKS == 512 and rpb == 1027 and G.n % rpb != 0 and egrid == lr.MAX_EGRID
    assert steps + 1 > lr.BLZ_MAX_NQ or steps == 6
    z = start_block(G.n, 1, 50 + steps, dev)[:, 0].contiguous() * 37.0
    a, b, Q = run_single(desc, z, steps)
    assert np.isfinite(a).all() and np.isfinite(b).all() and bool(torch.isfinite(Q).all())
    assert b.min() >= lr.PRECONDITION * normA
    L = lr.lz_chain(G.n)
    i0, i1, i2 = lr.invariants(z, a, b, Q, matmul64, normA)
    print("525k single steps=%d: I0 %.2f u (bound %.1f), I1 %.1f u, I2 %.2f u||A||" % (steps, i0, lr.i0_bound(L), i1, i2))
    assert i0 <= lr.i0_bound(L) and i1 <= lr.I1_BOUND and i2 <= lr.I2_BOUND, (i0, i1, i2)


# ================================================================================ d. independent columns, the zero column
def test_columns_are_independent_and_a_zero_column_stays_zero(mgp, dev, roll20k):
    """P = 12, 20 steps at 20,011 nodes.  Replacing ONE start column leaves every other column's alpha and beta bit-identical; an
    all-zero start column gives alpha = beta = 0 exactly (blz_normalize_kernel: `b > 0 ? 1 / b : 0`), nothing non-finite, and the
    other columns bit-identical again."""
    G = roll20k
    desc, matmul64, normA = G.operator(2, 3.0)
    P, steps, c = 12, 20, 5
    Z = start_block(G.n, P, 77, dev)
    A0, B0, _ = run_block(desc, Z, steps)
    others = [p for p in range(P) if p != c]
    Z1 = Z.clone()
    Z1[:, c] = start_block(G.n, 1, 78, dev)[:, 0] * 300.0
    A1, B1, _ = run_block(desc, Z1, steps)
    assert np.array_equal(A0[:, others], A1[:, others]) and np.array_equal(B0[:, others], B1[:, others])
    assert not np.array_equal(A0[:, c], A1[:, c])
    Z2 = Z.clone()
    Z2[:, c] = 0.0
    A2, B2, Q2 = run_block(desc, Z2, steps)
    assert np.isfinite(A2).all() and np.isfinite(B2).all() and bool(torch.isfinite(Q2).all())
    assert (A2[:, c] == 0).all() and (B2[:, c] == 0).all() and float(Q2[:, :, c].abs().max()) == 0.0
    assert np.array_equal(A0[:, others], A2[:, others]) and np.array_equal(B0[:, others], B2[:, others])


# ================================================================================ e. exhausted Krylov space
def test_exhausted_krylov_space_truncates_the_quadrature(mgp, dev):
    """Two components, a ring of 5 nodes and a ring of 400; column 0 lives on the small ring, so its Krylov space is exhausted
    after 5 of the 12 steps: beta_4 is round-off, what follows is noise, and slq._quadrature_log_sum must cut there.  With five
    exact steps e_1^T log f(T) e_1 IS z^T log f(A_5) z / z^T z on the 5-node block: within the project's 1e-5 relative bound of
    the dense float64 value for f of forms 0, 1 and 2.  The other columns keep I1 and I2 over their first 11 vectors.
    Measured: relative error 7.2e-9, 6.7e-9 and 1.9e-8 for forms 0, 1, 2; the other columns I1 4.3 u, I2 1.26 u ||A||."""
    from manifold_gp_amd import slq
    rng = np.random.default_rng(5)
    n, P, steps = 405, 5, 12
    idx, val = lr.ring_edges([5, 400], rng)
    G = _coo_graph(mgp, dev, idx, val, n)
    desc, matmul64, normA = G.operator(2, 2.0)
    Z = start_block(n, P, 9, dev)
    Z[:, 0] = 0.0
    Z[:5, 0] = T(rng.standard_normal(5).astype(np.float32), dev)
    A, B, Qall = run_block(desc, Z, steps)
    assert float(Qall[:5, 5:, 0].abs().max()) == 0.0                      # the column never leaves its component
    assert abs(B[4, 0]) < 1e-6 * abs(A[4, 0]) and (B[:4, 0] >= 1e-3 * np.abs(A[:4, 0])).all(), (B[:6, 0], A[:6, 0])
    E = torch.zeros(n, 5, dtype=torch.float64, device=dev)
    E[torch.arange(5), torch.arange(5)] = 1.0
    A5 = matmul64(E)[:5].cpu().numpy()
    assert float(matmul64(E)[5:].abs().max()) == 0.0
    lam, V = np.linalg.eigh(0.5 * (A5 + A5.T))
    z = Z[:5, 0].double().cpu().numpy()
    wgt = (V.T @ z) ** 2 / (z @ z)
    sn = 1e-2
    worst = 0.0
    for form, fun in ((0, None), (1, lambda th: th - sn * th * th + sn * sn * th * th * th), (2, lambda th: 1.0 + sn * th)):
        ref = float(np.sum(wgt * np.log(fun(lam) if fun is not None else lam)))
        got = slq._quadrature_log_sum(A[:, :1], B[:, :1], fun)
        err = abs(got - ref) / abs(ref)
        print("exhausted Krylov space, form %d: quadrature %.9g, dense %.9g, relative error %.2e" % (form, got, ref, err))
        assert np.isfinite(got) and err <= 1e-5, (form, got, ref)
        worst = max(worst, err)
    w = check_block(A, B, Qall, Z, matmul64, normA, lr.blz_chain(n, P), cols=range(1, P), upto=11, where="two rings")
    print("two rings: worst quadrature error %.2e; other columns I0 %.2f of its bound, I1 %.1f u, I2 %.2f u||A||" % (
        worst, w[0], w[1], w[2]))


# ================================================================================ f. end to end at size
@pytest.mark.parametrize("form", [1, 2])
def test_slq_logdet_at_size_vs_float64_same_probes(mgp, dev, roll525k, form):
    """slq_logdet of form 1 (Q - s Q^2 + s^2 Q^3) and form 2 (I + s Q), Q = 0.7 (tau I + L_sym)^2 on 525,319 nodes, 12 probes, 20
    steps, against oracle.solvers.slq_logdet_same_probes with the same probes and the float64 product: within 1e-5 relative (the
    project's bound of test_slq_logdet_vs_dense).
    Measured: relative error 3.8e-8 (form 1) and 2.0e-8 (form 2); 4.3 ... 5.7 s per form, nearly all of it the float64 reference on the host."""
    from manifold_gp_amd.slq import rademacher_probes, slq_logdet
    from oracle.solvers import slq_logdet_same_probes
    G = roll525k
    desc, matmul64, normA = G.operator(2, 3.0)
    sn = 1e-2

    class Op:
        def _descriptor(self):
            return desc.with_(form=form, noise=sn)
    ld = float(slq_logdet(Op(), num_probes=12, steps=20))
    Zp = rademacher_probes(G.n, 12, 1337, dev).double().cpu().numpy()
    fun = (lambda th: th - sn * th * th + sn * sn * th ** 3) if form == 1 else (lambda th: 1.0 + sn * th)

    def mm(v):
        return matmul64(torch.from_numpy(v).to(dev).view(-1, 1)).view(-1).cpu().numpy()
    ref = slq_logdet_same_probes(mm, Zp, 20, fun=fun)
    err = abs(ld - ref) / abs(ref)
    print("slq_logdet 525k form %d: device %.9g, float64 %.9g, relative error %.2e" % (form, ld, ref, err))
    assert np.isfinite(ld) and err <= 1e-5, (ld, ref)


# ================================================================================ g. refusals
def test_refusals(mgp, dev, roll20k):
    """Shapes past the limits (P = 17, steps = 48) have workspace 0 and are MGP_ERR_UNSUPPORTED; a workspace one byte short is
    MGP_ERR_WORKSPACE for begin, step and end alike; step j = steps is MGP_ERR_ARG.  None of these launches anything."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    G = roll20k
    desc, _, _ = G.operator(2, 3.0)
    op = desc.struct()
    n, P, steps = G.n, 4, 7
    st = _lib.stream()
    Z = start_block(n, 17, 1, dev)
    small = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = (ctypes.c_float * (64 * 17))()
    for p, s in ((17, 7), (4, 48), (17, 48)):
        assert lib.mgp_blz_workspace_bytes(n, p, s) == 0
        assert lib.mgp_lanczos_tridiag_block_workspace_bytes(ctypes.byref(op), p, s) == 0
        assert lib.mgp_blz_begin(_lib.ptr(Z), n, p, s, _lib.ptr(small), small.numel(), st) == ERR_UNSUPPORTED
        assert lib.mgp_blz_step(_lib.ptr(Z), n, p, s, 0, _lib.ptr(small), small.numel(), st) == ERR_UNSUPPORTED
        assert lib.mgp_blz_end(n, p, s, out, out, _lib.ptr(small), small.numel(), st) == ERR_UNSUPPORTED
        assert lib.mgp_blz_q(n, p, s, 0, _lib.ptr(small), small.numel()) is None
        assert lib.mgp_lanczos_tridiag_block(ctypes.byref(op), _lib.ptr(Z), p, s, out, out, _lib.ptr(small), small.numel(),
                                             st) == ERR_UNSUPPORTED
    assert lib.mgp_blz_workspace_bytes(n, 16, 47) > 0 and lib.mgp_blz_workspace_bytes(n, 1, 1) > 0
    wb = lib.mgp_blz_workspace_bytes(n, P, steps)
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    W = torch.zeros(n, P, device=dev)
    assert lib.mgp_blz_begin(_lib.ptr(Z), n, P, steps, _lib.ptr(work), wb - 1, st) == ERR_WORKSPACE
    assert lib.mgp_blz_step(_lib.ptr(W), n, P, steps, 0, _lib.ptr(work), wb - 1, st) == ERR_WORKSPACE
    assert lib.mgp_blz_end(n, P, steps, out, out, _lib.ptr(work), wb - 1, st) == ERR_WORKSPACE
    assert lib.mgp_blz_q(n, P, steps, 0, _lib.ptr(work), wb - 1) is None
    assert lib.mgp_blz_step(_lib.ptr(W), n, P, steps, steps, _lib.ptr(work), wb, st) == ERR_ARG
    assert lib.mgp_blz_step(_lib.ptr(W), n, P, steps, -1, _lib.ptr(work), wb, st) == ERR_ARG
    assert lib.mgp_blz_q(n, P, steps, steps + 1, _lib.ptr(work), wb) is None
    wbd = lib.mgp_lanczos_tridiag_block_workspace_bytes(ctypes.byref(op), P, steps)
    assert wbd > wb
    big = torch.zeros(wbd, dtype=torch.uint8, device=dev)
    assert lib.mgp_lanczos_tridiag_block(ctypes.byref(op), _lib.ptr(Z), P, steps, out, out, _lib.ptr(big), wbd - 1,
                                         st) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(work.float().abs().max()) == 0.0 and float(big.float().abs().max()) == 0.0       # nothing was written
