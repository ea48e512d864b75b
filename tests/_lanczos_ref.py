"""What the Lanczos tests share (tests/test_lanczos_cpu.py, tests/test_gpu_lanczos.py): the launch geometry of the Lanczos kernels
of csrc/eigen.hip restated, three float64 invariants of one Lanczos run, and a float32 numpy restatement of the kernels' algorithm
(with planted errors) that fixes the bounds of the invariants without the code under test.

Geometry (csrc/eigen.hip)
  block form   blz_layout: RL = 256 / P row lanes, nblk = min(256, ceil(n / 4 RL)) workgroups re-derived from rpb = ceil(n / nblk)
               rows each, element grids of min(2048, ceil(n P / 256)) workgroups; blz_reduce_kernel walks the nblk partials in four
               lanes (blocks part, part + 4, ...; 32 blocks per trip of its loop) and adds the lanes as (0 + 1) + (2 + 3).
  single form  mgp_lanczos_tridiag: nblk = min(512, ceil(n / 1024)) workgroups of 256 threads, a thread walks its rows with stride
               256, a wave adds its 64 lanes as a balanced tree (mgp_wave_sum), thread 0 adds the four waves and ONE thread adds
               all nblk partials in order; element grid min(2048, ceil(n / 256)).

Invariants of one run (start vector z, alpha[steps], beta[steps], basis Q[steps + 1, n] cast up to float64, a float64 product,
normA >= ||A||_2), all in units of u = 2^-24:
  I0  max_i |q_0,i - z_i / ||z||| / max_i |q_0,i|                          bound (L / 2 + 3) u, L the longest summation chain
  I1  max |Q Q^T - I| over all steps + 1 vectors                           bound I1_BOUND u
  I2  max_j ||A q_j - beta_{j-1} q_{j-1} - alpha_j q_j - beta_j q_{j+1}||_2 / normA    bound I2_BOUND u
I0's bound is derived: the sum of squares carries a relative error of at most L u (one rounding per product, L - 1 additions on the
longest chain), the square root halves it and rounds once, the reciprocal and the product round once each.  A start vector taken
from another column is O(1) in I0 and invisible to I1 and I2 (Lanczos from a wrong start satisfies them too).

I1_BOUND and I2_BOUND are 16 times the worst figure the restatement below reaches over the cases of tests/test_lanczos_cpu.py,
rounded up to a power of two.  Measured there (every figure is printed by that test):
  k = 10 swiss rolls of 9 ... 525,319 nodes, nu = 1, 2, 3, 5 ... 47 steps, widths 1 ... 16 and the single-vector geometry:
      I1 <= 5.3 u (67 nodes, P = 3),  I2 <= 1.4 u ||A|| (67 nodes, P = 16);  at 525,319 nodes 2.9 u and 0.6 u ||A||
  the rings of the width sweep (ring_cases below: every P, 2 ... 2,051 nodes, every column, 1 ... 6 steps):
      I1 <= 15.5 u,  I2 <= 3.1 u ||A||  (both at P = 1, 257 nodes)
  ->  I1_BOUND = 256,  I2_BOUND = 64.
The factor 16 is for what the restatement does not model: the kernels contract a product and a sum to one FMA, the operator
product is the library's SpMM (its own row order and float32 Laplacian entries), and sqrt / reciprocal are the device's.  The
smallest planted error the bounds must catch (one of 256 workgroup partials dropped at 525,319 rows: I1 72,300 u, I2 1,050 u ||A||)
sits 16 times above the I2 bound and 280 times above the I1 bound.  The bounds are never taken from a GPU run.
"""
import numpy as np

U = 2.0 ** -24
BLOCK = 256                 # csrc/eigen.hip kBlock
BLZ_MAX_BLOCKS = 256        # blz_layout: std::min<int64_t>(256, mgp_cdiv(n, 4 * b.RL))
BLZ_MAX_NQ = 48             # kBlzMaxNq: steps + 1 <= 48 (48 KB of dynamic LDS in blz_dots_kernel at RL P = 256)
BLZ_MAX_P = 16              # kBlzMaxP
BLZ_REDUCE_TRIP = 32        # blz_reduce_kernel: `b0 += 32`, eight loads per lane per trip
LZ_MAX_BLOCKS = 512         # mgp_lanczos_tridiag: std::min<int64_t>(512, mgp_cdiv(n, 1024))
LZ_ROWS = 1024
MAX_EGRID = 2048            # both forms: std::min<int64_t>(2048, ...)

I1_MEASURED, I2_MEASURED = 15.5, 3.1
I1_BOUND = 256
I2_BOUND = 64
PRECONDITION = 2.0 ** -6    # min_j beta_j >= 2^-6 normA, or normalising w amplifies round-off and I1 means nothing


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================ launch geometry
def blz_geometry(n, P):
    """blz_layout: (RL, nblk, rpb, egrid)."""
    RL = BLOCK // P
    nblk = max(1, min(BLZ_MAX_BLOCKS, _cdiv(n, 4 * RL)))
    rpb = _cdiv(n, nblk)
    nblk = _cdiv(n, rpb)
    return RL, nblk, rpb, min(MAX_EGRID, _cdiv(n * P, BLOCK))


def lz_geometry(n):
    """mgp_lanczos_tridiag: (nblk, rpb, egrid)."""
    nblk = max(1, min(LZ_MAX_BLOCKS, _cdiv(n, LZ_ROWS)))
    rpb = _cdiv(n, nblk)
    nblk = _cdiv(n, rpb)
    return nblk, rpb, min(MAX_EGRID, _cdiv(n, BLOCK))


def blz_reduce_trips(nblk):
    """Trips of blz_reduce_kernel's block loop for lane 0."""
    return _cdiv(nblk, BLZ_REDUCE_TRIP)


def blz_chain(n, P):
    """Longest summation chain of one dot product of the block form: a thread's rows, the RL row lanes added in order, a lane's walk
    over every fourth partial, the two quad additions."""
    RL, nblk, rpb, _ = blz_geometry(n, P)
    return _cdiv(rpb, RL) + RL + _cdiv(nblk, 4) + 2


def lz_chain(n):
    """The same for the single-vector form: a thread's rows, the wave tree (6), the four waves (3), all partials in order."""
    nblk, rpb, _ = lz_geometry(n)
    return _cdiv(rpb, BLOCK) + 6 + 3 + nblk


def i0_bound(L):
    return 0.5 * L + 3.0


def blz_dots_lds_bytes(P, nq):
    """Dynamic LDS of blz_dots_kernel: sh[nq][RL][P] floats."""
    return nq * (BLOCK // P) * P * 4


# ================================================================================ float64 invariants (torch, any device)
def invariants(z, alpha, beta, Q, matmul64, normA, upto=None):
    """(I0, I1, I2) in units of u for one run.  z [n], Q [steps + 1, n]: torch tensors (cast to float64 here); alpha, beta [steps]:
    anything array-like; matmul64: [n, C] float64 -> [n, C] float64.  upto: check the first `upto` basis vectors only (and the
    relation over the first upto - 1 steps).  A non-finite figure comes back as inf."""
    import torch
    Q = Q.double()
    z = z.double().to(Q.device)
    m = Q.shape[0] if upto is None else int(upto)
    steps = m - 1
    Q = Q[:m]
    a = torch.as_tensor(np.asarray(alpha, np.float64)[:steps]).to(Q.device)
    b = torch.as_tensor(np.asarray(beta, np.float64)[:steps]).to(Q.device)
    i0 = float((Q[0] - z / torch.linalg.vector_norm(z)).abs().max() / Q[0].abs().max()) / U
    G = Q @ Q.t()
    i1 = float((G - torch.eye(m, dtype=torch.float64, device=Q.device)).abs().max()) / U
    i2 = 0.0
    if steps > 0:
        R = matmul64(Q[:steps].t().contiguous()).t() - a[:, None] * Q[:steps] - b[:, None] * Q[1:m]
        R[1:] -= b[:steps - 1, None] * Q[:steps - 1]
        i2 = float(torch.linalg.vector_norm(R, dim=1).max()) / float(normA) / U
    return tuple(v if np.isfinite(v) else float("inf") for v in (i0, i1, i2))


def gershgorin_norm(L_abs_rowsum_max, tau, nu, scale=1.0, dmax=None):
    """Upper bound of ||A||_2 for A = scale (tau I + L_sym)^nu (x D^1/2 on both sides for the random walk: times max D)."""
    v = float(scale) * (float(tau) + float(L_abs_rowsum_max)) ** int(nu)
    return v * float(dmax) if dmax is not None else v


# ================================================================================ float32 restatement
def _tree(x):
    """Balanced tree over adjacent pairs of the last axis (a power of two long): mgp_wave_sum's order."""
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(np.float32)
    return x[..., 0]


class Summation:
    """The float32 summation order of one dot product over n rows, for a batch of products prod [..., n]."""

    def __init__(self, n, P=None):
        """P: the block form at that width; None: the single-vector form."""
        self.n, self.P = int(n), P
        if P is None:
            self.nblk, self.rpb, _ = lz_geometry(n)
            self.lanes = BLOCK
        else:
            self.lanes, self.nblk, self.rpb, _ = blz_geometry(n, P)
        self.chain = _cdiv(self.rpb, self.lanes)

    def partials(self, prod):
        """[..., nblk] workgroup partials."""
        prod = np.asarray(prod, np.float32)
        lead = prod.shape[:-1]
        full = np.zeros(lead + (self.nblk * self.rpb,), np.float32)
        full[..., :self.n] = prod
        pad = np.zeros(lead + (self.nblk, self.chain * self.lanes), np.float32)
        pad[..., :self.rpb] = full.reshape(lead + (self.nblk, self.rpb))
        pad = pad.reshape(lead + (self.nblk, self.chain, self.lanes))
        t = pad[..., 0, :].copy()
        for c in range(1, self.chain):                       # a thread's rows, in order
            t += pad[..., c, :]
        if self.P is None:                                   # wave trees, then the four waves in order
            w = _tree(t.reshape(lead + (self.nblk, 4, 64)))
            return ((w[..., 0] + w[..., 1]).astype(np.float32) + w[..., 2]).astype(np.float32) + w[..., 3]
        blk = np.zeros(lead + (self.nblk,), np.float32)
        for k in range(self.lanes):                          # the RL row lanes, in order
            blk += t[..., k]
        return blk

    def total(self, part):
        """Sum of the workgroup partials [..., nblk] in the kernels' order."""
        part = np.asarray(part, np.float32)
        if self.P is None:                                   # one thread, all partials in order
            s = np.zeros(part.shape[:-1], np.float32)
            for b in range(self.nblk):
                s += part[..., b]
            return s
        lanes = []
        for q in range(4):                                   # lane q: blocks q, q + 4, ...
            s = np.zeros(part.shape[:-1], np.float32)
            for b in range(q, self.nblk, 4):
                s += part[..., b]
            lanes.append(s)
        return ((lanes[0] + lanes[1]).astype(np.float32) + (lanes[2] + lanes[3]).astype(np.float32)).astype(np.float32)


PLANTS = ("drop_block", "skip_last_row", "double_row", "swap_columns")


def lanczos_f32(matmul32, z, steps, P=None, plant=None, z_other=None):
    """The kernels' algorithm in float32 numpy for ONE start vector z [n]: q_0 = z / ||z||; per step w = A q_j, two passes of
    classical Gram-Schmidt against q_0 .. q_j (alpha_j = the sum of both passes' coefficient on q_j), beta_j = ||w||,
    q_{j+1} = w / beta_j.  Every dot product is summed in the order of `Summation(n, P)`.  matmul32: [n] float32 -> [n] float32.
    Planted errors:
      drop_block     the partial of workgroup nblk // 2 is left out of every dot product and norm
      skip_last_row  row n - 1 is left out of every dot product and norm
      double_row     row n - 1 is counted twice (an unmasked clamped row)
      swap_columns   q_0 is made from z_other (the neighbouring column's start vector)
    Returns alpha[steps], beta[steps], Q[steps + 1, n] (float32)."""
    assert plant is None or plant in PLANTS
    z = np.asarray(z, np.float32)
    n = z.size
    S = Summation(n, P)

    def dots(W, V):
        prod = (W * V).astype(np.float32)
        if plant == "skip_last_row":
            prod[..., n - 1] = 0
        elif plant == "double_row":
            prod[..., n - 1] *= 2
        part = S.partials(prod)
        if plant == "drop_block":
            part[..., S.nblk // 2] = 0
        return S.total(part)

    start = np.asarray(z_other, np.float32) if plant == "swap_columns" else z
    Q = np.zeros((steps + 1, n), np.float32)
    with np.errstate(all="ignore"):
        Q[0] = start * (np.float32(1) / np.sqrt(dots(start, start)))
        al, be = np.zeros(steps, np.float32), np.zeros(steps, np.float32)
        for j in range(steps):
            w = np.asarray(matmul32(Q[j]), np.float32)
            a = np.float32(0)
            for _ in range(2):
                h = dots(w[None, :], Q[:j + 1])
                for i in range(j + 1):
                    w = (w - h[i] * Q[i]).astype(np.float32)
                a = np.float32(a + h[j])
            al[j] = a
            be[j] = np.sqrt(dots(w, w))
            Q[j + 1] = w * (np.float32(1) / be[j]) if be[j] > 0 else 0
    return al, be, Q


# ================================================================================ graphs on the host
def swiss_graph(n, k=10, seed=1337, order="random"):
    """k-NN graph of tools.synth.swiss_roll on the host (scipy cKDTree): (idx [2, M] int64 with row < col, val [M] float32 mean
    squared distance of an edge's two directions, eps by synth.bandwidth_rule)."""
    from scipy.spatial import cKDTree
    from tools import synth
    x, _ = synth.swiss_roll(n, seed=seed, order=order)
    x = x.astype(np.float64)
    k = min(k, n)
    d, i = cKDTree(x).query(x, k)
    rows = np.repeat(np.arange(n), k - 1)
    cols = i[:, 1:].ravel()
    vals = (d[:, 1:] ** 2).ravel()
    key = np.minimum(rows, cols) * n + np.maximum(rows, cols)
    uq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    s = np.zeros(len(uq))
    np.add.at(s, inv, vals)
    eps = synth.bandwidth_rule(d[:, 1] ** 2, 0.0)[0]
    return np.stack([uq // n, uq % n]), (s / cnt).astype(np.float32), float(eps)


def host_operator(idx, val, n, eps, nu, kappa, scale=1.0, normalization="symmetric"):
    """(SparsePrecision in float64, float32 product of the same matrix, normA): A = scale (tau I + L_sym)^nu, for the random walk
    D^1/2 (.) D^1/2 around it.  The float32 product rounds after every sparse product and every scaling, as a chain of nu fused
    launches does."""
    from oracle.laplacian import LaplacianOracle
    from oracle.sparse import SparsePrecision
    lap = LaplacianOracle(val, idx, n, eps, normalization, True, dtype=np.float64)
    Pm = SparsePrecision(lap, nu, kappa, scale)
    L32 = Pm.L.astype(np.float32)
    tau32, s32 = np.float32(Pm.tau), np.float32(scale)
    d32 = None if Pm.dsq is None else Pm.dsq.astype(np.float32)

    def matmul32(v):
        out = np.asarray(v, np.float32)
        out = out if d32 is None else (out * d32).astype(np.float32)
        for _ in range(nu):
            out = (tau32 * out + L32 @ out).astype(np.float32)
        out = out if d32 is None else (out * d32).astype(np.float32)
        return (s32 * out).astype(np.float32)
    gersh = float(abs(Pm.L).sum(1).max())
    dmax = float(lap.degree.max()) if normalization == "randomwalk" else None
    return Pm, matmul32, gershgorin_norm(gersh, Pm.tau, nu, scale, dmax)


# ================================================================================ the tiny and ragged rings of the width sweep
RING_EPS, RING_NU, RING_KAPPA_OVER_EPS, RING_SCALE, RING_STEPS = 0.5, 2, 4.0, 0.7, 6
RING_GATE = 2.0 ** -5.5      # the start blocks are drawn until the float64 run has min beta >= this x normA in every column


def ring_edges(sizes, rng):
    """Disjoint rings of the given sizes (2 nodes: one edge) with random squared distances: idx [2, M] (row < col, sorted), val [M]."""
    pairs, off = [], 0
    for m in sizes:
        if m == 2:
            pairs.append((off, off + 1))
        elif m > 2:
            pairs += [(off + min(i, (i + 1) % m), off + max(i, (i + 1) % m)) for i in range(m)]
        off += m
    pairs = np.unique(np.array(pairs, np.int64), axis=0)
    return np.ascontiguousarray(pairs.T), rng.uniform(0.05, 1.5, len(pairs)).astype(np.float32)


def start_block(n, P, seed):
    """Gaussian columns [n, P] (float32), column p scaled by 2^(p - 8): a norm taken from the wrong column shows."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, P)) * 2.0 ** (np.arange(P) - 8.0)).astype(np.float32)


def ring_sizes(P):
    RL = BLOCK // P
    return [n for n in sorted({2, 3, RL - 1, RL + 1, 4 * RL - 1, 4 * RL, 4 * RL + 1, 8 * RL + 3}) if n >= 2]


def ring_cases(P):
    """The rings of the width sweep at width P: for every n of ring_sizes(P) a dict(n, idx, val, Z, steps, Pm, matmul32, normA,
    min_beta).  A Gaussian start vector on 2 or 3 nodes is close to an eigenvector every 25th time or so, and then beta_0 is small
    against ||A||, q_1 amplifies round-off and I1 means nothing: such a column is redrawn (seeds 1000 P + n, + 10^6, ...) until
    its FLOAT64 Lanczos run has min beta >= 2^-5.5 normA.  The inputs are chosen by the reference alone."""
    from oracle.solvers import lanczos_tridiag_f64
    rng = np.random.default_rng(100 + P)
    for n in ring_sizes(P):
        idx, val = ring_edges([n], rng)
        Pm, matmul32, normA = host_operator(idx, val, n, RING_EPS, RING_NU, RING_KAPPA_OVER_EPS * RING_EPS, float(np.float32(RING_SCALE)))
        steps = min(n - 1, RING_STEPS)
        Z, mb, redrawn = start_block(n, P, 1000 * P + n), np.inf, 0
        for p in range(P):
            for attempt in range(100):
                b = lanczos_tridiag_f64(Pm.matmul, Z[:, p].astype(np.float64), steps + 1)[1][:steps].min()
                if b >= RING_GATE * normA:
                    break
                Z[:, p] = start_block(n, P, 1000 * P + n + 1000000 * (attempt + 1))[:, p]
                redrawn += 1
            else:
                raise AssertionError("no start vector with the precondition at P = %d, n = %d, column %d" % (P, n, p))
            mb = min(mb, b)
        yield dict(n=n, idx=idx, val=val, Z=Z, steps=steps, Pm=Pm, matmul32=matmul32, normA=normA, min_beta=mb, redrawn=redrawn)
