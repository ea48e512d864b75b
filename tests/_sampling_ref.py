"""numpy restatement of the GMRF noise generator (csrc/sampling.hip, docs/kernels/sampling.md) and of the dense factor
G = [sqrt(tau) I | E] with G G^T = tau I + L_sym.  Test infrastructure: float64 and vectorised, sized for the dumbbell
fixtures."""
import numpy as np

PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key, rounds=10):
    """Philox4x32-10 (Random123).  ctr: uint32 [..., 4], key: uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
    c = [np.asarray(ctr, np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    key = np.asarray(key, np.uint32)
    k0, k1 = key[..., 0].astype(np.uint64), key[..., 1].astype(np.uint64)
    for r in range(rounds):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(PHILOX_W0)) & MASK32
        k1 = (k1 + np.uint64(PHILOX_W1)) & MASK32
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def seed_key(seed):
    seed = int(seed)
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)


def box_muller(words, s):
    """The normal of global sample index s (array) from the Philox output words [..., 4] of its quad."""
    s = np.asarray(s, np.int64)
    p = (s & 3) >> 1
    a = np.take_along_axis(words, (2 * p)[..., None], axis=-1)[..., 0]
    b = np.take_along_axis(words, (2 * p + 1)[..., None], axis=-1)[..., 0]
    u = ((a >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    v = ((b >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return np.where((s & 1) == 0, r * np.cos(2 * np.pi * v), r * np.sin(2 * np.pi * v))


def _normals(c0, c1, tag, seed, offset, S):
    """N(0, 1) of counters (c0, c1, q, tag) for the S global sample indices offset .. offset + S - 1: [len(c0), S]."""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    s = offset + np.arange(S, dtype=np.int64)
    ctr = np.zeros((len(c0), S, 4), np.uint32)
    ctr[..., 0] = c0[:, None]
    ctr[..., 1] = c1[:, None]
    ctr[..., 2] = (s >> 2)[None, :]
    ctr[..., 3] = tag
    words = philox4x32(ctr, seed_key(seed))
    return box_muller(words, np.broadcast_to(s, (len(c0), S)))


def node_noise(n, tag, seed, offset, S):
    """w_tag [n, S]: counter (i, 0, q, tag)."""
    return _normals(np.arange(n), np.zeros(n, np.int64), tag, seed, offset, S)


def edge_noise(a, b, seed, offset, S):
    """w_edge [M, S] of the undirected edges (a < b): counter (a, b, q, 1)."""
    return _normals(a, b, 1, seed, offset, S)


def csr_edges(rowptr, col, vals):
    """The undirected edges (a < b) of a padded symmetric CSR with their S_ab (entries col == row or S == 0 skipped)."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    keep = (col != rows) & (vals != 0) & (rows < col)
    return rows[keep].astype(np.int64), col[keep].astype(np.int64), vals[keep].astype(np.float64)


def edge_factor(n, a, b, S_ab, dsqrt):
    """Dense E [n, M]: E[a, e] = sqrt(S_ab dsqrt_b / dsqrt_a), E[b, e] = -sqrt(S_ab dsqrt_a / dsqrt_b)."""
    dsqrt = np.asarray(dsqrt, np.float64)
    M = len(a)
    E = np.zeros((n, M))
    e = np.arange(M)
    E[a, e] = np.sqrt(S_ab * dsqrt[b] / dsqrt[a])
    E[b, e] = -np.sqrt(S_ab * dsqrt[a] / dsqrt[b])
    return E


def gmrf_noise_ref(rowptr, col, vals, dsqrt, node_coef, tag, edges, seed, offset, S):
    """float64 restatement of mgp_gmrf_noise: node_coef w_tag (+ E w_edge) [n, S], and max_i ||G_i,:||_1 (the scale of the
    test tolerance; G = [node_coef I | E])."""
    n = len(rowptr) - 1
    Y = node_coef * node_noise(n, tag, seed, offset, S)
    l1 = np.full(n, abs(node_coef))
    if edges:
        a, b, Sab = csr_edges(np.asarray(rowptr), np.asarray(col), np.asarray(vals))
        E = edge_factor(n, a, b, Sab, dsqrt)
        Y = Y + E @ edge_noise(a, b, seed, offset, S)
        l1 = l1 + np.abs(E).sum(1)
    return Y, float(l1.max())
