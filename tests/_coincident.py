"""Fixtures with coincident points: graphs that carry self edges (i, i).  Test infrastructure, no GPU, no fixture files of its
own: everything is generated from a seed or from tests/golden/dumbbell_k10_loop.npz.

The reference drops column 0 of every k-NN list unconditionally.  With ties ordered by (distance,
index) a repeated point i finds its lower-indexed twin in column 0 and itself in a later column, so the edge list carries
(i, i) with squared distance 0.  The rule every stage is held to: the edge list is the reference's, and the matrix is the one
the reference applies, L_sym = diag - S - S^T with a self edge counted in both scatters -- its diagonal is diag_i - 2 S_ii, its
degrees include 2 W_ii and 2 A_ii (oracle.laplacian.LaplacianOracle does exactly that, in float64 here).

  cloud300      300 standard-normal points in R^3, k = 6; x[40] = x[41] = x[7], x[299] = x[0], x[150] = x[151]
  dumbbell_dup  the 1,546 training points of the dumbbell fixture, k = 10, 12 rows overwritten by copies of other rows
  coo_self      a hand-written 65-node edge list: a ring over nodes 0..63, self edges with non-zero distance at 0, 63 and 64;
                node 64 has no other entry

Each is a dict with the keys of the golden fixtures that the descriptor helpers of the other test modules read (train_x,
train_y, edge_index, edge_value, eps, kappa, k, self_loops) plus knn_D / knn_I (the oracle's search), self_nodes, and `dense`:
{(normalization, self_loops): float64 [n, n]} = LaplacianOracle(..., dtype=float64).dense().
"""
import functools
import os

import numpy as np

from oracle import knn as oknn
from oracle.laplacian import LaplacianOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORMS = ("symmetric", "randomwalk")

# dumbbell_dup: row DST[j] becomes a copy of row SRC[j].  (3, 5) share a 16-row tile; (63, 64) and the triple (509, 511, 512)
# straddle a 64-row tile boundary; (100, 700), (200, 1000, 1001), (40, 1300) and (0, 1545) join distant parts of the curve.
DUP_DST = (5, 64, 700, 1000, 1001, 1545, 130, 257, 511, 512, 900, 1300)
DUP_SRC = (3, 63, 100, 200, 200, 0, 127, 256, 509, 509, 899, 40)


def bandwidth_rule(d2_first, floor):
    """The notebooks' rule: the smallest eps at which every node keeps a nearest-neighbour weight >= 1e-4, not below `floor`."""
    return max(float(floor), float(np.sqrt(np.max(d2_first) / (-4.0 * np.log(1e-4)))))


def oracle(g, norm, self_loops=True, eps=None):
    return LaplacianOracle(g["edge_value"], g["edge_index"], g["n"], float(g["eps"]) if eps is None else eps, norm, self_loops,
                           dtype=np.float64)


def _finish(g):
    idx = g["edge_index"]
    g["n"] = int(g["train_x"].shape[0])
    g["self_nodes"] = np.sort(idx[0][idx[0] == idx[1]])
    g["dense"] = {(norm, loops): oracle(g, norm, loops).dense() for norm in NORMS for loops in (True, False)}
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)          # shared among the tests: nobody edits it
    for v in g["dense"].values():
        v.setflags(write=False)
    return g


def _knn_fixture(x, y, k, eps_floor, kappa):
    x = np.ascontiguousarray(x, np.float32)
    D, I = oknn.knn_search(x, x, k)
    idx, val = oknn.knn_graph_from_search(D, I, x.shape[0])
    # the nearest OTHER point: column 1, or column 0 on the rows whose own index is not first
    first = np.where(I[:, 0] == np.arange(x.shape[0]), D[:, 1], D[:, 0])
    return _finish(dict(train_x=x, train_y=np.asarray(y, np.float32), knn_D=D, knn_I=I, edge_index=idx, edge_value=val,
                        eps=np.float32(bandwidth_rule(first, eps_floor)), kappa=np.float32(kappa), k=np.int32(k),
                        self_loops=np.bool_(True)))


@functools.lru_cache(maxsize=None)
def cloud300():
    rng = np.random.default_rng(300)
    x = rng.standard_normal((300, 3)).astype(np.float32)
    x[40] = x[41] = x[7]
    x[299] = x[0]
    x[150] = x[151]
    y = np.sin(2.0 * x[:, 0]) + 0.1 * rng.standard_normal(300)
    return _knn_fixture(x, y, 6, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def dumbbell_dup():
    g = np.load(os.path.join(GOLDEN, "dumbbell_k10_loop.npz"))
    x = g["train_x"].copy()
    x[list(DUP_DST)] = x[list(DUP_SRC)]
    return _knn_fixture(x, g["train_y"], int(g["k"]), float(g["eps"]), float(g["kappa"]))


@functools.lru_cache(maxsize=None)
def coo_self():
    rng = np.random.default_rng(65)
    ring = [(i, i + 1) for i in range(63)] + [(0, 63)]
    pairs = np.array(sorted(ring + [(0, 0), (63, 63), (64, 64)]), np.int64)
    val = rng.uniform(0.05, 1.5, len(pairs)).astype(np.float32)
    x = rng.standard_normal((65, 2)).astype(np.float32)          # (never searched: the edge list is the input)
    return _finish(dict(train_x=x, train_y=rng.standard_normal(65).astype(np.float32), edge_index=pairs.T.copy(),
                        edge_value=val, eps=np.float32(0.5), kappa=np.float32(1.0), k=np.int32(0), self_loops=np.bool_(True)))


FIXTURES = dict(cloud300=cloud300, dumbbell_dup=dumbbell_dup, coo_self=coo_self)
KNN_FIXTURES = ("cloud300", "dumbbell_dup")


def self_values(g, self_loops=True, eps=None):
    """(nodes, S_ii): the self edges' nodes and their values S in the float64 oracle (the same for both normalisations)."""
    lo = oracle(g, "symmetric", self_loops, eps)
    sel = lo.idx[0] == lo.idx[1]
    return lo.idx[0][sel], lo.triu[sel]
