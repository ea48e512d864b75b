"""Coincident points on the MI355X: every stage, from the search to the Laplace fits, on graphs that carry self edges (i, i)
(tests/_coincident.py), against float64.

The rule.  The edge list is the reference's, bit for bit, self edges included.  The matrix is the one the reference applies,
L_sym = diag - S - S^T with a self edge counted in both scatters (oracle.laplacian.LaplacianOracle in float64: its `dense()`):
diagonal diag_i - 2 S_ii, degrees with 2 W_ii and 2 A_ii.  A stage either agrees with that matrix to the bar its own test holds
it to on duplicate-free graphs (named at each assert), or raises a ValueError on the host that names the number of coincident
nodes.  A stage that computes from another matrix without saying so fails here.

Every test asserts graph.self_edges > 0, so that the fixtures cannot quietly lose their point.
"""
import ctypes
import math
import types
import warnings

import numpy as np
import pytest
import torch

import _coincident as co
import _counts_ref as cref
import _laplace_ref as lref
import _observed_ref as obref
import _ordinal_ref as ordref
from oracle import knn as oknn
from oracle.grad_ref import FLT_MIN, NAMES, laplacian_f64
from oracle.precision import dense_matern_precision
from test_gpu_gradients import _check_tangent
from test_gpu_parity import _tile_invariants

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NORMS = list(co.NORMS)
REFUSAL = r"self edges: \d+ coincident node"


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


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_GRAPHS = {}


def _graph(mgp, dev, name):
    """(fixture, KnnGraph on the device): through the search for the k-NN fixtures, from_coo for the edge list.  Built once."""
    if name not in _GRAPHS:
        g = co.FIXTURES[name]()
        if name in co.KNN_FIXTURES:
            knn = mgp.utils.NearestNeighbors(T(g["train_x"], dev))
            knn.graph(int(g["k"]))
            graph = knn.knn_graph
        else:
            graph = mgp.graph.KnnGraph.from_coo(T(g["edge_index"], dev), T(g["edge_value"], dev), g["n"])
        _GRAPHS[name] = (g, graph)
    g, graph = _GRAPHS[name]
    assert graph.self_edges == len(g["self_nodes"]) > 0
    return g, graph


def _lap(mgp, dev, name, norm, loops=True):
    g, graph = _graph(mgp, dev, name)
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    return mgp.operators.GraphLaplacianOperator(graph.edge_value, graph.edge_index, g["n"], eps, norm, loops, graph=graph)


def _precision(mgp, dev, name, norm, nu, scale=1.0):
    g, _ = _graph(mgp, dev, name)
    lap = _lap(mgp, dev, name, norm)
    kappa = torch.tensor([[float(g["kappa"])]], device=dev)
    return mgp.operators.PrecisionMaternOperator(lap, nu, kappa)._descriptor().with_(scale=scale)


def _q2(g, norm, nu, scale=1.0):
    """float64 Q2 = scale (tau I + L)^nu (x D for the random walk) from the oracle's dense applied matrix"""
    lo = co.oracle(g, norm)
    return scale * dense_matern_precision(g["dense"][(norm, True)], nu, float(g["kappa"]), lo.degree if norm == "randomwalk" else None)


def _form(Q2, form, s=0.0, w=None):
    n = Q2.shape[0]
    if form == 0:
        return Q2
    if form == 1:
        return Q2 - s * Q2 @ Q2 + s * s * Q2 @ Q2 @ Q2
    return (np.eye(n) if form == 2 else np.diag(w)) + s * Q2


# ================================================================================================ 1. search and build
def _csr_invariants(g, graph):
    """rowptr % 4 == 0; every edge id exactly twice; a self-edge row holds its own column twice, adjacent, with the edge's d2,
    ahead of the padding; padding is (col = row, d2 = inf, eid = -1); columns never decrease."""
    n = graph.n
    rp = graph.rowptr.cpu().numpy()
    col, eid, d2 = graph.col.cpu().numpy(), graph.eid.cpu().numpy(), graph.d2.cpu().numpy()
    val = graph.edge_value.cpu().numpy()
    assert (rp % 4 == 0).all() and rp[0] == 0 and rp[-1] == graph.nnz and (np.diff(rp) >= 0).all()
    real = eid >= 0
    assert real.sum() == 2 * graph.M and (np.bincount(eid[real], minlength=graph.M) == 2).all()
    assert np.array_equal(d2[real], val[eid[real]])
    assert np.isinf(d2[~real]).all() and (eid[~real] == -1).all()
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert (col[~real] == rows[~real]).all()
    tri_r, tri_c = graph.tri_row.cpu().numpy(), graph.tri_col.cpu().numpy()
    other = np.where(tri_r[eid[real]] == rows[real], tri_c[eid[real]], tri_r[eid[real]])
    assert np.array_equal(col[real], other)                                        # the entry names the edge's other end
    selfs = set(g["self_nodes"].tolist())
    for r in range(n):
        seg = slice(rp[r], rp[r + 1])
        live = real[seg]
        k = int(live.sum())
        assert live[:k].all()                                                      # entries first, the padding behind them
        c = col[seg][:k]
        own = np.flatnonzero(c == r)
        if r in selfs:
            assert len(own) == 2 and own[1] == own[0] + 1, (r, c)
            e = eid[seg][own]
            assert e[0] == e[1] and tri_r[e[0]] == tri_c[e[0]] == r and (d2[seg][own] == val[e[0]]).all()
            assert (np.diff(np.delete(c, own[1])) > 0).all()                       # strictly ascending but for the repeat
        else:
            assert len(own) == 0 and (np.diff(c) > 0).all()
        assert (np.diff(c) >= 0).all()


@pytest.mark.parametrize("name", co.KNN_FIXTURES)
def test_search_and_graph_bit_exact(mgp, dev, name):
    """Bars of test_knn_bit_exact_vs_golden: indices, distances, edge index and edge value bit for bit against oracle.knn, the
    (i, i) entries included; then the CSR invariants."""
    g, graph = _graph(mgp, dev, name)
    k = int(g["k"])
    x = T(g["train_x"], dev)
    knn = mgp.utils.NearestNeighbors(x)
    D, I = knn.search(x, k)
    assert I.dtype == torch.int64
    assert np.array_equal(I.cpu().numpy(), g["knn_I"]) and np.array_equal(D.cpu().numpy(), g["knn_D"])
    idx, val = knn.graph(k)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), g["edge_index"])
    assert np.array_equal(val.cpu().numpy(), g["edge_value"])
    sel = (idx[0] == idx[1]).cpu().numpy()
    assert np.array_equal(idx[0].cpu().numpy()[sel], g["self_nodes"]) and (val.cpu().numpy()[sel] == 0).all()
    assert knn.knn_graph.self_edges == len(g["self_nodes"]) > 0
    _csr_invariants(g, knn.knn_graph)
    _csr_invariants(g, graph)


@pytest.mark.parametrize("name", co.KNN_FIXTURES)
def test_graph_edges_flag_combinations(mgp, dev, name):
    """mgp_graph_edges for the four flag combinations against the numpy restatement of test_graph_variants_and_errors
    (nearest_neighbors.py:39-55).  With self_loop=True the kept column 0 of a copy is its twin, and its own index sits in a
    later column: the pair (j, j) is still named once, (i, j) twice."""
    g, graph = _graph(mgp, dev, name)
    assert graph.self_edges > 0
    n, k = g["n"], int(g["k"])
    D, I = g["knn_D"], g["knn_I"]
    knn = mgp.utils.NearestNeighbors(T(g["train_x"], dev))
    for symmetric in (False, True):
        for self_loop in (False, True):
            first = 0 if self_loop else 1
            rows = np.repeat(np.arange(n), k - first)
            cols, vals = I[:, first:].reshape(-1), D[:, first:].reshape(-1).astype(np.float32)
            if symmetric:
                lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
                uniq, inv, cnt = np.unique(lo * n + hi, return_inverse=True, return_counts=True)
                ssum = np.zeros(len(uniq), np.float64)
                np.add.at(ssum, inv, vals.astype(np.float64))
                want_idx, want_val = np.stack([uniq // n, uniq % n]), (ssum / cnt).astype(np.float32)
                # the longest run of equal (lo, hi) keys stays 2 on these fixtures (computed on the CPU from the oracle's lists:
                # a pair is named by its two rows at most, a self pair by its own row once), so the mean is over 1 or 2 values
                assert cnt.max() == 2
                if self_loop:                # column 0 of a copy is its twin: its own index, kept, sits in a later column
                    self_keys = g["self_nodes"] * n + g["self_nodes"]
                    assert (cnt[np.searchsorted(uniq, self_keys)] == 1).all() and np.isin(self_keys, uniq).all()
            else:
                want_idx, want_val = np.stack([rows, cols]), vals
            got_idx, got_val = knn.graph(k, symmetric=symmetric, self_loop=self_loop)
            assert got_idx.dtype == torch.int64 and got_val.dtype == torch.float32
            assert np.array_equal(got_idx.cpu().numpy(), want_idx), (symmetric, self_loop)
            assert np.allclose(got_val.cpu().numpy(), want_val, rtol=1e-6, atol=0), (symmetric, self_loop)


def test_from_coo_self_edges(mgp, dev):
    g, graph = _graph(mgp, dev, "coo_self")
    assert graph.self_edges == 3
    assert np.array_equal(graph.edge_index.cpu().numpy(), g["edge_index"])
    _csr_invariants(g, graph)
    rp = graph.rowptr.cpu().numpy()
    assert rp[65] - rp[64] == 4 and (graph.col.cpu().numpy()[rp[64]:rp[65]] == 64).all()   # its self edge twice, then padding
    assert (graph.eid.cpu().numpy()[rp[64]:rp[65]] >= 0).tolist() == [True, True, False, False]


# ================================================================================================ 2. Laplacian build, tangent
def _value_scale(val, idx, n, eps, loops, lap, wmag, constants):
    """Per-entry sum of the magnitudes of the terms of graph_laplacian_operator.py:52-106 (as oracle.grad_ref._term_scale does
    for the tangent): every float32 operation rounds its result by 2^-24, an exponential amplifies the rounding of its argument
    by the argument -- so a weight W counts as `wmag` = W (1 + d2 / (4 eps^2)) -- and the relative perturbations add through the
    products and quotients.  `constants`: the terms without a weight (the self loop's 1, the 1 of diag = (1 - ..) / eps^2).
    With wmag = 2^-126 (1 + arg) on the weights float32 cannot hold as normal numbers this gives the floor instead."""
    r, c = idx[0], idx[1]
    dt_, d_ = lap["degree_unnorm"], lap["degree"]
    one = 1.0 if constants else 0.0
    e2 = eps * eps
    s_dt = torch.zeros(n, dtype=torch.float64).index_add(0, r, wmag).index_add(0, c, wmag) + (one if loops else 0.0)
    rel_dt = s_dt / dt_
    a = lap["triu"] * lap["dsqrt"][r] * lap["dsqrt"][c] * e2
    s_a = wmag / (dt_[r] * dt_[c]) + a * (rel_dt[r] + rel_dt[c] + 2.0 * one)
    s_d = torch.zeros(n, dtype=torch.float64).index_add(0, r, s_a).index_add(0, c, s_a)
    self_a = dt_.pow(-2) if loops else torch.zeros(n, dtype=torch.float64)
    s_d = s_d + self_a * (2.0 * rel_dt + 2.0 * one)
    rel_d = s_d / d_
    s_triu = s_a / (lap["dsqrt"][r] * lap["dsqrt"][c] * e2) + lap["triu"] * (0.5 * rel_d[r] + 0.5 * rel_d[c] + 4.0 * one)
    s_diag = (one + self_a / d_ * (2.0 * rel_dt + rel_d + 3.0 * one)) / e2 if loops else torch.full((n,), one / e2, dtype=torch.float64)
    return dict(degree_unnorm=s_dt, degree=s_d, diag=s_diag, dsqrt=lap["dsqrt"] * (0.5 * rel_d + one),
                dinvsqrt=lap["dinvsqrt"] * (0.5 * rel_d + 2.0 * one), triu=s_triu, w=wmag, a=s_a)


def _check_values(graph, eps, loops):
    """Worst ratio |got - ref| / (2^-24 scale + floor / 64) over the six arrays of LaplacianData and edge_values(0 / 1 / 2): the
    ratio and the bound (64) of test_gpu_gradients._check_tangent, with the scales of _value_scale."""
    from manifold_gp_amd.graph import LaplacianData
    data = LaplacianData(graph, eps, loops)
    eps32 = float(np.float32(eps))
    n = graph.n
    val, idx = graph.edge_value.double().cpu(), graph.edge_index.cpu()
    e = torch.tensor(eps32, dtype=torch.float64)
    lap = laplacian_f64(val, idx, n, e, loops)
    arg = val / (4.0 * e * e)
    w = torch.exp(-arg)
    normal = w >= FLT_MIN
    scale = _value_scale(val, idx, n, e, loops, lap, torch.where(normal, w, torch.zeros_like(w)) * (1.0 + arg), True)
    floor = _value_scale(val, idx, n, e, loops, lap, torch.where(normal, torch.zeros_like(w), torch.full_like(w, FLT_MIN)) * (1.0 + arg),
                         False)
    eid = graph.eid.long().cpu()
    pad = eid < 0
    vals = data.vals.double().cpu()
    # The reference divides by the PRODUCT D~_i D~_j (graph_laplacian_operator.py:73-75; D~_i^2 on a padding entry), in float32,
    # and the kernel restates it.  Without self loops D~ has no floor of 1: where a product falls below 2^-126 the reference's
    # own float32 arithmetic gives 0 / 0 (test_tangent_golden_graphs runs its underflow bandwidth with self loops only, for the
    # same reason).  There, only what is computed ahead of that division is compared: D~ and W.
    dt_ = lap["degree_unnorm"]
    defined = bool(min(float((dt_[idx[0]] * dt_[idx[1]]).min()), float((dt_ * dt_).min())) >= FLT_MIN)
    assert defined or not loops
    if not defined:
        for name, got_, ref_ in (("degree_unnorm", data.degree_unnorm, dt_), ("w", data.edge_values(0), w)):
            ratio = (got_.double().cpu() - ref_).abs() / (U * scale[name] + floor[name] / 64.0)
            assert float(ratio.max()) <= 64.0, (name, float(ratio.max()))
        return None
    assert bool((vals[pad] == 0).all()), "padding entries of the CSR must be exactly 0"
    a64 = lap["triu"] * lap["dsqrt"][idx[0]] * lap["dsqrt"][idx[1]] * e * e
    got = {name: getattr(data, name).double().cpu() for name in NAMES if name != "triu"}
    ref = {name: lap[name] for name in NAMES if name != "triu"}
    got.update(csr=vals[~pad], w=data.edge_values(0).double().cpu(), a=data.edge_values(1).double().cpu(),
               s=data.edge_values(2).double().cpu())
    ref.update(csr=lap["triu"][eid[~pad]], w=w, a=a64, s=lap["triu"])
    sc = dict(scale, csr=scale["triu"][eid[~pad]], s=scale["triu"])
    fl = dict(floor, csr=floor["triu"][eid[~pad]], s=floor["triu"])
    worst = 0.0
    for name in got:
        assert bool(torch.isfinite(got[name]).all()), name
        ratio = (got[name] - ref[name]).abs() / (U * sc[name] + fl[name] / 64.0)
        rr = float(ratio.max())
        assert rr <= 64.0, (name, rr, int(ratio.argmax()))
        worst = max(worst, rr)
    # the self edges' values are real entries: S_ii > 0 twice in the row
    se = graph.self_edge_index().cpu()
    assert bool((got["s"][se] > 0).all())
    return worst


@pytest.mark.parametrize("bw", [1.0, 0.25])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("name", sorted(co.FIXTURES))
def test_laplacian_values_and_tangent(mgp, dev, name, loops, bw):
    """mgp_laplacian_build, mgp_edge_values and mgp_laplacian_tangent against oracle.grad_ref on the same edge list: both self-loop
    settings, the fixture's bandwidth and a quarter of it.  Bound 64 for both (measured: docs/scope.md)."""
    g, graph = _graph(mgp, dev, name)
    assert graph.self_edges > 0
    eps = float(g["eps"]) * bw
    wv = _check_values(graph, eps, loops)
    if wv is None:
        assert (name, loops, bw) == ("cloud300", False, 0.25)                  # the one case float32 does not define
        print("coincident laplacian %s loops=%s x%.2f: D~_i D~_j below 2^-126, D~ and W only" % (name, loops, bw))
        return
    wt = _check_tangent(mgp, graph, eps, loops)
    print("coincident laplacian %s loops=%s x%.2f: values %.2f tangent %.2f of 64" % (name, loops, bw, wv, wt))


# ================================================================================================ 3. apply
KNOBS = [("default", None, None), ("tile_mode", "mgp_spmm_set_tile_mode", 0), ("tile_small_mode", "mgp_spmm_set_tile_small_mode", 0),
         ("tile_wide_mode", "mgp_spmm_set_tile_wide_mode", 2), ("tile_wide_mode", "mgp_spmm_set_tile_wide_mode", 0),
         ("dict_mode", "mgp_spmm_set_dict_mode", 2), ("dict_mode", "mgp_spmm_set_dict_mode", 0),
         ("mt_mode", "mgp_spmm_set_mt_mode", 0), ("v4_mode", "mgp_spmm_set_v4_mode", 0), ("v4_mode", "mgp_spmm_set_v4_mode", 2)]
COLUMNS = [1, 3, 4, 12, 16, 33, 100]


def _matmul_errors(mgp, dev, g, graph, record, label):
    """op.matmul and op.T.matmul, both normalisations, every column count, under every knob: worst error / bar.  Bar of
    test_spmm_column_counts_vs_oracle: 3e-6 max |diag| max |X|."""
    from manifold_gp_amd._lib import MgpError
    lib = mgp._lib.lib()
    n = g["n"]
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    ops = {norm: mgp.operators.GraphLaplacianOperator(graph.edge_value, graph.edge_index, n, eps, norm, True, graph=graph)
           for norm in NORMS}
    dmax = float(np.abs(co.oracle(g, "symmetric").diag).max())
    X = {C: np.random.default_rng(C).normal(size=(n, C)).astype(np.float32) for C in COLUMNS}
    worst = 0.0
    for kname, setter, value in KNOBS:
        if setter:
            getattr(lib, setter)(value)
        try:
            for C in COLUMNS:
                Xd = T(X[C], dev)
                csr = ops["symmetric"].data.csr(wide=C >= 48)
                choice = lib.mgp_spmm_kernel_choice(ctypes.byref(csr), C, 0, 0)
                for norm in NORMS:
                    L = g["dense"][(norm, True)]
                    for transposed in (False, True):
                        op = ops[norm].T if transposed else ops[norm]
                        try:
                            out = op.matmul(Xd).double().cpu().numpy()
                        except MgpError as err:          # a knob value the entry point rejects for this shape: recorded
                            record.append((label, kname, value, C, norm, transposed, "rejected %d" % err.code))
                            continue
                        ref = (L.T if transposed else L) @ X[C].astype(np.float64)
                        ratio = np.abs(out - ref).max() / (3e-6 * dmax * np.abs(X[C]).max())
                        record.append((label, kname, value, C, norm, transposed, "kernel %d ratio %.3f" % (choice, ratio)))
                        assert ratio <= 1.0, (label, kname, value, C, norm, transposed, choice, ratio)
                        worst = max(worst, ratio)
        finally:
            if setter:
                getattr(lib, setter)(1)          # every knob's default (include/mgp_hip.h); only mt_mode returns the previous value
    return worst


@pytest.mark.parametrize("name", ["cloud300", "dumbbell_dup", "coo_self"])
def test_matmul_every_kernel_vs_dense_float64(mgp, dev, name):
    """GraphLaplacianOperator.matmul / .T.matmul against the dense float64 applied matrix, through every kernel the public knobs
    select at this size (natural row order), on a locality-ordered copy of the graph (bfs_order + build_tiles) and with the
    matrix-core tile image (its size threshold lowered, as test_spmm_matrix_core_tiles lowers the fill threshold)."""
    import manifold_gp_amd.graph as graph_mod
    from manifold_gp_amd.graph import KnnGraph, bfs_order, build_tiles, chain_order
    g, graph = _graph(mgp, dev, name)
    assert graph.self_edges > 0
    record = []
    worst = _matmul_errors(mgp, dev, g, graph, record, "natural")
    n = g["n"]
    # ---- a locality-ordered copy
    g2 = KnnGraph.from_coo(graph.edge_index, graph.edge_value, n, tiles=None)
    order = bfs_order(n, g2.rowptr, g2.col)
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(n))                  # a permutation, self edges or not
    chain = chain_order(n, g2.rowptr, g2.col, g2.d2)                                   # (both walks skip col == row: harmless)
    assert np.array_equal(np.sort(chain.cpu().numpy()), np.arange(n))
    tiles = build_tiles(n, g2.rowptr, g2.col, g2.nnz, order=order)
    assert tiles is not None and tiles.get("rowid") is not None
    view = types.SimpleNamespace(n=n, rowptr=tiles["tile_rowptr"], col=g2.col.index_select(0, tiles["emap"]))
    _tile_invariants(view, tiles)                                                       # the tile view, in the caller's labels
    rowid = order.long()
    assert torch.equal(tiles["tile_rowptr"][1:] - tiles["tile_rowptr"][:-1], (g2.rowptr[1:] - g2.rowptr[:-1]).index_select(0, rowid))
    g2.tiles = tiles
    assert g2.has_locality_order() and g2.self_edges == graph.self_edges
    worst = max(worst, _matmul_errors(mgp, dev, g, g2, record, "ordered"))
    # ---- the matrix-core tile image (48 <= C <= 256)
    keep = graph_mod.MT_MIN_NODES, graph_mod.MT_MIN_FILL
    graph_mod.MT_MIN_NODES, graph_mod.MT_MIN_FILL = 0, 0.0
    try:
        g3 = KnnGraph.from_coo(graph.edge_index, graph.edge_value, n)
        w3 = _matmul_errors(mgp, dev, g, g3, record, "matrix-core")
    finally:
        graph_mod.MT_MIN_NODES, graph_mod.MT_MIN_FILL = keep
    worst = max(worst, w3)
    kernels = sorted({(r[0], r[6].split()[1]) for r in record if r[6].startswith("kernel")})
    rejected = [r for r in record if r[6].startswith("rejected")]
    print("coincident matmul %s: worst ratio %.3f; (graph, kernel) pairs run: %s; rejected: %s" % (name, worst, kernels, rejected))
    ran = {k for _, k in kernels}
    if name == "dumbbell_dup":
        assert {"0", "1", "2", "3", "5", "6"} <= ran, ran      # row groups / gather, C = 1 tiles, small-C tiles, matrix cores, both dictionaries


def test_device_matrix_is_the_applied_matrix(mgp, dev):
    """_observed_ref.device_q2 (float64 from the device's own CSR: what the operator-level checks below compare with) against
    oracle.ref_torch.dense_model_precision on the edge list, self edges in both scatters.  nu = 2: Q2 sums products of two
    entries of B = tau I + L, each held to 1e-5 (diag) / 5e-6 (S) by test_laplacian_pieces_and_matmul: 4e-5 max |Q2|."""
    from oracle.ref_torch import dense_model_precision
    for name in ("cloud300", "dumbbell_dup"):
        g, graph = _graph(mgp, dev, name)
        assert graph.self_edges > 0
        for norm in NORMS:
            desc = _precision(mgp, dev, name, norm, 2, scale=0.7)
            got = obref.device_q2(desc).toarray()
            t = lambda v: torch.tensor(float(v), dtype=torch.float64)
            want = dense_model_precision(g["edge_value"], g["edge_index"], g["n"], t(g["eps"]), t(g["kappa"]), t(np.float32(0.7)), t(0.0),
                                         2, norm, True).numpy()
            err = np.abs(got - want).max() / np.abs(want).max()
            print("device_q2 %s %s: %.2e" % (name, norm, err))
            assert err <= 4e-5, (name, norm, err)
            assert np.abs(want - _q2(g, norm, 2, float(np.float32(0.7)))).max() <= 1e-12 * np.abs(want).max()   # the two oracles agree


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", ["cloud300", "dumbbell_dup"])
def test_operator_apply_forms(mgp, dev, name, norm, nu):
    """mgp_operator_apply, forms 0 .. 3, and mgp_operator_apply_double against the dense float64 chain of device_q2.  float32: 1e-6
    of the largest entry of the product (test_precision_and_wrappers); float64: 1e-12."""
    g, graph = _graph(mgp, dev, name)
    assert graph.self_edges > 0
    n = g["n"]
    s = float(np.float32(1e-2))
    desc = _precision(mgp, dev, name, norm, nu, scale=float(np.float32(0.7)))
    Q2 = obref.device_q2(desc).toarray()
    rng = np.random.default_rng(nu)
    w32 = T(np.where(rng.random(n) < 0.3, rng.choice([1.0, 0.25], n), 0.0).astype(np.float32), dev)
    w = w32.double().cpu().numpy()
    worst = [0.0, 0.0]
    for C in (1, 4, 33):
        X = rng.normal(size=(n, C)).astype(np.float32)
        for form in (0, 1, 2, 3):
            d = desc.with_(form=form, noise=s if form else 0.0, obs_w=w32 if form == 3 else None)
            ref = _form(Q2, form, s, w) @ X.astype(np.float64)
            e32 = np.abs(d.apply(T(X, dev)).double().cpu().numpy() - ref).max() / np.abs(ref).max()
            e64 = np.abs(d.apply_f64(T(X, dev).double()).cpu().numpy() - ref).max() / np.abs(ref).max()
            assert e32 <= 1e-6 and e64 <= 1e-12, (form, C, e32, e64)
            worst = [max(worst[0], e32), max(worst[1], e64)]
    print("coincident apply %s %s nu = %d: float32 %.2e (bar 1e-6), float64 %.2e (bar 1e-12)" % (name, norm, nu, worst[0], worst[1]))


# ================================================================================================ 4. solve
def _solve_case(g, norm, nu, form, seed):
    n = g["n"]
    rng = np.random.default_rng(seed)
    scale, s = float(np.float32(0.7)), float(np.float32(1e-2))
    w = np.where(rng.random(n) < 0.3, rng.choice([1.0, 0.25], n), 0.0).astype(np.float32)
    w[g["self_nodes"][0]] = 1.0                                  # one self-edge node observed, the others as drawn
    A = _form(_q2(g, norm, nu, scale), form, s, w.astype(np.float64))
    return scale, s, w, A


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("form", [0, 2, 3])
@pytest.mark.parametrize("norm", NORMS)
def test_cg_solve_vs_dense_float64(mgp, dev, norm, form, nu):
    """mgp_cg_solve / plans on cloud300, C in {1, 5}, Jacobi on and off, the factorised and the whole-chain solve of form 0,
    against np.linalg.solve of the float64 applied matrix: 1e-4 relative (test_cg_solve_vs_dense_fp64), no warning."""
    from manifold_gp_amd.solvers import cg_solve
    g, graph = _graph(mgp, dev, "cloud300")
    assert graph.self_edges > 0
    scale, s, w, A = _solve_case(g, norm, nu, form, nu)
    desc = _precision(mgp, dev, "cloud300", norm, nu, scale).with_(form=form, noise=s if form else 0.0,
                                                                  obs_w=T(w, dev) if form == 3 else None)
    rng = np.random.default_rng(7)
    worst = 0.0
    for C in (1, 5):
        B = rng.normal(size=(g["n"], C)).astype(np.float32)
        ref = np.linalg.solve(A, B.astype(np.float64))
        for jac in (False, True):
            for factorise in ((True, False) if form == 0 and nu > 1 else (True,)):
                with warnings.catch_warnings():
                    warnings.filterwarnings("error", message=".*(CG |factorised).*")
                    X, its, res = cg_solve(desc, T(B, dev), tol=1e-6, stop_mode=1, max_iter=5000, jacobi=jac, factorise=factorise)
                err = np.abs(X.double().cpu().numpy() - ref).max() / np.abs(ref).max()
                assert err < 1e-4, (C, jac, factorise, err, its)
                worst = max(worst, err)
    print("coincident cg %s form %d nu = %d: worst %.2e (bar 1e-4)" % (norm, form, nu, worst))


@pytest.mark.parametrize("norm", NORMS)
def test_cg_folded_and_single_rank_pcg(mgp, dev, norm):
    """dumbbell_dup, nu = 2, form 2 (the posterior-mean system of smoke()): the folded step (mgp_cg_set_fold_update, a repeated
    column inside a tile row), the unfolded plan, the Jacobi-preconditioned form 3 and the single-rank pcg plan, 1e-4 against the
    dense float64 solve."""
    from manifold_gp_amd.graph import LaplacianData
    from manifold_gp_amd.parallel import PcgPlan, RowPartition, pad_graph
    from manifold_gp_amd.solvers import CgPlan
    g, graph = _graph(mgp, dev, "dumbbell_dup")
    assert graph.self_edges > 0
    n = g["n"]
    lib = mgp._lib.lib()
    y = g["train_y"].astype(np.float64)
    yd = T(g["train_y"], dev).view(-1, 1).contiguous()
    for form in (2, 3):
        scale, s, w, A = _solve_case(g, norm, 2, form, 11)
        rhs = y if form == 2 else w * y
        ref = np.linalg.solve(A, rhs)
        desc = _precision(mgp, dev, "dumbbell_dup", norm, 2, scale).with_(form=form, noise=s, obs_w=T(w, dev) if form == 3 else None)
        b = yd if form == 2 else yd * T(w, dev).view(-1, 1)
        errs = {}
        for fold_mode in ((2, 0) if form == 2 else (0,)):
            prev, prev_cx = lib.mgp_cg_set_fold_update(fold_mode), lib.mgp_cg_set_complex_shift(0)
            try:
                plan = CgPlan(desc, 1, tol=1e-6, max_iter=5000, stop_mode=1, jacobi=form == 3)
                assert plan.folded == (fold_mode == 2)
                for _ in range(3):                                # eager, then captured
                    x = plan.solve(b).clone()
                assert plan.status == 1, (form, fold_mode, plan.status, plan.iters)
                plan.close()
            finally:
                lib.mgp_cg_set_fold_update(prev)
                lib.mgp_cg_set_complex_shift(prev_cx)
            errs["fold %d" % fold_mode] = np.abs(x.view(-1).double().cpu().numpy() - ref).max() / np.abs(ref).max()
        if form == 2:
            part = RowPartition(n, 1)
            gp = pad_graph(graph, part.n_pad)
            assert gp.self_edges == graph.self_edges
            data = LaplacianData(gp, float(g["eps"]), True)
            sq = data.dsqrt if norm == "randomwalk" else None
            # (Chronopoulos-Gear: at this bandwidth the pipelined recurrence stalls above 1e-6 in float32 with or without
            # coincident points, test_pcg_stagnation_guard_and_refinement_on_an_ill_conditioned_system)
            plan = PcgPlan(desc.with_(data=data, pre=sq, post=sq), part, 0, tol=1e-6, max_iter=20000, stop_mode=1,
                           recurrence="chronopoulos-gear")
            x = plan.solve(part.pad(T(g["train_y"], dev))).clone()
            assert plan.status == 1
            plan.close()
            errs["pcg"] = np.abs(x[:n].view(-1).double().cpu().numpy() - ref).max() / np.abs(ref).max()
        print("coincident solve %s form %d: %s" % (norm, form, {k: "%.2e" % v for k, v in errs.items()}))
        assert all(v < 1e-4 for v in errs.values()), errs


# ================================================================================================ 5. quantities read from entries
def _diag_errors(mgp, dev, g, graph):
    """{stage: max |got - diag(dense)| / max |diag(dense)|} for operator.diagonal(), to_dense() and the Jacobi diagonal of forms
    0 / 2 / 3 at nu = 1, 2, on any fixture dict with the golden keys (self edges or none)."""
    n = g["n"] if "n" in g else g["train_x"].shape[0]
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    kappa = torch.tensor([[float(g["kappa"])]], device=dev)
    from oracle.laplacian import LaplacianOracle
    out = {}
    scale, s = float(np.float32(0.7)), float(np.float32(1e-2))
    rng = np.random.default_rng(5)
    w = rng.choice([0.0, 0.25, 1.0], n).astype(np.float32)
    for norm in NORMS:
        lo = LaplacianOracle(g["edge_value"], g["edge_index"], n, float(g["eps"]), norm, True, dtype=np.float64)
        L = lo.dense()
        op = mgp.operators.GraphLaplacianOperator(graph.edge_value, graph.edge_index, n, eps, norm, True, graph=graph)
        dl = np.diag(L)
        out["diagonal " + norm] = np.abs(op.diagonal().double().cpu().numpy() - dl).max() / np.abs(dl).max()
        D = op.to_dense().double().cpu().numpy()
        out["to_dense " + norm] = np.abs(D - L).max() / np.abs(dl).max()
        for nu in (1, 2):
            Q2 = scale * dense_matern_precision(L, nu, float(g["kappa"]), lo.degree if norm == "randomwalk" else None)
            desc = mgp.operators.PrecisionMaternOperator(op, nu, kappa)._descriptor().with_(scale=scale)
            for form in (0, 2, 3):
                d = desc.with_(form=form, noise=s if form else 0.0, obs_w=T(w, dev) if form == 3 else None)
                want = np.diag(_form(Q2, form, s, w.astype(np.float64)))
                got = 1.0 / d.jacobi().double().cpu().numpy()
                out["jacobi %s nu %d form %d" % (norm, nu, form)] = np.abs(got - want).max() / np.abs(want).max()
    return out


def test_entry_read_quantities(mgp, golden, dev):
    """operator.diagonal(), to_dense() and mgp_operator_jacobi (nu = 1, 2, where the header says exact) against the diagonal of
    the dense applied matrix: at most 4x the error of the same stage on the duplicate-free golden graph, measured in the same
    run (float32 round-off of a sum of k squares).  mgp_operator_diag_exact refuses; laplacian_diag is the reference's array,
    which the benchmark's CPU baseline and every restatement of the reference's product read as such, and is pinned as that."""
    from manifold_gp_amd import sampling
    from manifold_gp_amd.graph import KnnGraph
    gg = golden("dumbbell_k10_loop")
    clean = KnnGraph.from_coo(T(gg["edge_index"].astype(np.int64), dev), T(gg["edge_value"], dev), gg["train_x"].shape[0])
    assert clean.self_edges == 0
    base = _diag_errors(mgp, dev, gg, clean)
    for name in sorted(co.FIXTURES):
        g, graph = _graph(mgp, dev, name)
        assert graph.self_edges > 0
        errs = _diag_errors(mgp, dev, g, graph)
        for k in sorted(errs):
            print("coincident diagonal %-12s %-28s %.2e (duplicate-free %.2e, ratio to the bar %.2f)"
                  % (name, k, errs[k], base[k], errs[k] / (4 * base[k])))
        bad = {k: (errs[k], base[k]) for k in errs if not errs[k] <= 4 * base[k]}
        assert not bad, (name, bad)
        # laplacian_diag stays the reference's ARRAY (the `diag` of diag v - S v - S^T v, which callers that restate the
        # reference's product read): the oracle's `diag` at the bar of test_laplacian_pieces_and_matmul, and it differs
        # from the applied diagonal by 2 S_ii at the self-edge nodes and nowhere else
        op = _lap(mgp, dev, name, "symmetric")
        lo = co.oracle(g, "symmetric")
        arr = op.laplacian_diag.double().cpu().numpy()
        np.testing.assert_allclose(arr, lo.diag, rtol=1e-5, atol=2e-5)
        gap = arr - op.diagonal().double().cpu().numpy()
        nodes, s = co.self_values(g)
        want_gap = np.zeros(g["n"])
        want_gap[nodes] = 2.0 * s
        assert np.array_equal(np.flatnonzero(gap), np.sort(nodes))
        np.testing.assert_allclose(gap, want_gap, rtol=1e-5, atol=1e-6 * np.abs(lo.diag).max())
        for nu in (1, 2, 3):
            with pytest.raises(ValueError, match=REFUSAL):
                sampling.operator_diag_exact(_precision(mgp, dev, name, "symmetric", nu).with_(form=2, noise=1e-2))
    # the duplicate-free graph keeps both
    op = mgp.operators.GraphLaplacianOperator(clean.edge_value, clean.edge_index, clean.n, torch.tensor([[0.05]], device=dev),
                                              "symmetric", True, graph=clean)
    assert torch.equal(op.laplacian_diag, op.diagonal())


# ================================================================================================ 6. eigensolver
def test_eigensolver_vs_dense_eigh(mgp, dev):
    """mgp_lanczos_smallest, m = 20, on dumbbell_dup against numpy.linalg.eigh of the dense float64 L_sym: 1e-5 lambda_max
    (test_eigensolver_vs_dense_eigh_k50)."""
    from manifold_gp_amd.solvers import lanczos_smallest
    g, graph = _graph(mgp, dev, "dumbbell_dup")
    assert graph.self_edges > 0
    op = _lap(mgp, dev, "dumbbell_dup", "symmetric")
    evals, evecs, resid = lanczos_smallest(op.data, 20, tol=1e-6)
    w = np.linalg.eigvalsh(g["dense"][("symmetric", True)])
    err = np.abs(evals.cpu().numpy() - w[:20]).max() / w[-1]
    print("coincident eigensolver: worst %.2e lambda_max (bar 1e-5)" % err)
    assert err <= 1e-5
    assert float((evecs.t() @ evecs - torch.eye(20, device=dev)).abs().max()) < 5e-5


# ================================================================================================ 7. samplers, variances, fits
@pytest.mark.parametrize("norm", NORMS)
def test_samplers_refuse_or_match_the_applied_matrix(mgp, dev, norm):
    """Odd nu needs the edge factor of tau I + L_sym, the Rao-Blackwell variance the exact diagonal: both refuse.  Even nu
    draws through applies and solves alone: statistics against the inverse of the dense applied matrix, bars of
    test_sample_statistics_match_exact_covariances (6 sqrt(2 / S), S = 2048), the probes including the unit vectors of the
    self-edge nodes."""
    from manifold_gp_amd import sampling
    g, graph = _graph(mgp, dev, "cloud300")
    assert graph.self_edges > 0
    n = g["n"]
    y = T(g["train_y"], dev)
    for nu in (1, 3):
        desc = _precision(mgp, dev, "cloud300", norm, nu, 1.3)
        for fn in (lambda: sampling.precision_samples(desc, 4, 1), lambda: sampling.prior_samples(desc, 4, 1),
                   lambda: sampling.posterior_samples(desc, y, 5e-2, 4, 1), lambda: sampling.posterior_variance(desc, 5e-2, 8, 1),
                   lambda: sampling.posterior_variance(desc, 5e-2, 8, 1, method="samples"),
                   lambda: sampling.gmrf_noise(desc.data, 4, 1, edges=True)):
            with pytest.raises(ValueError, match=REFUSAL):
                fn()
    scale, s, S = float(np.float32(1.3)), 5e-2, 2048
    desc = _precision(mgp, dev, "cloud300", norm, 2, scale)
    with pytest.raises(ValueError, match=REFUSAL):
        sampling.posterior_variance(desc, s, 8, 1)                                   # Rao-Blackwell: the exact diagonal
    Q2 = _q2(g, norm, 2, scale)
    V = np.concatenate([np.random.default_rng(8).standard_normal((n, 8)), np.eye(n)[:, g["self_nodes"]]], axis=1)
    bound = 6.0 * math.sqrt(2.0 / S)
    f = sampling.prior_samples(desc, S, 17).double().cpu().numpy()
    want = np.einsum("ip,ij,jp->p", V, np.linalg.inv(Q2), V)
    got = ((f @ V) ** 2).mean(0)
    print("prior %s: worst %.3f of %.3f" % (norm, np.abs(got / want - 1.0).max(), bound))
    assert (np.abs(got / want - 1.0) < bound).all(), got / want
    z = sampling.precision_samples(desc, S, 19).double().cpu().numpy()
    wantz = np.einsum("ip,ij,jp->p", V, Q2, V)
    gotz = ((z @ V) ** 2).mean(0)
    assert (np.abs(gotz / wantz - 1.0) < bound).all(), gotz / wantz
    x = sampling.posterior_samples(desc, y, s, S, 18).double().cpu().numpy()
    cov = np.linalg.inv(Q2 + np.eye(n) / s)
    mean = sampling.posterior_mean(desc, y, s).double().cpu().numpy()
    ref_mean = np.linalg.solve(np.eye(n) + s * Q2, g["train_y"].astype(np.float64))
    assert np.abs(mean - ref_mean).max() <= 1e-4 * np.abs(ref_mean).max()
    dv = (x - mean[None, :]) @ V
    want = np.einsum("ip,ij,jp->p", V, cov, V)
    got = (dv ** 2).mean(0)
    print("posterior %s: worst %.3f of %.3f" % (norm, np.abs(got / want - 1.0).max(), bound))
    assert (np.abs(got / want - 1.0) < bound).all(), got / want
    assert (np.abs(dv.mean(0)) < 6.0 * np.sqrt(want / S)).all()
    # posterior variance in precision form, the plain estimator: every node against the dense diagonal
    var, se = sampling.posterior_variance(desc, s, S, 23, method="samples")
    var = var.cpu().numpy()
    print("variance %s: worst node %.3f of %.3f" % (norm, np.abs(var / np.diag(cov) - 1.0).max(), bound))
    assert (np.abs(var / np.diag(cov) - 1.0) < bound).all()


def _scaled(mgp, dev, g, norm, nu):
    """(descriptor, float64 Q2) scaled to a prior marginal variance of about 9, as the fits' own tests scale theirs; the dense
    matrix is the oracle's, not the device's."""
    Q1 = _q2(g, norm, nu, 1.0)
    scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
    return _precision(mgp, dev, "dumbbell_dup", norm, nu, scale), scale * Q1


@pytest.mark.parametrize("norm,nu", [("symmetric", 2), ("randomwalk", 1)])
def test_laplace_fits_on_coincident_points(mgp, dev, norm, nu):
    """laplace_fit, laplace_fit_counts (Poisson) and laplace_fit_ordinal on dumbbell_dup: they apply and solve only, so the mode
    is within 1e-4 of the dense float64 Newton iteration on the applied matrix (the bar of each fit's own test).  What they hand
    to the samplers (latent_variance, predict_proba(S)) refuses, by the Rao-Blackwell default at every nu."""
    from manifold_gp_amd.classification import laplace_fit
    from manifold_gp_amd.counts import laplace_fit_counts
    from manifold_gp_amd.ordinal import laplace_fit_ordinal
    g, graph = _graph(mgp, dev, "dumbbell_dup")
    assert graph.self_edges > 0
    desc, Q = _scaled(mgp, dev, g, norm, nu)
    nan = lambda a, obs: T(np.where(obs, a, np.nan).astype(np.float32), dev)
    fits = {}
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        t, obs, y = lref.labels(g)
        fits["bernoulli"] = (laplace_fit(desc, T(y, dev), T(obs, dev), rtol=1e-5), lref.newton(Q, t, obs)[0])
        c = cref.counts(g)
        d = cref.poisson_data(c)
        fits["poisson"] = (laplace_fit_counts(desc, nan(d["y"], c["obs"]), T(c["obs"], dev), family="poisson", exposure=T(c["E"], dev)),
                           cref.newton(Q, d)[0])
        yo, oo = ordref.labels(g, 4)
        cuts = ordref.cutpoints(yo, 4, oo)
        lo, hi = ordref.intervals(yo, cuts)
        fits["ordinal"] = (laplace_fit_ordinal(desc, nan(yo, oo), 4, T(cuts, dev), T(oo, dev), rtol=1e-5), ordref.newton(Q, lo, hi, oo)[0])
    for kind, (fit, f_ref) in fits.items():
        err = np.abs(fit.mean.double().cpu().numpy() - f_ref).max()
        print("coincident %s fit %s nu = %d: %d steps, max |f - f_ref| = %.2e" % (kind, norm, nu, fit.iterations, err))
        assert fit.converged and err <= 1e-4, (kind, err)
        with pytest.raises(ValueError, match=REFUSAL):
            fit.latent_variance(8, seed=1)
    with pytest.raises(ValueError, match=REFUSAL):
        fits["bernoulli"][0].predict_proba(8, seed=1)
    with pytest.raises(ValueError, match=REFUSAL):
        fits["ordinal"][0].predict_proba(8, seed=1)
    with pytest.raises(ValueError, match=REFUSAL):
        fits["poisson"][0].predict_mean(8, seed=1)


# ================================================================================================ 8. out of sample
@pytest.mark.parametrize("norm", NORMS)
def test_features_at_training_points(mgp, dev, norm):
    """RiemannMaternKernel.features at test points that ARE training points (distance 0 to a neighbour, two of them for a copy)
    against oracle.spectral in float64.  Bars of test_kernel_eval_features_oos against its float64 goldens at the default
    eigensolver tolerance: eigenvalues 1e-7 (of 2 max diag), Gram and out-of-sample Gram 1e-4 of their largest entry."""
    from oracle import spectral
    g, graph = _graph(mgp, dev, "dumbbell_dup")
    assert graph.self_edges > 0
    n, k, eps, kappa = g["n"], int(g["k"]), float(g["eps"]), float(g["kappa"])
    lo = co.oracle(g, norm)
    w_all = np.linalg.eigvalsh(g["dense"][("symmetric", True)])
    m = 20 + int(np.argmax(np.diff(w_all[19:51])))                      # the widest gap behind a block of 20 .. 50 modes
    kern = mgp.kernels.RiemannMaternKernel(nu=1, x=T(g["train_x"], dev), nearest_neighbors=k, laplacian_normalization=norm,
                                           num_modes=m, bump_scale=1.0, bump_decay=0.01).to(dev)
    kern.initialize(graphbandwidth=eps, lengthscale=kappa)
    kern.eval()
    assert kern.knn.knn_graph.self_edges == graph.self_edges > 0
    assert np.array_equal(kern.edge_index.cpu().numpy(), g["edge_index"])
    ev, U = spectral.eval_eigenpairs(lo, m, np.float64)
    lam_max = 2.0 * float(np.abs(lo.diag).max())
    e_val = np.abs(kern.eigval.cpu().numpy()[1:] - ev[1:]).max() / lam_max
    Z64 = spectral.features_insample(ev, U, 1, kappa)
    pick = np.array(sorted(set(co.DUP_DST) | set(co.DUP_SRC) | {10, 500, 1234}))
    xt = g["train_x"][pick]
    Dt, It = oknn.knn_search(g["train_x"], xt, k)
    assert (Dt[:, 0] == 0).all() and (Dt[np.isin(pick, co.DUP_DST), 1] == 0).all()
    Zt64 = spectral.features_oos(lo, ev, U, 1, kappa, Dt.astype(np.float64), It, 1.0, 0.01)
    Z = kern.features(T(g["train_x"], dev)).double().cpu().numpy()
    Zt = kern.features(T(xt, dev)).double().cpu().numpy()
    r64, o64 = Z64[:64] @ Z64[:64].T, Zt64 @ Z64[:64].T
    e_gram = np.abs(Z[:64] @ Z[:64].T - r64).max() / np.abs(r64).max()
    e_oos = np.abs(Zt @ Z[:64].T - o64).max() / np.abs(o64).max()
    print("coincident features %s (m = %d): eigenvalues %.2e, Gram %.2e, out of sample %.2e" % (norm, m, e_val, e_gram, e_oos))
    assert e_val < 1e-7 and e_gram < 1e-4 and e_oos < 1e-4, (e_val, e_gram, e_oos)
