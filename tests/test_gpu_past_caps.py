"""The fused multi-column SpMM past its grid caps (csrc/spmm.hip), against float64.

A 300,071-node swiss roll (tests/_past_caps.py), k = 10, in two row orders: along a Z-curve (tiles in natural row order; the
CSR can carry the matrix-core image) and in generation order (the tile builder picks a locality order: tiles["rowid"], no
image).  At this size
  - tile_grid gives every workgroup of the tile families TWO tiles (4689 tiles of 64 rows > 4096 workgroups; the last workgroup
    holds one tile, of 39 rows) and the workgroup writes one dot partial for both;
  - make_plan widens the gather kernels' row range to several passes (2 of 64 rows at C = 4 ... 16, 3 of 32 at C = 20, 5 of 16
    from 33 columns up, 3 of 32 for the C = 1 row groups);
  - the 100-column X block is 120 MB: rules 4 and 5 of spmm_plan (lanes-over-columns dictionary, chunked dictionary) are taken by
    DEFAULT through `big_x`, with no lab switch set;
  - the matrix-core kernel writes 9,378 rows of dot partials.
Every cell asserts the family that ran (mgp_spmm_kernel_choice) and that its partial count is past the cap
(mgp_spmm_dot_blocks_csr), never n alone.

Measured ratios (error / bound, 1 is the limit): the test's docstring and docs/kernels/spmm.md, "Past the caps".  One-off cost of
the module: 0.4 s for the two graphs, 0.7 s for the Laplacian data and the two scipy matrices (module-scoped fixture); the 20 cases take 3 s together.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _past_caps import MAX_GRID, N, gather_plan, rows_per_pass, swiss300k

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
COLS = [1, 4, 5, 8, 9, 12, 16, 20, 33, 100]
A_COEF, B_COEF, CB, CO = 1.25, 1.0, 0.5, 2.0
# the lab switches of include/mgp_hip.h that pick the family, with their defaults
DEFAULTS = {"tile": 1, "v4": 1, "dict": 1, "tile_wide": 1}


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


@pytest.fixture(scope="module")
def rolls(mgp, dev):
    """Both row orders: the graph, its Laplacian data and the float64 scipy CSR of the device's own fp32 values."""
    from manifold_gp_amd.graph import LaplacianData
    out = {}
    for order in ("morton", "random"):
        g = swiss300k(mgp, dev, order)
        graph = g["graph"]
        data = LaplacianData(graph, g["eps"], True)
        S = sp.csr_matrix((data.vals.double().cpu().numpy(), graph.col.cpu().numpy().astype(np.int64),
                           graph.rowptr.cpu().numpy().astype(np.int64)), shape=(N, N))
        # `wide`: Laplacian data of its own for the one cell that builds the matrix-core image -- an image, once built, rides in
        # every struct of its data object, and the production cells must stay without one whatever order the tests run in
        wide = LaplacianData(graph, g["eps"], True) if order == "morton" else None
        out[order] = dict(graph=graph, data=data, wide=wide, S=S, diag=data.diag.double().cpu().numpy()[:, None])
    return out


def _cdiv(a, b):
    return -(-a // b)


def _set(lib, switches):
    s = dict(DEFAULTS, **switches)
    lib.mgp_spmm_set_tile_mode(s["tile"])
    lib.mgp_spmm_set_v4_mode(s["v4"])
    lib.mgp_spmm_set_dict_mode(s["dict"])
    lib.mgp_spmm_set_tile_wide_mode(s["tile_wide"])


def _cells(order, C):
    """(name, switches, wide CSR, expected family): production's own choice first, then the forced families."""
    prod = 1 if C == 1 else 2 if C in (4, 8, 12, 16) else 5 if C == 100 else 0
    cells = [("production", {}, False, prod)]
    if order == "random":
        cells.append(("gather", {"tile": 0, "v4": 2}, False, 0))               # C = 20, 100: the float4 member
        if C in (20, 100):
            cells.append(("gather per column", {"tile": 0, "v4": 0}, False, 0))
        if C == 20:
            cells.append(("dictionary forced", {"dict": 2}, False, 5))
            cells.append(("chunked dictionary forced", {"dict": 0, "tile_wide": 2}, False, 6))
        if C == 100:
            cells.append(("dictionary off", {"dict": 0}, False, 6))              # rule 5 by default, through big_x
    elif C == 100:
        cells.append(("matrix cores", {}, True, 3))
    return cells


def _mask_sets(graph, C, rng):
    """Row sets on which a masked dot weight lives: (name, rows).  Tile positions are mapped through the tiles' row order where
    there is one, and kept in natural order too (the gather kernels' ranges)."""
    n, tr = graph.n, graph.tiles["rows"]
    rowid = graph.tiles.get("rowid")
    ntiles = -(-n // tr)
    mid = (ntiles // 2) | 1                                  # an odd tile: the second of a two-tile workgroup
    pos = [("first row", np.array([0])), ("last row", np.array([n - 1])),
           ("ragged last tile", np.arange(n - n % tr, n)),
           ("second tile of a workgroup", np.arange(mid * tr, (mid + 1) * tr)),
           ("around row 64 x 4096", np.arange(64 * MAX_GRID - 64, 64 * MAX_GRID + 64)),
           ("200 random rows", np.sort(rng.choice(n, 200, replace=False)))]
    # the second pass of a mid-range gather workgroup (make_plan's row ranges, natural order), for the multi-column gather
    # kernels and for the C = 1 row groups
    rpp = rows_per_pass(C, graph.spmv_lanes)
    grid, rpb = gather_plan(n, rpp)
    w = grid // 2
    if rpb > rpp:
        pos.append(("second pass of a gather workgroup", np.arange(w * rpb + rpp, min(w * rpb + 2 * rpp, (w + 1) * rpb))))
    else:
        pos.append(("one gather workgroup", np.arange(w * rpb, (w + 1) * rpb)))
    assert n % tr != 0 and len(pos[2][1]) == n % tr
    sets = list(pos)
    if rowid is not None:
        ids = rowid.long().cpu().numpy()
        sets += [(name + " (tile order)", np.sort(ids[p])) for name, p in pos[:5]]
    return sets


@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("order", ["morton", "random"])
def test_spmm_fused_past_the_grid_caps(mgp, dev, rolls, order, C):
    """mgp_spmm_fused at n = 300,071 with every epilogue operand in play (a, b, pre, post, base and its coefficient, weighted dot
    partials), outputs and partials prefilled with NaN, against a float64 scipy CSR product of the device's fp32 values.

    1. Y entrywise within 2e-5 max|ref| (the bar of the small-n SpMM tests), no NaN.
    2. dot partials, a weight on all rows: their sum within 2e-4 scale sqrt(n).
    3. dot partials, a weight on a row set S and exactly zero elsewhere (a global dot cannot see one lost tile): S = row 0, row
       n - 1, the ragged last tile, the second tile of a two-tile workgroup, the rows around 64 x 4096, the second pass of a
       mid-range gather workgroup, 200 random rows.  Bound (derived: adding exact zeros is exact):
         sum_S |W| 2e-5 scale  +  64 x 2^-24 sum_S |W ref|
       -- the entrywise bound on Y, plus float32 summation of partials of at most 64 rows.
    4. the family that ran, and a partial count past the cap.
    Measured worst ratios error / bound over the 36 cells: Y 0.009 (C = 9 and 12), all-rows dot 3e-4 (C = 100, dictionary kernel),
    masked dots 0.003 (C = 16 and 100, locality-ordered tiles): the float32 grouping term of the bound was never the tight one,
    no family needed the measured-gap fallback.  A lost row moves a masked dot by about 300 times its bound."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    G = rolls[order]
    graph, data = G["graph"], G["data"]
    n, tr = N, graph.tiles["rows"]
    print("%s: tile rows %d, locality order %s, reuse %.2f, widest dictionary %d, longest tile %d entries, row-group lanes %d" % (
        order, tr, graph.tiles.get("rowid") is not None, graph.tiles["reuse"], graph.tiles["max_cols"], graph.tiles["max_entries"],
        graph.spmv_lanes))
    assert graph.n == n and tr == 64, "the tile builder is expected to keep 64-row tiles on this graph"
    ntiles = -(-n // tr)
    assert ntiles > MAX_GRID and ntiles % 2 == 1 and n % 64 == 39 and n % 16 == 7
    assert (graph.tiles.get("rowid") is not None) == (order == "random")
    gen = torch.Generator(device=dev).manual_seed(1000 + C)
    X = torch.randn(n, C, device=dev, generator=gen)
    pre = torch.rand(n, device=dev, generator=gen) + 0.5
    post = torch.rand(n, device=dev, generator=gen) + 0.5
    base = torch.randn(n, C, device=dev, generator=gen)
    W = torch.randn(n, C, device=dev, generator=gen)
    # float64 reference on the host, kept on the device for the comparisons (plain torch, no library kernel)
    Xs = pre.double().cpu().numpy()[:, None] * X.double().cpu().numpy()
    ref = CB * base.double().cpu().numpy() + CO * post.double().cpu().numpy()[:, None] * (
        A_COEF * Xs + B_COEF * (G["diag"] * Xs - G["S"] @ Xs))
    del Xs
    ref_d = torch.from_numpy(ref).to(dev)
    del ref
    scale = float(ref_d.abs().max())
    dref = (W.double() * ref_d).sum(0)
    sets = _mask_sets(graph, C, np.random.default_rng(C))
    worst = {"y": 0.0, "dot": 0.0, "masked": 0.0}
    try:
        for name, switches, wide, family in _cells(order, C):
            _set(lib, switches)
            csr = G["wide"].csr(wide=True) if wide else data.csr()
            assert bool(csr.mt_img) == wide, (order, C, name)     # only the matrix-core cell carries an image
            where = (order, C, name)
            assert lib.mgp_spmm_kernel_choice(ctypes.byref(csr), C, 1, 0) == family, where
            nb = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(csr), C)
            # ---- 4. the path past the cap ran
            if family in (1, 2, 6):
                assert nb == -(-ntiles // 2) and nb < ntiles, (where, nb)      # two tiles per workgroup
            elif family == 5:
                assert nb == MAX_GRID and nb < ntiles, (where, nb)             # a workgroup walks one or two tiles
            elif family == 3:
                # four (16-row tile, 64-column block) waves per workgroup, one row of partials each: past 4096
                assert nb == _cdiv(_cdiv(n, 16) * _cdiv(C, 64), 4) and nb > MAX_GRID, (where, nb)
            else:
                rpp = rows_per_pass(C, graph.spmv_lanes)
                grid, rpb = gather_plan(n, rpp)
                assert nb == grid, (where, nb, grid)
                if -(-n // rpp) > MAX_GRID:
                    assert rpb > rpp and nb < -(-n // rpp), (where, nb)       # several passes per workgroup
                else:
                    assert C == 5 and rpb == rpp == 128, where                # (128 rows per pass: 2,345 one-pass workgroups)
            Y = torch.full((n, C), float("nan"), device=dev)
            part = torch.full((nb, C), float("nan"), device=dev)

            def launch(w, p):
                _lib.check(lib.mgp_spmm_fused(ctypes.byref(csr), _lib.ptr(X), C, _lib.ptr(Y), A_COEF, B_COEF, _lib.ptr(pre),
                                              _lib.ptr(post), _lib.ptr(base), CB, CO, _lib.ptr(w), _lib.ptr(p), _lib.stream()),
                           "mgp_spmm_fused")
            launch(W, part)
            # ---- 1. Y entrywise
            assert not bool(torch.isnan(Y).any()), where
            ey = float((Y.double() - ref_d).abs().max()) / (2e-5 * scale)
            # ---- 2. all-rows dot
            assert not bool(torch.isnan(part).any()), where
            ed = float((part.double().sum(0) - dref).abs().max()) / (2e-4 * scale * n ** 0.5)
            print("%s C=%d %-26s family %d partials %5d: Y %.3f of the bound, dot %.4f" % (order, C, name, family, nb, ey, ed))
            assert ey < 1.0, (where, ey)
            assert ed < 1.0, (where, ed)
            worst["y"], worst["dot"] = max(worst["y"], ey), max(worst["dot"], ed)
            # ---- 3. masked dots
            for sname, rows in sets:
                r = torch.from_numpy(rows).to(dev)
                Wm = torch.zeros_like(W)
                Wm[r] = W[r]
                part.fill_(float("nan"))
                Y.fill_(float("nan"))
                launch(Wm, part)
                assert not bool(torch.isnan(part).any()), (where, sname)
                w64, r64 = W[r].double(), ref_d[r]
                d64 = (w64 * r64).sum(0)
                bound = w64.abs().sum(0) * (2e-5 * scale) + 64 * U * (w64 * r64).abs().sum(0)
                em = float(((part.double().sum(0) - d64).abs() / bound).max())
                assert em <= 1.0, (where, sname, em)
                worst["masked"] = max(worst["masked"], em)
    finally:
        _set(lib, {})
    print("%s C=%d worst ratios: Y %.3f, dot %.4f, masked dot %.3f" % (order, C, worst["y"], worst["dot"], worst["masked"]))
