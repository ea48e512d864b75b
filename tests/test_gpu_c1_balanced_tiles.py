"""GPU tests of the single-column tile kernels on the entry-balanced tile set (docs/kernels/spmm.md, round 8).

A graph whose fixed 64-row tiles include one over 4096 padded entries carries a second tile set, cut by entries (graph.py
c1_balanced_tiles), and spmv_tile_kernel / spmv_tile_cgstep_kernel run on it.  Row sums do not depend on the tiling (quad, then
stride-4 lanes, then xor tree), so with the switch graph.C1_BALANCED on and off

  * every product is compared BIT FOR BIT (plain, pre-scaled, with post / base / weighted dot), and nothing outside the n rows is
    written although the kernel walks 64 T >= n positions;
  * the dot partials, grouped by tile, are T instead of ceil(n / 64) and are held to the float64 sum of w_i y_i of the product that
    was written.  Bound: a lane holds one row's term (one rounding), the wave sum adds six levels, the workgroup three more and the
    product w_i y_i one: 11 roundings on terms of one sign-free magnitude sum, so |sum(partials) - ref| <= 16 eps32 sum |w_i y_i|
    (the partials themselves are summed in float64).

The folded CG plan on the balanced set (self-dot kernel, step kernel, deciding step kernel) is held to the solver contract of
tests/test_gpu_solver_contract.py and to the bit-for-bit identities of tests/test_gpu_cg_fold.py: decide_in_update 0 == 1, graph
replay == eager, alternating right-hand-side addresses, b = 0 with NaNs planted in x / p / s, the max_iter exit, a rebound plan ==
a fresh one.  The second set of partials of the first launch (||b||^2) and the copy of x have no public entry of their own: the
plans run them (the self-dot kernel writes both), and the contract holds their results.

Graphs (all small, all with a heavy 64-row tile):
  knn1500  random points, n = 1500, d = 8, k = 72: 24 fixed tiles, every one over the cap; about 40 balanced tiles of 30 to 45 rows,
           the last one partial;
  knn400   the same at n = 400: ten balanced tiles;
  knn256   the same at n = 256: fewer than eight balanced tiles (the hand-off's group count; n = 400 has ten);
  star     node 0 linked to 5000 nodes, every node to its eight successors on a ring: row 0 is a tile of its own over the cap
           (the loop behind the barrier still serves it), 5120 nodes: 80 fixed tiles, 81 balanced ones."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_solver_contract import R1, T, _check_plan, _desc, dev, mgp  # noqa: F401
from test_gpu_cg_fold import _is_folded, _records, _same, fold
from test_gpu_tile_head import _plan_records

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
CAP = 4096


class balanced:
    """with balanced(True / False): CSRs built inside carry / leave out the balanced set (graph.C1_BALANCED)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from manifold_gp_amd import graph
        self.prev = graph.C1_BALANCED[0]
        graph.C1_BALANCED[0] = bool(self.on)

    def __exit__(self, *exc):
        from manifold_gp_amd import graph
        graph.C1_BALANCED[0] = self.prev


def _knn(mgp, dev, n):
    gen = torch.Generator().manual_seed(100 + n)
    x = (0.25 * torch.randn(n, 8, generator=gen)).to(dev)            # squared neighbour distances of about 0.5
    knn = mgp.utils.NearestNeighbors(x)
    idx, val = knn.graph(72)
    laps = {norm: mgp.operators.GraphLaplacianOperator(val, idx, n, torch.tensor([[1.0]], device=dev), norm, graph=knn.knn_graph)
            for norm in ("randomwalk", "symmetric")}
    return dict(n=n, kappa=1.0, graph=knn.knn_graph, **laps)


def _star(mgp, dev):
    n, hub = 5120, 5000
    rng = np.random.default_rng(5)
    pairs = {(0, j) for j in range(1, hub + 1)}
    for i in range(n):
        for s in range(1, 9):
            j = (i + s) % n
            pairs.add((min(i, j), max(i, j)))
    pairs = np.asarray(sorted(pairs), np.int64)
    val = (rng.random(len(pairs)) * 0.05 + 0.01).astype(np.float32)
    laps = {norm: mgp.operators.GraphLaplacianOperator(T(val, dev), T(pairs.T.copy(), dev), n, torch.tensor([[0.2]], device=dev), norm, True)
            for norm in ("randomwalk", "symmetric")}
    return dict(n=n, kappa=1.0, graph=laps["randomwalk"].data.graph, **laps)


@pytest.fixture(scope="module")
def graphs(mgp, dev):
    out = {"knn1500": _knn(mgp, dev, 1500), "knn400": _knn(mgp, dev, 400), "knn256": _knn(mgp, dev, 256), "star": _star(mgp, dev)}
    for name, G in out.items():
        gen = torch.Generator().manual_seed(7)
        G["y"] = torch.randn(G["n"], 1, generator=gen).to(dev)
        G["y2"] = (torch.rand(G["n"], 1, generator=gen) - 0.3).to(dev)
    return out


def _set(G):
    t = G["graph"].tiles
    assert t is not None and t.get("rowid") is None and t["rows"] == 64, "the graph keeps its natural row order"
    assert t.get("c1") is not None, "the policy builds the balanced set on this graph"
    return t, t["c1"]


@pytest.mark.parametrize("name", ["knn1500", "knn400", "knn256", "star"])
def test_the_set(mgp, graphs, name):
    """What the builder left: the cut is the CPU-tested one on this graph's rowptr, no tile over the cap but a single row, the
    dictionaries and ids reproduce the columns entry by entry, and the shift words stand behind the offsets."""
    from manifold_gp_amd import graph as gmod
    G = graphs[name]
    n, g = G["n"], G["graph"]
    t, c1 = _set(G)
    rp = g.rowptr.cpu().long()
    fixed = rp[torch.clamp(torch.arange(-(-n // 64) + 1) * 64, max=n)]
    assert int((fixed[1:] - fixed[:-1]).max()) > CAP
    first, Tn = c1["first"], c1["T"]
    assert torch.equal(first, gmod.c1_balanced_cut(rp)) and first.numel() == Tn + 1
    e, h = rp[first[1:]] - rp[first[:-1]], first[1:] - first[:-1]
    assert bool(((e <= CAP) | (h == 1)).all()) and c1["max_entries"] == int(e.max())
    if name == "star":
        assert int(h[0]) == 1 and int(e[0]) > CAP                                    # the hub: a tile of its own, over the cap
    if name == "knn256":
        assert Tn < 8
    if name == "knn1500":
        assert 24 < Tn <= 48 and int(h.max()) < 64 and int(h[-1]) < int(h[:-1].min())
    pad, shift = gmod.c1_padded_positions(rp, first)
    assert torch.equal(c1["rowptr_pad"].cpu().long(), pad) and torch.equal(c1["tile_shift"].cpu().long(), shift)
    assert c1["tile_shift"].data_ptr() == c1["rowptr_pad"].data_ptr() + 4 * (64 * Tn + 1)
    tp, tc, lid, col = c1["tile_ptr"].cpu().long(), c1["tile_cols"].cpu().long(), c1["lid"].cpu().long() & 0xffff, g.col.cpu().long()
    assert c1["max_cols"] == int((tp[1:] - tp[:-1]).max())
    tile_of_entry = torch.repeat_interleave(torch.arange(Tn), e)
    assert torch.equal(tc[tp[tile_of_entry] + lid], col)
    print("balanced set %s: n %d, fixed tiles %d (max %d entries), balanced %d (max %d entries, %d columns), heights %d..%d"
          % (name, n, fixed.numel() - 1, int((fixed[1:] - fixed[:-1]).max()), Tn, c1["max_entries"], c1["max_cols"], int(h.min()), int(h.max())))


def _products(csr, n, dev, seed=3):
    """mgp_spmm_fused with every operand (pre, post, base, weighted dot), without pre, and bare.  The vectors stand in the middle of
    a canary block: nothing outside the n rows may be written."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(seed)
    x, base, w = (torch.randn(n, 1, generator=gen).to(dev) for _ in range(3))
    pre = (torch.rand(n, generator=gen) + 0.5).to(dev)
    assert lib.mgp_spmm_kernel_choice(ctypes.byref(csr), 1, 1, 0) == 1
    nb = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(csr), 1)
    out = []
    for p, dots in ((pre, True), (None, True), (None, False)):
        block = torch.full((n + 256, 1), 7.0, device=dev)
        y = block[128:128 + n]
        part = torch.full((nb + 64,), 7.0, device=dev)
        if dots:
            _lib.check(lib.mgp_spmm_fused(ctypes.byref(csr), _lib.ptr(x), 1, _lib.ptr(y), 1.25, 0.75, _lib.ptr(p), _lib.ptr(pre),
                                          _lib.ptr(base), 0.5, 2.0, _lib.ptr(w), _lib.ptr(part), _lib.stream()), "mgp_spmm_fused")
        else:
            _lib.check(lib.mgp_spmm_fused(ctypes.byref(csr), _lib.ptr(x), 1, _lib.ptr(y), 0.0, 1.0, None, None, None, 0.0, 1.0,
                                          None, None, _lib.stream()), "mgp_spmm_fused")
        torch.cuda.synchronize()
        assert bool((block[:128] == 7.0).all()) and bool((block[128 + n:] == 7.0).all()), "a store outside the n rows"
        assert bool((part[nb:] == 7.0).all()) and (not dots or not bool((part[:nb] == 7.0).any())), "partials: as many as the count says"
        out.append((y.clone(), part[:nb].clone() if dots else None))
    return out, nb, w


@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
@pytest.mark.parametrize("name", ["knn1500", "knn400", "knn256", "star"])
def test_products_on_against_off(mgp, graphs, dev, name, norm):
    G = graphs[name]
    n, lap = G["n"], G[norm]
    _, c1 = _set(G)
    with balanced(True):
        on, nb_on, w = _products(lap.data.csr(), n, dev)
    with balanced(False):
        off, nb_off, _ = _products(lap.data.csr(), n, dev)
    assert nb_on == c1["T"] and nb_off == -(-n // 64) and nb_on != nb_off          # one partial per tile of the set that ran
    for k, ((ya, pa), (yb, pb)) in enumerate(zip(on, off)):
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), (name, norm, "product", k)
        assert bool(torch.isfinite(ya).all()) and float(ya.abs().max()) > 0
        if pa is not None:
            terms = w.double() * ya.double()
            ref, bound = float(terms.sum()), 16 * EPS32 * float(terms.abs().sum())
            for what, p in (("balanced", pa), ("64-row", pb)):
                err = abs(float(p.double().sum()) - ref)
                print("dot partials %s %s %s product %d: |sum - ref| %.3g, bound %.3g" % (name, norm, what, k, err, bound))
                assert err <= bound, (name, norm, what, k, err, bound)


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
@pytest.mark.parametrize("name", ["knn1500", "knn400", "knn256", "star"])
def test_folded_plan_contract(mgp, graphs, dev, name, norm, form):
    """C1-C5 of the solver contract for the folded plan on the balanced set, both decision forms, and the max_iter exit."""
    from manifold_gp_amd import _lib
    G = graphs[name]
    lap = G[norm]
    _, c1 = _set(G)
    desc = _desc(mgp, lap, 2, G["kappa"], dev, form=form)
    sys = R1(lap, desc)
    assert _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(lap.data.csr()), 1) == c1["T"]
    for decide in (1, 0):
        with fold(1, complex_shift=0, decide=decide):
            assert _is_folded(desc)
            _check_plan(sys, desc, G["y"], 1e-3, label="balanced %s %s form %d decide %d" % (name, norm, form, decide))
            # the max_iter exit: form 0 is still at 8e-3 after two steps; form 2 is near the identity (1e-4 after ONE step), so it
            # is capped at one step under a tolerance it has not reached by then
            cap_tol, cap_it = (1e-3, 2) if form == 0 else (1e-5, 1)
            _check_plan(sys, desc, G["y"], cap_tol, max_iter=cap_it, repeats=2, label="balanced capped %s decide %d" % (name, decide))


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("name", ["knn1500", "knn400", "knn256", "star"])
def test_folded_plan_bit_for_bit(mgp, graphs, dev, name, form):
    """decide_in_update 0 == 1 in everything a solve reports; graph replay == eager in solution, iterations, status and residual
    (`applies` differs by design); right-hand sides at alternating addresses; b = 0 with NaNs planted in x / p / s; the max_iter
    exit; a rebound plan == a fresh one."""
    from manifold_gp_amd.solvers import CgPlan
    G = graphs[name]
    lap, n = G["randomwalk"], G["n"]
    _, c1 = _set(G)
    desc = _desc(mgp, lap, 2, G["kappa"], dev, form=form)
    y, y2 = G["y"], G["y2"]
    yc = y.clone()
    seq = [y, y, yc, y2, y, yc, y2]
    out = {}
    with fold(1, complex_shift=0):
        for decide in (1, 0):
            with fold(1, decide=decide):
                for use_graph in (True, False):
                    recs, folded = _records(desc, seq, use_graph=use_graph)
                    assert folded
                    capped, _ = _records(desc, [y, y, y2], tol=1e-12, max_iter=2, use_graph=use_graph)
                    out[(decide, use_graph)] = recs + capped
        _same(out[(1, True)], out[(0, True)], "decide_in_update 1 against 0")
        _same(out[(1, False)], out[(0, False)], "decide_in_update 1 against 0, eager")
        for decide in (1, 0):
            for k, (ra, rb) in enumerate(zip(out[(decide, True)], out[(decide, False)])):
                assert ra[1:4] == rb[1:4] and torch.equal(ra[0], rb[0]), (name, form, decide, k, ra[1:], rb[1:])
        for x, its, st, _, _ in out[(1, True)][:len(seq)]:
            assert st == 1 and its > 0 and bool(torch.isfinite(x).all())
        for x, its, st, _, _ in out[(1, True)][len(seq):]:
            assert st == 2 and its == 2
        # b = 0 with NaNs planted in the plan's x, p and s, between two ordinary solves (tests/test_gpu_tile_head.py _plan_records)
        for use_graph in (True, False):
            for decide in (1, 0):
                recs = _plan_records(desc, [y, y, None, y], n, use_graph, decide)
                x0, rep0 = recs[2][0], recs[2][1]
                assert rep0[0] == 0 and rep0[1] == 1 and float(x0.abs().max()) == 0.0 and rep0[2][0] == 0.0, rep0
                assert recs[2][2].numel() == 2 * c1["T"]                       # the plan's partials: one per balanced tile
                ref = out[(decide, use_graph)][0]
                for k in (0, 1, 3):
                    assert recs[k][1][:3] == (ref[1], ref[2], ref[3]) and torch.equal(recs[k][0], ref[0]), (use_graph, decide, k)
        # a rebound plan against a fresh one
        desc2 = _desc(mgp, lap, 2, 1.25 * G["kappa"], dev, form=form, scale=0.9)
        plan = CgPlan(desc, 1, tol=1e-6, max_iter=20000, stop_mode=1, check_every=8)
        try:
            for rhs in (y, y, y2):
                plan.solve(rhs)
            assert plan.rebind(desc2) and plan.folded
            reb = []
            for rhs in (y, y2, y, y):
                x = plan.solve(rhs).clone()
                reb.append((x, plan.iters, plan.status, tuple(plan.resid)))
        finally:
            plan.close()
        fresh, _ = _records(desc2, [y, y2, y, y])
        for k, (ra, rb) in enumerate(zip(reb, fresh)):
            assert ra[1:4] == rb[1:4] and torch.equal(ra[0], rb[0]), ("rebound", k, ra[1:], rb[1:4])


@pytest.mark.parametrize("name", ["knn1500", "star"])
def test_switch_off_is_the_64_row_plan(mgp, graphs, dev, name):
    """Switch off: ceil(n / 64) partials, and the solves of a plan equal, bit for bit, those of a plan on a CSR that never carried
    the set (the 64-row tiles alone); switch on, three steps: the solution within round 6's bound of it."""
    from manifold_gp_amd import _lib
    G = graphs[name]
    lap, n = G["randomwalk"], G["n"]
    t, c1 = _set(G)
    desc = _desc(mgp, lap, 2, G["kappa"], dev, form=2)
    seq = [G["y"], G["y"], G["y2"]]
    with fold(1, complex_shift=0):
        with balanced(False):
            assert _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(lap.data.csr()), 1) == -(-n // 64)
            off, folded = _records(desc, seq)
            assert folded
        bare = {k: v for k, v in t.items() if k != "c1"}
        G["graph"].tiles = bare
        try:
            with balanced(True):
                assert _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(lap.data.csr()), 1) == -(-n // 64)
                never, _ = _records(desc, seq)
        finally:
            G["graph"].tiles = t
        _same(off, never, "switch off against a graph without the set")
        # three steps on either set (the benchmark's solve length): alpha and beta differ in their last bits only, because the dot
        # partials are grouped by other tiles.  Ten roundings or so per step in the coefficients, three steps: 30 eps32 = 3.6e-6
        # of max |x|, which is round 6's bound of 4e-6 (docs/kernels/cg.md)
        with balanced(False):
            off3, _ = _records(desc, seq, tol=1e-12, max_iter=3)
        with balanced(True):
            on3, _ = _records(desc, seq, tol=1e-12, max_iter=3)
    for k, (ra, rb) in enumerate(zip(on3, off3)):
        assert ra[1] == rb[1] == 3 and ra[2] == rb[2] == 2, (name, k, ra[1:], rb[1:])
        scale, diff = float(rb[0].abs().max()), float((ra[0] - rb[0]).abs().max())
        print("on against off, three steps, %s solve %d: max |dx| / max |x| = %.3g" % (name, k, diff / scale))
        assert diff <= 4e-6 * scale, (name, k, diff, scale)
