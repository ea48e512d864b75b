"""GPU tests of the two forms of the C == 1 tile kernels (csrc/spmm.hip spmv_tile_body, docs/kernels/spmm.md round 7).

A graph of up to 4096 row tiles runs the SINGLE-TILE form (one tile per workgroup, no tile loop: the head of the launch is one
batch of kernel arguments and one round trip of offsets, tests/test_tile_head_isa_cpu.py); larger graphs, and every graph under
mgp_spmm_set_tile_loop_mode(1), run the LOOP form.  The two forms are the same arithmetic in the same order, so everything they
leave is compared BIT FOR BIT, never to a tolerance (what the kernels compute is held against float64 by tests/test_gpu_parity.py,
tests/test_gpu_solver_contract.py and tests/test_gpu_cg_fold.py, which run the single-tile form by default):

  * the product and its weighted dot partials (plain kernel), with and without `pre`;
  * for folded CG plans (self-dot kernel, step kernel, deciding step kernel): solution, iterations, status, residual, applies,
    and both sets of partials the kernels leave in the plan's workspace -- ||r||^2 in two parities (the first launch of a solve
    writes ||b||^2 there through its second set of partials) and |t|^2.

Shapes: hand-made CSRs of 1, 63, 64 and 65 rows (one ragged tile, one full tile, a second tile of one row); a hand-made CSR whose
first tile has 6400 padded entries and about 6300 dictionary columns (both tail loops behind the staged loads run: they start above 4096
entries and above 1024 columns); the golden dumbbell (25 tiles, the last one ragged); edge-list graphs of 63, 64, 65 nodes and one with
such a large tile for the plans (a one-node graph has no edge and no plan).  The 300,071-node roll of tests/_past_caps.py runs the loop
form whatever the switch says (two tiles per workgroup): there the loop form's product is compared with the single-tile form run on
the same arrays as two row slices of at most 4096 tiles (the row sum order does not depend on the tiling)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_solver_contract import T, _desc, dev, dumbbell, mgp  # noqa: F401
from test_gpu_cg_fold import fold

pytestmark = pytest.mark.gpu


class loop_form:
    """with loop_form(0 / 1): the single-tile form where the grid allows it (the default) / the loop form everywhere."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from manifold_gp_amd import _lib
        _lib.lib().mgp_spmm_set_tile_loop_mode(self.on)

    def __exit__(self, *exc):
        from manifold_gp_amd import _lib
        _lib.lib().mgp_spmm_set_tile_loop_mode(0)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what      # NaN == NaN, -0 != 0


# ----------------------------------------------------------------------------- hand-made CSRs: the plain kernel
def _hand_csr(n, degrees, ncand, seed, dev):
    """Rows of the given numbers of entries at distinct ascending columns (drawn from the first `ncand` columns), padded to whole
    quads with value-0 entries at the row's end, as the graph builders leave them."""
    from manifold_gp_amd import _lib
    from manifold_gp_amd.graph import build_tiles
    rng = np.random.default_rng(seed)
    rowptr, cols, vals = [0], [], []
    for i in range(n):
        d = int(degrees[i])
        c = np.sort(rng.choice(ncand, size=d, replace=False)) if d else np.zeros(0, np.int64)
        pad = (-d) % 4 if d else 4                      # an empty row keeps one quad of padding
        cols.append(np.concatenate([c, np.full(pad, c[-1] if d else i)]))
        vals.append(np.concatenate([rng.standard_normal(d), np.zeros(pad)]))
        rowptr.append(rowptr[-1] + d + pad)
    t = dict(rowptr=T(np.asarray(rowptr, np.int32), dev), col=T(np.concatenate(cols).astype(np.int32), dev),
             vals=T(np.concatenate(vals).astype(np.float32), dev), diag=T((rng.random(n) + 1.0).astype(np.float32), dev))
    t["tiles"] = build_tiles(n, t["rowptr"], t["col"], int(rowptr[-1]), tile_rows=64)
    assert t["tiles"] is not None
    t["csr"] = _lib.csr_struct(n, t["rowptr"], t["col"], t["vals"], t["diag"], tiles=t["tiles"], lanes=8)
    return t


def _products(csr, n_rows, n_vec, dev, row_offset=0, seed=3):
    """The plain kernel with every operand (pre, post, base, weighted dot) and bare: (y, partials, y without pre, partials, y bare)."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(seed)
    x, base, w = (torch.randn(n_vec, 1, generator=gen).to(dev) for _ in range(3))
    pre = (torch.rand(n_vec, generator=gen) + 0.5).to(dev)
    assert lib.mgp_spmm_kernel_choice(ctypes.byref(csr), 1, 1, row_offset) == 1           # the tile kernel
    nb = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(csr), 1)
    out = []
    for p in (pre, None):
        y = torch.full((n_vec, 1), 7.0, device=dev)
        part = torch.full((nb,), 7.0, device=dev)
        _lib.check(lib.mgp_spmm_fused_rows(ctypes.byref(csr), row_offset, _lib.ptr(x), 1, _lib.ptr(y), 1.25, 0.75, _lib.ptr(p),
                                           _lib.ptr(pre), _lib.ptr(base), 0.5, 2.0, _lib.ptr(w), _lib.ptr(part), _lib.stream()),
                   "mgp_spmm_fused_rows")
        out += [y, part]
    y = torch.full((n_vec, 1), 7.0, device=dev)
    _lib.check(lib.mgp_spmm_fused_rows(ctypes.byref(csr), row_offset, _lib.ptr(x), 1, _lib.ptr(y), 0.0, 1.0, None, None, None, 0.0,
                                       1.0, None, None, _lib.stream()), "mgp_spmm_fused_rows")
    torch.cuda.synchronize()
    return out + [y]


def _big_tile_degrees(n):
    d = np.full(n, 3)
    d[:64] = 100              # tile 0: 6400 padded entries (> 4 * 4 * 256), 6400 candidates for its dictionary (> 4 * 256)
    return d


@pytest.mark.parametrize("n", [1, 63, 64, 65, "big_tile"])
def test_plain_kernel_single_tile_against_loop(mgp, dev, n):
    if n == "big_tile":
        n = 8192
        t = _hand_csr(n, _big_tile_degrees(n), n, 11, dev)
        tp = t["tiles"]["tile_ptr"].cpu().numpy()
        rp = t["rowptr"].cpu().numpy()
        assert rp[64] - rp[0] > 4096 and tp[1] - tp[0] > 1024, (rp[64], tp[1])            # above BOTH limits
    else:
        t = _hand_csr(n, np.minimum(np.arange(n) % 7 + 1, n), n, 10 + n, dev)
    outs = {}
    for mode in (0, 1):
        with loop_form(mode):
            outs[mode] = _products(t["csr"], n, n, dev)
    for k, (a, b) in enumerate(zip(outs[0], outs[1])):
        _same_bits(a, b, ("n", n, "output", k))
    # the kernel ran: nothing keeps the fill value, and a product is not all zero
    assert not bool((outs[0][0] == 7.0).all()) and bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][4].abs().max()) > 0


def test_plain_kernel_dumbbell(mgp, dumbbell, dev):
    lap = dumbbell["randomwalk"]
    csr = lap.data.csr()
    n = dumbbell["n"]
    assert -(-n // 64) == 25 and n % 64 != 0
    outs = {}
    for mode in (0, 1):
        with loop_form(mode):
            outs[mode] = _products(csr, n, n, dev)
    for k, (a, b) in enumerate(zip(outs[0], outs[1])):
        _same_bits(a, b, ("dumbbell output", k))


def test_loop_form_past_4096_tiles_against_single_tile_slices(mgp, dev):
    """300,071 rows, 4689 tiles, two per workgroup: only the loop form can run.  The same arrays as two row slices (4096 tiles and
    593 tiles, the second through the row-partitioned entry) run the single-tile form; the products agree bit for bit."""
    import _past_caps
    from manifold_gp_amd import _lib
    from manifold_gp_amd.graph import LaplacianData
    lib = _lib.lib()
    g = _past_caps.swiss300k(mgp, dev, "morton")
    graph, N = g["graph"], _past_caps.N
    assert graph.tiles is not None and graph.tiles.get("rowid") is None and graph.tiles["rows"] == 64
    data = LaplacianData(graph, g["eps"], True)
    whole = data.csr()
    assert lib.mgp_spmm_dot_blocks_csr(ctypes.byref(whole), 1) < -(-N // 64)                 # more than one tile per workgroup
    ref = _products(whole, N, N, dev)
    cut = 4096 * 64
    t = graph.tiles
    head = _lib.csr_struct(cut, graph.rowptr, graph.col, data.vals, data.diag, ncols=N, tiles=t, lanes=graph.spmv_lanes)
    tail_tiles = dict(t, tile_ptr=t["tile_ptr"][4096:])
    tail = _lib.csr_struct(N - cut, graph.rowptr[cut:], graph.col, data.vals, data.diag[cut:], ncols=N, tiles=tail_tiles,
                           lanes=graph.spmv_lanes)
    assert lib.mgp_spmm_dot_blocks_csr(ctypes.byref(head), 1) == 4096 and lib.mgp_spmm_dot_blocks_csr(ctypes.byref(tail), 1) == 593
    a = _products(head, cut, N, dev)
    b = _products(tail, N - cut, N, dev, row_offset=cut)
    for k in (0, 2, 4):                                          # the three products (the partials are grouped by workgroup)
        _same_bits(ref[k][:cut], a[k][:cut], ("head slice", k))
        _same_bits(ref[k][cut:], b[k][cut:], ("tail slice", k))


# ----------------------------------------------------------------------------- folded plans: self dot, step, deciding step
def _edge_graph(mgp, dev, n, big_tile=False, seed=21):
    """A connected edge-list graph: every node and its eight successors on a ring (enough shared neighbours per tile that the tile
    builder keeps the given row order); big_tile: the first 64 nodes also reach 90 far nodes each."""
    rng = np.random.default_rng(seed)
    pairs = set()
    for i in range(n):
        for s in range(1, 9):
            j = (i + s) % n
            if i != j:
                pairs.add((min(i, j), max(i, j)))
    if big_tile:
        for i in range(64):
            for j in rng.choice(np.arange(64, n), size=90, replace=False):
                pairs.add((i, int(j)))
    pairs = np.asarray(sorted(pairs), np.int64)
    val = (rng.random(len(pairs)) * 0.05 + 0.01).astype(np.float32)
    lap = mgp.operators.GraphLaplacianOperator(T(val, dev), T(pairs.T.copy(), dev), n, torch.tensor([[0.2]], device=dev), "randomwalk", True)
    gen = torch.Generator().manual_seed(seed)
    return dict(lap=lap, n=n, kappa=1.0, y=torch.randn(n, 1, generator=gen).to(dev), y2=(torch.rand(n, 1, generator=gen) - 0.3).to(dev))


def _plan_partials(plan, n, nbs):
    """The partials a folded plan's kernels left: (||r||^2 [2][nbs], |t|^2 [nbs]).  Offsets: csrc/cg_policy.h cg_carve takes x r
    ubuf w p s usbuf [n] each, the operator scratch (4 n-vectors + 256 bytes), pd_gamma and pd_rr [2][4096], pd_delta [nbs];
    every take is rounded up to 256 bytes."""
    nb = (4 * n + 255) // 256 * 256
    off = 7 * nb + (4 * nb + 256) + 2 * 4096 * 4
    rr = plan.work[off: off + 2 * nbs * 4].view(torch.float32).clone()
    off += 2 * 4096 * 4
    return rr, plan.work[off: off + nbs * 4].view(torch.float32).clone()


def _plan_records(desc, seq, n, use_graph, decide, tol=1e-6, max_iter=20000):
    """One folded plan, the right-hand sides of `seq` in order (None: b = 0 with NaNs planted in the plan's x, p and s beforehand):
    per solve the solution, (iterations, status, residual, applies) and the two sets of partials."""
    from manifold_gp_amd.solvers import CgPlan
    with fold(1, complex_shift=0, decide=decide) as lib:
        plan = CgPlan(desc, 1, tol=tol, max_iter=max_iter, stop_mode=1, check_every=8, use_graph=use_graph)
        try:
            assert plan.folded
            nbs = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(plan.op.L), 1)
            nb = (4 * n + 255) // 256 * 256
            recs = []
            for rhs in seq:
                if rhs is None:
                    for slot in (0, 4, 5):
                        plan.work[slot * nb: slot * nb + 4 * n].view(torch.float32).fill_(float("nan"))
                    rhs = torch.zeros(n, 1, device=plan.work.device)
                x = plan.solve(rhs).clone()
                recs.append((x, (plan.iters, plan.status, tuple(plan.resid), plan.applies)) + _plan_partials(plan, n, nbs))
            return recs
        finally:
            plan.close()


def _compare_plans(desc, seq, n, label, **kw):
    out = {}
    for mode in (0, 1):
        with loop_form(mode):
            out[mode] = {(g, d): _plan_records(desc, seq, n, g, d, **kw) for g in (True, False) for d in (1, 0)}
    for key in out[0]:
        for k, (ra, rb) in enumerate(zip(out[0][key], out[1][key])):
            assert ra[1] == rb[1], (label, key, k, ra[1], rb[1])          # iterations, status, residual bits, applies
            _same_bits(ra[0], rb[0], (label, key, k, "solution"))
            _same_bits(ra[2], rb[2], (label, key, k, "||r||^2 partials"))
            _same_bits(ra[3], rb[3], (label, key, k, "|t|^2 partials"))
    return out[0]


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("case", [63, 64, 65, "big_tile", "dumbbell"])
def test_folded_plan_single_tile_against_loop(mgp, request, dev, case, form):
    """Graph replays and eager launches, both decision forms (the deciding step kernel and the plain one), forms 0 and 2 (form 2:
    delta = gamma + c |t|^2 and w = r + ...), b = 0 with NaNs planted in x / p / s, a max_iter exit, and solves whose first graph ends
    undecided (shown through applies == iterations + 1)."""
    if case == "dumbbell":
        G = request.getfixturevalue("dumbbell")
        lap, n, kappa, y, y2 = G["randomwalk"], G["n"], G["kappa"], G["y"], G["gauss"]
    else:
        G = _edge_graph(mgp, dev, 4096 if case == "big_tile" else case, big_tile=case == "big_tile")
        lap, n, kappa, y, y2 = G["lap"], G["n"], G["kappa"], G["y"], G["y2"]
    if case == "big_tile":
        t = lap.data.graph.tiles
        tp, rp = t["tile_ptr"].cpu().numpy(), (t.get("tile_rowptr") if t.get("rowid") is not None else lap.data.graph.rowptr).cpu().numpy()
        assert max(rp[min(n, 64 * (k + 1))] - rp[64 * k] for k in range(-(-n // 64))) > 4096 and int((tp[1:] - tp[:-1]).max()) > 1024
    desc = _desc(mgp, lap, 2, kappa, dev, form=form)
    seq = [y, y, y, y2, y2, None, y, y2]
    R = _compare_plans(desc, seq, n, (case, form))
    for key, recs in R.items():
        for (x, rep, _, _), rhs in zip(recs, seq):
            assert rep[1] == 1 or (case != "dumbbell" and rep[1] == 2), (case, form, key, rep)      # converged (never NaN / breakdown)
            if rhs is None:
                assert rep[0] == 0 and float(x.abs().max()) == 0.0 and rep[2][0] == 0.0
    # an undecided first graph: some replay was ended by a step launch, not by the decision alone
    undecided = [rep for _, rep, _, _ in R[(True, 1)][1:] if rep[0] > 0 and rep[3] == rep[0] + 1]
    print("tile head %s form %d: (iters, applies) %s" % (case, form, [(r[1][0], r[1][3]) for r in R[(True, 1)]]))
    if case == "dumbbell":
        assert undecided, [r[1] for r in R[(True, 1)]]           # more than 64 steps: every first graph ends undecided
    capped = _compare_plans(desc, [y, y, y2], n, (case, form, "max_iter 2"), tol=1e-12, max_iter=2)
    for recs in capped.values():
        assert all(rep[1] == 2 and rep[0] == 2 for _, rep, _, _ in recs)
