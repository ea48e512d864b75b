"""GPU tests of the folded CG step (docs/kernels/cg.md, round 6): nu = 2, C = 1 plans whose vector update runs in the epilogue of
the apply's second SpMV (spmv_tile_cgstep_kernel), with delta = [gamma +] c |B P u|^2 from the first one.

The folded plan answers to the contract written at the top of tests/test_gpu_solver_contract.py (C1-C5, float64 residuals formed
outside the kernels: `contract`, `R1`, `_check_plan` are imported from there), never to closeness with the unfolded plan: fold on
against off only share status and, within the slack test_cg_init_free_start_matches_classic allows, the iteration count.

Graphs: the golden dumbbell (1,546 nodes: 7 SpMV workgroups, fewer than the eight arrival groups of the deciding launch), a
20,000-node swiss roll at k = 16 (79 workgroups) and, once, the 300,071-node roll of tests/_past_caps.py (2,345 partials: 16
slots per lane, two tiles per workgroup, relabelled matrix).

tol.  The contract asserts its own floor, F = 4 eps32 ||A|| ||x|| / ||b|| <= tol / 4, and F >= 4 eps32 = 4.8e-7 for every
system: no float32 solve can be held to it at tol = 1e-6.  The contract cases therefore run at 1e-3 (and 1e-4 where F allows);
at 1e-6 (test_fold_at_1e6) the same inequalities C1 / C3 / C5 are asserted on the near-identity swiss-roll systems against the same
float64 residuals, with F added as the contract adds it but without the clause F <= tol / 4."""
import numpy as np
import pytest
import torch

from test_gpu_solver_contract import R1, T, _check_plan, _desc, contract, dev, dumbbell, mgp, swiss_roll  # noqa: F401

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)

# The swiss roll's form-2 systems are near the identity (two to four steps).  One system must run 20 steps or more, so that both
# parities of the partials and of gamma_old / alpha_old are written many times: form 0, random walk, kappa = LONG_KAPPA (tau =
# 4 / kappa^2 = 1.78 against lambda_max(L_sym) = 9.6).  Chosen beforehand with a float64 CG on the host over k-d tree neighbours of
# the same points (oracle.laplacian.LaplacianOracle, scale 0.7, Gaussian right-hand side), as tests/test_gpu_solver_contract.py chose
# its 300k systems: kappa 1.5 -> 28 iterations at tol 1e-3 (F / tol 0.004) and 56 at 1e-6; kappa 0.6 -> 9; kappa 0.45 -> 7; kappa
# 0.35 -> 6 (a smaller length scale moves A towards a multiple of P^2).  Measured on the GPU, folded: 28 at 1e-3, 37 at 1e-4.
LONG_KAPPA = 1.5
LONG_MIN_ITERS = 20


class fold:
    """with fold(0 / 1 / 2): plans created inside never take the folded step / take it up to 1024 SpMV workgroups (the default) /
    wherever the shape allows (mgp_cg_set_fold_update)."""

    def __init__(self, on, complex_shift=None, decide=None):
        self.on, self.cx, self.decide = on, complex_shift, decide

    def __enter__(self):
        from manifold_gp_amd import _lib
        lib = _lib.lib()
        self.prev = lib.mgp_cg_set_fold_update(self.on)
        self.prev_cx = lib.mgp_cg_set_complex_shift(self.cx) if self.cx is not None else None
        self.prev_dec = lib.mgp_cg_set_decide_in_update(self.decide) if self.decide is not None else None
        return lib

    def __exit__(self, *exc):
        from manifold_gp_amd import _lib
        lib = _lib.lib()
        lib.mgp_cg_set_fold_update(self.prev)
        if self.prev_cx is not None:
            lib.mgp_cg_set_complex_shift(self.prev_cx)
        if self.prev_dec is not None:
            lib.mgp_cg_set_decide_in_update(self.prev_dec)


def _is_folded(desc, **kw):
    from manifold_gp_amd.solvers import CgPlan
    plan = CgPlan(desc, kw.pop("C", 1), tol=1e-3, max_iter=10, stop_mode=1, **kw)
    try:
        return plan.folded
    finally:
        plan.close()


def _records(desc, seq, tol=1e-6, max_iter=20000, **kw):
    """One plan, the right-hand sides of `seq` in order: (x, iters, status, resid, applies) per solve."""
    from manifold_gp_amd.solvers import CgPlan
    plan = CgPlan(desc, 1, tol=tol, max_iter=max_iter, stop_mode=1, check_every=8, **kw)
    try:
        recs = []
        for rhs in seq:
            x = plan.solve(rhs).clone()
            recs.append((x, plan.iters, plan.status, tuple(plan.resid), plan.applies))
        return recs, plan.folded
    finally:
        plan.close()


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[1:] == rb[1:], (what, k, ra[1:], rb[1:])          # iterations, status, residual bits, applies
        assert torch.equal(ra[0], rb[0]), (what, k)                   # the solution, bit for bit


# ----------------------------------------------------------------------------- the contract
@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
@pytest.mark.parametrize("graph", ["dumbbell", "swiss_roll"])
def test_fold_contract(mgp, request, dev, graph, norm, form):
    """C1-C5 for the folded plan: forms 0 and 2, both normalisations, eager first solve and graph replays (three solves per plan),
    both decision forms, and the max_iter exit (C4)."""
    G = request.getfixturevalue(graph)
    lap = G[norm]
    desc = _desc(mgp, lap, 2, 1.5 if graph == "swiss_roll" else G["kappa"], dev, form=form)
    sys = R1(lap, desc)
    tols = (1e-3, 1e-4) if graph == "swiss_roll" else (1e-3,)       # the dumbbell's floor F is above 1e-4 / 4
    for decide in (1, 0):
        with fold(1, complex_shift=0, decide=decide):                # (symmetric, form 2: CG on A, not the complex-shift plan)
            assert _is_folded(desc)
            for tol in tols:
                _, cx, _ = _check_plan(sys, desc, G["gauss"], tol, label="fold %s %s form %d decide %d" % (graph, norm, form, decide))
                assert not cx
            capped = (1e-3, 5) if graph == "dumbbell" else (1e-4, 2)  # (near the identity: two steps at 1e-4 leave it unconverged)
            _check_plan(sys, desc, G["gauss"], capped[0], max_iter=capped[1], repeats=2, label="fold capped decide %d" % decide)


def test_fold_contract_long_solve(mgp, swiss_roll, dev):
    """A folded solve of LONG_MIN_ITERS steps or more (the parities flip many times; continuation graphs; re-capture)."""
    lap = swiss_roll["randomwalk"]
    desc = _desc(mgp, lap, 2, LONG_KAPPA, dev, form=0)
    sys = R1(lap, desc)
    with fold(1):
        assert _is_folded(desc)
        recs, _, _ = _check_plan(sys, desc, swiss_roll["gauss"], 1e-3, label="fold long")
    for _, its, _, _, _ in recs:
        assert its >= LONG_MIN_ITERS, its


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
def test_fold_at_1e6(mgp, swiss_roll, dev, norm, form):
    """tol = 1e-6 (the benchmark's): C1, C3, C5 with the floor added and not asserted (module docstring), float64 residuals of R1,
    both normalisations (symmetric: no pre / post vector, the first launch without pre-scaling; form 2 as CG on A, complex shift
    off).  These are the cases that notice a wrong delta (docs/kernels/cg.md, "The checks bite (round 6)").  The dumbbell is left
    out at this tolerance: its floor F is 1e-5 ... 3e-4 (cond ~ 1e5), so 2 tol + F would hold for any answer near the solution."""
    lap = swiss_roll[norm]
    desc = _desc(mgp, lap, 2, 1.5, dev, form=form)
    sys = R1(lap, desc)
    tol = 1e-6
    z = torch.zeros_like(swiss_roll["gauss"])
    with fold(1, complex_shift=0):
        recs, folded = _records(desc, [swiss_roll["gauss"], swiss_roll["gauss"], swiss_roll["y"], z, swiss_roll["gauss"]], tol=tol)
    assert folded
    for (x, its, st, res, _), rhs in zip(recs, (swiss_roll["gauss"], swiss_roll["gauss"], swiss_roll["y"], z, swiss_roll["gauss"])):
        assert st == 1
        b = rhs.double().cpu().numpy()
        x64 = x.double().cpu().numpy()
        if not b.any():
            assert its == 0 and not x64.any() and res[0] == 0.0                   # C5
            continue
        true_rel = np.linalg.norm(b - sys.apply(x64)) / np.linalg.norm(b)
        F = 4 * EPS32 * sys.norm2 * np.linalg.norm(x64) / np.linalg.norm(b)
        print("fold 1e-6 %s form %d: iters %d true_rel %.3g resid %.3g F %.3g" % (norm, form, its, true_rel, res[0], F))
        assert true_rel <= 2 * tol + F                                            # C1
        assert true_rel <= 2 * res[0] + F                                         # C3


# ----------------------------------------------------------------------------- fold on against off
@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
@pytest.mark.parametrize("graph", ["dumbbell", "swiss_roll"])
def test_fold_on_against_off(mgp, request, dev, graph, norm, form):
    """Same status; iteration counts within max(8, 4 %) (test_cg_init_free_start_matches_classic's slack).  No closeness bound."""
    G = request.getfixturevalue(graph)
    desc = _desc(mgp, G[norm], 2, 1.5 if graph == "swiss_roll" else G["kappa"], dev, form=form)
    seq = [G["y"], G["y"], G["gauss"], G["y"]]
    out = {}
    for mode in (0, 1):
        with fold(mode, complex_shift=0):
            out[mode], folded = _records(desc, seq, tol=1e-6)
            assert folded == bool(mode)
    for (x0, it0, st0, _, _), (x1, it1, st1, _, _) in zip(out[0], out[1]):
        assert st0 == st1 == 1
        assert abs(it0 - it1) <= max(8, it0 // 25), (it0, it1)


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("graph,norm,form", [("dumbbell", "randomwalk", 0), ("dumbbell", "randomwalk", 2), ("swiss_roll", "randomwalk", 0),
                                             ("swiss_roll", "randomwalk", 2), ("swiss_roll", "symmetric", 0), ("dumbbell", "symmetric", 2)])
def test_fold_bit_for_bit(mgp, request, dev, graph, norm, form):
    """With the fold on: graph replay == eager launches; decide_in_update 0 == 1; right-hand sides at alternating addresses (the
    graph's root node re-pointed); a first graph that ends undecided (a right-hand side that needs more steps than the captured
    length) and its re-capture, shown through `applies`; the max_iter exit; a rebound plan == a fresh plan.  Graph against eager
    compares solution, iterations, status and residual: `applies` differs by design, only a graph ends in the decision alone."""
    from manifold_gp_amd.solvers import CgPlan
    G = request.getfixturevalue(graph)
    lap = G[norm]
    kappa = 1.5 if graph == "swiss_roll" else G["kappa"]
    desc = _desc(mgp, lap, 2, kappa, dev, form=form)
    y, y2 = G["y"], G["gauss"]
    z, yc = torch.zeros_like(y), y.clone()
    seq = [y, y, y, y2, y2, y, z, y, yc, y, yc, y2, y]
    out = {}
    with fold(1, complex_shift=0):
        for decide in (1, 0):
            with fold(1, decide=decide):
                for use_graph in (True, False):
                    recs, folded = _records(desc, seq, use_graph=use_graph)
                    assert folded
                    capped, _ = _records(desc, [y, y, y2, y], tol=1e-12, max_iter=5, use_graph=use_graph)
                    out[(decide, use_graph)] = recs + capped
        _same(out[(1, True)], out[(0, True)], "decide_in_update 1 against 0")
        for decide in (1, 0):
            a, b = out[(decide, True)], out[(decide, False)]
            for k, (ra, rb) in enumerate(zip(a, b)):              # `applies` differs by design: only a graph ends in the decision alone
                assert ra[1:4] == rb[1:4] and torch.equal(ra[0], rb[0]), (decide, k, ra[1:], rb[1:])
        for x, its, st, _, _ in out[(1, True)][len(seq):]:
            assert st == 2 and its == 5
        for k, rhs in enumerate(seq):
            x, its, st, _, _ = out[(1, True)][k]
            assert st == 1
            if rhs is z:
                assert its == 0 and float(x.abs().max()) == 0.0
        # The undecided first graph and its re-capture, made explicit.  `applies` == iters when the first graph ended in the decision
        # alone (it held exactly the steps the solve needed) and iters + 1 when a step launch took the decision (cg_policy.h:
        # cg_first_len, cg_recapture_first: single-graph solves up to 64 steps).
        #  * swiss roll, form 0 (y and y2 need 40 ... 60 steps, different counts).  y2 the longer: solve 3 (the first y2 behind three
        #    y) runs a graph captured for y to its end undecided, a continuation chunk decides, the graph is re-captured at once and
        #    solve 4 ends in the decision alone.  y2 the shorter: the graph shrinks after the two y2 (solves 3, 4), solve 5 (y
        #    again) is the undecided one and solve 7 (y, behind the zero right-hand side) runs the re-captured graph.
        #  * swiss roll, random walk, form 2: both need the same few steps, every replay ends in the decision alone.
        #  * dumbbell: more than 64 steps, no single-graph form -- EVERY first graph (4 steps) ends undecided and continuation
        #    chunks carry the solve: a step launch decides every time.
        for decide in (1, 0):
            R = out[(decide, True)]
            ny, n2 = R[1][1], R[3][1]
            print("bit for bit %s %s form %d decide %d: iters y %d y2 %d, (iters, applies) %s" % (
                graph, norm, form, decide, ny, n2, [(r[1], r[4]) for r in R[:len(seq)]]))
            nonzero = [r for r, rhs in zip(R, seq) if rhs is not z]
            if graph == "dumbbell":
                assert min(ny, n2) > 64 and all(r[4] == r[1] + 1 for r in nonzero)
            elif form == 0:
                assert ny != n2 and 2 <= min(ny, n2) and max(ny, n2) < 64
                und, rec = (3, 4) if n2 > ny else (5, 7)
                assert R[und][4] == R[und][1] + 1, (und, R[und][1:])            # undecided first graph: a step launch decided
                assert R[rec][4] == R[rec][1], (rec, R[rec][1:])                # re-captured: the decision alone
            else:
                assert ny == n2 and all(r[4] == r[1] for r in nonzero[1:])      # (solve 0 is eager)
        # a rebound plan against a fresh one: the same structure at another length scale and scale
        desc2 = _desc(mgp, lap, 2, 1.25 * kappa, dev, form=form, scale=0.9)
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


# ----------------------------------------------------------------------------- edge solves
def test_fold_edge_solves(mgp, dumbbell, dev):
    from manifold_gp_amd.solvers import CgPlan
    lap = dumbbell["randomwalk"]
    desc = _desc(mgp, lap, 2, dumbbell["kappa"], dev, form=2)
    sys = R1(lap, desc)
    y = dumbbell["gauss"]
    z = torch.zeros_like(y)
    with fold(1):
        for use_graph in (True, False):
            plan = CgPlan(desc, 1, tol=1e-3, max_iter=20000, stop_mode=1, check_every=8, use_graph=use_graph)
            try:
                assert plan.folded
                # b = 0 with stale NaNs in the plan's x, p and s (byte offsets of the workspace: cg_carve takes x r ubuf w p s)
                nb = (4 * desc.n + 255) // 256 * 256
                for solve in range(3):                                  # eager, the capturing solve, a replay
                    for slot in (0, 4, 5):
                        plan.work[slot * nb: slot * nb + 4 * desc.n].view(torch.float32).fill_(float("nan"))
                    x = plan.solve(z).clone()
                    assert plan.status == 1 and plan.iters == 0 and float(x.abs().max()) == 0.0 and plan.resid[0] == 0.0, solve
                    x = plan.solve(y).clone()
                    contract(sys, y, x, 1e-3, 1, plan.status, plan.iters, plan.resid, label="after b = 0")
                    assert plan.status == 1
                # NaN in b
                bn = y.clone()
                bn[7, 0] = float("nan")
                plan.solve(bn)
                assert plan.status == 3
                x = plan.solve(y).clone()
                assert plan.status == 1 and bool(torch.isfinite(x).all())
            finally:
                plan.close()
        # max_iter = 5: status 2 and iters == 5 (C4)
        _check_plan(sys, desc, y, 1e-3, max_iter=5, repeats=3, label="fold max_iter 5")
        # refine = 2: the true residual of the float64 solution, max(resid) <= 2 tol
        plan = CgPlan(desc, 1, tol=1e-6, max_iter=20000, stop_mode=1, refine=2)
        try:
            assert plan.folded
            for _ in range(2):
                plan.solve(y)
                assert plan.status == 1 and max(plan.resid) <= 2e-6, plan.resid
        finally:
            plan.close()


# ----------------------------------------------------------------------------- gating
def test_fold_gating(mgp, dumbbell, dev):
    """nu = 1, nu = 3, a masked descriptor (pre != post), Jacobi and C = 2 keep the (apply, update) launches: `folded` is False and
    the knob changes nothing, bit for bit."""
    from manifold_gp_amd.solvers import CgPlan
    lap = dumbbell["randomwalk"]
    n = dumbbell["n"]
    mask = torch.ones(n, device=dev)
    mask[::7] = 0.5
    cases = [("nu1", _desc(mgp, lap, 1, dumbbell["kappa"], dev), {}, 1),
             ("nu3", _desc(mgp, lap, 3, dumbbell["kappa"], dev), {}, 1),
             ("masked", _desc(mgp, lap, 2, dumbbell["kappa"], dev, form=0).masked(mask, mask), {}, 1),      # pre and post: two tensors
             ("jacobi", _desc(mgp, lap, 2, dumbbell["kappa"], dev), dict(jacobi=True), 1),
             ("C2", _desc(mgp, lap, 2, dumbbell["kappa"], dev), {}, 2)]
    for label, desc, kw, C in cases:
        rhs = torch.cat([dumbbell["gauss"], dumbbell["y"]], 1)[:, :C].contiguous()
        out = {}
        for mode in (0, 1):
            with fold(mode):
                plan = CgPlan(desc, C, tol=1e-3, max_iter=20000, stop_mode=1, check_every=8, **kw)
                try:
                    assert not plan.folded, label
                    out[mode] = [(plan.solve(rhs).clone(), plan.iters, plan.status, tuple(plan.resid)) for _ in range(3)]
                finally:
                    plan.close()
        for a, b in zip(out[0], out[1]):
            assert a[1:] == b[1:] and torch.equal(a[0], b[0]), label
    with fold(1):
        assert _is_folded(_desc(mgp, lap, 2, dumbbell["kappa"], dev))            # the qualifying shape, for contrast


# ----------------------------------------------------------------------------- past 1024 partials
def test_fold_past_1024_partials(mgp, dev):
    """The 300,071-node roll in generation order (relabelled matrix, two tiles per workgroup, 2,345 partials: 16 slots per lane in
    the step kernel, in its hand-off and in cg_decide_c1_kernel), form 0, random walk, at tests/test_gpu_solver_contract.py's
    BIG_KAPPA / BIG_SCALE: the contract, 20 iterations or more.  Past 1024 workgroups the default keeps the update launches (the
    fold was measured slower there), so the plan is folded through knob 2."""
    import ctypes
    import _past_caps
    from manifold_gp_amd import _lib
    from manifold_gp_amd.solvers import CgPlan
    from test_gpu_solver_contract import BIG_KAPPA, BIG_MIN_ITERS, BIG_SCALE
    g = _past_caps.swiss300k(mgp, dev, "random")
    lap = mgp.operators.GraphLaplacianOperator(g["val"], g["idx"], _past_caps.N, torch.tensor([[g["eps"]]], device=dev), "randomwalk",
                                               graph=g["graph"])
    desc = _desc(mgp, lap, 2, BIG_KAPPA, dev, form=0, scale=BIG_SCALE)
    sys = R1(lap, desc)
    rhs = torch.randn(_past_caps.N, 1, generator=torch.Generator().manual_seed(43)).to(dev)
    with fold(1):
        assert not _is_folded(desc)
    with fold(2) as lib:
        plan = CgPlan(desc, 1, tol=1e-3, max_iter=10, stop_mode=1)
        try:
            nbs = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(plan.op.L), 1)
            assert plan.folded and nbs > 1024 and plan._rg is not None, nbs
            assert nbs < -(-_past_caps.N // int(plan.op.L.tile_rows))            # more than one tile per workgroup
        finally:
            plan.close()
        recs, _, _ = _check_plan(sys, desc, rhs, 1e-3, repeats=2, label="fold 300k")
    for _, its, _, _, _ in recs:
        assert its >= BIG_MIN_ITERS, its
