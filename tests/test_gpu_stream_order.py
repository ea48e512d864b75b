"""Every covered entry point, and the package, on a side stream behind pending work (docs/stream_contract.md).

The header promises that every entry point is asynchronous on `stream`, and the package hands the library torch's current stream,
keeps plans and scratch per stream and replays captured graphs on the caller's stream.  On the null stream with nothing pending --
where the rest of the suite runs -- a launch that drops its stream argument, a memset on stream 0 or a graph replayed on its capture
stream cannot be told from a correct one.  Here each case of tests/_entry_cases.py runs once on the default stream and once on a
fresh torch.cuda.Stream behind a bounded delay, with its inputs arriving on that stream behind the delay (_guarded.run_stream_order):
work issued anywhere but on the side stream reads decoy inputs and has its writes wiped.

  controls   a torch "entry point" that issues its work on the default stream, and mgp_scale_rows / mgp_permute_rows called with a
             null stream argument, must be reported as `order`; the same toy on the current stream must pass
  entries    all parameters of the memory contract: rc, guards, inputs, order, window all empty
  package    operator matmul, CG plans (per-stream plans, graph replay), k-NN graph + Lanczos, a Bernoulli Laplace fit and sampling,
             inside `with torch.cuda.stream(side):` behind the delay, against the default-stream result
  scratch    _lib.workspace is keyed by the current stream
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guarded as G                      # noqa: E402
import _entry_cases as E                  # noqa: E402
from manifold_gp_amd import _lib          # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: stream order is checked on the MI355X only")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def delay(dev):
    return G.Delay(dev)


# ------------------------------------------------------------------------------------------------------------------- controls
def toy(on_default_stream):
    """out = 2 x + w as one torch kernel; with `on_default_stream` issued there whatever the current stream is: the planted defect."""
    def case(carve, shape):
        n = shape["n"]
        rng = np.random.default_rng(n)
        x, w = carve("x", F32, n, "in", rng.normal(0, 1, n)), carve("w", F32, n, "in", rng.normal(0, 1, n))
        out = carve("out", F32, n, "out")

        def run(work_bytes):
            ctx = torch.cuda.stream(torch.cuda.default_stream(out.device)) if on_default_stream else contextlib.nullcontext()
            with ctx:
                torch.add(w, x, alpha=2.0, out=out)
            E._sync()
            return 0, {}
        return G.Call(run)
    return case


def on_null_stream(case_fn):
    """The registry's case with a null stream argument: its one launch goes to stream 0 while the run stages on the side stream."""
    def case(carve, shape):
        keep = E._stream
        E._stream = lambda: ctypes.c_void_p(0)
        try:
            return case_fn(carve, shape)
        finally:
            E._stream = keep
    return case


CONTROLS = {
    "toy-default-stream": (toy(True), dict(n=257), True),
    "scale_rows-null-stream": (on_null_stream(E.case_scale_rows), dict(n=257, P=7, with_x=1), True),
    "permute_rows-null-stream": (on_null_stream(E.case_permute_rows), dict(n=257, C=7), True),
    "toy-current-stream": (toy(False), dict(n=257), False),
}


@pytest.mark.parametrize("control", sorted(CONTROLS))
def test_the_helper_reports_work_issued_off_the_side_stream(dev, delay, control):
    case, shape, planted = CONTROLS[control]
    found, info = G.run_stream_order(case, shape, dev, E, delay)
    print("%s: %s %s" % (control, {c: len(found[c]) for c in G.ORDER_CHECKS}, info))
    hit = {c for c in G.ORDER_CHECKS if found[c]}
    assert hit == ({"order"} if planted else set()), "%s: reported %s\n%s" % (control, sorted(hit), G.report_order(found))
    assert info["decoys"] >= 1 and info["rearms"] >= 1              # (mgp_permute_rows has one float array, its source)
    assert E.SYNC_HOOK is None and E._stream() is not None


# -------------------------------------------------------------------------------------------------------------- every entry point
@pytest.mark.parametrize("name,family,shape_id", E.params(), ids=["%s-%s-%s" % p for p in E.params()])
def test_entry_point_is_ordered_on_its_stream(dev, delay, name, family, shape_id):
    case = E.CASES[name]
    with case.families[family]():
        found, info = G.run_stream_order(case.fn, case.shapes_of(family)[shape_id], dev, E, delay)
    print("%s %s %s: %d arrays with a decoy, %d re-arms, delay %.1f ms (default stream %.2f ms); %s"
          % (name, family, shape_id, info["decoys"], info["rearms"], info["delay_ms"], info["ref_ms"],
             {c: len(found[c]) for c in G.ORDER_CHECKS}))
    for check in G.ORDER_CHECKS:
        assert not found[check], "%s [%s, %s] breaks check `%s`:\n%s" % (name, family, shape_id, check, G.report_order(found))


# ---------------------------------------------------------------------------------------------------- the package, side stream
@pytest.fixture(scope="module")
def mgp():
    import manifold_gp_amd
    _lib.lib()
    return manifold_gp_amd


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def dumbbell(mgp, golden, dev):
    """The golden dumbbell (n = 1546): both normalisations, its targets, its length scale."""
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    out = dict(g=g, n=n, kappa=float(g["kappa"]), y=T(g["train_y"], dev))
    for norm in ("symmetric", "randomwalk"):
        out[norm] = mgp.operators.GraphLaplacianOperator(T(g["edge_value"], dev), T(g["edge_index"].astype(np.int64), dev), n,
                                                         torch.tensor([[float(g["eps"])]], device=dev), norm, bool(g["self_loops"]))
    return out


def _same(a, b):
    """Bitwise equality of two results: tensors, numbers, or lists / tuples of them."""
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


class Behind:
    """A side stream, and tensor inputs that arrive on it behind a delay: stage(x=...) -- called under `with
    torch.cuda.stream(self.side)` -- gives each float tensor as a copy rolled by one element (the decoy; integer and bool tensors
    true), written synchronously, then enqueues the delay and the copy_ of the true values behind it.  Work issued on another
    stream meanwhile reads the decoy.  The window is asserted at every stage."""

    def __init__(self, dev, delay, ref_ms):
        self.delay, self.ms = delay, min(G.DELAY_CAP_MS, max(20.0 * ref_ms, G.DELAY_FLOOR_MS))
        self.side = G.side_stream(dev, delay)
        self.stages = 0

    def stage(self, **true):
        assert torch.cuda.current_stream() == self.side
        torch.cuda.synchronize()
        staged = {k: (torch.roll(v.reshape(-1), 1).view_as(v) if v.is_floating_point() else v).clone() for k, v in true.items()}
        torch.cuda.synchronize()
        ok, _ = G.window_open(self.delay, self.ms, lambda: [staged[k].copy_(true[k]) for k in staged])
        assert ok, "the delay of %.1f ms had run out before a marker on the default stream completed" % self.ms
        self.stages += 1
        return staged


def _timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return out, t0.elapsed_time(t1)


def _default_then_side(dev, delay, fn, true, label, bar=None):
    """fn(**tensors) twice on the default stream, then once under the side stream with its tensors staged behind the delay.
    Bitwise equal to the default-stream result where the two default-stream runs are; otherwise `bar(result)` must hold."""
    first = fn(**true)
    second, ref_ms = _timed(lambda: fn(**true))
    repeatable = _same(first, second)
    behind = Behind(dev, delay, ref_ms)
    try:
        with torch.cuda.stream(behind.side):
            got = fn(**behind.stage(**true))
    finally:
        torch.cuda.synchronize()
    print("%s: default stream %.2f ms, repeatable bit for bit: %s, delay %.1f ms" % (label, ref_ms, repeatable, behind.ms))
    if repeatable:
        assert _same(first, got), "%s: the side-stream result differs from the default-stream one" % label
    else:
        assert bar is not None, "%s: two default-stream runs differ and the path has no bar to fall back to" % label
        bar(got)
    return first, got


@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("C", [1, 12, 64])
def test_operator_matmul_under_a_side_stream(mgp, dumbbell, dev, delay, norm, C):
    Q = mgp.operators.PrecisionMaternOperator(dumbbell[norm], 2, torch.tensor([[dumbbell["kappa"]]], device=dev))
    X = torch.randn(dumbbell["n"], C, generator=torch.Generator().manual_seed(7 + C)).to(dev)
    with torch.no_grad():
        ref, _ = _default_then_side(dev, delay, lambda X: Q.matmul(X), dict(X=X), "matmul %s C = %d" % (norm, C))
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0


CG_TOL = 1e-3


@pytest.mark.parametrize("path", ["complex-shift", "folded", "C12"])
def test_cg_plans_are_kept_per_stream(mgp, dumbbell, dev, delay, path):
    """Three solves on each stream (eager, capture, graph replay), each side-stream solve behind the delay with a staged right-hand
    side; then the two streams in turn on the same operator: two plans in the cache, every solve equal to its stream's first."""
    from manifold_gp_amd import solvers
    from test_gpu_solver_contract import R1, _desc, contract
    lap = dumbbell["symmetric"]
    desc = _desc(mgp, lap, 2, dumbbell["kappa"], dev, form=2)
    C = 12 if path == "C12" else 1
    rhs = torch.randn(dumbbell["n"], C, generator=torch.Generator().manual_seed(41)).to(dev)
    lib = _lib.lib()
    prev = lib.mgp_cg_set_complex_shift(0 if path == "folded" else 1)
    solvers.clear_plan_cache()
    solve = lambda b: solvers.cg_solve(desc, b, tol=CG_TOL, stop_mode=1)
    try:
        (ref, ref_ms) = _timed(lambda: [solve(rhs) for _ in range(3)])
        assert len(solvers._PLAN_CACHE) == 1
        plan = next(iter(solvers._PLAN_CACHE.values()))
        assert (plan.complex_shift, plan.folded) == (path == "complex-shift", path == "folded"), (path, plan.complex_shift, plan.folded)
        repeatable = all(_same(r, ref[0]) for r in ref)
        behind = Behind(dev, delay, ref_ms / 3)
        sys = None if repeatable else R1(lap, desc)

        def holds(got, want, label):
            if repeatable:
                assert _same(got, want), "%s %s: differs from the first solve" % (path, label)
            else:           # the contract of tests/test_gpu_solver_contract.py, C1 and C3 (status 1: cg_solve warns otherwise)
                contract(sys, rhs, got[0], CG_TOL, 1, 1, got[1], got[2], label="%s %s" % (path, label))
        try:
            got = []
            with torch.cuda.stream(behind.side):
                for i in range(3):
                    got.append(solve(behind.stage(rhs=rhs)["rhs"]))
            torch.cuda.synchronize()
            for i in range(3):
                holds(got[i], ref[0], "side-stream solve %d" % i)
            keys = list(solvers._PLAN_CACHE)
            assert len(keys) == 2 and keys[0][:-1] == keys[1][:-1] and {keys[0][-1], keys[1][-1]} == \
                {int(torch.cuda.default_stream(dev).cuda_stream), int(behind.side.cuda_stream)}, keys
            plans = list(solvers._PLAN_CACHE.values())
            assert plans[0] is not plans[1] and plans[0].work.data_ptr() != plans[1].work.data_ptr()
            for turn in range(3):
                holds(solve(rhs), ref[0], "default stream, turn %d" % turn)
                with torch.cuda.stream(behind.side):
                    x = solve(behind.stage(rhs=rhs)["rhs"])
                torch.cuda.synchronize()
                holds(x, got[0], "side stream, turn %d" % turn)
            assert list(solvers._PLAN_CACHE) == keys and list(solvers._PLAN_CACHE.values()) == plans
        finally:
            torch.cuda.synchronize()
            solvers.clear_plan_cache()               # while the side stream is alive
        print("cg %s: repeatable bit for bit: %s, %d staged solves, delay %.1f ms, iterations %s"
              % (path, repeatable, behind.stages, behind.ms, [r[1] for r in ref]))
    finally:
        lib.mgp_cg_set_complex_shift(prev)


def test_knn_graph_and_eigensolver_under_a_side_stream(mgp, dev, delay):
    import warnings
    from manifold_gp_amd import solvers
    from tools import synth
    x_np, _, length = synth.dumbbell_resampled(2000)
    n = x_np.shape[0]
    eps = torch.tensor([[10.0 * length / n]], device=dev)

    def pipeline(x):
        knn = mgp.utils.NearestNeighbors(x)
        idx, val = knn.graph(10)
        lap = mgp.operators.GraphLaplacianOperator(val, idx, n, eps, "symmetric", graph=knn.knn_graph)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solvers.EigenFloorWarning)
            evals, evecs, resid = solvers.lanczos_smallest(lap.data, 12)
        return idx, val, evals, evecs, resid

    with torch.no_grad():
        ref, _ = _default_then_side(dev, delay, pipeline, dict(x=T(x_np, dev)), "k-NN graph + 12 modes")
    assert ref[0].shape[0] == 2 and ref[3].shape == (n, 12) and abs(float(ref[2][0])) < 1e-3      # a connected curve: lambda_0 = 0


def test_bernoulli_laplace_fit_under_a_side_stream(mgp, golden, dev, delay):
    import warnings
    from manifold_gp_amd.classification import laplace_fit
    from test_gpu_laplace import _problem
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)

    def fit(y):
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=".*not converged.*")
            f = laplace_fit(p["desc"], y, p["observed"], max_newton=3)
        return f.mean, f.iterations, f.history

    ref, _ = _default_then_side(dev, delay, fit, dict(y=p["y"]), "laplace_fit, three Newton steps")
    assert ref[1] == 3 and len(ref[2]) == 3


def test_sampling_under_a_side_stream(mgp, dumbbell, dev, delay):
    from manifold_gp_amd import sampling
    desc = mgp.operators.PrecisionMaternOperator(dumbbell["randomwalk"], 2, torch.tensor([[dumbbell["kappa"]]], device=dev)) \
        ._descriptor().with_(scale=0.7)

    def draw(y):
        return sampling.prior_samples(desc, 4, 4242), sampling.posterior_samples(desc, y, 1e-2, 4, 4242)

    ref, _ = _default_then_side(dev, delay, draw, dict(y=dumbbell["y"]), "prior and posterior samples, S = 4")
    assert ref[0].shape == (4, dumbbell["n"]) and ref[1].shape == (4, dumbbell["n"])


# ---------------------------------------------------------------------------------------------------------------- scratch cache
def test_scratch_is_kept_per_stream(dev):
    tag = "stream-order-test"
    _lib.release_workspace(tag)
    a = _lib.workspace(1000, tag, dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        b = _lib.workspace(1000, tag, dev)
        assert _lib.workspace(500, tag, dev) is b                               # the same stream: the same buffer
    assert _lib.workspace(1000, tag, dev) is a and a is not b
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    assert lo_a + a.numel() <= lo_b or lo_b + b.numel() <= lo_a, "the two streams' scratch buffers overlap"
    assert _lib.workspace_bytes(tag, dev) == a.numel() + b.numel()
    with torch.cuda.stream(side):
        grown = _lib.workspace(4 * b.numel(), tag, dev)                         # outgrown on the side stream: the default stream's stays
    assert grown.numel() >= 4 * b.numel() and _lib.workspace(1000, tag, dev) is a
    _lib.release_workspace(tag)
    assert _lib.workspace_bytes(tag, dev) == 0 and not [k for k in _lib._WORK if k[0] == tag]
