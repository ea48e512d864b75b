"""The guard-band helper and the registry of the memory contract, checked without a GPU.

1. The helper on CPU tensors: Python "entry points" that each commit one defect must be reported by exactly the matching check of
   _guarded.run_contract -- the evidence that tests/test_gpu_memory_contract.py fails on a kernel with that defect.
2. Completeness: CASES, COVERED_BY, EXEMPT and PENDING of _entry_cases are a partition of _lib.SIGNATURES.
3. Refusals return before any launch, so the library loads here: a workspace one byte short is MGP_ERR_WORKSPACE.
4. The host-side parts of the stream-order run (_guarded.run_stream_order, tests/test_gpu_stream_order.py): the decoy keeps integer
   arrays and rolls float arrays, constant arrays have no decoy, the sync hook is restored after an exception.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guarded as G                      # noqa: E402
import _entry_cases as E                  # noqa: E402
from manifold_gp_amd import _lib          # noqa: E402

CPU = torch.device("cpu")


# --------------------------------------------------------------------------------------------------------------- the fakes
def fake(defect):
    """out[i] = 2 x[i] + 1 through a workspace of n floats; sums[0..2] = (sum x, sum out, n).  `defect` plants one fault."""
    def case(carve, shape):
        n = shape["n"]
        x = carve("x", torch.float32, n, "in", np.arange(1, n + 1, dtype=np.float32))
        out = carve("out", torch.float32, n, "out")
        sums = carve("sums", torch.float64, 3, "out")                       # the caller is promised three entries
        wsp = carve("work", torch.uint8, 4 * n, "work", floor=8)
        arena_bytes = getattr(getattr(carve, "__self__", None), "mem", None)   # the whole arena, for the out-of-bounds fakes

        def at(view, index):
            """Element `index` of `view`, any index: the fake's stray pointer arithmetic."""
            isz = view.element_size()
            off = view.data_ptr() - arena_bytes.data_ptr() + index * isz
            return arena_bytes[off:off + isz].view(view.dtype)

        def run(work_bytes):
            if work_bytes is not None and work_bytes < 4 * n:
                return G.ERR_WORKSPACE, {}
            w = wsp.view(torch.float32)
            if defect == "stale_workspace":
                w[:n - 1] = 2 * x[:n - 1]                                    # w[n - 1] is what the last caller left
            else:
                w[:] = 2 * x
            if defect == "unwritten":
                out[:n - 1] = w[:n - 1] + 1                                  # the last entry of the extent is left out
            else:
                out[:] = w + 1
            if defect == "past_output":
                at(out, n)[:] = 7.0
            if defect == "before_output":
                at(out, -1)[:] = 7.0
            if defect == "over_read":
                out[n - 1] += at(x, n)[0] * 1e-3
            if defect == "modify_input":
                x[0] = -x[0]
            sums[0], sums[1], sums[2] = float(x.double().sum()), float(out[:n - 1].double().sum()), float(n)
            if defect == "sums3":
                at(sums, 3)[:] = 1.0
            return 0, {}
        return G.Call(run, query=4 * n, extent={"out": n, "sums": 3})
    return case


EXPECT = {"correct": None, "past_output": "guards", "before_output": "guards", "stale_workspace": "fill", "over_read": "fill",
          "modify_input": "inputs", "sums3": "guards", "unwritten": "extent"}


@pytest.mark.parametrize("defect", sorted(EXPECT))
@pytest.mark.parametrize("n", [1, 5, 257])
def test_planted_defect_is_reported_by_its_own_check(defect, n):
    found = G.run_contract(fake(defect), dict(n=n), CPU)
    hit = {c for c in G.CHECKS if found[c]}
    want = set() if EXPECT[defect] is None else {EXPECT[defect]}
    assert hit == want, "%s: reported %s, expected %s\n%s" % (defect, sorted(hit), sorted(want), G.report(found))
    if want:
        # under both fills and both placements: one message per combination the check sees
        msgs = found[EXPECT[defect]]
        per = {"guards": 4, "inputs": 4, "fill": 2, "extent": 2}[EXPECT[defect]]
        assert len(msgs) == per, G.report(found)
        for placement in G.PLACEMENTS:
            assert any(m.startswith(placement) for m in msgs), G.report(found)


def test_check_names_the_array_and_the_offset():
    rec = G.Recorder()
    fake("correct")(rec, dict(n=5))
    for placement in G.PLACEMENTS:
        arena = G.Arena(rec.specs, placement, G.LO, G.HI, CPU)
        assert arena.check() == []
        out, sums = arena.spec("out"), arena.spec("sums")
        assert out.start % 256 == (0 if placement == "aligned" else 4) and sums.start % 256 == (0 if placement == "aligned" else 8)
        assert arena.spec("work").start % 256 == (0 if placement == "aligned" else 8)
        assert sums.start - (out.start + out.nbytes) >= G.GUARD and arena.specs[0].start >= G.GUARD
        assert arena.size - (arena.specs[-1].start + arena.specs[-1].nbytes) == G.GUARD
        arena.mem[out.start + out.nbytes] = 1                                # the byte after the last element is guard already
        arena.mem[out.start + out.nbytes + 11] = 1
        arena.mem[sums.start - 3] = 1
        got = arena.check()
        assert got == [dict(array="out", side="after", first=0, last=11, count=2),
                       dict(array="sums", side="before", first=-3, last=-3, count=1)], got
        assert "out" in G.describe(got) and "+11" in G.describe(got)
        # a stray write cannot match both fills
        other = G.Arena(rec.specs, placement, G.HI, G.LO, CPU)
        other.mem[out.start + out.nbytes] = 0xFF
        arena2 = G.Arena(rec.specs, placement, G.LO, G.HI, CPU)
        arena2.mem[out.start + out.nbytes] = 0xFF
        assert bool(other.check()) != bool(arena2.check())


def test_short_workspace_must_be_refused_and_touch_nothing():
    def sloppy(carve, shape):
        call = fake("correct")(carve, shape)
        inner = call.run
        call.run = lambda work_bytes: inner(None)                            # ignores the size it is given
        return call
    found = G.run_contract(sloppy, dict(n=5), CPU)
    assert {c for c in G.CHECKS if found[c]} == {"short"}, G.report(found)


# ------------------------------------------------------------------------------------------- stream order: the host-side parts
def test_decoy_rolls_float_inputs_and_keeps_everything_else():
    def case(carve, shape):
        n = shape["n"]
        carve("x", torch.float32, n, "in", np.arange(1, n + 1, dtype=np.float32))
        carve("acc", torch.float64, n, "inout", np.linspace(0.5, 2.0, n))
        carve("ones", torch.float32, n, "in", np.ones(n))                              # constant: its roll is itself
        carve("col", torch.int32, n, "in", np.arange(n)[::-1])
        carve("mask", torch.uint8, n, "in", np.arange(n) % 2)
        carve("out", torch.float32, n, "out")
        carve("work", torch.uint8, 64, "work", floor=8)
        return G.Call(lambda work_bytes: (0, {}))
    rec = G.Recorder()
    case(rec, dict(n=5))
    arena = G.Arena(rec.specs, "aligned", G.HI, G.LO, CPU)
    true = arena.mem.numpy().copy()
    image, differ, constant = G.decoy_image(arena.specs, true)
    assert differ == ["x", "acc"] and constant == ["ones"]
    assert (true == arena.mem.numpy()).all(), "the true image is left alone"
    part = lambda img, name, dt: img[arena.spec(name).start:arena.spec(name).start + arena.spec(name).nbytes].view(dt)
    assert part(image, "x", np.float32).tolist() == [5.0, 1.0, 2.0, 3.0, 4.0]
    assert part(image, "acc", np.float64).tolist() == np.roll(np.linspace(0.5, 2.0, 5), 1).tolist()
    changed = np.nonzero(image != true)[0]
    inside = np.zeros(true.size, bool)
    for name in ("x", "acc"):
        inside[arena.spec(name).start:arena.spec(name).start + arena.spec(name).nbytes] = True
    assert changed.size and inside[changed].all(), "only the float inputs differ: indices, masks, guards, outputs and workspace are true"
    assert (part(image, "out", np.uint8) == G.LO).all() and (part(image, "work", np.uint8) == G.LO).all()
    # a decoy is a valid input: every value of it is a value of the true array
    assert sorted(part(image, "x", np.float32).tolist()) == sorted(part(true, "x", np.float32).tolist())
    # one element: no decoy either
    rec1 = G.Recorder()
    case(rec1, dict(n=1))
    one = G.Arena(rec1.specs, "aligned", G.HI, G.LO, CPU)
    assert G.decoy_image(one.specs, one.mem.numpy())[1:] == ([], ["x", "acc", "ones"])


def test_every_registered_case_builds_a_decoy_from_its_own_values():
    """Over the whole registry, on host stand-ins: integer arrays never change, and the cases without any decoy are the ones
    docs/stream_contract.md lists (one-element shapes and the integer-only graph_tiles / bfs_order)."""
    doc = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "docs", "stream_contract.md")).read()
    none = set()
    for name, fam, sid in E.params():
        case = E.CASES[name]
        rec = G.Recorder()
        case.fn(rec, case.shapes_of(fam)[sid])
        arena = G.Arena(rec.specs, "aligned", G.HI, G.LO, CPU)
        true = arena.mem.numpy().copy()
        image, differ, constant = G.decoy_image(arena.specs, true)
        for s in arena.specs:
            if s.name not in differ:
                assert (image[s.start:s.start + s.nbytes] == true[s.start:s.start + s.nbytes]).all(), (name, sid, s.name)
        if not differ:
            none.add(name)
            assert all(s.numel <= 1 or not G.carries_decoy(s) or s.name in constant for s in arena.specs)
    for name in none:
        assert "`%s`" % name in doc.split("## Cases without a decoy")[1].split("##")[0], name


def test_sync_hook_runs_behind_the_sync_and_is_restored_after_an_exception():
    calls = []
    assert E.SYNC_HOOK is None
    with G.sync_hook(E, lambda: calls.append(1)):
        E._sync()
        E._sync()
    assert calls == [1, 1] and E.SYNC_HOOK is None
    with pytest.raises(RuntimeError, match="planted"):
        with G.sync_hook(E, lambda: calls.append(2)):
            E._sync()
            raise RuntimeError("planted")
    assert calls == [1, 1, 2] and E.SYNC_HOOK is None
    E._sync()
    assert calls == [1, 1, 2]

    def failing():
        raise RuntimeError("planted in the hook")
    with pytest.raises(RuntimeError, match="in the hook"):
        with G.sync_hook(E, failing):
            E._sync()
    assert E.SYNC_HOOK is None
    outer = lambda: calls.append(3)
    with G.sync_hook(E, outer):                                                    # nested: the outer hook comes back
        with G.sync_hook(E, lambda: calls.append(4)):
            E._sync()
        assert E.SYNC_HOOK is outer
    assert E.SYNC_HOOK is None and calls[-1] == 4


def test_scratch_key_names_the_stream_on_the_host_too():
    tag = "stream-order-cpu"
    a = _lib.workspace(100, tag, CPU)
    assert _lib.workspace(50, tag, CPU) is a and [k for k in _lib._WORK if k[0] == tag] == [(tag, "cpu", 0)]
    assert _lib.workspace_bytes(tag, CPU) == a.numel()
    _lib.release_workspace(tag)
    assert _lib.workspace_bytes(tag, CPU) == 0


# ------------------------------------------------------------------------------------------------------------ completeness
def test_every_entry_point_is_a_case_part_of_one_exempt_or_pending():
    names = set(_lib.SIGNATURES)
    sets = {"CASES": set(E.CASES), "COVERED_BY": set(E.COVERED_BY), "EXEMPT": set(E.EXEMPT), "PENDING": set(E.PENDING)}
    assert set(E.COVERED_BY.values()) <= set(E.CASES)
    for a in sets:
        assert sets[a] <= names, "%s names no entry point: %s" % (a, sorted(sets[a] - names))
        for b in sets:
            if a < b:
                assert not sets[a] & sets[b], "%s and %s both hold %s" % (a, b, sorted(sets[a] & sets[b]))
    missing = names - set().union(*sets.values())
    assert not missing, "entry points without a case, an exemption or a pending note: %s" % sorted(missing)


def test_every_exemption_matches_a_category():
    for name, cat in E.EXEMPT.items():
        assert cat in E.EXEMPT_CATEGORIES and re.match(E.EXEMPT_CATEGORIES[cat], name), name
    # what launches device work on caller memory is never exempt by accident: no exempt signature but the communicator ones
    # and the benchmark loop takes both a device array and a stream
    for name in ("mgp_spmm_fused", "mgp_cg_solve", "mgp_knn_search", "mgp_pcg_plan_create", "mgp_blz_step"):
        assert name not in E.EXEMPT


def test_every_case_has_its_documentation_row():
    doc = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "docs", "memory_contract.md")).read()
    for name in list(E.CASES) + list(E.COVERED_BY) + list(E.PENDING) + list(E.EXEMPT):
        assert "`%s`" % name in doc, "docs/memory_contract.md has no row for %s" % name


# ---------------------------------------------------------------------------------------------------------------- refusals
def _smallest(case):
    return next(iter(case.shapes_of(next(iter(case.families))).values()))


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_one_byte_short_workspace_is_refused_before_any_launch(name):
    case = E.CASES[name]
    rec = G.Recorder()
    call = case.fn(rec, _smallest(case))
    if call.query == 0:
        return                            # nothing to refuse: the entry point takes no sized workspace at this shape
    arena = G.Arena(rec.specs, "aligned", G.LO, G.HI, CPU)
    call = case.fn(arena.carve, _smallest(case))
    rc, _ = call.run(call.query - 1)
    assert rc == G.ERR_WORKSPACE, "%s(work_bytes = %d - 1) returned %d" % (name, call.query, rc)
    assert arena.check() == [] and all(arena.changed(s.name) is None for s in arena.specs)
