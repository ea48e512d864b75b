"""The plan of a CG solve (manifold_gp_amd/csrc/cg_policy.h over mgp_arena.h) on the CPU: both headers compile with a host
compiler alone, so a small C++ probe calls the functions the driver in cg.hip calls -- cg_choose, cg_carve over a counting and
over a real arena, cg_workspace_bytes and the rules of the graph driver -- and prints what they return.

The assertions are the contracts of docs/kernels/cg.md ("Plan policy"): what the kernels need of a grid and of each buffer,
stated here from the kernels' indexing, never a transliteration of the rules.  Two tables are recorded from the parent of the
change that introduced the header: the choices at default knobs and the old hand-written workspace formula, which the
carved size must never exceed."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

PROBE = r"""
#include <stdio.h>
#include <sys/mman.h>
#include "cg_policy.h"

static bool rdi(int* v) { return scanf("%d", v) == 1; }

// shape: n world is_dist C nb_loc nb4 minv pre post form nu noise_scale stop_mode tile_plan
static bool read_shape(CgShape* s) {
  long long n; int d, mi, pr, po, tp; double cc;
  if (scanf("%lld", &n) != 1 || !rdi(&s->world) || !rdi(&d) || !rdi(&s->C) || !rdi(&s->nb_loc) || !rdi(&s->nb4) || !rdi(&mi) || !rdi(&pr) ||
      !rdi(&po) || !rdi(&s->form) || !rdi(&s->nu) || scanf("%lf", &cc) != 1 || !rdi(&s->stop_mode) || !rdi(&tp)) return false;
  s->n = n; s->is_dist = d != 0; s->has_minv = mi != 0; s->has_pre = pr != 0; s->has_post = po != 0; s->noise_scale = (float)cc;
  s->tile_plan = tp != 0;
  return true;
}
// knobs: complex_shift reduce_once update_quads poll_spin init_free decide_in_update
static bool read_knobs(CgKnobs* k) {
  return rdi(&k->complex_shift) && rdi(&k->reduce_once) && rdi(&k->update_quads) && rdi(&k->poll_spin) && rdi(&k->init_free) &&
         rdi(&k->decide_in_update);
}

static int carve(const CgShape& sh, const CgChoice& ch) {
  const size_t counted = cg_workspace_bytes(sh, ch);
  MgpArena count;
  CgBuffers nb;
  cg_carve(count, sh, ch, &nb);
  const bool count_null = !nb.x && !nb.arrive && !nb.pd_bb && !nb.work64 && !nb.sc;
  // a real arena over exactly the counted bytes.  The arena never touches its memory, so the range is only reserved
  char* base = (char*)mmap(nullptr, counted, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (base == (char*)MAP_FAILED) return 1;
  MgpArena ar(base, counted);
  CgBuffers b;
  cg_carve(ar, sh, ch, &b);
  const void* p[] = {b.x, b.r, b.ubuf, b.w, b.p, b.s, b.usbuf, b.op_work, b.pd_gamma, b.pd_rr, b.pd_delta, b.blk, b.tot, b.xacc, b.rbuf,
                     b.tbuf, b.rpart, b.xacc64, b.t64, b.work64, b.rpart64, b.cz, b.cr, b.cp, b.cs, b.u4, b.w4, b.y4, b.op_work4, b.pd4,
                     b.pd_g, b.sc, b.pd_bb, b.arrive};
  printf("V %zu %zu %zu %d %d %zu %zu", counted, count.off, ar.off, ar.ok() ? 1 : 0, count_null ? 1 : 0, b.op_work_bytes, b.op_work4_bytes);
  for (const void* q : p) printf(" %lld", q ? (long long)((const char*)q - base) : -1LL);
  printf("\n");
  munmap(base, counted);
  return 0;
}

int main(void) {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'c' || cmd == 'v') {
      CgShape sh{}; CgKnobs k;
      if (!read_shape(&sh) || !read_knobs(&k)) return 1;
      const CgChoice c = cg_choose(sh, k);
      if (cmd == 'c')
        printf("C %d %d %d %d %lld %d %d %d %d %d %d %d\n", c.TC, c.TS, c.CQ, c.TSQ, (long long)c.rows_per_block, c.nbv, c.nbs,
               c.reduce_once ? 1 : 0, c.upd_quads, c.c1_family ? 1 : 0, c.cx ? 1 : 0, c.init_free ? 1 : 0);
      else if (carve(sh, c)) return 1;
    } else if (cmd == 'k') {
      printf("K %d %d %d %d %d %d %d %d %zu\n", kBlock, kMaxC, kMaxGridVec, kMaxPartials, kReduceOnceAbove, kC1GammaSlots, kC1DeltaSlots,
             kCxDeltaSlots, kStampWords);
    } else if (cmd == 'f') {            // first length: last_need chunk
      int a, b; if (!rdi(&a) || !rdi(&b)) return 1;
      printf("F %d\n", cg_first_len(a, b));
    } else if (cmd == 'd') {            // the last step decides: len is_dist c1_family
      int a, b, c; if (!rdi(&a) || !rdi(&b) || !rdi(&c)) return 1;
      printf("D %d\n", cg_last_step_decides(a, b != 0, c != 0) ? 1 : 0);
    } else if (cmd == 'r') {            // re-capture: need len_first last_need
      int a, b, c; if (!rdi(&a) || !rdi(&b) || !rdi(&c)) return 1;
      printf("R %d\n", cg_recapture_first(a, b, c) ? 1 : 0);
    } else if (cmd == 'e') {            // eager chunk: first chunk
      int a, b; if (!rdi(&a) || !rdi(&b)) return 1;
      printf("E %d\n", cg_eager_len(a != 0, b));
    } else if (cmd == 'g') {            // guard: max_iter chunk
      int a, b; if (!rdi(&a) || !rdi(&b)) return 1;
      printf("G %d\n", cg_guard_chunks(a, b));
    } else if (cmd == 'b') {            // poll budget: last_solve_ns
      long long a; if (scanf("%lld", &a) != 1) return 1;
      printf("B %lld\n", (long long)cg_poll_budget_ns(a));
    } else return 1;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("cg_policy")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.check_output([str(exe)], input="\n".join(lines) + "\n", text=True)
        rows = [ln.split() for ln in out.strip().splitlines()]
        assert len(rows) == len(lines), (len(rows), len(lines))
        return rows
    return run


@pytest.fixture(scope="module")
def K(probe):
    t = probe(["k"])[0]
    assert t[0] == "K"
    names = ("kBlock", "kMaxC", "kMaxGridVec", "kMaxPartials", "kReduceOnceAbove", "kC1GammaSlots", "kC1DeltaSlots", "kCxDeltaSlots",
             "kStampWords")
    k = dict(zip(names, (int(v) for v in t[1:])))
    # the kernels are written for these: 256-thread workgroups of four waves, shared arrays of kMaxC columns
    assert k["kBlock"] == 256 and k["kMaxC"] == 256 and k["kStampWords"] == 0, k
    return k


NS = (1, 255, 256, 257, 4097, 60000, 200000)
CS = (1, 2, 3, 4, 12, 16, 17, 20, 64, 255, 256)
WORLDS = (1, 4)
NB_LOCS = (1, 235, 4096)
DEFAULT_KNOBS = dict(complex_shift=1, reduce_once=1, update_quads=1, poll_spin=64, init_free=1, decide_in_update=1)
# the shape every C == 1 feature accepts (complex shift and, with that knob off, the init-free start) ...
ELIGIBLE = dict(nb4=940, minv=0, pre=0, post=0, form=2, nu=2, cc=0.007, stop_mode=1, tile=1)
# ... and shapes that each break one of their conditions
VARIANTS = [ELIGIBLE] + [dict(ELIGIBLE, **d) for d in (
    dict(minv=1), dict(pre=1), dict(post=1), dict(form=0), dict(form=3), dict(nu=1), dict(cc=0.0), dict(stop_mode=0), dict(tile=0),
    dict(nb4=0), dict(nb4=4097), dict(form=1, nu=3, tile=0, stop_mode=0))]


def _shape(n, C, world, nb_loc, is_dist=None, **v):
    v = dict(ELIGIBLE, **v)
    is_dist = (world > 1) if is_dist is None else is_dist
    nb4 = v["nb4"] if (C == 1 and not is_dist) else 0            # the driver's rule for nb4
    return dict(n=n, world=world, is_dist=int(is_dist), C=C, nb_loc=nb_loc, nb4=nb4, minv=v["minv"], pre=v["pre"], post=v["post"],
                form=v["form"], nu=v["nu"], cc=v["cc"], stop_mode=v["stop_mode"], tile=v["tile"])


def _text(cmd, sh, knobs):
    k = dict(DEFAULT_KNOBS, **knobs)
    return "%s %d %d %d %d %d %d %d %d %d %d %d %.9g %d %d  %d %d %d %d %d %d" % (
        cmd, sh["n"], sh["world"], sh["is_dist"], sh["C"], sh["nb_loc"], sh["nb4"], sh["minv"], sh["pre"], sh["post"], sh["form"],
        sh["nu"], sh["cc"], sh["stop_mode"], sh["tile"], k["complex_shift"], k["reduce_once"], k["update_quads"], k["poll_spin"],
        k["init_free"], k["decide_in_update"])


CHOICE = ("TC", "TS", "CQ", "TSQ", "rows_per_block", "nbv", "nbs", "reduce_once", "upd_quads", "c1_family", "cx", "init_free")


def _choices(probe, shapes_knobs):
    rows = probe([_text("c", sh, kn) for sh, kn in shapes_knobs])
    assert all(r[0] == "C" for r in rows)
    return [dict(zip(CHOICE, (int(v) for v in r[1:]))) for r in rows]


def _grid():
    for n, C, world, nb_loc in itertools.product(NS, CS, WORLDS, NB_LOCS):
        dists = (False, True) if world == 1 else (True,)      # a row-partitioned plan may have a single rank
        for is_dist in dists:
            yield n, C, world, nb_loc, is_dist


def test_choice_invariants_over_the_grid(probe, K):
    """What the kernels need of every choice, at every knob setting."""
    cases = []
    for (n, C, world, nb_loc, is_dist), ro, quads, v in itertools.product(_grid(), (0, 1, 2), (0, 1), VARIANTS):
        if C > 1 and v is not ELIGIBLE and v is not VARIANTS[-1]:
            continue                                              # the single-column conditions do not bear on C > 1
        cases.append((_shape(n, C, world, nb_loc, is_dist, **v), dict(reduce_once=ro, update_quads=quads)))
    B = K["kBlock"]
    seen = dict(cx=0, init_free=0, quads=0, reduce_once=0, c1=0, capped=0)
    for (sh, kn), c in zip(cases, _choices(probe, cases)):
        ctx = (sh, kn, c)
        n, C = sh["n"] * sh["world"], sh["C"]
        assert c["TC"] >= C and c["TC"] & (c["TC"] - 1) == 0 and c["TC"] < 2 * C, ctx          # least power of two >= C
        assert c["TC"] * c["TS"] == B, ctx
        rpb, nbv = c["rows_per_block"], c["nbv"]
        assert nbv * rpb >= n and (nbv - 1) * rpb < n, ctx                                    # the grid covers the rows, no idle workgroup
        assert rpb % (c["TSQ"] if c["upd_quads"] else c["TS"]) == 0, ctx
        assert 1 <= nbv <= K["kMaxPartials"], ctx
        assert c["nbs"] == sh["nb_loc"] * sh["world"], ctx
        if c["c1_family"]:
            assert C == 1 and nbv <= K["kC1GammaSlots"] * B and c["nbs"] <= K["kC1DeltaSlots"] * B, ctx
        if c["upd_quads"]:
            assert C % 4 == 0 and c["reduce_once"] and c["CQ"] == C // 4 and c["TSQ"] >= 1 and c["CQ"] * c["TSQ"] <= B, ctx
            assert c["upd_quads"] == B, ctx                       # the only instantiation launched (cg_update_q_kernel<kBlock>)
        if c["reduce_once"]:
            assert C > 1 and kn["reduce_once"] and (C > K["kReduceOnceAbove"] or kn["reduce_once"] == 2), ctx
        if c["init_free"]:
            assert c["c1_family"] and not sh["is_dist"] and not sh["minv"] and not c["cx"] and sh["form"] in (0, 2) and sh["tile"], ctx
        if c["cx"]:
            assert C == 1 and not sh["is_dist"] and not (sh["minv"] or sh["pre"] or sh["post"]) and sh["form"] == 2 and sh["nu"] == 2, ctx
            assert sh["cc"] > 0 and sh["stop_mode"] == 1 and 1 <= sh["nb4"] <= K["kCxDeltaSlots"] * B and c["c1_family"], ctx
        seen["cx"] += c["cx"]; seen["init_free"] += c["init_free"]; seen["quads"] += bool(c["upd_quads"])
        seen["reduce_once"] += c["reduce_once"]; seen["c1"] += c["c1_family"]; seen["capped"] += rpb > max(c["TS"], c["TSQ"])
    assert all(v > 0 for v in seen.values()), seen               # every feature and the grid cap occur somewhere on the grid
    print(len(cases), "choices", seen)


def test_a_knob_turns_off_its_own_feature_only(probe):
    """Against the choice at default knobs: update_quads = 0 takes the quad form away and leaves the reduction scheme; reduce_once
    = 0 takes cg_reduce_kernel away (and with it the quad form, which runs behind it only); complex_shift = 0 and init_free = 0 take
    their start away and leave the grid alone -- without the complex shift the plan may start init-free instead; poll_spin and
    decide_in_update choose nothing."""
    base = [_shape(n, C, world, nb_loc, is_dist, **v) for (n, C, world, nb_loc, is_dist), v in itertools.product(_grid(), VARIANTS[:2])]
    D = _choices(probe, [(sh, {}) for sh in base])
    grid_fields = ("TC", "TS", "CQ", "TSQ", "rows_per_block", "nbv", "nbs", "reduce_once", "upd_quads", "c1_family")
    for knob, own in (("update_quads", "upd_quads"), ("reduce_once", "reduce_once"), ("complex_shift", "cx"), ("init_free", "init_free"),
                      ("poll_spin", None), ("decide_in_update", None)):
        for sh, d, c in zip(base, D, _choices(probe, [(sh, {knob: 0}) for sh in base])):
            ctx = (knob, sh, d, c)
            if own is None:
                assert c == d, ctx
                continue
            assert not c[own], ctx
            if not d[own]:
                assert c == d, ctx                                # the feature was not in use: nothing changes
            if knob == "update_quads":
                assert {k: c[k] for k in CHOICE if k not in ("upd_quads", "TSQ", "rows_per_block", "nbv")} == \
                       {k: d[k] for k in CHOICE if k not in ("upd_quads", "TSQ", "rows_per_block", "nbv")}, ctx
            elif knob == "reduce_once":
                assert not c["upd_quads"] and all(c[k] == d[k] for k in ("TC", "TS", "nbs", "c1_family", "cx", "init_free")), ctx
            elif knob == "complex_shift":
                assert all(c[k] == d[k] for k in grid_fields), ctx
                assert c["init_free"] == d["init_free"] or d["cx"], ctx
            else:
                assert all(c[k] == d[k] for k in grid_fields + ("cx",)), ctx


# n, C, knobs -> reduce_once, upd_quads, CQ, TSQ, rows_per_block, nbv: recorded from plan_create_impl as it stood before cg_policy.h
RECORDED = [
    (60000, 1, {}, (0, 0, None, None, 256, 235)),
    (200000, 1, {}, (0, 0, None, None, 512, 391)),
    (60000, 12, {}, (0, 0, None, None, 240, 250)),
    (60000, 12, dict(reduce_once=2), (1, 256, 3, 85, 85, 706)),
    (60000, 17, {}, (1, 0, None, None, 32, 1875)),
    (60000, 20, {}, (1, 256, 5, 51, 51, 1177)),
    (60000, 64, {}, (1, 256, 16, 16, 32, 1875)),
    (60000, 256, {}, (1, 256, 64, 4, 32, 1875)),
]


def test_recorded_choices_at_default_knobs(probe):
    got = _choices(probe, [(_shape(n, C, 1, 235), kn) for n, C, kn, _ in RECORDED])
    for (n, C, kn, (ro, uq, cq, tsq, rpb, nbv)), c in zip(RECORDED, got):
        assert (c["reduce_once"], c["upd_quads"], c["rows_per_block"], c["nbv"]) == (ro, uq, rpb, nbv), (n, C, kn, c)
        if uq:
            assert (c["CQ"], c["TSQ"]) == (cq, tsq), (n, C, kn, c)


BUFFERS = ("x", "r", "ubuf", "w", "p", "s", "usbuf", "op_work", "pd_gamma", "pd_rr", "pd_delta", "blk", "tot", "xacc", "rbuf", "tbuf", "rpart",
           "xacc64", "t64", "work64", "rpart64", "cz", "cr", "cp", "cs", "u4", "w4", "y4", "op_work4", "pd4", "pd_g", "sc", "pd_bb", "arrive")
CX_BUFFERS = ("cz", "cr", "cp", "cs", "u4", "w4", "y4", "op_work4", "pd4", "pd_g", "sc")


def _align(x, a=256):
    return (x + a - 1) // a * a


def _parent_bytes(K, n_loc, C, world, nb_loc):
    """cg_bytes() as it was written out by hand before the workspace was carved once: the recorded cap."""
    nc = _align(n_loc * world * C * 4)
    nbs = nb_loc * world
    b = 10 * nc
    b += 4 * nc + 256
    b += 4 * _align(K["kMaxPartials"] * C * 4)
    b += 2 * _align(nbs * C * 4)
    b += _align((6 * C + 16 + 1024 + 8192) * 4)
    b += _align(3 * C * 4)
    b += _align(9 * 32 * 4)
    b += _align(256 * C * 2 * 4)
    b += 6 * 2 * nc + _align(256 * C * 2 * 8)
    if C == 1 and world == 1:
        b += 4 * _align(n_loc * 8) + 3 * _align(n_loc * 16) + 4 * _align(n_loc * 16) + 256
        b += _align(K["kCxDeltaSlots"] * K["kBlock"] * 4 * 4) + _align(2 * K["kMaxGridVec"] * 4 * 4) + 256
    return b + 1024


def _needed_bytes(K, sh, v):
    """Bytes each buffer must hold, from the indexing of the kernels and of the operator chain that use it (CgArgs, CxArgs, the
    refinement kernels of cg.hip)."""
    C, nn = sh["C"], sh["n"] * sh["world"]
    nc, nbs = nn * C, sh["nb_loc"] * sh["world"]
    need = dict.fromkeys(("x", "r", "ubuf", "w", "p", "s", "usbuf", "xacc", "rbuf", "tbuf"), 4 * nc)      # [n, C] float vectors
    need["op_work"] = v["op_work_bytes"]
    assert v["op_work_bytes"] >= 4 * 4 * nc, (sh, v)                         # four chain buffers of global length
    need["pd_gamma"] = need["pd_rr"] = 4 * 2 * K["kMaxPartials"] * C          # [2][nbv <= kMaxPartials][C]
    need["pd_delta"] = need["pd_bb"] = 4 * nbs * C                            # [nbs][C]
    need["blk"] = 4 * (6 * C + 16)                                            # gamma_old[2] alpha_old[2] bb resid [C] + 16 state words
    need["tot"] = 4 * 3 * C
    need["rpart"] = 4 * 256 * C * 2                                           # 256 refinement workgroups x {||r||^2, ||b||^2} x C
    need["xacc64"] = need["t64"] = 8 * nc
    need["work64"] = 8 * 4 * nc
    need["rpart64"] = 8 * 256 * C * 2
    need["arrive"] = 4 * 9 * 32
    if sh["C"] == 1 and not sh["is_dist"]:
        need.update(dict.fromkeys(("cz", "cr", "cp", "cs"), 8 * nn))           # float2 [n]
        need.update(dict.fromkeys(("u4", "w4", "y4"), 16 * nn))                # float4 [n]
        need["op_work4"] = v["op_work4_bytes"]
        assert v["op_work4_bytes"] >= 4 * 16 * nn, (sh, v)
        need["pd4"] = 4 * K["kCxDeltaSlots"] * K["kBlock"] * 4                # [nbs4 <= slots * kBlock][4]
        need["pd_g"] = 4 * 2 * K["kMaxGridVec"] * 4                           # [2][nbv <= kMaxGridVec][4]
        need["sc"] = 4 * 9                                                    # {gamma_old, alpha_old} re im x 2 parities, ||b||^2
    return need


def test_carving_over_the_grid(probe, K):
    """A real arena over exactly the counted bytes hands out every buffer, 256-byte aligned, pairwise disjoint, inside the
    workspace and as long as its kernels index; the counted size covers the walk and never exceeds the old formula."""
    shapes = [_shape(n, C, world, nb_loc, is_dist) for n, C, world, nb_loc, is_dist in _grid()]
    rows = probe([_text("v", sh, {}) for sh in shapes])
    for sh, r in zip(shapes, rows):
        assert r[0] == "V"
        v = dict(counted=int(r[1]), count_off=int(r[2]), used=int(r[3]), ok=int(r[4]), count_null=int(r[5]), op_work_bytes=int(r[6]),
                 op_work4_bytes=int(r[7]))
        off = dict(zip(BUFFERS, (int(t) for t in r[8:])))
        assert len(r) == 8 + len(BUFFERS)
        ctx = (sh, v, off)
        assert v["ok"] and v["count_null"], ctx                    # the counting arena returns null, the real one is not exhausted
        assert v["used"] == v["count_off"] <= v["counted"], ctx    # both arenas walk the same bytes; the count covers them
        assert v["counted"] <= _parent_bytes(K, sh["n"], sh["C"], sh["world"], sh["nb_loc"]), ctx
        need = _needed_bytes(K, sh, v)
        has_cx = sh["C"] == 1 and not sh["is_dist"]
        for name in BUFFERS:
            if name in CX_BUFFERS and not has_cx:
                assert off[name] == -1, (name, ctx)
            else:
                assert off[name] >= 0 and off[name] % 256 == 0, (name, ctx)
        spans = sorted((off[name], off[name] + need[name], name) for name in need)
        assert len(spans) == len(BUFFERS) - (0 if has_cx else len(CX_BUFFERS))
        for (a0, a1, na), (b0, b1, nb) in zip(spans, spans[1:]):
            assert a1 <= b0, (na, nb, ctx)                         # disjoint, each long enough
        assert spans[-1][1] <= v["used"], (spans[-1], ctx)
    # the layout is the parent's: the same order of takes, so every offset of the flagship plan is where it was
    sh = _shape(60000, 1, 1, 235)
    r = probe([_text("v", sh, {})])[0]
    off = dict(zip(BUFFERS, (int(t) for t in r[8:])))
    assert [n for _, n in sorted((o, n) for n, o in off.items())] == list(BUFFERS), off
    assert off["x"] == 0 and off["r"] == _align(240000) and off["op_work"] == 7 * _align(240000), off


def test_graph_rules(probe):
    """The rules of the graph driver, on the cases their comments describe."""
    rows = probe(["r 7 5 3", "r 4 5 9", "r 4 5 4", "r 65 5 65", "r 65 5 3", "r 5 5 5", "r 0 5 0",
                  "f 0 10", "f 0 2", "f 7 10", "f 64 10", "f 65 10",
                  "d 1 0 1", "d 2 0 1", "d 2 1 1", "d 2 0 0", "d 5 0 1",
                  "e 1 10", "e 0 10", "e 1 2", "e 0 2",
                  "g 1000 10", "g 1000 2", "g 1 10", "b 0", "b 100000"])
    got = [int(r[1]) for r in rows]
    # re-capture: longer than the captured graph -> at once; shorter once -> no; shorter twice with the same value -> yes;
    # beyond 64 steps (no single-graph form) never; the captured length itself and an undecided solve (need 0): no
    assert got[:7] == [1, 0, 1, 0, 0, 0, 0], got[:7]
    # first length: what the eager solve needed when that is 1..64, else min(chunk, 4)
    assert got[7:12] == [4, 2, 7, 64, 4], got[7:12]
    # the last step only decides from two steps up, on single-GPU plans of the single-column family
    assert got[12:17] == [0, 1, 0, 0, 1], got[12:17]
    assert got[17:21] == [4, 10, 2, 2], got[17:21]                 # eager chunk: the first one is cut to 4 bodies
    # the guard lets max_iter steps run: every chunk runs at least min(chunk, 4) of them
    for (mi, ch), g in zip(((1000, 10), (1000, 2), (1, 10)), got[21:24]):
        assert g * min(ch, 4) >= mi and g >= 1, (mi, ch, g)
    assert got[24] == 2000000 and got[25] == 3000000, got[24:]     # ten times the last decided solve, at least 2 ms
