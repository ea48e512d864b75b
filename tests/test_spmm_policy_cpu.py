"""The plan of an SpMM launch (manifold_gp_amd/csrc/spmm_policy.h) on the CPU: the header compiles with a host compiler alone, so
a small C++ probe calls what spmm.hip calls -- spmm_plan and the functions its entry points answer from -- and prints every field
of the plan.  Every device-pointer field of the descriptors the probe builds is an address inside a PROT_NONE mapping: the plan
may read the numbers of an mgp_csr_t and the host descriptor behind c1_tiles, never a device pointer, so a probe that runs to its
end is itself a check.

(a) The contracts of docs/kernels/spmm.md ("Plan policy"): what each kernel needs of its grid, LDS and tile set, stated here from
    the kernels' indexing, never a transliteration of the rules.
(b) A table recorded from the parent of the change that introduced the header (tests/golden/spmm_plan_table.rle.xz): the pair
    (mgp_spmm_kernel_choice, mgp_spmm_dot_blocks_csr) of the parent's library over the product the probe enumerates (table_rows),
    at every knob setting of KNOB_SETTINGS.  It was recorded by the probe's own enumeration (`t lib`), compiled against the parent's header with the
    balanced descriptor attached the way the parent carried it (behind tile_rowptr, tagged); nothing else differed.  The header
    (`t header`) and the library's two entry points (`t lib`) must reproduce it exactly.  One input changed on purpose and is
    therefore not a cell: "tile_rowptr alone + descriptor", which the parent could not tell from the descriptor itself, no longer
    exists -- the partial order of the table is tile_rowptr + tile_vals, which means the same on both sides
    (tests/test_host_cpu.py covers tile_rowptr alone).  Where the parent could not attach a descriptor at all (a CSR with a row
    order, whole or partial: the field was taken), the table holds the parent's answer without one and the new code, which can be
    handed both, must give that answer.

    The table has 99,878,400 cells; it is stored as the run lengths of the pair in enumeration order ("count choice dot_blocks"
    per line: 1.65 million runs), which xz takes to 8 KB, and compared as text, so a mismatch names the first differing run."""
import itertools
import lzma
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
TABLE = os.path.join(ROOT, "tests", "golden", "spmm_plan_table.rle.xz")

PROBE = r"""
#include <stdio.h>
#include <string.h>
#include <dlfcn.h>
#include <sys/mman.h>
#include <string>
#include <thread>
#include <vector>
#include "spmm_policy.h"

// ---- device pointers: distinct addresses inside one PROT_NONE mapping (a read through any of them ends the probe) ----
static char* g_dev;
enum { kPage = 4096, kShiftBase = 64 * kPage, kDevBytes = 64 << 20 };
static const void* dev(int id) { return g_dev + (size_t)id * kPage; }
static long long dev_id(const void* p) { return p ? (long long)((const char*)p - g_dev) / kPage : -1; }
// ids: 1 rowptr 2 col 3 vals 4 diag 5 tile_ptr 6 tile_cols 7 lid 8 tile_rowptr 9 tile_vals 10 tile_rowid 11 mt_sptr 12 mt_dcol 13 mt_img
//      20 set.tile_ptr 21 set.tile_cols 22 set.lid; set.rowptr_pad = g_dev + kShiftBase (id 64), tile_shift behind it

struct Csr { long long n, ncols; int tile_rows, max_cols, max_entries, lanes, ptrs, mt_tiles, mt_steps; };
struct Bal { int on; long long n; int tiles, max_cols, max_entries, ptrs; long long shift_delta; };

static void make(const Csr& c, const Bal& b, mgp_csr_t* L, mgp_c1_tiles_t* s) {
  memset(L, 0, sizeof(*L));
  memset(s, 0, sizeof(*s));
  L->n = c.n; L->ncols = c.ncols;
  L->rowptr = (const int32_t*)dev(1); L->col = (const int32_t*)dev(2); L->vals = (const float*)dev(3); L->diag = (const float*)dev(4);
  if (c.ptrs & 1) L->tile_ptr = (const int32_t*)dev(5);
  if (c.ptrs & 2) L->tile_cols = (const int32_t*)dev(6);
  if (c.ptrs & 4) L->lid = (const uint16_t*)dev(7);
  if (c.ptrs & 8) L->tile_rowptr = (const int32_t*)dev(8);
  if (c.ptrs & 16) L->tile_vals = (const float*)dev(9);
  if (c.ptrs & 32) L->tile_rowid = (const int32_t*)dev(10);
  if (c.ptrs & 64) L->mt_sptr = (const int32_t*)dev(11);
  if (c.ptrs & 128) L->mt_dcol = (const int32_t*)dev(12);
  if (c.ptrs & 256) L->mt_img = (const float*)dev(13);
  L->tile_rows = c.tile_rows; L->tile_max_cols = c.max_cols; L->tile_max_entries = c.max_entries; L->spmv_lanes = c.lanes;
  L->mt_tiles = c.mt_tiles; L->mt_steps = c.mt_steps;
  if (!b.on) return;
  s->n = b.n; s->tiles = b.tiles; s->max_cols = b.max_cols; s->max_entries = b.max_entries;
  if (b.ptrs & 1) s->tile_ptr = (const int32_t*)dev(20);
  if (b.ptrs & 2) s->tile_cols = (const int32_t*)dev(21);
  if (b.ptrs & 4) s->lid = (const uint16_t*)dev(22);
  if (b.ptrs & 8) s->rowptr_pad = (const int32_t*)(g_dev + kShiftBase);
  if (b.ptrs & 16) s->tile_shift = (const int32_t*)(g_dev + kShiftBase) + ((long long)b.tiles * 64 + 1) + b.shift_delta;
  L->c1_tiles = s;
}

static bool rdi(int* v) { return scanf("%d", v) == 1; }
static bool rdl(long long* v) { return scanf("%lld", v) == 1; }
static bool read_knobs(SpmmKnobs* k) {
  return rdi(&k->tile) && rdi(&k->tile_loop) && rdi(&k->tile_small) && rdi(&k->tile_wide) && rdi(&k->v4) && rdi(&k->dict) && rdi(&k->mt) &&
         rdi(&k->group_hint) && rdi(&k->rows_in_flight);
}

// ---- the recorded table: the product, in this order, as run lengths of (choice, dot blocks) ----
static const long long NS[] = {1, 63, 64, 65, 262144, 262145, 300071, 393215, 393216, 1000000};
static const int CS[] = {1, 2, 3, 4, 5, 8, 12, 16, 17, 20, 32, 44, 48, 64, 100, 128, 256};
static const int TILE_ROWS[] = {0, 32, 64, 128};
static const int MAX_COLS[] = {1, 300, 2000, 16000};
static const int MAX_ENTRIES[] = {4, 1024, 4096, 4098, 20000};
enum { kBalVariants = 12 };
// knob settings: the default, then every knob at each of its other values
static const int KNOBS[][9] = {
  {1, 0, 1, 1, 1, 1, 1, 16, 1}, {0, 0, 1, 1, 1, 1, 1, 16, 1}, {1, 1, 1, 1, 1, 1, 1, 16, 1}, {1, 0, 0, 1, 1, 1, 1, 16, 1},
  {1, 0, 1, 0, 1, 1, 1, 16, 1}, {1, 0, 1, 2, 1, 1, 1, 16, 1}, {1, 0, 1, 1, 0, 1, 1, 16, 1}, {1, 0, 1, 1, 2, 1, 1, 16, 1},
  {1, 0, 1, 1, 1, 0, 1, 16, 1}, {1, 0, 1, 1, 1, 2, 1, 16, 1}, {1, 0, 1, 1, 1, 1, 0, 16, 1}, {1, 0, 1, 1, 1, 1, 1, 4, 1},
  {1, 0, 1, 1, 1, 1, 1, 8, 1}, {1, 0, 1, 1, 1, 1, 1, 32, 1}, {1, 0, 1, 1, 1, 1, 1, 64, 1}, {1, 0, 1, 1, 1, 1, 1, 16, 2},
  {1, 0, 1, 1, 1, 1, 1, 16, 4}, {1, 0, 1, 1, 1, 1, 1, 16, 8}};

// the balanced descriptor of a cell: 0 absent, 1 valid, 2 valid on a CSR with ncols = n, then one violation each
static Bal bal_variant(int v, const Csr& c, long long* ncols) {
  Bal b{};
  *ncols = 0;
  if (v == 0) return b;
  const long long fixed = (c.n + 63) / 64;
  long long T = fixed + 3 < c.n ? fixed + 3 : c.n;          // a few tiles more than the 64-row set, each with a row
  if (T > 4096 && fixed <= 4096) T = 4096;
  b.on = 1; b.n = c.n; b.tiles = (int)T; b.ptrs = 31;
  b.max_cols = c.max_cols;
  b.max_entries = (c.max_entries < 4096 ? c.max_entries : 4096) & ~3;
  switch (v) {
    case 2: *ncols = c.n; break;
    case 3: *ncols = c.n + 64; break;                       // a row slice
    case 4: b.tiles = 4097; break;                          // more tiles than kMaxGrid
    case 5: b.max_entries += 2; break;                      // not quad padded
    case 6: b.shift_delta = 1; break;                       // tile_shift not behind the offsets
    case 7: b.tiles = (int)fixed - 1; break;                // a row outside every tile (n <= 64: no tile at all)
    case 8: b.tiles = (int)(c.n < 100000 ? c.n + 1 : 4096 * 300); break;      // a tile without a row
    case 9: b.n = c.n + 1; break;                           // cut for another CSR
    case 10: b.ptrs = 31 - 8; break;                        // no offsets
    case 11: b.max_cols = 16200; break;                     // the set's own dictionary past the LDS
  }
  return b;
}

struct Backend {
  int (*choice)(const mgp_csr_t*, int, int, int64_t) = nullptr;      // the library's entry points; null: the header
  int (*dot)(const mgp_csr_t*, int) = nullptr;
  SpmmKnobs k;
};

static void table_rows(const Backend& be, long long n, std::string* out) {
  long long run = 0; int last_c = 0, last_d = 0;
  char line[64];
  mgp_csr_t L; mgp_c1_tiles_t s;
  for (int C : CS) for (int tr : TILE_ROWS) for (int mc : MAX_COLS) for (int me : MAX_ENTRIES)
  for (int ord = 0; ord < 3; ++ord) for (int mt = 0; mt < 3; ++mt) for (int ro = 0; ro < 2; ++ro) for (int wd = 0; wd < 2; ++wd)
  for (int bv = 0; bv < kBalVariants; ++bv) {
    Csr c{n, 0, tr, mc, me, 0, 0, 0, 0};
    if (tr) c.ptrs |= 7;
    if (ord == 1) c.ptrs |= 8 + 16 + 32;                    // a complete row order
    if (ord == 2) c.ptrs |= 8 + 16;                         // a partial one
    if (mt) { c.ptrs |= 64 + 128 + 256; c.mt_tiles = (int)((n + 15) / 16); c.mt_steps = 16 * c.mt_tiles + (mt == 2 ? 8 : 0); }
    const Bal b = bal_variant(bv, c, &c.ncols);
    make(c, b, &L, &s);
    const int ch = be.choice ? be.choice(&L, C, wd, ro ? 64 : 0) : spmm_kernel_choice(&L, C, wd, ro ? 64 : 0, be.k);
    const int db = be.dot ? be.dot(&L, C) : spmm_dot_blocks_csr(&L, C, be.k);
    if (run && ch == last_c && db == last_d) { ++run; continue; }
    if (run) { snprintf(line, sizeof line, "%lld %d %d\n", run, last_c, last_d); *out += line; }
    run = 1; last_c = ch; last_d = db;
  }
  snprintf(line, sizeof line, "%lld %d %d\n", run, last_c, last_d);
  *out += line;
}

static int table(const char* lib_path) {
  Backend be;
  int (*set_i[9])(int) = {};
  if (lib_path) {
    void* h = dlopen(lib_path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    be.choice = (int (*)(const mgp_csr_t*, int, int, int64_t))dlsym(h, "mgp_spmm_kernel_choice");
    be.dot = (int (*)(const mgp_csr_t*, int))dlsym(h, "mgp_spmm_dot_blocks_csr");
    const char* names[9] = {"mgp_spmm_set_tile_mode", "mgp_spmm_set_tile_loop_mode", "mgp_spmm_set_tile_small_mode", "mgp_spmm_set_tile_wide_mode",
                            "mgp_spmm_set_v4_mode", "mgp_spmm_set_dict_mode", "mgp_spmm_set_mt_mode", "mgp_spmm_set_group_hint",
                            "mgp_spmm_set_rows_in_flight"};
    for (int i = 0; i < 9; ++i) if (!(set_i[i] = (int (*)(int))dlsym(h, names[i]))) return 1;
    if (!be.choice || !be.dot) return 1;
  }
  const int NN = sizeof(NS) / sizeof(NS[0]);
  for (const auto& kn : KNOBS) {
    be.k = SpmmKnobs{kn[0], kn[1], kn[2], kn[3], kn[4], kn[5], kn[6], kn[7], kn[8]};
    if (lib_path) for (int i = 0; i < 9; ++i) set_i[i](kn[i]);        // process-wide: set before the threads of this setting start
    std::vector<std::string> parts(NN);
    std::vector<std::thread> th;
    for (int i = 0; i < NN; ++i) th.emplace_back(table_rows, std::cref(be), NS[i], &parts[i]);
    for (auto& t : th) t.join();
    printf("K %d %d %d %d %d %d %d %d %d\n", kn[0], kn[1], kn[2], kn[3], kn[4], kn[5], kn[6], kn[7], kn[8]);
    for (int i = 0; i < NN; ++i) { printf("N %lld\n", NS[i]); fputs(parts[i].c_str(), stdout); }
  }
  if (lib_path) for (int i = 0; i < 9; ++i) set_i[i](KNOBS[0][i]);
  return 0;
}

int main(int argc, char** argv) {
  g_dev = (char*)mmap(nullptr, kDevBytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (g_dev == (char*)MAP_FAILED) return 1;
  if (argc >= 3 && !strcmp(argv[1], "t")) return table(strcmp(argv[2], "header") ? argv[2] : nullptr);
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'k') {
      printf("K %d %d %d %d %d %d %zu %zu %zu %d %d %d %d\n", kBlock, kMaxGrid, kWideCap, kDictThreads, kDictLdsBudget, kMtMinCols, kLdsWorkgroup,
             kLdsStaticRoom, kCgStepStaticLds, dict_max_u(1), dict_max_u(2), dict_max_u(3), dict_max_u(4));
    } else if (cmd == 'p') {
      // csr: n ncols tile_rows max_cols max_entries lanes ptrs mt_tiles mt_steps | call: C row_offset with_dot |
      // set: on n tiles max_cols max_entries ptrs shift_delta | knobs
      Csr c{}; Bal b{}; SpmmKnobs k; int C, wd; long long ro;
      if (!rdl(&c.n) || !rdl(&c.ncols) || !rdi(&c.tile_rows) || !rdi(&c.max_cols) || !rdi(&c.max_entries) || !rdi(&c.lanes) || !rdi(&c.ptrs) ||
          !rdi(&c.mt_tiles) || !rdi(&c.mt_steps) || !rdi(&C) || !rdl(&ro) || !rdi(&wd) || !rdi(&b.on) || !rdl(&b.n) || !rdi(&b.tiles) ||
          !rdi(&b.max_cols) || !rdi(&b.max_entries) || !rdi(&b.ptrs) || !rdl(&b.shift_delta) || !read_knobs(&k)) return 1;
      mgp_csr_t L; mgp_c1_tiles_t s;
      make(c, b, &L, &s);
      const SpmmPlan pl = spmm_plan(&L, C, ro, wd != 0, k);
      const SpmmTileSet& t = pl.set;
      printf("P %d %d %d %zu %d %d %lld %d %d %d %d %d %d %d %d %d %d  %lld %d %d %lld %lld %lld %lld %lld %lld %lld  %d %d %d %d %d\n", pl.err,
             (int)pl.family, pl.grid, pl.lds, pl.dot_blocks, pl.align16 ? 1 : 0, (long long)pl.rows_per_block, pl.lanes, pl.rows_in_flight,
             pl.v4_ok ? 1 : 0, pl.tiles_per_block, pl.one_tile ? 1 : 0, pl.balanced ? 1 : 0, pl.window, pl.slots, pl.stream_cap, pl.wide_cap,
             (long long)t.tiles, t.max_cols, t.max_entries, (long long)t.n, dev_id(t.tile_ptr), dev_id(t.tile_cols), dev_id(t.lid),
             dev_id(t.rowptr_t), dev_id(t.vals_t), dev_id(t.rowid), spmm_kernel_choice(&L, C, wd, ro, k), spmm_dot_blocks_csr(&L, C, k),
             spmm_dot_blocks_for(&L, C, k), spmm_tile_plan(&L, k) ? 1 : 0, spmm_cgstep_fits(&L, k) ? 1 : 0);
    } else if (cmd == 'g') {            // rows per pass / column group: C lanes rows_in_flight
      int C, l, r; if (!rdi(&C) || !rdi(&l) || !rdi(&r)) return 1;
      printf("G %d %d\n", spmm_rows_per_pass(C, l, r), spmm_cols_group(C));
    } else if (cmd == 'd') {            // no CSR: n C knobs
      long long n; int C; SpmmKnobs k; if (!rdl(&n) || !rdi(&C) || !read_knobs(&k)) return 1;
      printf("D %d\n", spmm_dot_blocks(n, C, k));
    } else return 1;
  }
  return 0;
}
"""

FAMILIES = ("RowGroups", "Gather", "TileC1", "TileSmall", "MatrixCore", "Dict", "TileWide")
CHOICE_OF = dict(RowGroups=0, Gather=0, TileC1=1, TileSmall=2, MatrixCore=3, Dict=5, TileWide=6)
PLAN = ("err", "family", "grid", "lds", "dot_blocks", "align16", "rows_per_block", "lanes", "rows_in_flight", "v4_ok", "tiles_per_block",
        "one_tile", "balanced", "window", "slots", "stream_cap", "wide_cap", "set_tiles", "set_max_cols", "set_max_entries", "set_n",
        "set_tile_ptr", "set_tile_cols", "set_lid", "set_rowptr_t", "set_vals_t", "set_rowid", "choice", "dot_csr", "dot_for", "tile_plan",
        "cgstep_fits")
KNOB_NAMES = ("tile", "tile_loop", "tile_small", "tile_wide", "v4", "dict", "mt", "group_hint", "rows_in_flight")
DEFAULT_KNOBS = dict(tile=1, tile_loop=0, tile_small=1, tile_wide=1, v4=1, dict=1, mt=1, group_hint=16, rows_in_flight=1)
# every knob at its default and at each of its other settings (the order of KNOBS in the probe)
KNOB_SETTINGS = [{}, dict(tile=0), dict(tile_loop=1), dict(tile_small=0), dict(tile_wide=0), dict(tile_wide=2), dict(v4=0), dict(v4=2),
                 dict(dict=0), dict(dict=2), dict(mt=0), dict(group_hint=4), dict(group_hint=8), dict(group_hint=32), dict(group_hint=64),
                 dict(rows_in_flight=2), dict(rows_in_flight=4), dict(rows_in_flight=8)]
# the device-pointer ids of the probe
P_TILE_PTR, P_TILE_COLS, P_LID, P_ROWPTR_T, P_VALS_T, P_ROWID = 5, 6, 7, 8, 9, 10
S_TILE_PTR, S_TILE_COLS, S_LID, S_ROWPTR_PAD = 20, 21, 22, 64


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("spmm_policy")
    src, out = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(out), "-ldl"])
    return str(out)


@pytest.fixture(scope="module")
def probe(exe):
    def run(lines):
        out = subprocess.check_output([exe], input="\n".join(lines) + "\n", text=True)       # a read through a device pointer ends it
        rows = [ln.split() for ln in out.strip().splitlines()]
        assert len(rows) == len(lines), (len(rows), len(lines))
        return rows
    return run


@pytest.fixture(scope="module")
def K(probe):
    t = probe(["k"])[0]
    names = ("kBlock", "kMaxGrid", "kWideCap", "kDictThreads", "kDictLdsBudget", "kMtMinCols", "kLdsWorkgroup", "kLdsStaticRoom",
             "kCgStepStaticLds", "u1", "u2", "u3", "u4")
    k = dict(zip(names, (int(v) for v in t[1:])))
    # the hardware's and the kernels' own: 64 KB of LDS per workgroup, 160 KB per CU, four waves per workgroup
    assert k["kBlock"] == 256 and k["kLdsWorkgroup"] == 65536 and k["kLdsStaticRoom"] == 64 and k["kDictLdsBudget"] <= 160 * 1024, k
    assert k["kCgStepStaticLds"] >= 76 and k["kDictThreads"] == 1024 and k["kWideCap"] % 64 == 0, k
    return k


def _csr(n, tile_rows=64, max_cols=300, max_entries=1024, order="none", mt="absent", ncols=0, lanes=0, dict_ptrs=7):
    ptrs = (dict_ptrs if tile_rows else 0) | dict(none=0, complete=56, partial=24, rowptr=8, vals=16, rowid=32)[order]
    mt_tiles = mt_steps = 0
    if mt != "absent":
        ptrs |= 448
        mt_tiles = -(-n // 16)
        mt_steps = 16 * mt_tiles + (8 if mt == "odd" else 0)
    return dict(n=n, ncols=ncols, tile_rows=tile_rows, max_cols=max_cols, max_entries=max_entries, lanes=lanes, ptrs=ptrs,
                mt_tiles=mt_tiles, mt_steps=mt_steps)


NO_SET = dict(on=0, n=0, tiles=0, max_cols=0, max_entries=0, ptrs=0, shift_delta=0)


def _set(n, tiles, max_cols=200, max_entries=4096, ptrs=31, shift_delta=0, set_n=None):
    return dict(on=1, n=n if set_n is None else set_n, tiles=tiles, max_cols=max_cols, max_entries=max_entries, ptrs=ptrs,
                shift_delta=shift_delta)


def _text(c, C, ro=0, wd=0, s=NO_SET, knobs=()):
    k = dict(DEFAULT_KNOBS, **dict(knobs))
    return "p %d %d %d %d %d %d %d %d %d  %d %d %d  %d %d %d %d %d %d %d  %s" % (
        c["n"], c["ncols"], c["tile_rows"], c["max_cols"], c["max_entries"], c["lanes"], c["ptrs"], c["mt_tiles"], c["mt_steps"], C, ro, wd,
        s["on"], s["n"], s["tiles"], s["max_cols"], s["max_entries"], s["ptrs"], s["shift_delta"], " ".join(str(k[q]) for q in KNOB_NAMES))


def _plans(probe, cases):
    rows = probe([_text(*c) for c in cases])
    assert all(r[0] == "P" for r in rows)
    out = []
    for r in rows:
        p = dict(zip(PLAN, (int(v) for v in r[1:])))
        p["family"] = FAMILIES[p["family"]]
        out.append(p)
    return out


NS = (1, 63, 64, 65, 4097, 60000, 262144, 262145, 300071, 393216, 1000000)
CS = (1, 2, 3, 4, 5, 8, 12, 16, 17, 20, 32, 44, 48, 64, 100, 128, 256)
SHAPES = [(0, 0, 0)] + [(tr, mc, me) for tr in (32, 64, 128) for mc, me in ((1, 4), (300, 1024), (2000, 4096), (2000, 4098), (16000, 20000),
                                                                             (300, 20000), (16000, 4096))]


def _check(case, p, K):
    """What the kernels index, for one plan."""
    c, C, ro, wd, s, knobs = case
    k = dict(DEFAULT_KNOBS, **dict(knobs))
    ctx = (case, p)
    n, B = c["n"], K["kBlock"]
    lds_max = K["kLdsWorkgroup"] - K["kLdsStaticRoom"]
    if p["err"]:
        # refused: a bad spmv_lanes, or the tile image with a row offset and dot partials
        assert p["err"] in (-1, -3) and p["choice"] == p["err"], ctx
        return
    fam = p["family"]
    assert p["choice"] == CHOICE_OF[fam], ctx
    assert p["dot_blocks"] == p["grid"] >= 1, ctx                 # every workgroup writes one row of dot partials
    if ro == 0:
        assert p["dot_csr"] == p["dot_for"] and (wd or p["dot_csr"] == p["grid"]), ctx
    tile_fams = ("TileC1", "TileSmall", "TileWide", "Dict")
    if fam in ("RowGroups", "Gather"):
        assert p["grid"] <= K["kMaxGrid"], ctx
        if fam == "RowGroups":
            assert C == 1 and p["lanes"] in (4, 8, 16, 32, 64) and p["lanes"] == (c["lanes"] or k["group_hint"]), ctx
            assert 1 <= p["rows_in_flight"] <= p["lanes"], ctx                    # lane t of a group finishes row t
            per_pass = B // p["lanes"] * p["rows_in_flight"]                        # groups of a workgroup x rows in flight
        else:
            assert C > 1, ctx
            # a row is owned by min(pow2 >= C, 64) lanes, four rows in flight; C in {4, 8, 12, 16}: 16 lanes
            g = 16 if (C <= 16 and C % 4 == 0) else min(64, max(4, 1 << (C - 1).bit_length()))
            per_pass = B // g * 4
            if p["v4_ok"]:
                assert C % 4 == 0 and 16 < C <= 256 and c["max_entries"] % 4 == 0 and c["ptrs"] & 4, ctx     # float4 lanes over quad-padded rows
        rpb = p["rows_per_block"]
        assert rpb % per_pass == 0 and p["grid"] * rpb >= n, ctx
        assert p["grid"] == 1 or (p["grid"] - 1) * rpb < n, ctx                  # no workgroup without a row
    elif fam in tile_fams:
        assert c["ptrs"] & 7 == 7 and c["tile_rows"] in ((32, 64, 128) if fam == "TileC1" else (64,)), ctx
        order = c["ptrs"] & 56
        assert order in (0, 56), ctx                                              # a row order is whole or absent
        tiles, tpb = p["set_tiles"], p["tiles_per_block"]
        assert p["grid"] <= K["kMaxGrid"], ctx
        if fam == "Dict":
            # workgroup b walks tiles b, b + grid, ...
            assert tpb == 1 and p["grid"] == min(tiles, K["kMaxGrid"]), ctx
        else:
            assert p["grid"] * tpb >= tiles and (p["grid"] - 1) * tpb < tiles, ctx          # all tiles covered, no empty workgroup
        assert not p["one_tile"] or (fam == "TileC1" and tpb == 1), ctx
        if not p["balanced"]:
            # the CSR's own tiles, position = row (or its row order)
            assert tiles == -(-n // c["tile_rows"]) and p["set_n"] == n, ctx
            assert (p["set_tile_ptr"], p["set_tile_cols"], p["set_lid"]) == (P_TILE_PTR, P_TILE_COLS, P_LID), ctx
            want = (P_ROWPTR_T, P_VALS_T, P_ROWID) if order else (-1, -1, -1)
            assert (p["set_rowptr_t"], p["set_vals_t"], p["set_rowid"]) == want, ctx
            assert (p["set_max_cols"], p["set_max_entries"]) == (c["max_cols"], c["max_entries"]), ctx
        if fam == "TileC1":
            assert C == 1, ctx
            # xl[max_cols] floats and one partial sum per quad of the largest tile
            assert p["lds"] >= (p["set_max_cols"] + p["set_max_entries"] // 4) * 4 and p["lds"] <= lds_max, ctx
            assert p["one_tile"] == (tpb == 1 and not k["tile_loop"]), ctx
        else:
            assert not p["balanced"] and p["align16"] and c["max_entries"] % 4 == 0, ctx
        if fam == "TileSmall":
            assert C in (4, 8, 12, 16), ctx
            w, max_q = p["window"], c["max_entries"] // 4
            assert w % 256 == 0 and w >= 256, ctx
            # float4 per dictionary column and per staged quad; the dot partials cross the same LDS: 64 rows x C floats
            assert p["lds"] >= (c["max_cols"] + min(max_q, w)) * 16 and p["lds"] >= 64 * C * 4 and p["lds"] <= lds_max, ctx
        if fam == "TileWide":
            cap = p["wide_cap"]
            assert cap % 64 == 0 and 64 <= cap <= K["kWideCap"] and p["lds"] >= max(4096, cap * 64), ctx
            assert p["lds"] <= K["kLdsWorkgroup"], ctx
        if fam == "Dict":
            nv = -(-C // 64)
            S = p["slots"]
            assert S % 16 == 0 and S >= 32, ctx
            assert S * 16 * nv <= K["u%d" % nv] * K["kDictThreads"], ctx         # staged float4 per thread (16 nv per slot)
            assert p["stream_cap"] >= c["max_entries"] and p["stream_cap"] % 8 == 0, ctx
            # S slots and the zero slot of nv * 256 bytes, the stream at 6 bytes per entry; the reduction: 64 rows x nv x 256 bytes
            assert p["lds"] >= (S + 1) * nv * 256 + p["stream_cap"] * 6 and p["lds"] >= 64 * nv * 256, ctx
            assert p["lds"] <= K["kDictLdsBudget"], ctx
    else:
        assert fam == "MatrixCore" and ro == 0 and K["kMtMinCols"] <= C <= 256 and C % 4 == 0 and p["align16"], ctx
        assert c["mt_steps"] % 16 == 0 and c["mt_tiles"] == -(-n // 16) and not c["ptrs"] & 32, ctx
        waves = c["mt_tiles"] * -(-C // 64)                                       # one wave per 16-row tile and 64-column block
        assert p["grid"] == -(-waves // (B // 64)), ctx
    if p["balanced"]:
        assert fam == "TileC1" and C == 1 and ro == 0 and c["ptrs"] & 56 == 0 and c["ncols"] in (0, n) and c["tile_rows"] == 64, ctx
        assert s["on"] and s["ptrs"] == 31 and s["shift_delta"] == 0 and s["n"] == n, ctx
        T = s["tiles"]
        assert 1 <= T <= K["kMaxGrid"] and s["max_entries"] % 4 == 0 and 64 * T >= n >= T, ctx
        assert p["grid"] == T and p["tiles_per_block"] == 1 and p["set_tiles"] == T and p["set_n"] == 64 * T, ctx
        assert p["lds"] == (s["max_cols"] + s["max_entries"] // 4) * 4, ctx                  # the set's own maxima
        assert (p["set_tile_ptr"], p["set_tile_cols"], p["set_lid"]) == (S_TILE_PTR, S_TILE_COLS, S_LID), ctx
        assert (p["set_rowptr_t"], p["set_vals_t"], p["set_rowid"]) == (S_ROWPTR_PAD, -1, -1), ctx
        assert (p["set_max_cols"], p["set_max_entries"]) == (s["max_cols"], s["max_entries"]), ctx
    if C == 1 and ro == 0:
        assert p["tile_plan"] == (fam == "TileC1"), ctx
        if p["cgstep_fits"]:
            # the step kernel: 256-lane workgroups on 64 positions, its static words on top of the dynamic LDS
            assert fam == "TileC1" and c["tile_rows"] == 64 and p["lds"] + K["kCgStepStaticLds"] <= K["kLdsWorkgroup"], ctx


def test_contracts_over_the_grid(probe, K):
    """Every family's grid, LDS and tile set, at every knob setting, with and without the balanced set."""
    cases = []
    for n, C, (tr, mc, me), knobs in itertools.product(NS, CS, SHAPES, KNOB_SETTINGS):
        if len(knobs) and (n in (63, 65, 60000, 262144, 262145) or C in (2, 3, 5, 8, 20, 44, 100) or (mc, me) in ((1, 4), (300, 20000))):
            continue                                              # off-default knobs on a thinner grid
        for order, mt, ro, wd in (("none", "absent", 0, 0), ("complete", "absent", 0, 1), ("partial", "absent", 0, 0), ("none", "fits", 0, 1),
                                  ("none", "fits", 64, 0), ("none", "fits", 64, 1), ("none", "odd", 0, 0), ("complete", "fits", 0, 0)):
            cases.append((_csr(n, tr, mc, me, order, mt), C, ro, wd, NO_SET, tuple(knobs.items())))
        T = min(-(-n // 64) + 3, n, K["kMaxGrid"])
        if C in (1, 4, 64) and tr:
            cases.append((_csr(n, tr, mc, me), C, 0, 1, _set(n, T, 200, min(me, 4096) & ~3), tuple(knobs.items())))
    plans = _plans(probe, cases)
    seen = dict.fromkeys(FAMILIES, 0)
    seen.update(balanced=0, capped_rows=0, many_tiles=0, refused=0, cgstep=0, one_tile=0)
    for case, p in zip(cases, plans):
        _check(case, p, K)
        if p["err"]:
            seen["refused"] += 1
            continue
        seen[p["family"]] += 1
        seen["balanced"] += p["balanced"]; seen["cgstep"] += p["cgstep_fits"]; seen["one_tile"] += p["one_tile"]
        seen["capped_rows"] += p["family"] in ("RowGroups", "Gather") and p["grid"] == K["kMaxGrid"]
        seen["many_tiles"] += p["tiles_per_block"] > 1
    assert all(v > 0 for v in seen.values()), seen               # every family, both caps, the refusal and the set occur on the grid
    print(len(cases), "plans", seen)


def _violations(n, T):
    """The valid set of a CSR with n rows, then one violation each (name, csr changes, call changes, set)."""
    ok = _set(n, T)
    return [("valid", {}, {}, ok), ("valid, ncols = n", dict(ncols=n), {}, ok),
            ("C = 4", {}, dict(C=4), ok), ("row offset", {}, dict(ro=64), ok), ("row order", dict(order="complete"), {}, ok),
            ("tile_rowptr alone", dict(order="rowptr"), {}, ok), ("tile_vals alone", dict(order="vals"), {}, ok),
            ("tile_rowid alone", dict(order="rowid"), {}, ok),
            ("row slice", dict(ncols=n + 64), {}, ok), ("32-row tiles", dict(tile_rows=32), {}, ok), ("128-row tiles", dict(tile_rows=128), {}, ok),
            ("too many tiles", {}, {}, _set(n, 4097)), ("not quad padded", {}, {}, _set(n, T, max_entries=4094)),
            ("shift elsewhere", {}, {}, _set(n, T, shift_delta=1)), ("shift elsewhere", {}, {}, _set(n, T, shift_delta=-1)),
            ("row outside", {}, {}, _set(n, -(-n // 64) - 1)), ("empty tile", {}, {}, _set(n, n + 1)), ("no tiles", {}, {}, _set(n, 0)),
            ("another n", {}, {}, _set(n, T, set_n=n + 1)), ("LDS", {}, {}, _set(n, T, max_cols=16200))] + \
           [("null pointer %d" % b, {}, {}, _set(n, T, ptrs=31 - (1 << b))) for b in range(5)]


@pytest.mark.parametrize("n", (5000, 4097 * 64 - 64, 100))
def test_balanced_set_is_taken_only_where_it_may_be(probe, K, n):
    """The valid descriptor is taken; every single violation of its conditions runs the 64-row set, whose plan is the plan of the
    same CSR without a descriptor."""
    T = min(-(-n // 64) + 3, K["kMaxGrid"])
    names, cases, bare = [], [], []
    for name, dc, dcall, s in _violations(n, T):
        if name == "too many tiles" and n < 4097:
            continue                                              # (also an empty tile there)
        c = _csr(n, **dict(dict(tile_rows=64, max_cols=300, max_entries=8192), **dc))
        call = dict(dict(C=1, ro=0), **dcall)
        names.append(name)
        cases.append((c, call["C"], call["ro"], 1, s, ()))
        bare.append((c, call["C"], call["ro"], 1, NO_SET, ()))
    got, want = _plans(probe, cases), _plans(probe, bare)
    for name, case, g, w in zip(names, cases, got, want):
        _check(case, g, K)
        if name.startswith("valid"):
            assert g["balanced"] and g["family"] == "TileC1" and g["grid"] == T and g["dot_csr"] == T and g["set_n"] == 64 * T, (name, g)
            assert g["lds"] == (200 + 4096 // 4) * 4 and g["cgstep_fits"], (name, g)
            assert w["grid"] == -(-n // 64) and w["lds"] == (300 + 8192 // 4) * 4, (name, w)
        else:
            if case[2]:                                           # the sizing calls know no row offset: theirs is the plan at offset 0
                g, w = ({q: v for q, v in d.items() if q not in ("dot_csr", "dot_for", "tile_plan", "cgstep_fits")} for d in (g, w))
            assert not g["balanced"] and g == w, (name, g, w)
    # the loop form of the kernel runs the same set, one tile per workgroup
    loop = _plans(probe, [(cases[0][0], 1, 0, 1, cases[0][4], (("tile_loop", 1),))])[0]
    assert loop["balanced"] and not loop["one_tile"] and loop["grid"] == T and loop["tiles_per_block"] == 1


def test_a_partial_row_order_selects_no_dictionary_kernel(probe, K):
    """tile_rowptr, tile_vals and tile_rowid are all set or none: one or two of them leave the gather kernels, whatever else the
    CSR carries (the matrix-core image included, unless tile_rowid is there) -- and nothing is read through any of them."""
    for C in (1, 4, 32, 64, 128):
        base = _plans(probe, [(_csr(393216, 0, 0, 0), C, 0, 0, NO_SET, (("tile_wide", 2), ("dict", 2)))])[0]
        for order in ("rowptr", "vals", "rowid", "partial"):
            for s in (NO_SET, _set(393216, 4096)):
                p = _plans(probe, [(_csr(393216, 64, 300, 1024, order), C, 0, 0, s, (("tile_wide", 2), ("dict", 2)))])[0]
                assert p["family"] == base["family"] and p["family"] in ("RowGroups", "Gather") and p["grid"] == base["grid"], (C, order, p)
                assert not p["balanced"] and p["rows_per_block"] == base["rows_per_block"], (C, order, p)


def test_rows_per_pass_and_the_count_without_a_csr(probe, K):
    """spmm_rows_per_pass is the rows one pass of a workgroup's lane groups covers; mgp_spmm_dot_blocks(n, C) is the gather
    kernels' grid, at C == 1 with the process-default lanes."""
    B = K["kBlock"]
    for C in CS:
        rpp, g = (int(v) for v in probe(["g %d 16 1" % C])[0][1:])
        assert g >= min(C, 64) and g & (g - 1) == 0 and 4 <= g <= 64 and (g < 2 * C or g == 4), (C, g)
        if C > 1:
            assert rpp == (64 if C <= 16 and C % 4 == 0 else B // g * 4), (C, rpp, g)
    for lanes, rif in itertools.product((4, 8, 16, 32, 64), (1, 2, 4, 8)):
        assert int(probe(["g 1 %d %d" % (lanes, rif)])[0][1]) == B // lanes * rif
    for n, C, lanes, rif in itertools.product((1, 300071, 5000000), (1, 4, 20), (4, 16, 64), (1, 8)):
        kn = dict(DEFAULT_KNOBS, group_hint=lanes, rows_in_flight=rif)
        d = int(probe(["d %d %d %s" % (n, C, " ".join(str(kn[q]) for q in KNOB_NAMES))])[0][1])
        p = _plans(probe, [(_csr(n, 0, 0, 0), C, 0, 0, NO_SET, tuple(kn.items()))])[0]
        assert d == p["grid"] and p["family"] in ("RowGroups", "Gather"), (n, C, lanes, rif, d, p)
    assert int(probe(["d 0 1 " + " ".join(str(DEFAULT_KNOBS[q]) for q in KNOB_NAMES)])[0][1]) == -1


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "line %d: got %r, recorded %r (after %r)" % (i + 1, a, b, w[max(0, i - 3):i])
    return "lengths differ: %d lines against %d recorded" % (len(g), len(w))


@pytest.fixture(scope="module")
def recorded():
    return lzma.open(TABLE, "rt").read()


def test_header_reproduces_the_recorded_table(exe, recorded):
    """(b), the header: spmm_kernel_choice / spmm_dot_blocks_csr over the whole product, at every knob setting."""
    got = subprocess.check_output([exe, "t", "header"], text=True)
    cells = sum(int(ln.split()[0]) for ln in got.splitlines() if ln[0] not in "KN")
    assert cells == len(KNOB_SETTINGS) * 10 * 17 * 4 * 4 * 5 * 3 * 3 * 2 * 2 * 12, cells
    assert got == recorded, _first_difference(got, recorded)


def test_library_reproduces_the_recorded_table(exe, recorded):
    """(b), the library: mgp_spmm_kernel_choice / mgp_spmm_dot_blocks_csr under the mgp_spmm_set_* switches.  Both are host
    arithmetic: no device is touched."""
    from manifold_gp_amd import _lib
    got = subprocess.check_output([exe, "t", _lib.LIB_PATH], text=True)
    assert got == recorded, _first_difference(got, recorded)
