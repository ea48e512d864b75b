// The plan of an SpMM launch (spmm.hip): which kernel family runs on a CSR at a width, and the grid, LDS and tile set it is launched
// with.  Plain structs and pure functions of the numbers in an mgp_csr_t: no HIP, no atomics, no I/O, and no DEVICE pointer is ever
// read through (the host descriptor mgp_csr_t.c1_tiles is).  spmm.hip launches what spmm_plan returns;
// tests/test_spmm_policy_cpu.py runs the same functions on the CPU.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "mgp_hip.h"

// shared with the kernels of spmm.hip
constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;
constexpr int kWideCap = 1024;     // spmm_tile_wide_kernel: dictionary columns staged per slice (64 bytes each)
constexpr int kDictThreads = 1024;
constexpr int kDictLdsBudget = 160 * 1024 - 2048;   // spmm_dict_kernel: bytes of LDS a workgroup may carve (160 KiB per CU)
// spmm_dict_kernel: staged float4 per thread and slice (their registers are live across the walk: what the 128-VGPR budget of a
// 16-wave workgroup leaves)
constexpr int dict_max_u(int nv) { return nv == 1 ? 7 : (nv == 2 ? 5 : 4); }
constexpr int kMtMinCols = 48;     // below 48 columns most lanes of a wave's 64-column block idle (mt_image_fits)
// LDS of a workgroup of the tile kernels: 64 KB, of which the plan leaves 64 bytes to the kernels' static words (the plain C == 1
// tile kernel has 32)
constexpr size_t kLdsWorkgroup = 65536;
constexpr size_t kLdsStaticRoom = 64;
// Static LDS of spmv_tile_cgstep_kernel on top of the tile SpMV's dynamic LDS (wave sums, state, hand-off words: 76 bytes, rounded up)
constexpr size_t kCgStepStaticLds = 128;

// The lab switches (mgp_spmm_set_*, include/mgp_hip.h): one instance in spmm.hip, read ONCE per call and passed down by value --
// the helpers of one call cannot see two settings.  (Two CALLS -- sizing the dot partials, then launching -- can still see
// different settings: the header says the switches are not to be flipped while another thread is inside this family of calls.)
struct SpmmKnobs {
  int tile = 1;             // C == 1: use the tile dictionaries when present
  int tile_loop = 0;        // C == 1 tile kernel: 1 = the tile-loop form even where every workgroup owns one tile
  int tile_small = 1;       // C in {4, 8, 12, 16}: spmm_tile_q_kernel
  int tile_wide = 1;        // 0 never, 1 where it was measured to win, 2 wherever the shape allows
  int v4 = 1;               // float4 member of the gather family: 0 never, 1 measured, 2 wherever the shape allows
  int dict = 1;             // 0 never, 1 measured, 2 wherever the shape allows
  int mt = 1;               // matrix-core kernel when the CSR carries the image
  // C == 1 row-group shape: lanes per row (4 entries per lane per pass) and rows in flight per lane group.  The lanes are a
  // property of the matrix and travel with it (mgp_csr_t.spmv_lanes: the host wrapper derives them from the mean padded row
  // length of the graph it built); group_hint is only the default for structs that leave the field 0
  // (mgp_spmm_set_group_hint).  Measured best on the 60k and 500k graphs: 8 lanes x 1 row (tools/tune_spmv.py).
  int group_hint = 16;
  int rows_in_flight = 1;
};

inline int64_t spmm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// mgp_csr_t.spmv_lanes: 0 = the process default (the same set as mgp_spmv_lanes_ok, mgp_internal.h; spmm.hip asserts that they agree)
constexpr bool spmm_lanes_ok(int lanes) { return lanes == 0 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64; }

// ---- launch geometry of the kernel families: pure functions of the CSR and the width --------------------------------------

struct RowPlan {
  int grid;
  int64_t rows_per_block;
};

inline RowPlan make_plan(int64_t n, int rows_per_pass) {
  // contiguous row range per workgroup (a multiple of one pass of its lane groups), grid <= kMaxGrid
  int64_t rpb = rows_per_pass;
  int64_t grid = spmm_cdiv(n, rpb);
  if (grid > kMaxGrid) {
    rpb = spmm_cdiv(spmm_cdiv(n, kMaxGrid), rows_per_pass) * rows_per_pass;
    grid = spmm_cdiv(n, rpb);
  }
  if (grid < 1) grid = 1;
  return RowPlan{(int)grid, rpb};
}

inline int spmm_cols_group(int C) {
  int g = 4;
  while (g < C && g < 64) g <<= 1;
  return g;
}

// rows a workgroup covers per pass (the grid / dot-partial count follows from it).  C in {4,8,12,16}
// uses 64 whichever kernel runs (the row16 kernel needs 16-byte aligned X, the generic one does not)
inline int spmm_rows_per_pass(int C, int lanes, int rows_in_flight) {
  if (C == 1) return (kBlock / lanes) * rows_in_flight;
  if (C <= 16 && (C & 3) == 0) return (kBlock / 16) * 4;
  return kBlock / spmm_cols_group(C) * 4;
}

// ---- the tile set a dictionary kernel runs on: the row tiles of the CSR, or (C == 1) its entry-balanced set --------------------
// Computed once by spmm_plan and carried in the plan: grid, LDS and the kernel's TileArgs all follow from this one view.
struct SpmmTileSet {
  const int32_t* tile_ptr;
  const int32_t* tile_cols;
  const uint16_t* lid;
  int64_t tiles;
  int max_cols, max_entries;
  int64_t n;                  // positions the kernel walks (SpmmArgs::n): the rows of the CSR; balanced: the padded 64 * tiles
  const int32_t* rowptr_t;    // tiles over a row order: all three; balanced: rowptr_pad alone (tile_shift stands behind it)
  const float* vals_t;
  const int32_t* rowid;
};

// the row tiles of the CSR itself (a row order is all three arrays or none: spmm_plan)
inline SpmmTileSet tile_set_rows(const mgp_csr_t* L) {
  return SpmmTileSet{L->tile_ptr, L->tile_cols, L->lid, spmm_cdiv(L->n, L->tile_rows), L->tile_max_cols, L->tile_max_entries, L->n,
                     L->tile_rowptr, L->tile_vals, L->tile_rowid};
}
inline SpmmTileSet tile_set_balanced(const mgp_c1_tiles_t* s) {
  return SpmmTileSet{s->tile_ptr, s->tile_cols, s->lid, s->tiles, s->max_cols, s->max_entries, (int64_t)s->tiles * 64,
                     s->rowptr_pad, nullptr, nullptr};
}

// THE statement of when the balanced set (mgp_csr_t.c1_tiles) runs; what builds it states when it exists (graph.py
// c1_balanced_policy: natural order, a 64-row tile over MGP_C1_TILE_CAP entries, the folded CG step kept).  It serves C == 1 only,
// positions that are rows (no row order), whole graphs (no row offset, no row slice) and one tile per workgroup (at most kMaxGrid
// tiles: the single-tile form of the kernel; the lab switch mgp_spmm_set_tile_loop_mode runs the same set through the loop form,
// one pass per workgroup, so that the two forms stay comparable bit for bit).  Everything else, and every other kernel, reads
// the 64-row set and computes what it computed before the set existed.
inline bool c1_balanced(const mgp_csr_t* L, int C, int64_t row_offset) {
  if (C != 1 || row_offset != 0) return false;
  const mgp_c1_tiles_t* s = L->c1_tiles;
  if (!s || !s->tile_ptr || !s->tile_cols || !s->lid || !s->rowptr_pad || !s->tile_shift) return false;
  // the set is cut over the natural row order: a CSR with a row order (whole or partial) does not take it
  if (L->tile_rowptr || L->tile_vals || L->tile_rowid) return false;
  if (L->tile_rows != 64 || s->n != L->n) return false;
  if (L->ncols != 0 && L->ncols != L->n) return false;
  if (s->tiles < 1 || s->tiles > kMaxGrid || (s->max_entries & 3) != 0) return false;
  // one allocation: the kernel finds the shift words behind the offsets (TileArgs)
  if (s->tile_shift != s->rowptr_pad + ((int64_t)s->tiles * 64 + 1)) return false;
  return (int64_t)s->tiles * 64 >= L->n && L->n >= s->tiles;       // every row in a tile, no tile without a row
}

// C == 1 tile kernel: the dictionary of a tile and one partial sum per quad of its entries
inline size_t tile_lds_bytes(const SpmmTileSet& s) { return ((size_t)s.max_cols + (size_t)(s.max_entries >> 2)) * sizeof(float); }

// at most kMaxGrid workgroups over the tiles (the balanced set, at most kMaxGrid tiles: one workgroup per tile)
inline int tile_grid(const SpmmTileSet& s, int* tiles_per_block) {
  const int64_t tpb = spmm_cdiv(s.tiles, kMaxGrid);
  if (tiles_per_block) *tiles_per_block = (int)tpb;
  return (int)spmm_cdiv(s.tiles, tpb);
}

// small-C tile kernel: quads of partial sums staged at once: what is left of a quarter of the CU's LDS (160 KB, four
// workgroups) behind the dictionary, in steps of 256, at least 1024 (the quads a workgroup holds in registers), at most the
// largest tile
inline int tile_small_window(const mgp_csr_t* L) {
  const int max_q = L->tile_max_entries >> 2;
  const long budget = 40448 - (long)L->tile_max_cols * 16;
  long w = budget > 0 ? budget / 16 / 256 * 256 : 0;
  if (w < 1024) w = 1024;
  if (w > max_q) w = (max_q + 255) / 256 * 256;
  return (int)(w > 0 ? w : 256);
}
inline size_t tile_small_lds_bytes(const mgp_csr_t* L, int C) {
  const size_t max_q = (size_t)(L->tile_max_entries >> 2), w = (size_t)tile_small_window(L);
  size_t b = ((size_t)L->tile_max_cols + (max_q < w ? max_q : w)) * 16;
  const size_t red = (size_t)64 * C * sizeof(float);        // dot-partial staging reuses the same LDS
  return b > red ? b : red;
}

inline int tile_wide_cap(const mgp_csr_t* L) {
  int cap = (L->tile_max_cols + 63) / 64 * 64;
  if (cap > kWideCap) cap = kWideCap;
  if (cap < 64) cap = 64;
  return cap;
}
inline size_t tile_wide_lds_bytes(const mgp_csr_t* L) {
  const size_t b = (size_t)tile_wide_cap(L) * 64;
  return b > 4096 ? b : 4096;                                // (dot-partial staging: 64 x 16 floats)
}

// lanes-over-columns dictionary kernel: slots per slice from what the stream leaves of the CU's LDS
inline int dict_nv(int C) { return (C + 63) / 64; }
inline int dict_stream_cap(const mgp_csr_t* L) { return (L->tile_max_entries + 7) / 8 * 8; }
inline int dict_slots(const mgp_csr_t* L, int C) {
  const int nv = dict_nv(C);
  const long left = (long)kDictLdsBudget - (long)dict_stream_cap(L) * 6 - (long)nv * 256;      // (the zero slot)
  long s = left / (nv * 256L);
  const long cap = (long)dict_max_u(nv) * kDictThreads / (16 * nv);      // staged float4 per thread <= dict_max_u
  if (s > cap) s = cap;
  s = s / 16 * 16;
  // no point in slices larger than the largest dictionary
  const long need = ((long)L->tile_max_cols + 15) / 16 * 16;
  if (s > need) s = need;
  return (int)s;
}
inline size_t dict_lds_bytes(const mgp_csr_t* L, int C) {
  const size_t d = (size_t)(dict_slots(L, C) + 1) * dict_nv(C) * 256 + (size_t)dict_stream_cap(L) * 6;
  const size_t red = (size_t)64 * dict_nv(C) * 256;
  return d > red ? d : red;
}
inline int dict_grid(const SpmmTileSet& s) { return (int)(s.tiles < kMaxGrid ? s.tiles : kMaxGrid); }

// the CSR carries a usable dense 16-row tile image (mgp_spmm_mt_fill) for this width
inline bool mt_image_fits(const mgp_csr_t* L, int C) {
  if (!L->mt_img || !L->mt_sptr || !L->mt_dcol || L->mt_tiles <= 0 || L->mt_steps <= 0) return false;
  // below 48 columns most lanes of a wave's 64-column block idle: the gather kernel is faster there (C = 32: 34 us against 41)
  if (C < kMtMinCols || C > 256 || (C & 3) != 0 || L->tile_rowid) return false;
  if (L->ncols != 0 && L->ncols != L->n) return false;        // a row slice of a partitioned operator never carries an image
  if ((int64_t)L->n * C * 4 >= (int64_t(1) << 31) || ((int64_t)L->mt_steps + 32) * 256 >= (int64_t(1) << 31)) return false;
  if ((L->mt_steps & 15) != 0) return false;           // every tile a whole number of bodies of four blocks
  return L->mt_tiles == (int32_t)spmm_cdiv(L->n, 16);
}

// ---- which kernel runs: the ONE statement of the policy -------------------------------------------------------------------
// spmm_plan applies the precedence order once and returns everything that follows from the choice.
// The sizing call (mgp_spmm_dot_blocks_csr), the reporting call (mgp_spmm_kernel_choice) and the launch (spmm_launch) all
// read this value: the planned kernel and the launched one cannot disagree.
enum class SpmmFamily { RowGroups, Gather, TileC1, TileSmall, MatrixCore, Dict, TileWide };

struct SpmmPlan {
  int err;                  // MGP_OK; MGP_ERR_ARG (spmv_lanes); MGP_ERR_UNSUPPORTED (tile image + row offset + dot partials)
  SpmmFamily family;
  int grid;
  size_t lds;               // dynamic LDS bytes
  int dot_blocks;           // workgroups that write dot partials
  bool align16;             // X, Y, base and dotw must be 16-byte aligned: MGP_ERR_ARG at launch otherwise
  int64_t rows_per_block;   // RowGroups, Gather: contiguous row range of a workgroup
  int lanes, rows_in_flight;    // RowGroups
  bool v4_ok;               // Gather: switch and shape allow the float4 member (the launch adds the alignment test)
  SpmmTileSet set;          // TileC1, TileSmall, Dict, TileWide: the tile set the launch runs on
  int tiles_per_block;      // TileC1, TileSmall, TileWide (Dict: 1)
  bool one_tile;            // TileC1: the single-tile form of the kernel (tiles_per_block == 1 and the loop form not forced)
  bool balanced;            // TileC1: `set` is the entry-balanced one (c1_balanced); grid, dot_blocks and lds are that set's
  int window;               // TileSmall: quads of partial sums staged per window
  int slots, stream_cap;    // Dict
  int wide_cap;             // TileWide
};

inline SpmmPlan spmm_plan(const mgp_csr_t* L, int C, int64_t row_offset, bool with_dot, const SpmmKnobs k) {
  SpmmPlan pl{};
  pl.tiles_per_block = 1;
  if (!spmm_lanes_ok(L->spmv_lanes)) { pl.err = MGP_ERR_ARG; return pl; }
  // row-tile dictionaries present and switched on; an ordered tile view is all three arrays or none
  const int ord = (L->tile_rowptr != nullptr) + (L->tile_vals != nullptr) + (L->tile_rowid != nullptr);
  const bool dicts = k.tile && (ord == 0 || ord == 3) && L->lid && L->tile_ptr && L->tile_cols;
  const bool dicts64 = dicts && L->tile_rows == 64 && (L->tile_max_entries & 3) == 0;      // 64-row tiles, quad-padded rows
  const bool wide = C > 16 && C <= 256 && (C & 3) == 0;
  const bool big_x = (size_t)L->n * (size_t)C * sizeof(float) >= ((size_t)96 << 20);   // the X block does not sit in the caches
  const size_t lds_max = kLdsWorkgroup - kLdsStaticRoom;

  // 1. C == 1 on 32 / 64 / 128-row tiles: the column dictionary of a tile staged in LDS (spmv_tile_kernel)
  if (C == 1 && dicts && (L->tile_rows == 32 || L->tile_rows == 64 || L->tile_rows == 128) && tile_lds_bytes(tile_set_rows(L)) <= lds_max) {
    pl.family = SpmmFamily::TileC1;
    pl.set = tile_set_rows(L);
    if (c1_balanced(L, C, row_offset) && tile_lds_bytes(tile_set_balanced(L->c1_tiles)) <= lds_max) {
      pl.balanced = true;
      pl.set = tile_set_balanced(L->c1_tiles);
    }
    pl.grid = pl.dot_blocks = tile_grid(pl.set, &pl.tiles_per_block);
    pl.one_tile = pl.tiles_per_block == 1 && !k.tile_loop;
    pl.lds = tile_lds_bytes(pl.set);
    return pl;
  }
  // 2. C in {4, 8, 12, 16} on 64-row tiles whose staged data (dictionary rows + matrix stream) fits the LDS budget
  //    (spmm_tile_q_kernel); [n, C] blocks with C a multiple of 4 are 16-byte aligned row by row
  if ((C == 4 || C == 8 || C == 12 || C == 16) && k.tile_small && dicts64 && tile_small_lds_bytes(L, C) <= lds_max) {
    pl.family = SpmmFamily::TileSmall;
    pl.align16 = true;
    pl.set = tile_set_rows(L);
    pl.grid = pl.dot_blocks = tile_grid(pl.set, &pl.tiles_per_block);
    pl.lds = tile_small_lds_bytes(L, C);
    pl.window = tile_small_window(L);
    return pl;
  }
  // 3. 48 <= C <= 256 on the matrix cores (spmm_mt_kernel): taken when the CSR carries the dense 16-row tile image
  //    (mgp_spmm_mt_fill; the host wrapper builds it for graphs in natural row order whose tiles are at least 1/8 full) and the
  //    call has no row offset (weighted dot-product partials included: one row of partials per workgroup).
  //    mgp_spmm_set_mt_mode(0) = never (A/B runs, tests).
  if (k.mt && mt_image_fits(L, C)) {
    if (row_offset == 0) {
      pl.family = SpmmFamily::MatrixCore;
      pl.align16 = true;
      pl.grid = pl.dot_blocks = (int)spmm_cdiv((int64_t)L->mt_tiles * ((C + 63) / 64), kBlock / 64);
      return pl;
    }
    // a CSR that carries the tile image, a row offset AND dot partials: mgp_spmm_dot_blocks_csr sized them for the matrix-core
    // kernel, which takes no row offset -- the one combination that is refused.  Without dot partials the rules below apply.
    if (with_dot) { pl.err = MGP_ERR_UNSUPPORTED; return pl; }
  }
  // 4. 16 < C <= 256 on 64-row tiles with lanes over columns (spmm_dict_kernel), at least 32 slots per slice.
  //    mgp_spmm_set_dict_mode: 0 never, 1 (default) where it was measured to win, 2 wherever the shape allows.
  //    Measured (tools/lab/time_spmm_wide.py, round 3; us: this kernel | chunked dictionary kernel | float4 gather | per-column
  //    gather):  60k graph  C = 64: 52 | 84 | 54 | 63   C = 128: 90 | 160 | 101 | 91   C = 256: 176 | 319 | 204 | 186
  //              1M graph   C = 64: 704 | 777 | 1020 | 1188   C = 128: 1201 | 1458 | 2084 | 3037   C = 256: 2380 | 2871 | 6515 | 6828
  //    -> taken from 64 columns up when the X block (n x C floats) is 96 MB or more, i.e. does not sit in the caches.
  if (wide && k.dict && dicts64 && dict_slots(L, C) >= 32 && (k.dict == 2 || (C >= 64 && big_x))) {
    pl.family = SpmmFamily::Dict;
    pl.align16 = true;       // the kernel moves 16 bytes per lane (C % 4 == 0 makes every row aligned once the block is)
    pl.set = tile_set_rows(L);
    pl.grid = pl.dot_blocks = dict_grid(pl.set);
    pl.lds = dict_lds_bytes(L, C);
    pl.slots = dict_slots(L, C);
    pl.stream_cap = dict_stream_cap(L);
    return pl;
  }
  // 5. 16 < C <= 256 on 64-row tiles in 16-column chunks (spmm_tile_wide_kernel).
  //    Measured (tools/lab/time_spmm_wide.py): on the 60k graph the per-entry gather kernel reads its X rows out of L2 and
  //    wins from 64 columns up (63 vs 84 us at C = 64, 91 vs 158 us at C = 128; 47 vs 59 us at C = 32 the other way, but see below); on
  //    the 1M graph, whose X block does not fit the caches, the dictionary kernel is 1.5-2.4x faster at every width
  //    (1.48 vs 3.04 ms at C = 128).  mode 2 forces it at any size (tests, A/B).
  //    (and up to 64 columns the float4-lane gather kernel beats both on a cache-resident X block: 33 us at C = 32)
  if (wide && k.tile_wide && dicts64 && (k.tile_wide == 2 || big_x)) {
    pl.family = SpmmFamily::TileWide;
    pl.align16 = true;
    pl.set = tile_set_rows(L);
    pl.grid = pl.dot_blocks = tile_grid(pl.set, &pl.tiles_per_block);
    pl.lds = tile_wide_lds_bytes(L);
    pl.wide_cap = tile_wide_cap(L);
    return pl;
  }
  // 6. C == 1 without dictionaries: a row per lane group (spmv_kernel); the lanes are the matrix's own, 0 = process default
  if (C == 1) {
    pl.family = SpmmFamily::RowGroups;
    pl.lanes = L->spmv_lanes ? L->spmv_lanes : k.group_hint;
    pl.rows_in_flight = k.rows_in_flight;
    if (pl.rows_in_flight > pl.lanes) pl.rows_in_flight = pl.lanes;   // lane t finishes row t: needs R <= G
    const RowPlan rows = make_plan(L->n, spmm_rows_per_pass(1, pl.lanes, pl.rows_in_flight));
    pl.grid = pl.dot_blocks = rows.grid;
    pl.rows_per_block = rows.rows_per_block;
    return pl;
  }
  // 7. C > 1 gather from memory.  The plan fixes the FAMILY and its grid; the launch picks the member (row16, float4 lanes,
  //    per-column) by pointer alignment, which a sizing call cannot know.  That is sound because all three cover the same
  //    make_plan(n, spmm_rows_per_pass(C)) row ranges and therefore write the same dot-partial blocks.
  //    float4 member, measured (tools/lab/time_spmm_wide.py): 33 vs 59 us at C = 32 and 54 vs 63 us at C = 64 on the 60k graph, but
  //    101 vs 91 us at C = 128 (the X block no longer sits in L2 and the per-column kernel's whole-line pieces use
  //    the Infinity Cache path better); on the 1M graph, when the dictionaries are not there, it wins at every width.
  //    (quad-padded rows are what the tile builder guarantees: the CSR of a graph without dictionaries keeps the per-column kernel)
  pl.family = SpmmFamily::Gather;
  pl.v4_ok = k.v4 && wide && (k.v4 == 2 || C <= 64 || big_x) && (L->tile_max_entries & 3) == 0 && L->lid != nullptr;
  const RowPlan rows = make_plan(L->n, spmm_rows_per_pass(C, 0, 0));
  pl.grid = pl.dot_blocks = rows.grid;
  pl.rows_per_block = rows.rows_per_block;
  return pl;
}

// ---- what the entry points of spmm.hip answer from a plan -------------------------------------------------------------------

// the C == 1 tile kernel would run on L (mgp_tile_plan)
inline bool spmm_tile_plan(const mgp_csr_t* L, const SpmmKnobs k) {
  if (!L) return false;
  const SpmmPlan pl = spmm_plan(L, 1, 0, false, k);
  return pl.err == MGP_OK && pl.family == SpmmFamily::TileC1;
}

// spmv_tile_cgstep_kernel can run on this plan of L: the 64-row C == 1 tile plan, with room for the step's static LDS
inline bool spmm_cgstep_ok(const SpmmPlan& pl, const mgp_csr_t* L) {
  return pl.err == MGP_OK && pl.family == SpmmFamily::TileC1 && L->tile_rows == 64 && pl.lds + kCgStepStaticLds <= kLdsWorkgroup;
}
inline bool spmm_cgstep_fits(const mgp_csr_t* L, const SpmmKnobs k) { return L && spmm_cgstep_ok(spmm_plan(L, 1, 0, true, k), L); }

inline int spmm_dot_blocks_for(const mgp_csr_t* L, int C, const SpmmKnobs k) {
  if (!L) return MGP_ERR_ARG;
  const SpmmPlan pl = spmm_plan(L, C, 0, false, k);
  return pl.err != MGP_OK ? pl.err : pl.dot_blocks;
}
inline int spmm_dot_blocks_csr(const mgp_csr_t* L, int C, const SpmmKnobs k) {
  if (!L || L->n <= 0 || C <= 0) return MGP_ERR_ARG;
  return spmm_dot_blocks_for(L, C, k);
}
// no CSR: the gather kernels' count, C == 1 with the process-default lanes
inline int spmm_dot_blocks(int64_t n, int C, const SpmmKnobs k) {
  if (n <= 0 || C <= 0) return MGP_ERR_ARG;
  const int lanes = k.group_hint, rif = k.rows_in_flight;
  return make_plan(n, spmm_rows_per_pass(C, lanes, rif < lanes ? rif : lanes)).grid;
}

// the public numbers of the families (include/mgp_hip.h; 4 was round 4's persistent 8-lanes-per-row dictionary kernel:
// measured slower, removed in round 5)
inline int spmm_kernel_choice(const mgp_csr_t* L, int C, int with_dot, int64_t row_offset, const SpmmKnobs k) {
  if (!L || L->n <= 0 || C <= 0 || C > 256) return MGP_ERR_ARG;
  const SpmmPlan pl = spmm_plan(L, C, row_offset, with_dot != 0, k);
  if (pl.err != MGP_OK) return pl.err;
  switch (pl.family) {
    case SpmmFamily::TileC1: return 1;
    case SpmmFamily::TileSmall: return 2;
    case SpmmFamily::MatrixCore: return 3;
    case SpmmFamily::Dict: return 5;
    case SpmmFamily::TileWide: return 6;
    default: return 0;      // gather (C == 1: row groups)
  }
}
