// The plan of a CG solve (cg.hip): which kernel family and grid a plan runs, how its workspace is carved, and the small rules of
// the graph driver.  Plain structs and pure functions: no HIP, no I/O, no environment.  cg.hip drives the GPU with them;
// tests/test_cg_policy_cpu.py runs the same functions on the CPU.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "mgp_hip.h"
#include "mgp_arena.h"

// shared with the kernels of cg.hip
constexpr int kBlock = 256;
constexpr int kMaxC = 256;
constexpr int kMaxGridVec = 512;
constexpr int kMaxPartials = 4096;   // capacity of the gamma / rr partial arrays
constexpr int kReduceOnceAbove = 16;
constexpr int kC1GammaSlots = 2;     // nbv <= kMaxGridVec = 2 * 256
constexpr int kC1DeltaSlots = 16;    // nbs <= 4096
constexpr int kCxDeltaSlots = 16;    // nbs4 <= 4096
#ifdef MGP_STAMP
constexpr size_t kStampWords = 1024 + 8192;   // lab builds: the stamp rings behind the 16 state words
#else
constexpr size_t kStampWords = 0;
#endif

// The lab switches (mgp_cg_set_*): one instance in cg.hip, read once at plan creation -- except poll_spin, read per chunk.
struct CgKnobs {
  int complex_shift = 1;    // form 2, nu = 2, symmetric normalisation, C = 1: the complex-shift solve (0: CG on A)
  int reduce_once = 1;      // 0: every update workgroup re-reduces the partials at any C (A/B, tests); 2: cg_reduce_kernel from two columns up
  int update_quads = 1;     // C % 4 == 0 plans update through cg_update_q_kernel (0: the element form at every C)
  int poll_spin = 64;       // flag reads between two looks at the clock in the flag-only poll window; 0: no such window
  int init_free = 1;        // C == 1 plans start without a cg_init launch (0: classic start)
  int decide_in_update = 1; // the first graph's last update decides + marks (0: separate launches)
  int fold_update = 1;      // nu = 2, C == 1: delta from |B P u|^2, the vector update in the epilogue of the apply's second SpMV (0: update
                            // launches; 1: where it was measured to win, nbs <= 4 kBlock; 2: wherever the shape allows)
};

// What a plan is created from.  nb_loc: SpMM workgroups per rank that write dot partials (mgp_spmm_dot_blocks_for(L, C)); nb4: the
// same for 4 columns (the complex-shift product; the driver computes it only when C == 1 && !is_dist, else 0); tile_plan: the
// C == 1 tile SpMV runs on L (mgp_tile_plan).
struct CgShape {
  int64_t n;                // local rows; vectors have the global length n * world
  int world;
  bool is_dist;             // row-partitioned plan (a single rank, world == 1, included)
  int C, nb_loc, nb4;
  bool has_minv, has_pre, has_post;
  int form, nu;
  float noise_scale;        // noise * scale
  int stop_mode;
  bool tile_plan;
  bool pre_is_post;         // op->pre == op->post as pointers, both null included: Q2 = scale P B^nu P with one vector P
  int tile_rows;            // rows per tile of the C == 1 tile SpMV when the step kernel can run on it (mgp_spmm_cgstep_fits: 64-row tiles,
                            // four waves per workgroup, LDS room for the step's words), else 0
};

struct CgChoice {
  int TC, TS;               // element form: TC = least power of two >= C column lanes x TS row slices = kBlock threads
  int CQ, TSQ;              // quad form: CQ = C / 4 column quads x TSQ row slices (CQ * TSQ active threads); TSQ = 0: not in use
  int64_t rows_per_block;
  int nbv, nbs;             // update grid; dot partials of one apply (all ranks)
  bool reduce_once;         // cg_reduce_kernel sums the partials of a step once; the update reads 3 C totals
  int upd_quads;            // 0: cg_update_kernel; else the workgroup size of cg_update_q_kernel
  bool c1_family, cx, init_free;
  bool fold;                // a step is two launches: the first SpMV with the self dot, then spmv_tile_cgstep_kernel (no update launch)
};

inline int cg_tile_cols(int C) { int t = 1; while (t < C) t <<= 1; return t; }   // least power of two >= C

inline CgChoice cg_choose(const CgShape& sh, const CgKnobs& k) {
  CgChoice c{};
  const int C = sh.C;
  const int64_t n = sh.n * sh.world;        // global vector length
  c.TC = cg_tile_cols(C); c.TS = kBlock / c.TC;
  // contiguous row ranges per workgroup, at most kMaxGridVec workgroups.  C > 1: every workgroup of the
  // update kernel re-reduces ALL dot partials of ALL columns (nbv x (2 nbv + nbs) x C loads per launch),
  // so the grid is kept to one workgroup per CU (their loads go out in batches of 8 / 32 per lane)
  // C > 16: the partials are summed once by cg_reduce_kernel, the update grid is free to fill the chip
  c.reduce_once = k.reduce_once && C > (k.reduce_once == 2 ? 1 : kReduceOnceAbove);
  const int max_grid_vec = (C == 1) ? kMaxGridVec : (c.reduce_once ? 2048 : 256);
  // C % 4 == 0 behind cg_reduce_kernel (C > 16): the quad form of the update (cg_update_q_kernel).  Up to 16 columns, where every
  // workgroup re-reduces the partials, the element form stays: measured at 60k x 12 (tools/lab/cg12.py) 12.2 us against 15.4 for the
  // quad form in 1024-thread workgroups and 17.4 in 512-thread ones (the kernel can do it: reduce_once = 2)
  c.upd_quads = (C % 4 == 0 && c.reduce_once && k.update_quads != 0) ? kBlock : 0;
  c.CQ = C / 4;
  c.TSQ = c.upd_quads ? c.upd_quads / c.CQ : 0;
  const int64_t step = c.upd_quads ? c.TSQ : c.TS;
  int64_t rpb = step, nbv = mgp_cdiv(n, rpb);
  if (nbv > max_grid_vec) { rpb = mgp_cdiv(mgp_cdiv(n, max_grid_vec), step) * step; nbv = mgp_cdiv(n, rpb); }
  c.rows_per_block = rpb; c.nbv = (int)nbv;
  c.nbs = sh.nb_loc * sh.world;
  // The single-column kernel family (cg_update_c1_kernel, cg_decide_c1_kernel, cx_update_kernel) can run this plan: one column
  // whose partials fit the slots a lane of those kernels sums.  (One column on one device always does: the update grid is at most
  // kMaxGridVec and the SpMV grids at most 4096 workgroups; a row-partitioned plan has `world` times the SpMV partials.)
  c.c1_family = C == 1 && c.nbv <= kC1GammaSlots * kBlock && c.nbs <= kC1DeltaSlots * kBlock;
  // complex-shift solve (cx_update_kernel): (K + s I) in precision form, symmetric normalisation, nu = 2, no preconditioner,
  // per-column relative stop; its product runs on the 4-column SpMM, whose partials must fit the slots of a lane
  c.cx = k.complex_shift && C == 1 && !sh.is_dist && !sh.has_minv && sh.form == 2 && sh.nu == 2 && !sh.has_pre && !sh.has_post &&
         sh.noise_scale > 0.f && c.c1_family && sh.stop_mode == 1 && sh.nb4 >= 1 && sh.nb4 <= kCxDeltaSlots * kBlock;
  // init-free start: no cg_init launch, the first apply (tile SpMV) reads the right-hand side itself
  c.init_free = k.init_free && c.c1_family && !sh.is_dist && !sh.has_minv && !c.cx && (sh.form == 0 || sh.form == 2) && sh.tile_plan;
  // folded step: with A = [I +] c P B^2 P and u = r, u . A u = [gamma +] c |B P u|^2 is known after the FIRST SpMV of the apply, so
  // the second one takes the whole step in its epilogue.  It builds on the init-free start (the first SpMV leaves ||b||^2 where the
  // step looks for gamma) and on the 64-row tile kernel; its ||r||^2 partials, one per SpMV workgroup, share pd_rr with stride nbs.
  // Every one of the nbs SpMV workgroups re-reduces 3 nbs partials: free at 235 workgroups (60k nodes: -6 us per 3-step solve),
  // 66 MB of L2 reads per launch at 2345 (300k nodes: measured +2.4 us per iteration against the update launch, whose grid is capped
  // at kMaxGridVec for the same reason) -- so the default takes it up to 4 slots of kBlock partials per lane
  c.fold = k.fold_update && c.init_free && sh.nu == 2 && sh.pre_is_post && sh.tile_rows == 64 && c.nbs <= kMaxPartials &&
           (k.fold_update == 2 || c.nbs <= 4 * kBlock);
  return c;
}

// Every buffer a plan takes from its workspace ([..]: floats unless a type is named; nc = n * world * C, nn = n * world).
struct CgBuffers {
  float *x, *r, *ubuf, *w, *p, *s, *usbuf;       // [nc] each; ubuf / usbuf are in use with minv / op->pre only
  char* op_work; size_t op_work_bytes;           // operator chain scratch (global length)
  float *pd_gamma, *pd_rr;                       // [2][kMaxPartials][C]
  float* pd_delta;                               // [nbs][C]
  float* blk;                                    // gamma_old[2][C] alpha_old[2][C] bb[C] resid[C] state[16] (+ kStampWords)
  float* tot;                                    // [3][C] (cg_reduce_kernel)
  float *xacc, *rbuf, *tbuf, *rpart;             // refinement: [nc] accumulated solution, residual rhs, A x; [256][C][2] partials
  double *xacc64, *t64, *work64, *rpart64;       // single GPU, fp64: [nc], [nc], [4 nc] chain buffers, [256][C][2]
  // complex-shift solve (C == 1 && !is_dist, else null): z r p s [nn] float2, u4 w4 y4 [nn] float4, the 4-column chain scratch,
  // pd4 [kCxDeltaSlots * kBlock][4], pd_g [2][kMaxGridVec][4], sc [64]
  float *cz, *cr, *cp, *cs, *u4, *w4, *y4;
  char* op_work4; size_t op_work4_bytes;
  float *pd4, *pd_g, *sc;
  float* pd_bb;                                  // [nbs][C] partials of ||b||^2 written by the first apply (init-free)
  int* arrive;                                   // [9][32] arrival counters (cg_update_c1_kernel<true>)
};

// THE sequence of takes: the order fixes every buffer's address relative to the workspace.  Arena: MgpArena, real or counting.
template <class Arena>
void cg_carve(Arena& ar, const CgShape& sh, const CgChoice& ch, CgBuffers* b) {
  const size_t C = (size_t)sh.C, nn = (size_t)(sh.n * sh.world), nc = nn * C;
  *b = CgBuffers{};
  auto f32 = [&ar](size_t count) { return ar.template take<float>(count); };
  auto f64 = [&ar](size_t count) { return ar.template take<double>(count); };
  b->x = f32(nc); b->r = f32(nc); b->ubuf = f32(nc); b->w = f32(nc); b->p = f32(nc); b->s = f32(nc); b->usbuf = f32(nc);
  b->op_work_bytes = 4 * mgp_align(nc * sizeof(float)) + 256;
  b->op_work = ar.template take<char>(b->op_work_bytes);
  b->pd_gamma = f32(2 * (size_t)kMaxPartials * C); b->pd_rr = f32(2 * (size_t)kMaxPartials * C);
  b->pd_delta = f32((size_t)ch.nbs * C);
  // one contiguous block: for C == 1 {gamma_old[2], alpha_old[2], bb, resid, state[0], state[1]} are 32
  // consecutive bytes, which the C == 1 kernels fetch with a single scalar load (CgScalars)
  b->blk = f32(6 * C + 16 + kStampWords);
  b->tot = f32(3 * C);
  b->xacc = f32(nc); b->rbuf = f32(nc); b->tbuf = f32(nc); b->rpart = f32(256 * C * 2);
  b->xacc64 = f64(nc); b->t64 = f64(nc); b->work64 = f64(4 * nc); b->rpart64 = f64(256 * C * 2);
  if (sh.C == 1 && !sh.is_dist) {      // taken whenever the shape could use them, whatever cg_choose said
    b->cz = f32(2 * nn); b->cr = f32(2 * nn); b->cp = f32(2 * nn); b->cs = f32(2 * nn);
    b->u4 = f32(4 * nn); b->w4 = f32(4 * nn); b->y4 = f32(4 * nn);
    b->op_work4_bytes = 4 * mgp_align(nn * 16) + 256;
    b->op_work4 = ar.template take<char>(b->op_work4_bytes);
    b->pd4 = f32((size_t)kCxDeltaSlots * kBlock * 4); b->pd_g = f32((size_t)2 * kMaxGridVec * 4); b->sc = f32(64);
  }
  b->pd_bb = f32((size_t)ch.nbs * C);
  b->arrive = ar.template take<int>(9 * 32);
}

// mgp_cg_workspace_bytes / mgp_cg_dist_workspace_bytes: what the plan carves, and 1024 bytes of slack
inline size_t cg_workspace_bytes(const CgShape& sh, const CgChoice& ch) {
  MgpArena count;
  CgBuffers b;
  cg_carve(count, sh, ch, &b);
  return count.off + 1024;
}

// ---- the graph driver's rules (capture_graphs, record_first, run_cg)
// Length of the first graph (cg_init + len x (apply, update)) at its first capture: what the previous (eager) solve needed
inline int cg_first_len(int last_need, int chunk) { return last_need >= 1 && last_need <= 64 ? last_need : (chunk < 4 ? chunk : 4); }

// `len` = steps until the stopping rule fires: the last of them only detects (see cg_decide_c1_kernel), so a first graph of the
// single-column family holds len - 1 bodies and the decision
inline bool cg_last_step_decides(int len, bool is_dist, bool c1_family) { return len >= 2 && !is_dist && c1_family; }

// The first graph follows the workload.  After a solve that needed `need` steps -- longer than the captured graph: re-capture at
// once (an undecided first graph costs the flag-only window and a second launch); shorter: only when two solves in a row agree
// (the extra bodies of a graph that is one or two steps too long return at their first load); a few hundred us, once, so that
// the next solve of this kind is exactly one graph launch with no skipped launches behind the stopping decision
inline bool cg_recapture_first(int need, int len_first, int last_need) {
  return need >= 1 && need <= 64 && (need > len_first || (need < len_first && need == last_need));
}

// eager path (no graph): bodies enqueued per chunk; short solves stop early
inline int cg_eager_len(bool first, int chunk) { return (first && chunk > 4) ? 4 : chunk; }

// chunks after which run_cg gives up on a decision that never comes (every chunk runs at least min(chunk, 4) steps)
inline int cg_guard_chunks(int max_iter, int chunk) { return max_iter / (chunk < 4 ? chunk : 4) + 4; }

// The flag-only poll window of a first graph.  The graph's last node (cg_marker_kernel) reports a first graph that ran to its end
// undecided; the time budget -- ten times the last decided solve, at least 2 ms -- is only the guard against a marker that never comes.
inline int64_t cg_poll_budget_ns(int64_t last_solve_ns) { return 10 * last_solve_ns + 2000000; }
