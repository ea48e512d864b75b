// Pipelined conjugate gradients (Ghysels-Vanroose recurrence) with PARTITIONED vectors: the row-partitioned
// multi-GPU form of the (K + s I) x = y solve -- one process per GPU, ONE RCCL collective per iteration -- and,
// with world = 1, a single-GPU variant of the solver in cg.hip.
//
// The reference has no distributed code; the solve it replaces is linear_cg behind
// precision_matern_operator.py:53 / train_model.py:68.  Why this recurrence for the partitioned form:
//   classic / Chronopoulos-Gear CG needs the WHOLE new search vector for the next SpMV and, separately, the dot
//   products of that SpMV's output for the next update: two global synchronisations per iteration (a vector
//   gather and a scalar reduction).  In the pipelined recurrence
//       gamma_i = (r_i, r_i),  delta_i = (w_i, r_i),  q_i = A w_i                     [w_i = A r_i by recurrence]
//       beta_i = gamma_i / gamma_{i-1},  alpha_i = gamma_i / (delta_i - beta_i gamma_i / alpha_{i-1})
//       z = q + beta z,  s = w + beta s,  p = r + beta p,  x += alpha p,  r -= alpha s,  w -= alpha z
//   both the dots and the SpMV input depend only on (r_i, w_i), i.e. on the previous vector update.  So per iteration
//   every rank: updates ITS rows of x, r, p, s, z, w and writes its partial dots; ONE grouped all-gather moves the
//   w slices and the partials; the SpMVs of A w follow.  The update needs alpha_i, beta_i -- sums of the gathered
//   partials, re-reduced in a fixed order by every workgroup: all ranks take bit-identical decisions, hence issue
//   identical collective sequences.
//
// Row partition with ghost layers (nu >= 2 without a second exchange): A w = (I +) c D^1/2 (tau I + L)^nu D^1/2 w is a
// chain of nu SpMVs.  Rank p owns a contiguous row block R_p; launch s of the chain must produce its output on
// R_p grown by (nu - 1 - s) neighbour layers.  The host orders the rows as [R_p, G_1, G_2, ..., rest] and builds the
// tile view of the graph over that order (mgp_graph_tiles with `order`): launch s simply runs the tile SpMV on the
// first launch_rows[s] rows of the view.  All vectors live at the global length and are indexed by global row id
// (the tile view's row ids); a rank touches its own rows of them, the full gathered w, and the chain's
// intermediate on R_p + ghosts.
//
// Attainable accuracy.  The pipelined recurrence carries two more vector recurrences (w, z) than classic CG and
// its residual stagnates EARLIER in fp32 (measured on the dumbbell test systems, cond 3e3 .. 1e5: recurrence residual
// 2e-4 .. 4e-2 where the Chronopoulos-Gear solver of cg.hip reaches a true residual of 2e-4 .. 3e-3), and past that
// point the iterates drift.  Two guards: (1) stagnation detection -- the smallest residual norm seen and its
// iteration are tracked; no new minimum for 50 + it_best / 4 iterations ends the solve with status 4; (2) with
// max_refine > 0 the solve is the inner solver of an iterative refinement: the accumulated solution's TRUE residual
// b - A x is formed (one more gather + apply), and A d = residual is solved again until the true residual meets the
// tolerance -- every round restarts the recurrences, which is also what repairs the drift.  `resid` then reports
// the true relative residual.  Well-conditioned systems (the C3 / C4 posterior: 3 iterations) never see either.
//
// `comm == NULL` with world > 1 is the VIRTUAL mode of the tests: several plans (one per virtual rank) live in one
// process on one GPU and share the double-buffered w / partial arrays, so that the all-gather is the identity;
// the host enqueues the phases of every virtual rank in lock step (mgp_pcg_plan_enqueue).
#include <math.h>
#include <chrono>
#include <new>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>
#include "mgp_common.h"
#include "mgp_internal.h"
#include "cg_rule.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxNu = 8;
constexpr int kMaxSlots = 16;        // partial slots per lane of the consuming kernels: <= 4096 workgroups in all

struct PcgArgs {
  int64_t row0, n_loc;     // this rank's rows [row0, row0 + n_loc) (global ids)
  int64_t n_real;          // rows >= n_real are padding (isolated nodes, b = 0)
  float *x, *r, *p, *s, *z;         // global length, own rows touched
  const float* q;          // A w on own rows
  float* w[2];             // gathered w, double-buffered by the iteration parity
  float* pd[2];            // [2][world * nbu]: gamma partials then delta partials
  float* pdd;              // Chronopoulos-Gear form: [world] delta = (u, A u) of every rank's rows (gathered)
  float* pdd_loc;          // [nb2] this rank's SpMV-epilogue partials, folded into pdd[rank] by cgp_delta_kernel
  int nb2;                 // SpMV workgroups of this rank that write them (<= 4096)
  int nbu;                 // workgroups of this kernel per rank
  int world, rank;
  float* scal;             // [0..1] gamma_old by parity, [2..3] alpha_old by parity, [4] bb, [5] resid,
                           // [6] tolerance of this round, [8..9] best residual by parity, [10..11] its iteration
  int* state;              // [0] operator applies of the iteration loop so far (ticked by the chain's last SpMV:
                           //     the update of iteration i reads i + 1), [1] done, [2] status
  int* host_state;         // host-mapped mirror
  float* host_resid;
  float tol;
  int max_iter, min_iter, stop_mode;
};

// fixed-order reduction of the gathered partials: lane slots in order, DPP wave sum, (w0 + w1) + (w2 + w3)
__device__ __forceinline__ void reduce_two(const float* __restrict__ pg, const float* __restrict__ pdl, int count,
                                           float (*sh)[2], float* g_out, float* d_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float gv[kMaxSlots], dv[kMaxSlots];
#pragma unroll
  for (int k = 0; k < kMaxSlots; ++k) {
    const int b = tid + k * kBlock;
    const int bc = b < count ? b : count - 1;
    gv[k] = pg[bc];
    dv[k] = pdl[bc];
  }
  float g = 0.f, d = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxSlots; ++k) {
    const bool on = tid + k * kBlock < count;
    g += on ? gv[k] : 0.f;
    d += on ? dv[k] : 0.f;
  }
  g = mgp_wave_sum(g);
  d = mgp_wave_sum(d);
  if (lane == 0) { sh[wave][0] = g; sh[wave][1] = d; }
  __syncthreads();
  *g_out = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
  *d_out = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
}

// after the first apply (w_0 = A b on this rank's rows, already in w[0]): r = b, x = p = s = z = 0 on own rows,
// partials of gamma_0 = (b, b) and delta_0 = (w_0, b); iteration state reset by workgroup 0
__global__ __launch_bounds__(kBlock) void pcg_start_kernel(PcgArgs a, const float* __restrict__ B, int round) {
  __shared__ float sh[kBlock / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    a.state[0] = 0; a.state[1] = 0; a.state[2] = 0;
    if (round == 0) a.scal[6] = a.tol;                  // later rounds: set by the refinement's finalize kernel
    a.scal[8] = 3.0e38f; a.scal[9] = 3.0e38f;
    reinterpret_cast<int*>(a.scal)[10] = 0; reinterpret_cast<int*>(a.scal)[11] = 0;
  }
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float g = 0.f, d = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float b = r < a.n_real ? B[r] : 0.f;
    const float w0 = a.w[0][r];
    a.r[r] = b; a.x[r] = 0.f; a.p[r] = 0.f; a.s[r] = 0.f; a.z[r] = 0.f;
    g = fmaf(b, b, g);
    d = fmaf(w0, b, d);
  }
  g = mgp_wave_sum(g);
  d = mgp_wave_sum(d);
  if (lane == 0) { sh[wave][0] = g; sh[wave][1] = d; }
  __syncthreads();
  if (tid == 0) {
    const int slot = a.rank * a.nbu + blockIdx.x;
    a.pd[0][slot] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    a.pd[0][a.world * a.nbu + slot] = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  }
}

// ---- One step of the two partitioned update kernels (pcg_update_kernel, cgp_update_kernel), everything but their reductions
// and vector passes: the scalar prologue, the decision (cg_rule.h, plus the stagnation guard), the coefficients and the
// scal[] / publication writes of workgroup 0.
// Everything another workgroup of THIS launch may rewrite is read through the parity: workgroup 0 stores gamma / alpha of
// iteration i in slot i & 1 while the others still read slot (i - 1) & 1; the iteration counter is ticked by the SpMV launch
// in front, never here; bb is written at i = 0 only and read from i = 1 on.  All of these reads, and one lane's view of the
// done flag (so that all waves take the same branch), are issued before `reduce`, whose barrier publishes that flag.
struct PcgStep {
  int par;
  float alpha, beta;
  bool done;
};

template <class Reduce>
__device__ __forceinline__ PcgStep pcg_step(const PcgArgs& a, int* sh_done, Reduce reduce) {
  const int tid = threadIdx.x;
  const int it = a.state[0] - 1;
  if (tid == 0) *sh_done = a.state[1];
  const int par = it & 1;
  const float gamma_old = a.scal[par ^ 1], alpha_old = a.scal[2 + (par ^ 1)], bb_old = a.scal[4];
  const float tol = a.scal[6];
  const float best_old = a.scal[8 + (par ^ 1)];
  const int it_best_old = reinterpret_cast<const int*>(a.scal)[10 + (par ^ 1)];
  float gamma, delta;
  reduce(par, &gamma, &delta);
  PcgStep s = {par, 0.f, 0.f, true};
  if (*sh_done) return s;
  const float bb = it == 0 ? gamma : bb_old;
  const float rel = cg_rel(gamma, bb);
  // `it` counts from 0 here and cg_rule.h's step from 1: this call is the only place the two counters meet
  CgStop st = cg_stop(a.stop_mode, a.min_iter, a.max_iter, tol, it + 1, rel);
  // stagnation: no new minimum of the residual norm for 50 + it_best / 4 iterations (file header)
  const float best = rel < best_old ? rel : best_old;
  const int it_best = rel < best_old ? it : it_best_old;
  if (!st.done && it - it_best >= 50 + it_best / 4) { st.done = 1; st.status = kCgStagnated; }
  // never frozen: a solve that goes on takes a full step
  const CgCoef k = cg_coef(it == 0, false, gamma, delta, gamma_old, alpha_old);
  if (blockIdx.x == 0 && tid == 0) {
    a.scal[5] = rel;
    if (it == 0) a.scal[4] = bb;
    if (st.done) {
      // (a workgroup that starts late and reads done = 1 returns at once: it would have decided the same)
      cg_publish(a.state, a.host_state, a.host_resid, &rel, 1, it, st.status);
    } else {
      a.scal[par] = gamma; a.scal[2 + par] = k.alpha;
      a.scal[8 + par] = best;
      reinterpret_cast<int*>(a.scal)[10 + par] = it_best;
    }
  }
  s.alpha = k.alpha; s.beta = k.beta; s.done = st.done != 0;
  return s;
}

// one pipelined-CG vector update on this rank's rows (see the file header); takes the stopping decision on
// ||r_i|| BEFORE updating, so that x is the iterate the decision was taken on
__global__ __launch_bounds__(kBlock) void pcg_update_kernel(PcgArgs a) {
  __shared__ float sh[kBlock / 64][2];
  __shared__ float sh2[kBlock / 64][2];
  __shared__ int sh_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int count = a.world * a.nbu;
  const PcgStep st = pcg_step(a, &sh_done, [&](int par, float* gamma, float* delta) {
    reduce_two(a.pd[par], a.pd[par] + count, count, sh, gamma, delta);
  });
  if (st.done) return;
  const int par = st.par;
  const float alpha = st.alpha, beta = st.beta;
  const float* __restrict__ wc = a.w[par];
  float* __restrict__ wn = a.w[par ^ 1];
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float ng = 0.f, nd = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float q = a.q[r], w = wc[r], rr = a.r[r];
    const float z = fmaf(beta, a.z[r], q);
    const float s = fmaf(beta, a.s[r], w);
    const float p = fmaf(beta, a.p[r], rr);
    a.z[r] = z; a.s[r] = s; a.p[r] = p;
    a.x[r] = fmaf(alpha, p, a.x[r]);
    const float rn = fmaf(-alpha, s, rr);
    const float wv = fmaf(-alpha, z, w);
    a.r[r] = rn;
    wn[r] = wv;
    ng = fmaf(rn, rn, ng);
    nd = fmaf(wv, rn, nd);
  }
  ng = mgp_wave_sum(ng);
  nd = mgp_wave_sum(nd);
  if (lane == 0) { sh2[wave][0] = ng; sh2[wave][1] = nd; }
  __syncthreads();
  if (tid == 0) {
    const int slot = a.rank * a.nbu + blockIdx.x;
    a.pd[par ^ 1][slot] = (sh2[0][0] + sh2[1][0]) + (sh2[2][0] + sh2[3][0]);
    a.pd[par ^ 1][count + slot] = (sh2[0][1] + sh2[1][1]) + (sh2[2][1] + sh2[3][1]);
  }
}

// ---- iterative refinement around the pipelined solve (own rows; fp64 accumulation of the solution)
__global__ void pcg_accumulate_kernel(PcgArgs a, double* __restrict__ xacc, float* __restrict__ xfull, int first) {
  for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < a.n_loc; l += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = a.row0 + l;
    const double v = first ? (double)a.x[r] : xacc[r] + (double)a.x[r];
    xacc[r] = v;
    xfull[r] = (float)v;
  }
}

// R = B - A xacc on own rows (A xacc in t), partials of sum R^2 and sum B^2 in the slots of pd[0]
__global__ __launch_bounds__(kBlock) void pcg_residual_kernel(PcgArgs a, const float* __restrict__ B, const float* __restrict__ t,
                                                              float* __restrict__ rfull) {
  __shared__ float sh[kBlock / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float rr = 0.f, bb = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float b = r < a.n_real ? B[r] : 0.f;
    const float d = r < a.n_real ? b - t[r] : 0.f;
    rfull[r] = d;
    rr = fmaf(d, d, rr);
    bb = fmaf(b, b, bb);
  }
  rr = mgp_wave_sum(rr);
  bb = mgp_wave_sum(bb);
  if (lane == 0) { sh[wave][0] = rr; sh[wave][1] = bb; }
  __syncthreads();
  if (tid == 0) {
    const int slot = a.rank * a.nbu + blockIdx.x;
    a.pd[0][slot] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    a.pd[0][a.world * a.nbu + slot] = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  }
}

// every rank: true relative residual from the gathered partials (same order everywhere) -> host; tolerance of
// the next round relative to ITS right-hand side (the residual): half of what is still missing, within [tol, 0.1]
__global__ __launch_bounds__(kBlock) void pcg_refine_finalize_kernel(PcgArgs a, float* __restrict__ host_true_rel) {
  __shared__ float sh[kBlock / 64][2];
  float rr, bb;
  const int count = a.world * a.nbu;
  reduce_two(a.pd[0], a.pd[0] + count, count, sh, &rr, &bb);
  if (threadIdx.x == 0) {
    const float rel = cg_rel(rr, bb);
    float next = rel > 0.f ? 0.5f * a.tol / rel : a.tol;
    next = next < a.tol ? a.tol : (next > 0.1f ? 0.1f : next);
    a.scal[6] = next;
    host_true_rel[0] = rel;
  }
}

// ---- residual replacement (own rows): dst = src, dst = b - t, and the partials of (r, r), (w, r)
__global__ void pcg_copy_rows_kernel(PcgArgs a, float* __restrict__ dst, const float* __restrict__ src) {
  for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < a.n_loc; l += (int64_t)gridDim.x * blockDim.x)
    dst[a.row0 + l] = src[a.row0 + l];
}

__global__ void pcg_sub_rows_kernel(PcgArgs a, float* __restrict__ dst, const float* __restrict__ b, const float* __restrict__ t) {
  for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < a.n_loc; l += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = a.row0 + l;
    dst[r] = r < a.n_real ? b[r] - t[r] : 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void pcg_dots_kernel(PcgArgs a, int par) {
  __shared__ float sh[kBlock / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    // the replaced residual is the TRUE one: the stagnation window restarts from it
    a.scal[8] = 3.0e38f; a.scal[9] = 3.0e38f;
    reinterpret_cast<int*>(a.scal)[10] = a.state[0]; reinterpret_cast<int*>(a.scal)[11] = a.state[0];
  }
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float g = 0.f, d = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float rv = a.r[r];
    g = fmaf(rv, rv, g);
    d = fmaf(a.w[par][r], rv, d);
  }
  g = mgp_wave_sum(g);
  d = mgp_wave_sum(d);
  if (lane == 0) { sh[wave][0] = g; sh[wave][1] = d; }
  __syncthreads();
  if (tid == 0) {
    const int slot = a.rank * a.nbu + blockIdx.x;
    a.pd[par][slot] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    a.pd[par][a.world * a.nbu + slot] = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  }
}

__global__ void pcg_publish_kernel(PcgArgs a, const double* __restrict__ xacc) {
  for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < a.n_loc; l += (int64_t)gridDim.x * blockDim.x)
    a.x[a.row0 + l] = (float)xacc[a.row0 + l];
}

// ---- Chronopoulos-Gear recurrence with partitioned vectors (recurrence = 1): the recurrence of cg.hip -- robust on
// ill-conditioned systems where the pipelined one stagnates early (file header) -- at the price of a second, tiny
// collective per iteration.  w[.] holds the gathered u = r; the SpMV chain's last launch leaves the partials of
// delta = (u, A u) (pdd, gathered: collective A, ~100 floats per rank); this update takes gamma = (r, r) from the
// partials gathered WITH the vector (collective B), updates own rows and writes the new r into w[par ^ 1].
__global__ __launch_bounds__(kBlock) void cgp_start_kernel(PcgArgs a, const float* __restrict__ B, int round) {
  __shared__ float sh[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    a.state[0] = 0; a.state[1] = 0; a.state[2] = 0;
    if (round == 0) a.scal[6] = a.tol;
    a.scal[8] = 3.0e38f; a.scal[9] = 3.0e38f;
    reinterpret_cast<int*>(a.scal)[10] = 0; reinterpret_cast<int*>(a.scal)[11] = 0;
  }
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float g = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float b = r < a.n_real ? B[r] : 0.f;
    a.r[r] = b; a.x[r] = 0.f; a.p[r] = 0.f; a.s[r] = 0.f;
    a.w[0][r] = b;                                    // own slice of u_0 = b (gathered next)
    g = fmaf(b, b, g);
  }
  g = mgp_wave_sum(g);
  if (lane == 0) sh[wave] = g;
  __syncthreads();
  if (tid == 0) a.pd[0][a.rank * a.nbu + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// this rank's delta partials (one per SpMV workgroup, up to 4096) -> ONE float, fixed order: what is gathered
__global__ __launch_bounds__(kBlock) void cgp_delta_kernel(PcgArgs a) {
  __shared__ float sh[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float dv[kMaxSlots];
#pragma unroll
  for (int k = 0; k < kMaxSlots; ++k) {
    const int b = tid + k * kBlock;
    dv[k] = a.pdd_loc[b < a.nb2 ? b : a.nb2 - 1];
  }
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxSlots; ++k) d += (tid + k * kBlock < a.nb2) ? dv[k] : 0.f;
  d = mgp_wave_sum(d);
  if (lane == 0) sh[wave] = d;
  __syncthreads();
  if (tid == 0) a.pdd[a.rank] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(kBlock) void cgp_update_kernel(PcgArgs a) {
  __shared__ float sh[kBlock / 64][2];
  __shared__ float sh2[kBlock / 64];
  __shared__ int sh_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // gamma from the update-kernel partials (world * nbu), delta from the SpMV partials (world * nb2)
  const PcgStep st = pcg_step(a, &sh_done, [&](int par, float* gamma, float* delta) {
    const int cg = a.world * a.nbu, cd = a.world;
    float gv[kMaxSlots], dv[kMaxSlots];
#pragma unroll
    for (int k = 0; k < kMaxSlots; ++k) {
      const int b = tid + k * kBlock;
      gv[k] = a.pd[par][b < cg ? b : cg - 1];
      dv[k] = a.pdd[b < cd ? b : cd - 1];
    }
    float g = 0.f, d = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxSlots; ++k) {
      g += (tid + k * kBlock < cg) ? gv[k] : 0.f;
      d += (tid + k * kBlock < cd) ? dv[k] : 0.f;
    }
    g = mgp_wave_sum(g);
    d = mgp_wave_sum(d);
    if (lane == 0) { sh[wave][0] = g; sh[wave][1] = d; }
    __syncthreads();
    *gamma = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    *delta = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  });
  if (st.done) return;
  const int par = st.par;
  const float alpha = st.alpha, beta = st.beta;
  float* __restrict__ un = a.w[par ^ 1];
  const int64_t rows_per = (a.n_loc + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows_per;
  int64_t l1 = l0 + rows_per;
  if (l1 > a.n_loc) l1 = a.n_loc;
  float ng = 0.f;
  for (int64_t l = l0 + tid; l < l1; l += kBlock) {
    const int64_t r = a.row0 + l;
    const float rr = a.r[r], w = a.q[r];
    const float p = fmaf(beta, a.p[r], rr);
    const float sv = fmaf(beta, a.s[r], w);
    a.p[r] = p; a.s[r] = sv;
    a.x[r] = fmaf(alpha, p, a.x[r]);
    const float rn = fmaf(-alpha, sv, rr);
    a.r[r] = rn;
    un[r] = rn;
    ng = fmaf(rn, rn, ng);
  }
  ng = mgp_wave_sum(ng);
  if (lane == 0) sh2[wave] = ng;
  __syncthreads();
  if (tid == 0) a.pd[par ^ 1][a.rank * a.nbu + blockIdx.x] = (sh2[0] + sh2[1]) + (sh2[2] + sh2[3]);
}

struct PcgPlan {
  bool poisoned = false;     // a solve ended in MGP_ERR_TIMEOUT: destroy leaks instead of waiting
  int recurrence;            // 0 pipelined (one collective per iteration), 1 Chronopoulos-Gear (two)
  mgp_operator_t op;
  int64_t launch_rows[kMaxNu];
  PcgArgs args;
  ncclComm_t comm;
  int world, rank;
  bool virt;                 // world > 1 without a communicator: buffers shared with the other virtual ranks
  float *t0, *t1;            // chain intermediates, global length
  float* q;
  double* xacc;              // refinement: accumulated solution (own rows)
  float *xfull, *rfull;      // refinement: gathered solution / residual (global length)
  float* host_true_rel;      // host-mapped
  float* dev_true_rel;
  mgp_cg_params_t prm;
  hipStream_t stream, cap_stream;
  hipGraphExec_t exec;       // `chunk` iterations (SpMV chain, update, collective)
  bool has_graph, graphs_tried;
  int chunk, solves;
  int32_t* host_state;
  int64_t last_solve_ns;       // host time of the previous solve when its first chunk took the decision (0: it did not)
  float* host_resid;
  int64_t n_glob;
};

size_t pcg_private_floats(int64_t n_glob) { return 12 * (size_t)n_glob + 4096 + 256; }   // x r p s z q t0 t1 xfull rfull xacc(f64) + scalars

int nbu_for(int64_t n_loc) {
  int64_t nb = mgp_cdiv(n_loc, kBlock);
  if (nb > 512) nb = 512;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// launch `s` of the chain on the first launch_rows[s] rows of the tile view
int chain_launch(PcgPlan* pl, int s, const float* in, float* out, const float* base, const int* skip, int* tick,
                 hipStream_t st, const float* dotw = nullptr, float* dot_partials = nullptr) {
  const mgp_operator_t& op = pl->op;
  const float tau = 2.0f * (float)op.nu / (op.kappa * op.kappa);
  const bool first = s == 0, last = s == op.nu - 1;
  mgp_csr_t L = op.L;
  L.n = pl->launch_rows[s];
  float cb = 0.f, co = 1.f;
  const float* bs = nullptr;
  if (last) {
    co = op.scale;
    if (op.form == 2) { bs = base; cb = 1.f; co = op.noise * op.scale; }
  }
  const MgpSpmmOpts o{0, nullptr, skip, last ? tick : nullptr};      // row_offset, cbv, skip, tick
  return mgp_spmm_fused_opts(&L, in, 1, out, tau, 1.0f, first ? op.pre : nullptr, last ? op.post : nullptr, bs, cb, co,
                             last ? dotw : nullptr, last ? dot_partials : nullptr, o, st);
}

// q (or w_0) = A v on this rank's rows; v gathered at the global length
int enqueue_apply(PcgPlan* pl, const float* v, float* out, const int* skip, int* tick, hipStream_t st,
                  bool delta_partials = false) {
  const float* in = v;
  for (int s = 0; s < pl->op.nu; ++s) {
    const bool last = s == pl->op.nu - 1;
    float* o = last ? out : ((s & 1) ? pl->t1 : pl->t0);
    MGP_TRY(chain_launch(pl, s, in, o, v, skip, tick, st, delta_partials ? v : nullptr,
                         delta_partials ? pl->args.pdd_loc : nullptr));
    in = o;
  }
  return MGP_OK;
}

// the one collective of an iteration: this rank's slice of w[par] and its partials, grouped
int enqueue_gather(PcgPlan* pl, int par, hipStream_t st) {
  if (!pl->comm) return MGP_OK;        // no communicator: a single rank, or virtual ranks sharing the buffers
  // (with a communicator of size 1 the in-place gathers are issued all the same: that is how the RCCL path and its
  // graph capture are exercised on a one-GPU box)
  const PcgArgs& a = pl->args;
  const int count = a.world * a.nbu;
  ncclResult_t r = ncclGroupStart();
  if (r != ncclSuccess) return 1000 + (int)r;
  int rc = MGP_OK;
  r = ncclAllGather(a.w[par] + a.row0, a.w[par], (size_t)a.n_loc, ncclFloat, pl->comm, st);
  if (r != ncclSuccess) rc = 1000 + (int)r;
  for (int k = 0; k < 2 && rc == MGP_OK; ++k) {
    float* seg = a.pd[par] + (size_t)k * count;
    r = ncclAllGather(seg + (size_t)a.rank * a.nbu, seg, (size_t)a.nbu, ncclFloat, pl->comm, st);
    if (r != ncclSuccess) rc = 1000 + (int)r;
  }
  r = ncclGroupEnd();                                  // always closed, also on error
  if (rc == MGP_OK && r != ncclSuccess) rc = 1000 + (int)r;
  return rc;
}

// all-gather of one global-length vector whose own rows this rank has just written (+ the partials of pd[0])
int enqueue_gather_vec(PcgPlan* pl, float* buf, bool with_partials, hipStream_t st) {
  if (!pl->comm) return MGP_OK;
  const PcgArgs& a = pl->args;
  const int count = a.world * a.nbu;
  ncclResult_t r = ncclGroupStart();
  if (r != ncclSuccess) return 1000 + (int)r;
  int rc = MGP_OK;
  r = ncclAllGather(buf + a.row0, buf, (size_t)a.n_loc, ncclFloat, pl->comm, st);
  if (r != ncclSuccess) rc = 1000 + (int)r;
  for (int k = 0; with_partials && k < 2 && rc == MGP_OK; ++k) {
    float* seg = a.pd[0] + (size_t)k * count;
    r = ncclAllGather(seg + (size_t)a.rank * a.nbu, seg, (size_t)a.nbu, ncclFloat, pl->comm, st);
    if (r != ncclSuccess) rc = 1000 + (int)r;
  }
  r = ncclGroupEnd();
  if (rc == MGP_OK && r != ncclSuccess) rc = 1000 + (int)r;
  return rc;
}

// collective A of the Chronopoulos-Gear form: the delta partials of every rank
int enqueue_gather_delta(PcgPlan* pl, hipStream_t st) {
  if (!pl->comm) return MGP_OK;
  const PcgArgs& a = pl->args;
  ncclResult_t r = ncclAllGather(a.pdd + a.rank, a.pdd, 1, ncclFloat, pl->comm, st);
  return r == ncclSuccess ? MGP_OK : 1000 + (int)r;
}

// collective B: the u = r slices of w[par] and the gamma partials of pd[par], grouped
int enqueue_gather_u(PcgPlan* pl, int par, hipStream_t st) {
  if (!pl->comm) return MGP_OK;
  const PcgArgs& a = pl->args;
  ncclResult_t r = ncclGroupStart();
  if (r != ncclSuccess) return 1000 + (int)r;
  int rc = MGP_OK;
  r = ncclAllGather(a.w[par] + a.row0, a.w[par], (size_t)a.n_loc, ncclFloat, pl->comm, st);
  if (r != ncclSuccess) rc = 1000 + (int)r;
  if (rc == MGP_OK) {
    r = ncclAllGather(a.pd[par] + (size_t)a.rank * a.nbu, a.pd[par], (size_t)a.nbu, ncclFloat, pl->comm, st);
    if (r != ncclSuccess) rc = 1000 + (int)r;
  }
  r = ncclGroupEnd();
  if (rc == MGP_OK && r != ncclSuccess) rc = 1000 + (int)r;
  return rc;
}

int enqueue_start(PcgPlan* pl, const float* B, int round, hipStream_t st) {
  if (pl->recurrence == 1) {
    hipLaunchKernelGGL(cgp_start_kernel, dim3(pl->args.nbu), dim3(kBlock), 0, st, pl->args, B, round);
    MGP_LAUNCH_CHECK();
    return MGP_OK;
  }
  MGP_TRY(enqueue_apply(pl, B, pl->args.w[0], nullptr, nullptr, st));   // w_0 = A b on own rows
  hipLaunchKernelGGL(pcg_start_kernel, dim3(pl->args.nbu), dim3(kBlock), 0, st, pl->args, B, round);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// one iteration of parity `par`: q = A w[par] (own rows), update -> w[par ^ 1] slice + partials
int enqueue_iteration(PcgPlan* pl, int par, hipStream_t st) {
  MGP_TRY(enqueue_apply(pl, pl->args.w[par], pl->q, pl->args.state + 1, pl->args.state, st));
  hipLaunchKernelGGL(pcg_update_kernel, dim3(pl->args.nbu), dim3(kBlock), 0, st, pl->args);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// Chronopoulos-Gear form, the two halves of an iteration (a collective sits behind each)
int enqueue_cgp_apply(PcgPlan* pl, int par, hipStream_t st) {
  MGP_TRY(enqueue_apply(pl, pl->args.w[par], pl->q, pl->args.state + 1, pl->args.state, st, true));
  hipLaunchKernelGGL(cgp_delta_kernel, dim3(1), dim3(kBlock), 0, st, pl->args);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
int enqueue_cgp_update(PcgPlan* pl, hipStream_t st) {
  hipLaunchKernelGGL(cgp_update_kernel, dim3(pl->args.nbu), dim3(kBlock), 0, st, pl->args);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// one whole iteration of either recurrence WITH its collective(s): parity `par` in, `par ^ 1` out
int enqueue_step(PcgPlan* pl, int par, hipStream_t st) {
  if (pl->recurrence == 1) {
    MGP_TRY(enqueue_cgp_apply(pl, par, st));
    MGP_TRY(enqueue_gather_delta(pl, st));
    MGP_TRY(enqueue_cgp_update(pl, st));
    return enqueue_gather_u(pl, par ^ 1, st);
  }
  MGP_TRY(enqueue_iteration(pl, par, st));
  return enqueue_gather(pl, par ^ 1, st);
}

// Residual replacement at a chunk boundary (parity 0): the recurrences of r, w, s, z are re-anchored on what they
// stand for -- r = rhs - A x, w = A r, s = A p, z = A s -- which is what keeps the pipelined recurrence at the
// attainable accuracy of classic CG on ill-conditioned systems (file header).  4 applies + 5 gathers per chunk.
int enqueue_replacement(PcgPlan* pl, const float* rhs, hipStream_t st) {
  const PcgArgs& a = pl->args;
  const int egrid = (int)(mgp_cdiv(a.n_loc, kBlock) > 1024 ? 1024 : mgp_cdiv(a.n_loc, kBlock));
  float* tmp = pl->xfull;
  auto full_of = [&](const float* own) -> int {
    hipLaunchKernelGGL(pcg_copy_rows_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->args, tmp, own);
    MGP_LAUNCH_CHECK();
    return enqueue_gather_vec(pl, tmp, false, st);
  };
  MGP_TRY(full_of(a.x));
  MGP_TRY(enqueue_apply(pl, tmp, pl->q, nullptr, nullptr, st));
  hipLaunchKernelGGL(pcg_sub_rows_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->args, a.r, rhs, (const float*)pl->q);
  MGP_LAUNCH_CHECK();
  MGP_TRY(full_of(a.r));
  MGP_TRY(enqueue_apply(pl, tmp, a.w[0], nullptr, nullptr, st));
  MGP_TRY(full_of(a.p));
  MGP_TRY(enqueue_apply(pl, tmp, a.s, nullptr, nullptr, st));
  MGP_TRY(full_of(a.s));
  MGP_TRY(enqueue_apply(pl, tmp, a.z, nullptr, nullptr, st));
  hipLaunchKernelGGL(pcg_dots_kernel, dim3(a.nbu), dim3(kBlock), 0, st, pl->args, 0);
  MGP_LAUNCH_CHECK();
  return enqueue_gather(pl, 0, st);
}

void try_capture(PcgPlan* pl) {
  pl->graphs_tried = true;
  if (!pl->prm.use_graph || pl->virt) return;
  // Capture with RCCL calls inside is validated with a communicator of size 1 only (the build box has one GPU):
  // with more ranks the loop is launched eagerly unless MGP_PCG_GRAPH_DIST=1 asks for the capture
  if (pl->comm && pl->world > 1) {
    const char* e = getenv("MGP_PCG_GRAPH_DIST");
    if (!e || e[0] != '1') return;
  }
  if (hipStreamCreateWithFlags(&pl->cap_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return; }
  bool ok = hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
  if (ok) {
    int rc = MGP_OK;
    // a chunk is an even number of iterations: it starts and ends on parity 0
    for (int i = 0; i < pl->chunk && rc == MGP_OK; ++i) rc = enqueue_step(pl, i & 1, pl->cap_stream);
    hipGraph_t graph = nullptr;
    const hipError_t e2 = hipStreamEndCapture(pl->cap_stream, &graph);
    ok = rc == MGP_OK && e2 == hipSuccess && graph != nullptr;
    if (ok) ok = hipGraphInstantiate(&pl->exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
  }
  (void)hipGetLastError();
  pl->has_graph = ok;
}

}  // namespace

// floats of the buffers that virtual ranks share (w[2] and pd[2]); real ranks keep them in their own workspace
extern "C" size_t mgp_pcg_shared_floats(int64_t n_glob, int64_t n_loc, int world) {
  if (n_glob <= 0 || n_loc <= 0 || world < 1) return 0;
  // w[2], pd[2] (gamma + delta partials per update workgroup), pdd (one delta per rank)
  return 2 * (size_t)n_glob + 2 * 2 * (size_t)world * nbu_for(n_loc) + (size_t)world + 64;
}

extern "C" size_t mgp_pcg_workspace_bytes(int64_t n_glob, int64_t n_loc, int world) {
  if (n_glob <= 0 || n_loc <= 0 || world < 1) return 0;
  return (pcg_private_floats(n_glob) + mgp_pcg_shared_floats(n_glob, n_loc, world)) * sizeof(float) + 16 * 256;
}

// op->L: the tile view of the WHOLE (padded) graph over this rank's row order [own rows, ghost layers, rest]
// (mgp_graph_tiles with `order`; tile_rowptr / tile_vals / tile_rowid set), vectors pre / post / diag at the global
// length.  launch_rows[s]: rows of the view launch s of the chain covers (own rows + (nu - 1 - s) ghost layers, a
// multiple of the tile height; launch_rows[nu - 1] = n_loc).  shared (nullable): w / partial buffers shared between
// virtual ranks (mgp_pcg_shared_floats).  Forms 0 and 2, C = 1.
extern "C" int mgp_pcg_plan_create(const mgp_operator_t* op, const int64_t* launch_rows, int64_t row0, int64_t n_loc,
                                   int64_t n_real, void* comm, int rank, int world, float* shared, int recurrence,
                                   const mgp_cg_params_t* params, void* work, size_t work_bytes, void* stream,
                                   void** plan_out) {
  if (!op || !launch_rows || !params || !work || !plan_out || !mgp_spmv_lanes_ok(op->L.spmv_lanes)) return MGP_ERR_ARG;
  if (recurrence != 0 && recurrence != 1) return MGP_ERR_ARG;
  if (op->nu < 1 || op->nu > kMaxNu || (op->form != 0 && op->form != 2)) return MGP_ERR_UNSUPPORTED;
  if (world < 1 || rank < 0 || rank >= world || n_loc <= 0 || row0 < 0) return MGP_ERR_ARG;
  const int64_t n_glob = op->L.n;
  if (row0 + n_loc > n_glob || n_real > n_glob) return MGP_ERR_ARG;
  if (!op->L.tile_ptr || !op->L.tile_cols || !op->L.lid || op->L.tile_rows <= 0) return MGP_ERR_UNSUPPORTED;
  if (world > 1 && (!op->L.tile_rowptr || !op->L.tile_vals || !op->L.tile_rowid)) return MGP_ERR_ARG;
  if (world > 1 && row0 != (int64_t)rank * n_loc) return MGP_ERR_ARG;     // equal contiguous blocks (all-gather layout)
  for (int s = 0; s < op->nu; ++s) {
    if (launch_rows[s] <= 0 || launch_rows[s] > n_glob) return MGP_ERR_ARG;
    if (launch_rows[s] % op->L.tile_rows != 0 && launch_rows[s] != n_glob) return MGP_ERR_ARG;
    if (s > 0 && launch_rows[s] > launch_rows[s - 1]) return MGP_ERR_ARG;
  }
  if (launch_rows[op->nu - 1] < n_loc) return MGP_ERR_ARG;
  if ((int64_t)world * nbu_for(n_loc) > (int64_t)kMaxSlots * kBlock) return MGP_ERR_UNSUPPORTED;
  // the boundary contract: scratch is the size the query returns, whether or not the caller brings the shared buffers (a virtual
  // rank's plan carves less, but the query cannot know and a caller must not learn to pass less)
  if (work_bytes < mgp_pcg_workspace_bytes(n_glob, n_loc, world)) return MGP_ERR_WORKSPACE;
  PcgPlan* pl = new (std::nothrow) PcgPlan();
  if (!pl) return MGP_ERR_ARG;
  memset(pl, 0, sizeof(*pl));
  pl->op = mgp_operator_copy(op);
  pl->recurrence = recurrence;
  memcpy(pl->launch_rows, launch_rows, sizeof(int64_t) * op->nu);
  pl->comm = static_cast<ncclComm_t>(comm);
  pl->world = world; pl->rank = rank;
  pl->virt = world > 1 && comm == nullptr;
  pl->prm = *params;
  if (pl->prm.max_iter <= 0) pl->prm.max_iter = 1000;
  if (pl->prm.min_iter < 0) pl->prm.min_iter = 0;
  pl->chunk = pl->prm.check_every > 0 ? pl->prm.check_every : 8;
  pl->chunk += pl->chunk & 1;                                    // even: a chunk starts and ends on parity 0
  pl->stream = mgp_stream(stream);
  pl->n_glob = n_glob;
  MgpArena ar(work, work_bytes);
  PcgArgs& a = pl->args;
  a.row0 = row0; a.n_loc = n_loc; a.n_real = n_real;
  a.x = ar.take<float>(n_glob); a.r = ar.take<float>(n_glob); a.p = ar.take<float>(n_glob);
  a.s = ar.take<float>(n_glob); a.z = ar.take<float>(n_glob);
  pl->q = ar.take<float>(n_glob); a.q = pl->q;
  pl->t0 = ar.take<float>(n_glob); pl->t1 = ar.take<float>(n_glob);
  pl->xfull = ar.take<float>(n_glob); pl->rfull = ar.take<float>(n_glob);
  pl->xacc = ar.take<double>(n_glob);
  a.scal = ar.take<float>(16);
  a.state = reinterpret_cast<int*>(ar.take<float>(16));
  a.nbu = nbu_for(n_loc);
  a.world = world; a.rank = rank;
  const size_t npd = 2 * (size_t)world * a.nbu;
  {
    mgp_csr_t Ll = op->L;
    Ll.n = launch_rows[op->nu - 1];
    a.nb2 = mgp_spmm_dot_blocks_for(&Ll, 1);
  }
  if (a.nb2 <= 0 || a.nb2 > kMaxSlots * kBlock || world > kMaxSlots * kBlock) { delete pl; return MGP_ERR_UNSUPPORTED; }
  a.pdd_loc = ar.take<float>(a.nb2);
  float* sh = shared ? shared : ar.take<float>(mgp_pcg_shared_floats(n_glob, n_loc, world));
  if (sh) {
    a.w[0] = sh; a.w[1] = sh + n_glob;
    a.pd[0] = sh + 2 * (size_t)n_glob; a.pd[1] = a.pd[0] + npd;
    a.pdd = a.pd[1] + npd;
  }
  a.tol = pl->prm.tol; a.max_iter = pl->prm.max_iter; a.min_iter = pl->prm.min_iter; a.stop_mode = pl->prm.stop_mode;
  if (!ar.ok() || !sh) { delete pl; return MGP_ERR_WORKSPACE; }
  hipError_t e = hipHostMalloc((void**)&pl->host_state, 16 * sizeof(int32_t), hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostMalloc((void**)&pl->host_resid, 4 * sizeof(float), hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&a.host_state, pl->host_state, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&a.host_resid, pl->host_resid, 0);
  if (e == hipSuccess) e = hipHostMalloc((void**)&pl->host_true_rel, 4 * sizeof(float), hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&pl->dev_true_rel, pl->host_true_rel, 0);
  if (e != hipSuccess) { delete pl; return (int)e; }
  *plan_out = pl;
  return MGP_OK;
}

// Lock-step driver for virtual ranks (and building block of the solve): phase 0 = first apply + start kernel (B read
// at the global length), phase 1 = one iteration of the parity the device state is at, given by the caller as `par`
// (0 for the first iteration after phase 0, alternating).  No collective is issued here.
extern "C" int mgp_pcg_plan_enqueue(void* plan, int phase, int par, const float* B) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  if (!pl || (phase == 0 && !B)) return MGP_ERR_ARG;
  if (phase == 0) { pl->host_state[1] = 0; return enqueue_start(pl, B, 0, pl->stream); }
  if (pl->recurrence == 1) return phase == 1 ? enqueue_cgp_apply(pl, par & 1, pl->stream) : enqueue_cgp_update(pl, pl->stream);
  return phase == 1 ? enqueue_iteration(pl, par & 1, pl->stream) : MGP_OK;
}

extern "C" int mgp_pcg_plan_poll(void* plan, int32_t* iters, float* resid, int32_t* status) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  if (!pl) return MGP_ERR_ARG;
  if (!pl->host_state[1]) return 1;                       // undecided
  if (iters) *iters = pl->host_state[0];
  if (status) *status = pl->host_state[2];
  if (resid) *resid = pl->host_resid[0];
  return MGP_OK;
}

// full solve (single rank, or one rank of an RCCL job): the solution is left in the plan's x buffer at the global
// length, own rows valid (mgp_pcg_plan_x); X (nullable): own rows copied to X[0 .. n_loc)
static int pcg_plan_solve_body(void* plan, const float* B, float* X_loc, int32_t* iters, float* resid, int32_t* status) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  if (!pl || !B) return MGP_ERR_ARG;
  if (pl->virt) return MGP_ERR_UNSUPPORTED;               // virtual ranks are driven by mgp_pcg_plan_enqueue
  hipStream_t st = pl->stream;
  const bool multi = pl->comm && pl->world > 1;     // waits are bounded (MGP_ERR_TIMEOUT): a dead peer must not hang this rank
  if (pl->solves++ >= 1 && !pl->graphs_tried) try_capture(pl);
  const int max_refine = pl->prm.max_refine > 0 ? pl->prm.max_refine : 0;
  const PcgArgs& a = pl->args;
  const int egrid = (int)(mgp_cdiv(a.n_loc, kBlock) > 1024 ? 1024 : mgp_cdiv(a.n_loc, kBlock));
  volatile int32_t* flag = pl->host_state + 1;
  int total_iters = 0, last_status = 0;
  const float* rhs = B;
  const auto t_begin = std::chrono::steady_clock::now();
  for (int round = 0; round <= max_refine; ++round) {
    pl->host_state[1] = 0;
    MGP_TRY(enqueue_start(pl, rhs, round, st));
    MGP_TRY(pl->recurrence == 1 ? enqueue_gather_u(pl, 0, st) : enqueue_gather(pl, 0, st));
    int guard = 0;
    for (;;) {
      if (pl->has_graph) {
        MGP_HIP_TRY(hipGraphLaunch(pl->exec, st));
      } else {
        for (int i = 0; i < pl->chunk; ++i) MGP_TRY(enqueue_step(pl, i & 1, st));
      }
      // every rank launches whole chunks; the decisions are bit-identical on all ranks and the flag only ever rises
      // inside the chunk that takes the decision, so all ranks stop behind the same chunk and their collective
      // sequences match -- whether a rank sees the flag while that chunk still drains (first chunk: the host reads
      // nothing but the flag for up to twice the previous solve's time, as in cg.hip) or after it has (blocking wait)
      if (guard == 0 && pl->last_solve_ns > 0) {
        const int64_t budget = 2 * pl->last_solve_ns + 20000;
        const auto t_spin = std::chrono::steady_clock::now();
        while (!*flag) {
          for (int spin = 0; spin < 64 && !*flag; ++spin) __builtin_ia32_pause();
          if (std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_spin).count() > budget) break;
        }
      }
      if (!*flag) MGP_STREAM_WAIT(st, multi);
      if (*flag) {
        if (guard == 0 && round == 0)
          pl->last_solve_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
        break;
      }
      pl->last_solve_ns = 0;
      if (++guard > pl->prm.max_iter / pl->chunk + 2) break;
      if (pl->chunk >= 16 && pl->recurrence == 0) MGP_TRY(enqueue_replacement(pl, rhs, st));   // long pipelined solves: re-anchor the recurrences
    }
    total_iters += pl->host_state[0];
    last_status = pl->host_state[2];
    if (max_refine == 0) break;
    // accumulate, gather the accumulated solution, true residual of the ORIGINAL system on own rows, gather it
    hipLaunchKernelGGL(pcg_accumulate_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->args, pl->xacc, pl->xfull, round == 0 ? 1 : 0);
    MGP_LAUNCH_CHECK();
    MGP_TRY(enqueue_gather_vec(pl, pl->xfull, false, st));
    MGP_TRY(enqueue_apply(pl, pl->xfull, pl->q, nullptr, nullptr, st));
    hipLaunchKernelGGL(pcg_residual_kernel, dim3(a.nbu), dim3(kBlock), 0, st, pl->args, B, pl->q, pl->rfull);
    MGP_LAUNCH_CHECK();
    MGP_TRY(enqueue_gather_vec(pl, pl->rfull, true, st));
    hipLaunchKernelGGL(pcg_refine_finalize_kernel, dim3(1), dim3(kBlock), 0, st, pl->args, pl->dev_true_rel);
    MGP_LAUNCH_CHECK();
    MGP_STREAM_WAIT(st, multi);
    pl->host_resid[0] = pl->host_true_rel[0];                         // `resid` reports the TRUE relative residual
    if (pl->host_true_rel[0] <= 2.0f * pl->prm.tol) { last_status = 1; break; }
    if (round == max_refine || last_status == 3) { if (last_status == 1) last_status = 2; break; }
    rhs = pl->rfull;
  }
  if (max_refine > 0) {
    hipLaunchKernelGGL(pcg_publish_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->args, pl->xacc);
    MGP_LAUNCH_CHECK();
    MGP_STREAM_WAIT(st, multi);
    pl->host_state[0] = total_iters;
    pl->host_state[2] = last_status;
  }
  if (X_loc) {
    MGP_HIP_TRY(hipMemcpyAsync(X_loc, pl->args.x + pl->args.row0, (size_t)pl->args.n_loc * sizeof(float),
                               hipMemcpyDeviceToDevice, st));
    MGP_STREAM_WAIT(st, multi);
  }
  if (iters) *iters = pl->host_state[0];
  if (status) *status = pl->host_state[2];
  if (resid) *resid = pl->host_resid[0];
  return MGP_OK;
}

extern "C" float* mgp_pcg_plan_x(void* plan) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  return pl ? pl->args.x : nullptr;
}

// MGP_ERR_TIMEOUT poisons the plan (cg.hip, mgp_cg_plan_solve): destroy then leaks instead of waiting on a dead peer
extern "C" int mgp_pcg_plan_solve(void* plan, const float* B, float* X_loc, int32_t* iters, float* resid, int32_t* status) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  if (pl && pl->poisoned) return MGP_ERR_TIMEOUT;
  const int rc = pcg_plan_solve_body(plan, B, X_loc, iters, resid, status);
  if (rc == MGP_ERR_TIMEOUT && pl) pl->poisoned = true;
  return rc;
}

extern "C" int mgp_pcg_plan_poisoned(void* plan) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  return pl && pl->poisoned ? 1 : 0;
}

extern "C" int mgp_pcg_plan_destroy(void* plan) {
  PcgPlan* pl = static_cast<PcgPlan*>(plan);
  if (!pl) return MGP_ERR_ARG;
  if (pl->poisoned) return MGP_OK;
  if (pl->exec) (void)hipGraphExecDestroy(pl->exec);
  if (pl->cap_stream) (void)hipStreamDestroy(pl->cap_stream);
  if (pl->host_state) (void)hipHostFree(pl->host_state);
  if (pl->host_resid) (void)hipHostFree(pl->host_resid);
  if (pl->host_true_rel) (void)hipHostFree(pl->host_true_rel);
  delete pl;
  return MGP_OK;
}
