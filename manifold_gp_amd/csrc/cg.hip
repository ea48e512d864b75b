// (Preconditioned) conjugate gradients for the precision-side operators, multi right-hand side.
//
// Replaces linear_operator.utils.linear_cg as reached from the reference at
// precision_matern_operator.py:53, schur_complement_operator.py:28 and train_model.py:68
// (per iteration there: one operator apply = s x (2 spmm + elementwise) launches, then ~15 tiny
// reduction / elementwise launches, host-side convergence test every iteration).
//
// MI355X design
//   * single-reduction (Chronopoulos-Gear) recurrence: per iteration ONE fused vector kernel
//     (p,s,x,r,u updates + the two dot products of the new residual) and the s SpMM launches of
//     the operator chain, whose last launch carries the third dot product (u . A u);
//   * dot products are per-workgroup partials reduced again, in a fixed order, by every
//     workgroup of the consuming kernel: no atomics, no separate reduction launch, bitwise
//     reproducible, and a kernel boundary (~1.5 us) is the only synchronisation;
//   * the iteration index and the convergence flag live in device memory, so whole solves are
//     hipGraphs: cg_init + k x (apply, update) is ONE launch (rhs pointer patched into the graph, k
//     follows the previous solves), longer solves continue with `check_every`-step graphs; launches
//     behind the stopping decision return after their first loads; graphs are captured at a plan's
//     second solve; the host polls the host-mapped decision word instead of sleeping on the stream;
//   * column freezing / stopping follow linear_cg (stop_mode 0) or a per-column relative
//     residual (stop_mode 1).
#include <math.h>
#include <chrono>
#include <mutex>
#include <new>
#include <vector>
#include <string.h>
#include <algorithm>
#include "mgp_common.h"
#include "mgp_internal.h"
#include "cg_rule.h"
#include "cg_policy.h"
#include "cg_handoff.h"

namespace {

#ifndef MGP_LAB_UPD
#define MGP_LAB_UPD 0      // lab builds (tools/lab/upd_bounds.sh): 4 = never converge, alpha = beta = 0; | 1 skip the partial reads; | 2 skip the vector pass
#endif

typedef float mgp_cg_v4f __attribute__((ext_vector_type(4)));

struct CgArgs {
  int64_t n;
  int C, TC, TS;
  float *x, *r, *u, *w, *p, *s;
  float* us;          // nullable: pre (.) u, the pre-scaled SpMM input (op->pre != NULL)
  const float* pre;   // op->pre
  const float* minv;
  float* pd_gamma;  // [2][nbv][C]
  float* pd_rr;     // [2][nbv][C]
  int nbv;
  const float* pd_delta;  // [nbs][C]
  int nbs;
  float* gamma_old;  // [2][C]
  float* alpha_old;  // [2][C]
  float* bb;         // [C]  ||b||^2
  float* resid;      // [C]  relative residual norm
  int* state;        // [0] iteration (1-based), [1] done, [2] status
  int* host_state;   // host-mapped mirror of state[0..3], written when the solve ends
  float* host_resid; // host-mapped [C]
  float tol;
  int max_iter, min_iter, stop_mode;
  int64_t rows_per_block;
  // init-free solve (C == 1, tile SpMV, no preconditioner): there is no cg_init launch -- the first apply read the
  // right-hand side itself, copied it to r and left the partials of ||b||^2 here (one slot per SpMV workgroup);
  // at iteration 1 the update takes gamma = ||r||^2 from them and treats p, s, x as zero.  NULL: classic start.
  const float* pd_bb;   // [nbs]
  // many columns (C > 16): cg_reduce_kernel has summed the partials of this step -> [3][C] gamma, ||r||^2, delta;
  // the update kernel reads 3 C floats instead of re-reducing (2 nbv + nbs) C of them in every workgroup.  NULL: off.
  float* tot;
  // quad form of the update (cg_update_q_kernel, C % 4 == 0): CQ = C / 4 column quads, TSQ row slices per workgroup (CQ * TSQ active threads)
  int CQ, TSQ;
  int* arrive;   // [9][32] arrival counters of the deciding update launch (8 groups + top, a 128-byte line each), zero between launches
};

// sh[k][sl * TC + cc] holds the partial of slice sl for column cc; result in sh[k][cc] for cc < TC.
// TC <= 64: the slices of a column sit TC lanes apart inside a wave -> xor-shuffle tree in registers,
// then one LDS hop across the four waves (1 barrier).  TC > 64: LDS tree over the remaining 1-2 slices.
// Fixed order in both cases (bitwise reproducible).  A single thread summing 256 LDS words serially
// cost ~2.5 us per call and an 8-barrier LDS tree ~1 us (profiled).
template <int K>
__device__ __forceinline__ void reduce_slices(float (*sh)[kBlock], int TC, int TS, int sl, int cc) {
  const int tid = threadIdx.x;
  if (TC <= 64) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k][tid];
    for (int o = TC; o < 64; o <<= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    __syncthreads();                       // everyone has read its own slot
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < TC) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][wave * 64 + lane] = v[k];
    }
    __syncthreads();
    if (tid < TC) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][tid] = (sh[k][tid] + sh[k][64 + tid]) + (sh[k][128 + tid] + sh[k][192 + tid]);
    }
    __syncthreads();
    return;
  }
  for (int stride = TS >> 1; stride > 0; stride >>= 1) {
    __syncthreads();
    if (sl < stride) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][sl * TC + cc] += sh[k][(sl + stride) * TC + cc];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void cg_init_kernel(CgArgs a, const float* __restrict__ B) {
  __shared__ float sh[2][kBlock];
  const int tid = threadIdx.x, cc = tid % a.TC, sl = tid / a.TC;
  const int lb = mgp_xcd_block(blockIdx.x, gridDim.x);
  const int64_t r0 = (int64_t)lb * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  if (blockIdx.x == 0 && tid == 0) { a.state[0] = 0; a.state[1] = 0; a.state[2] = 0; }   // the first apply ticks it to 1
  float g = 0.f, rr = 0.f;
  if (cc < a.C) {
    for (int64_t r = r0 + sl; r < r1; r += a.TS) {
      const int64_t i = r * a.C + cc;
      const float b = B[i];
      const float u = a.minv ? a.minv[r] * b : b;
      a.x[i] = 0.f; a.p[i] = 0.f; a.s[i] = 0.f;
      a.r[i] = b;
      if (a.minv) a.u[i] = u;
      if (a.us) a.us[i] = a.pre[r] * u;
      g = fmaf(b, u, g);
      rr = fmaf(b, b, rr);
    }
  }
  sh[0][tid] = g; sh[1][tid] = rr;
  reduce_slices<2>(sh, a.TC, a.TS, sl, cc);
  if (tid < a.TC && tid < a.C) {
    a.pd_gamma[(int64_t)blockIdx.x * a.C + tid] = sh[0][tid];   // parity slot 0 = "previous" of iteration 1
    a.pd_rr[(int64_t)blockIdx.x * a.C + tid] = sh[1][tid];
  }
}

// ---- Partial sums of one step, many columns.  cg_update_kernel lets every workgroup re-reduce all partials, which is
// the cheapest scheme while they are few: at C = 100 on the 60k graph it is 256 workgroups x (2 x 2 x 256 + 3750
// SpMM blocks) x 100 columns = 490 MB of L2 reads per launch, more than the vectors themselves (240 MB) -- profiled:
// 103 us per update against 89 us per SpMM.  Here each (array, 4-column group) is summed ONCE by one workgroup --
// 64 slices x 4 columns, slice sl takes blocks sl, sl + 64, ... in batches of 16 independent loads, xor tree inside
// the wave, four waves through LDS: a fixed order -- and the update reads the 3 C totals.
__global__ __launch_bounds__(kBlock) void cg_reduce_kernel(CgArgs a) {
  __shared__ float sh[kBlock / 64][4];
  const int st_it = a.state[0], st_done = a.state[1];
  if (st_done) return;
  const int prev = (st_it & 1) ^ 1;
  const int tid = threadIdx.x, cc = tid & 3, sl = tid >> 2;
  const int c = blockIdx.x * 4 + cc;
  const int cl = c < a.C ? c : a.C - 1;
  const int k = blockIdx.y;
  const int nb = (k == 2) ? a.nbs : a.nbv;
  const float* __restrict__ src = (k == 0) ? a.pd_gamma + (int64_t)prev * a.nbv * a.C
                                : (k == 1) ? a.pd_rr + (int64_t)prev * a.nbv * a.C : a.pd_delta;
  float t = 0.f;
  constexpr int U = 16;
  for (int b0 = sl; b0 < nb; b0 += U * 64) {
    float v[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int b = b0 + q * 64;
      v[q] = src[(int64_t)(b < nb ? b : nb - 1) * a.C + cl];
    }
#pragma unroll
    for (int q = 0; q < U; ++q) t += (b0 + q * 64 < nb) ? v[q] : 0.f;
  }
  for (int o = 4; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
  if ((tid & 63) < 4) sh[tid >> 6][cc] = t;
  __syncthreads();
  if (tid < 4 && c < a.C) a.tot[(int64_t)k * a.C + c] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// ---- One step of the multi-column update kernels (cg_update_kernel, cg_update_q_kernel), from "thread c < C holds the totals
// of column c" to "sh_alpha / sh_beta hold this step's coefficients": the rule of cg_rule.h per column, gamma_old / alpha_old /
// bb / resid written by workgroup 0, the block's stopping decision taken by thread 0 and published.  Returns true, in every
// thread, when the solve has ended.  `go` / `ao` are the previous step's gamma / alpha (the caller selects the parity);
// `lab`: MGP_LAB_UPD builds never converge and hold the vectors still (alpha = beta = 0); max_iter still ends them.
__device__ __forceinline__ bool cg_columns_step(const CgArgs& a, int it, float gamma, float rr, float delta, float go, float ao,
                                                float bb_old, bool lab, float* sh_alpha, float* sh_beta, float* sh_rel,
                                                int* sh_done) {
  const int tid = threadIdx.x, C = a.C, par = it & 1;
  if (tid < C) {
    const float bb = (it == 1) ? rr : bb_old;
    const float rel = cg_rel(rr, bb);
    sh_rel[tid] = rel;
    CgCoef k = cg_coef(it == 1, cg_frozen(a.stop_mode, a.tol, rel), gamma, delta, go, ao);
    if (lab) { k.alpha = 0.f; k.beta = 0.f; }
    sh_alpha[tid] = k.alpha;
    sh_beta[tid] = k.beta;
    if (blockIdx.x == 0) {
      a.gamma_old[par * C + tid] = gamma;
      a.alpha_old[par * C + tid] = k.alpha;
      if (it == 1) a.bb[tid] = bb;
      a.resid[tid] = rel;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const CgStop st = lab ? cg_stop_rest(0, true, a.max_iter, it)
                          : cg_stop_columns(a.stop_mode, a.min_iter, a.max_iter, a.tol, it, sh_rel, C);
    *sh_done = st.done;
    if (st.done && blockIdx.x == 0) cg_publish(a.state, a.host_state, a.host_resid, sh_rel, C, it, st.status);
  }
  __syncthreads();
  return *sh_done != 0;
}

__global__ __launch_bounds__(kBlock) void cg_update_kernel(CgArgs a) {
  __shared__ float sh[3][kBlock];
  __shared__ float sh_alpha[kMaxC], sh_beta[kMaxC], sh_rel[kMaxC];
  __shared__ int sh_done;
  __shared__ int sh_state[2];
  const int tid = threadIdx.x, cc = tid % a.TC, sl = tid / a.TC;
  const int C = a.C;
  // Every first touch of a line in a kernel is served from beyond L2 (~0.7 us), so the prologue is ONE
  // round trip: iteration counter + done flag, the dot partials of BOTH parities and gamma_old / alpha_old
  // of both parities are all requested before the first wait; the parity (a function of the iteration
  // counter) only selects among values already in registers.
  const int st_it = a.state[0], st_done = a.state[1];

  const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  const int64_t rf = r0 + sl;
  // ---- every workgroup reduces the partials in the same fixed order: thread (sl, cc) sums
  // partials sl, sl+TS, ... of column cc with independent loads, LDS combines the TS slices
  float g2[2] = {0.f, 0.f}, rr2[2] = {0.f, 0.f}, d = 0.f;
  float go2[2] = {0.f, 0.f}, ao2[2] = {0.f, 0.f}, bb_old = 0.f;
  if (a.tot) {
    // totals of this step from cg_reduce_kernel: slice 0 carries them through the slice reduction below
    if (cc < C && sl == 0) {
      g2[0] = g2[1] = a.tot[cc];
      rr2[0] = rr2[1] = a.tot[C + cc];
      d = a.tot[2 * C + cc];
    }
  } else if (cc < C && !(MGP_LAB_UPD & 1)) {
    // batches of 8 / 32 loads on clamped indices, masked afterwards: all in flight together (one round trip per
    // batch: with 256 workgroups and TS = 16 slices the gamma / rr partials are two batches, the ~940 delta
    // partials of a 12-column SpMM two as well)
    constexpr int UG = 8, UD = 32;
    // the first two batches of each array are requested TOGETHER (128 loads per lane in flight: the whole reduction of
    // a 12-column solve on the 60k graph, 256 + 938 partial rows, in one round trip instead of four); sums in the same
    // order as before
    float gv0[2][2][UG], rv0[2][2][UG], dv0[2][UD];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int b0 = sl + t * UG * a.TS;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* pg = a.pd_gamma + (int64_t)h * a.nbv * C;
        const float* pr = a.pd_rr + (int64_t)h * a.nbv * C;
#pragma unroll
        for (int q = 0; q < UG; ++q) {
          const int b = b0 + q * a.TS;
          const int bc = b < a.nbv ? b : a.nbv - 1;
          gv0[t][h][q] = pg[(int64_t)bc * C + cc];
          rv0[t][h][q] = pr[(int64_t)bc * C + cc];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int b0 = sl + t * UD * a.TS;
#pragma unroll
      for (int q = 0; q < UD; ++q) {
        const int b = b0 + q * a.TS;
        const int bc = b < a.nbs ? b : a.nbs - 1;
        dv0[t][q] = a.pd_delta[(int64_t)bc * C + cc];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int b0 = sl + t * UG * a.TS;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < UG; ++q) {
          const bool on = b0 + q * a.TS < a.nbv;
          g2[h] += on ? gv0[t][h][q] : 0.f;
          rr2[h] += on ? rv0[t][h][q] : 0.f;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int b0 = sl + t * UD * a.TS;
#pragma unroll
      for (int q = 0; q < UD; ++q) d += (b0 + q * a.TS < a.nbs) ? dv0[t][q] : 0.f;
    }
    for (int b0 = sl + 2 * UG * a.TS; b0 < a.nbv; b0 += UG * a.TS) {
      float gv[2][UG], rv[2][UG];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* pg = a.pd_gamma + (int64_t)h * a.nbv * C;
        const float* pr = a.pd_rr + (int64_t)h * a.nbv * C;
#pragma unroll
        for (int q = 0; q < UG; ++q) {
          const int b = b0 + q * a.TS;
          const int bc = b < a.nbv ? b : a.nbv - 1;
          gv[h][q] = pg[(int64_t)bc * C + cc];
          rv[h][q] = pr[(int64_t)bc * C + cc];
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < UG; ++q) {
          const bool on = b0 + q * a.TS < a.nbv;
          g2[h] += on ? gv[h][q] : 0.f;
          rr2[h] += on ? rv[h][q] : 0.f;
        }
      }
    }
    for (int b0 = sl + 2 * UD * a.TS; b0 < a.nbs; b0 += UD * a.TS) {
      float dv[UD];
#pragma unroll
      for (int q = 0; q < UD; ++q) {
        const int b = b0 + q * a.TS;
        const int bc = b < a.nbs ? b : a.nbs - 1;
        dv[q] = a.pd_delta[(int64_t)bc * C + cc];
      }
#pragma unroll
      for (int q = 0; q < UD; ++q) d += (b0 + q * a.TS < a.nbs) ? dv[q] : 0.f;
    }
  }
  if (tid < C) {
    go2[0] = a.gamma_old[tid]; go2[1] = a.gamma_old[C + tid];
    ao2[0] = a.alpha_old[tid]; ao2[1] = a.alpha_old[C + tid];
    bb_old = a.bb[tid];
  }
  // workgroup 0 may raise the done flag while this launch runs: one thread's view is published to
  // the whole workgroup so that all its waves take the same branch
  if (tid == 0) { sh_state[0] = st_it; sh_state[1] = st_done; }
  __syncthreads();
  if (sh_state[1]) return;
  const int it = sh_state[0];
  const int par = it & 1, prev = par ^ 1;
  const float g = prev ? g2[1] : g2[0], rr = prev ? rr2[1] : rr2[0];
  sh[0][tid] = g; sh[1][tid] = rr; sh[2][tid] = d;
  reduce_slices<3>(sh, a.TC, a.TS, sl, cc);
  float gamma = 0.f, rrn = 0.f, delta = 0.f;
  if (tid < C) { gamma = sh[0][tid]; rrn = sh[1][tid]; delta = sh[2][tid]; }
  if (cg_columns_step(a, it, gamma, rrn, delta, prev ? go2[1] : go2[0], prev ? ao2[1] : ao2[0], bb_old, MGP_LAB_UPD != 0,
                      sh_alpha, sh_beta, sh_rel, &sh_done)) return;

  // ---- fused vector update over this workgroup's contiguous rows
  float ng = 0.f, nrr = 0.f;
  if (cc < C && !(MGP_LAB_UPD & 2)) {
    const float alpha = sh_alpha[cc], beta = sh_beta[cc];
    // eight row passes per batch, all their loads (clamped rows, masked afterwards) in flight before the
    // first use: with one pass at a time a workgroup's 30 passes were 30 dependent round trips (27 us per
    // launch at 60k x 12); the per-element arithmetic and the order of the two running sums are unchanged
    constexpr int U = 8;
    for (int64_t rb = rf; rb < r1; rb += (int64_t)U * a.TS) {
      float un[U], po[U], so[U], wo[U], xo[U], ro[U], mo[U], pr[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t r = rb + (int64_t)k * a.TS;
        const int64_t rc = r < r1 ? r : rf;
        const int64_t i = rc * C + cc;
        un[k] = a.u[i]; po[k] = a.p[i]; so[k] = a.s[i]; wo[k] = a.w[i]; xo[k] = a.x[i]; ro[k] = a.r[i];
        mo[k] = a.minv ? a.minv[rc] : 1.f;
        pr[k] = a.us ? a.pre[rc] : 1.f;
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t r = rb + (int64_t)k * a.TS;
        if (r < r1) {
          const int64_t i = r * C + cc;
          const float p = fmaf(beta, po[k], un[k]);
          const float s = fmaf(beta, so[k], wo[k]);
          a.p[i] = p;
          a.s[i] = s;
          a.x[i] = fmaf(alpha, p, xo[k]);
          const float rn = fmaf(-alpha, s, ro[k]);
          a.r[i] = rn;
          float u2 = rn;
          if (a.minv) { u2 = mo[k] * rn; a.u[i] = u2; }
          if (a.us) a.us[i] = pr[k] * u2;
          ng = fmaf(rn, u2, ng);
          nrr = fmaf(rn, rn, nrr);
        }
      }
    }
  }
  __syncthreads();
  sh[0][tid] = ng; sh[1][tid] = nrr;
  reduce_slices<2>(sh, a.TC, a.TS, sl, cc);
  if (tid < a.TC && tid < C) {
    a.pd_gamma[((int64_t)par * a.nbv + blockIdx.x) * C + tid] = sh[0][tid];
    a.pd_rr[((int64_t)par * a.nbv + blockIdx.x) * C + tid] = sh[1][tid];
  }
}

// ---- Quad form of the update for C % 4 == 0 (the column counts of training: 12 probes, 32, 100 one-hot columns).
// cg_update_kernel gives a lane one (row, column) ELEMENT: dword loads and stores, cg_tile_cols(C) - C lanes idle (12 of 16, 100 of 128),
// a wave's stores covering 48-byte rows.  Here the [n, C] arrays are streams of float4: thread (slq, cq) owns column quad cq of the
// rows slq, slq + TSQ, ... of its workgroup's contiguous row range -- CQ * TSQ of BLOCK threads active (255 of 256 at C = 12, 250
// at C = 100), every load / store a dwordx4, a wave's accesses 1 KB contiguous.  Same arithmetic per element, same
// single-reduction recurrence, same decision code as cg_update_kernel; the per-column sums run in a fixed order (rows of a slice in
// order, slices in groups, groups left to right): bitwise reproducible, but not the order of cg_update_kernel.
// Launched behind cg_reduce_kernel only (C > 16: the step's totals are 3 C floats).  Measured on the 60k graph, C = 100, Jacobi +
// pre-scaling on (12 arrays, tools/lab/cg12.py): 57.7 -> 50.3 us per launch.  For 2 <= C <= 16, where every workgroup re-reduces
// the partials itself, the same form was slower than cg_update_kernel (12.2 us: 15.4 in 1024-thread workgroups, 17.4 in 512) and
// is not used.
template <int K, int BLOCK>
__device__ __forceinline__ void reduce_quads(mgp_cg_v4f (*shq)[BLOCK], float (*sh2)[BLOCK], float (*out)[kMaxC], const mgp_cg_v4f* v,
                                             bool act, int C, int TSQ) {
  // shq[k] as floats is P[slq][c] (flat slq * C + c): phase A every active thread stores its quad; phase B thread (g, c), g < G,
  // sums the rows g, g + G, ... of column c; phase C thread c sums the G group values
  const int tid = threadIdx.x;
  if (act) {
#pragma unroll
    for (int k = 0; k < K; ++k) shq[k][tid] = v[k];
  }
  __syncthreads();
  int G = BLOCK / C;
  if (G > 32) G = 32;
  if (G > TSQ) G = TSQ;
  const int g = tid / C, c = tid - g * C;
  if (g < G) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* P = reinterpret_cast<const float*>(shq[k]);
      float t = 0.f;
      for (int r = g; r < TSQ; r += G) t += P[r * C + c];
      sh2[k][tid] = t;
    }
  }
  __syncthreads();
  if (tid < C) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float t = 0.f;
      for (int q = 0; q < G; ++q) t += sh2[k][q * C + tid];
      out[k][tid] = t;
    }
  }
  __syncthreads();
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void cg_update_q_kernel(CgArgs a) {
  __shared__ mgp_cg_v4f shq[2][BLOCK];
  __shared__ float sh2[2][BLOCK];
  __shared__ float sh_tot[2][kMaxC];
  __shared__ __attribute__((aligned(16))) float sh_alpha[kMaxC];
  __shared__ __attribute__((aligned(16))) float sh_beta[kMaxC];
  __shared__ float sh_rel[kMaxC];
  __shared__ int sh_done;
  __shared__ int sh_state[2];
  const int tid = threadIdx.x;
  const int C = a.C, CQ = a.CQ, TSQ = a.TSQ;
  const bool act = tid < CQ * TSQ;
  const int slq = tid / CQ, cq = tid - slq * CQ;
  // one round trip for everything the prologue needs (first touches of a line come from beyond L2): state, the partials of BOTH
  // parities (or the step's totals), gamma_old / alpha_old of both parities -- the parity only selects among registers
  const int st_it = a.state[0], st_done = a.state[1];
  const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  const int64_t rf = r0 + slq;
  const mgp_cg_v4f z4 = {0.f, 0.f, 0.f, 0.f};
  float go2[2] = {0.f, 0.f}, ao2[2] = {0.f, 0.f}, bb_old = 0.f, tg = 0.f, trr = 0.f, td = 0.f;
  // (the step's totals come from cg_reduce_kernel: this form is only launched behind it)
  if (tid < C) { tg = a.tot[tid]; trr = a.tot[C + tid]; td = a.tot[2 * C + tid]; }
  if (tid < C) {
    go2[0] = a.gamma_old[tid]; go2[1] = a.gamma_old[C + tid];
    ao2[0] = a.alpha_old[tid]; ao2[1] = a.alpha_old[C + tid];
    bb_old = a.bb[tid];
  }
  if (tid == 0) { sh_state[0] = st_it; sh_state[1] = st_done; }
  __syncthreads();
  if (sh_state[1]) return;
  const int it = sh_state[0];
  const int par = it & 1, prev = par ^ 1;
  if (cg_columns_step(a, it, tg, trr, td, prev ? go2[1] : go2[0], prev ? ao2[1] : ao2[0], bb_old, false,
                      sh_alpha, sh_beta, sh_rel, &sh_done)) return;

  // ---- fused vector update: U row passes per batch, every load of a batch in flight before the first use
  mgp_cg_v4f ng = z4, nrr = z4;
  if (act) {
    const mgp_cg_v4f alpha = *reinterpret_cast<const mgp_cg_v4f*>(&sh_alpha[4 * cq]);
    const mgp_cg_v4f beta = *reinterpret_cast<const mgp_cg_v4f*>(&sh_beta[4 * cq]);
    const mgp_cg_v4f *U4 = reinterpret_cast<const mgp_cg_v4f*>(a.u), *W4 = reinterpret_cast<const mgp_cg_v4f*>(a.w);
    mgp_cg_v4f *P4 = reinterpret_cast<mgp_cg_v4f*>(a.p), *S4 = reinterpret_cast<mgp_cg_v4f*>(a.s), *X4 = reinterpret_cast<mgp_cg_v4f*>(a.x),
               *R4 = reinterpret_cast<mgp_cg_v4f*>(a.r);
    constexpr int U = 2;
    for (int64_t rb = rf; rb < r1; rb += (int64_t)U * TSQ) {
      mgp_cg_v4f un[U], po[U], so[U], wo[U], xo[U], ro[U];
      float mo[U], pr[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t r = rb + (int64_t)k * TSQ;
        const int64_t rc = r < r1 ? r : rf;
        const int64_t i = rc * CQ + cq;
        un[k] = U4[i]; po[k] = P4[i]; so[k] = S4[i]; wo[k] = W4[i]; xo[k] = X4[i]; ro[k] = R4[i];
        mo[k] = a.minv ? a.minv[rc] : 1.f;
        pr[k] = a.us ? a.pre[rc] : 1.f;
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t r = rb + (int64_t)k * TSQ;
        if (r < r1) {
          const int64_t i = r * CQ + cq;
          mgp_cg_v4f p, sv, xn, rn, u2;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            p[j] = fmaf(beta[j], po[k][j], un[k][j]);
            sv[j] = fmaf(beta[j], so[k][j], wo[k][j]);
            xn[j] = fmaf(alpha[j], p[j], xo[k][j]);
            rn[j] = fmaf(-alpha[j], sv[j], ro[k][j]);
            u2[j] = a.minv ? mo[k] * rn[j] : rn[j];
            ng[j] = fmaf(rn[j], u2[j], ng[j]);
            nrr[j] = fmaf(rn[j], rn[j], nrr[j]);
          }
          P4[i] = p; S4[i] = sv; X4[i] = xn; R4[i] = rn;
          if (a.minv) reinterpret_cast<mgp_cg_v4f*>(a.u)[i] = u2;
          if (a.us) {
            mgp_cg_v4f us;
#pragma unroll
            for (int j = 0; j < 4; ++j) us[j] = pr[k] * u2[j];
            reinterpret_cast<mgp_cg_v4f*>(a.us)[i] = us;
          }
        }
      }
    }
  }
  {
    const mgp_cg_v4f v[2] = {ng, nrr};
    reduce_quads<2, BLOCK>(shq, sh2, sh_tot, v, act, C, TSQ);
  }
  if (tid < C) {
    a.pd_gamma[((int64_t)par * a.nbv + blockIdx.x) * C + tid] = sh_tot[0][tid];
    a.pd_rr[((int64_t)par * a.nbv + blockIdx.x) * C + tid] = sh_tot[1][tid];
  }
}

// ---- C == 1 specialisation of cg_update_kernel (the GP-mean solve).  Same arithmetic per element,
// but built for latency: at N = 60k the kernel is a chain of dependent waits, not bandwidth.
//   * ONE memory round trip: state, both parities of the gamma / rr partials (<= 2 per lane), the
//     delta partials (<= 16 per lane), gamma_old / alpha_old of both parities and the lane's first
//     vector element are all requested before the first wait;
//   * TWO barriers: the wave sums of the five partial totals and the state words cross the
//     workgroup through LDS once, then EVERY lane derives alpha, beta and the stopping decision
//     redundantly (no broadcast round), and the new partials take the second barrier.
// Summation order is fixed (lane slots in order, xor tree, (w0 + w1) + (w2 + w3)).
// The scalar block (CgScalars) and the hand-off of the deciding launch are in cg_handoff.h, shared with the folded step
// (spmv_tile_cgstep_kernel, spmm.hip).
//
// DECIDE (the LAST update of a plan's first graph): the workgroup whose partials arrive last also takes the stopping decision
// of the NEXT step -- ||r_k||^2 summed over the partials this very launch wrote, in cg_decide_c1_kernel's order, decided by
// cg_rule.h -- and leaves the end-of-graph mark.  The single-workgroup decision launch + the marker launch (4.5 + 4.0 us
// and two kernel boundaries of a ~57 us solve at N = 60k) go away (cg_handoff_decide).
__device__ __forceinline__ CgHandoff cg_handoff_of(const CgArgs& a) {
  return CgHandoff{a.arrive, a.state, a.host_state, a.resid, a.tol, a.max_iter, a.min_iter, a.stop_mode};
}

// DS: slots of 256 SpMV-workgroup partials a lane sums (4 covers nbs <= 1024, i.e. graphs up to 65 536 nodes: each slot is two
// loads with their address arithmetic -- 24 fewer loads in front of the kernel's one wait than the general 16)
template <bool DECIDE, int DS>
__global__ __launch_bounds__(kBlock) void cg_update_c1_kernel(CgArgs a) {
  __shared__ float sh_w[kBlock / 64][6];
  __shared__ float sh_o[kBlock / 64][2];
  __shared__ int sh_state[2];
  __shared__ int sh_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CgScalars sc = *reinterpret_cast<const CgScalars*>(a.gamma_old);
  const int st_it = sc.it, st_done = sc.done;
#ifdef MGP_STAMP
  if (blockIdx.x == 0 && tid == 0) {
    const int si = atomicAdd(a.state + 8, 1);
    reinterpret_cast<unsigned long long*>(a.state + 16)[si & 255] = wall_clock64() * 8 + 2;
  }
#endif
  // same block -> XCD -> row-range mapping as the SpMV kernels (mgp_xcd_block): the vector slices this
  // workgroup writes are the ones the SpMV workgroups of the same XCD read next, and vice versa
  const int lb = mgp_xcd_block(blockIdx.x, gridDim.x);
  const int64_t r0 = (int64_t)lb * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  const int64_t rf = r0 + tid;
  const int64_t rs = rf < r1 ? rf : 0;
  const float f_u = a.u[rs], f_p = a.p[rs], f_s = a.s[rs], f_w = a.w[rs], f_x = a.x[rs], f_r = a.r[rs];
  const float l_m = (a.minv ? a.minv : a.x)[rs], l_pre = (a.us ? a.pre : a.x)[rs];
  const float f_m = a.minv ? l_m : 1.f, f_pre = a.us ? l_pre : 1.f;
  float gv[2][kC1GammaSlots], rv[2][kC1GammaSlots], dv[DS];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < kC1GammaSlots; ++q) {
      const int b = tid + q * kBlock;
      const int bc = b < a.nbv ? b : a.nbv - 1;
      gv[h][q] = a.pd_gamma[(int64_t)h * a.nbv + bc];
      rv[h][q] = a.pd_rr[(int64_t)h * a.nbv + bc];
    }
  }
  float bv[DS];
  const float* __restrict__ pbb = a.pd_bb ? a.pd_bb : a.pd_delta;     // stand-in: unconditional loads
#pragma unroll
  for (int q = 0; q < DS; ++q) {
    const int b = tid + q * kBlock;
    const int bc = b < a.nbs ? b : a.nbs - 1;
    dv[q] = a.pd_delta[bc];
    bv[q] = pbb[bc];
  }
  const float go0 = sc.go0, go1 = sc.go1, ao0 = sc.ao0, ao1 = sc.ao1;
  const float bb_old = sc.bb;
  float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < kC1GammaSlots; ++q) {
    const bool on = tid + q * kBlock < a.nbv;
    t[0] += on ? gv[0][q] : 0.f; t[1] += on ? gv[1][q] : 0.f;
    t[2] += on ? rv[0][q] : 0.f; t[3] += on ? rv[1][q] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < DS; ++q) {
    const bool on = tid + q * kBlock < a.nbs;
    t[4] += on ? dv[q] : 0.f;
    t[5] += on ? bv[q] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) t[k] = mgp_wave_sum(t[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sh_w[wave][k] = t[k];
  }
  // workgroup 0 may raise the done flag while this launch runs: one lane's view of the state is
  // published so that all waves of a workgroup take the same branch
  if (tid == 0) { sh_state[0] = st_it; sh_state[1] = st_done; }
  __syncthreads();
  const int it = sh_state[0];
  if (sh_state[1]) {
    // init-free solve, iteration 1, flag already up: the first apply reset it, so workgroup 0 raised it in THIS launch
    // (b = 0 or not finite) before this workgroup started -- the solve ends here and x, which nobody has
    // initialised, must still come out zero (every workgroup that gets to the decision itself does the same below)
    if (a.pd_bb != nullptr && it == 1) for (int64_t r = rf; r < r1; r += kBlock) a.x[r] = 0.f;
    if (DECIDE && blockIdx.x == 0 && tid == 0) cg_mark_end_of_graph(a.state, a.host_state);     // decided earlier: nobody arrives below
    return;
  }
  const int par = it & 1, prev = par ^ 1;
#pragma unroll
  for (int k = 0; k < 6; ++k) t[k] = (sh_w[0][k] + sh_w[1][k]) + (sh_w[2][k] + sh_w[3][k]);
  const bool fresh = a.pd_bb != nullptr && it == 1;       // init-free solve, first update: r = b, p = s = x = 0
  const float gamma = fresh ? t[5] : (prev ? t[1] : t[0]), rr2 = fresh ? t[5] : (prev ? t[3] : t[2]), delta = t[4];
  const float bb = (it == 1) ? rr2 : bb_old;
  // the rule of cg_rule.h, derived redundantly by every lane
  const float rel = cg_rel(rr2, bb);
  const CgCoef k = cg_coef(it == 1, cg_frozen(a.stop_mode, a.tol, rel), gamma, delta, prev ? go1 : go0, prev ? ao1 : ao0);
  const float alpha = k.alpha, beta = k.beta;
  const CgStop st = cg_stop(a.stop_mode, a.min_iter, a.max_iter, a.tol, it, rel);
  const int done = st.done;
  if (blockIdx.x == 0 && tid == 0) {
    a.gamma_old[par] = gamma;
    a.alpha_old[par] = alpha;
    if (it == 1) a.bb[0] = bb;
    // DECIDE and not done: the last arriver of this launch writes the residual of step it + 1 to the same word, possibly
    // through another XCD's L2 -- one writer per launch, so that the device value is defined
    if (!DECIDE || done) a.resid[0] = rel;
    if (done) cg_publish(a.state, a.host_state, a.host_resid, &rel, 1, it, st.status);
  }
  if (done) {
    // an init-free solve that ends before its first update (b = 0): nobody has zeroed x
    if (fresh) for (int64_t r = rf; r < r1; r += kBlock) a.x[r] = 0.f;
    if (DECIDE && blockIdx.x == 0 && tid == 0) cg_mark_end_of_graph(a.state, a.host_state);     // every workgroup takes this exit: nobody arrives
    return;
  }

  float ng = 0.f, nrr = 0.f;
  // first element: prefetched in the prologue (the only one at N = 60k); the rest of a long row range in
  // batches of four with all their loads in flight (at N = 1M a lane walks 8 elements: one round trip each
  // made the kernel run at ~1 TB/s)
  auto step = [&](int64_t r, float un, float po, float so, float wo, float xo, float ro, float mo, float pr) {
    if (fresh) { po = 0.f; so = 0.f; xo = 0.f; }      // whatever the previous solve left there (possibly NaN)
    const float p = fmaf(beta, po, un);
    const float s = fmaf(beta, so, wo);
    a.p[r] = p;
    a.s[r] = s;
    a.x[r] = fmaf(alpha, p, xo);
    const float rn = fmaf(-alpha, s, ro);
    a.r[r] = rn;
    float u2 = rn;
    if (a.minv) { u2 = mo * rn; a.u[r] = u2; }
    if (a.us) a.us[r] = pr * u2;
    ng = fmaf(rn, u2, ng);
    nrr = fmaf(rn, rn, nrr);
  };
  if (rf < r1) step(rf, f_u, f_p, f_s, f_w, f_x, f_r, f_m, f_pre);
  constexpr int U = 4;
  for (int64_t rb = rf + kBlock; rb < r1; rb += (int64_t)U * kBlock) {
    float un[U], po[U], so[U], wo[U], xo[U], ro[U], mo[U], pr[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = rb + (int64_t)k * kBlock;
      const int64_t rc = r < r1 ? r : rf;
      un[k] = a.u[rc]; po[k] = a.p[rc]; so[k] = a.s[rc]; wo[k] = a.w[rc]; xo[k] = a.x[rc]; ro[k] = a.r[rc];
      mo[k] = a.minv ? a.minv[rc] : 1.f;
      pr[k] = a.us ? a.pre[rc] : 1.f;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = rb + (int64_t)k * kBlock;
      if (r < r1) step(r, un[k], po[k], so[k], wo[k], xo[k], ro[k], mo[k], pr[k]);
    }
  }
  ng = mgp_wave_sum(ng);
  nrr = mgp_wave_sum(nrr);
  if (lane == 0) { sh_o[wave][0] = ng; sh_o[wave][1] = nrr; }
  __syncthreads();
  float o_rr = 0.f;
  if (tid == 0) {
    const float o_g = (sh_o[0][0] + sh_o[1][0]) + (sh_o[2][0] + sh_o[3][0]);
    const float o_r = (sh_o[0][1] + sh_o[1][1]) + (sh_o[2][1] + sh_o[3][1]);
    a.pd_gamma[(int64_t)par * a.nbv + lb] = o_g;                     // read by the next launch only
    if (!DECIDE) a.pd_rr[(int64_t)par * a.nbv + lb] = o_r;
    else o_rr = o_r;                                                   // stored by the hand-off
  }
#ifdef MGP_STAMP
  if (blockIdx.x == 0 && tid == 0) {
    const int si = atomicAdd(a.state + 8, 1);
    reinterpret_cast<unsigned long long*>(a.state + 16)[si & 255] = wall_clock64() * 8 + 3;
  }
#endif
  if (!DECIDE) return;
  cg_handoff_decide<kC1GammaSlots>(cg_handoff_of(a), a.pd_rr + (int64_t)par * a.nbv, a.nbv, lb, o_rr, it, bb, &sh_o[0][0], &sh_last);
}

// ---- Stopping decision alone (C == 1).  The update kernel of step k+1 is where ||r_k|| <= tol is noticed, after
// apply k+1 has already run for nothing: at 3 iterations per solve that is 2 of 8 SpMVs + a launch, ~14 us of
// ~76.  The first graph of a plan is captured for the step count the previous solves needed, so its last
// (apply, update) pair -- the one that only detects -- is replaced by this single-workgroup launch: the same
// partial sums in the same order, decided and published through cg_rule.h as cg_update_c1_kernel would at
// it + 1.  Not converged: it writes nothing and the continuation graph carries on as before.
// SLOTS: partials a lane sums; a.nbv is their count and the stride between the two parities -- the update grid (kC1GammaSlots),
// or the SpMV grid of a folded plan (its ||r||^2 partials come from spmv_tile_cgstep_kernel: 4 slots up to 1024, else 16).
template <int SLOTS>
__global__ __launch_bounds__(kBlock) void cg_decide_c1_kernel(CgArgs a) {
  __shared__ float sh_w[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CgScalars sc = *reinterpret_cast<const CgScalars*>(a.gamma_old);
#ifdef MGP_STAMP
  if (tid == 0) {
    const int si = atomicAdd(a.state + 8, 1);
    reinterpret_cast<unsigned long long*>(a.state + 16)[si & 255] = wall_clock64() * 8 + 4;
  }
#endif
  if (sc.done) return;
  const int it = sc.it + 1;                 // the step whose update would take this decision
  const int prev = (it & 1) ^ 1;            // slot the last update wrote
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < SLOTS; ++q) {
    const int b = tid + q * kBlock;
    const float v = a.pd_rr[(int64_t)prev * a.nbv + (b < a.nbv ? b : a.nbv - 1)];
    t += (b < a.nbv) ? v : 0.f;
  }
  t = mgp_wave_sum(t);
  if (lane == 0) sh_w[wave] = t;
  __syncthreads();
  if (tid != 0) return;
  const float rr2 = (sh_w[0] + sh_w[1]) + (sh_w[2] + sh_w[3]);
  const float bb = sc.bb;                   // it >= 2 here: written by the first update
  const float rel = cg_rel(rr2, bb);
  const CgStop st = cg_stop(a.stop_mode, a.min_iter, a.max_iter, a.tol, it, rel);
  if (!st.done) return;
  a.resid[0] = rel;
  a.host_state[3] = 1;                      // decided without running apply `it`
  cg_publish(a.state, a.host_state, a.host_resid, &rel, 1, it, st.status);
}

// ---- End-of-graph marker.  The host reads the stopping flag alone while the first graph of a solve runs (a stream query
// during a ~55 us solve costs ~5 us of it); a first graph that ends UNdecided (the solve needs more steps than the graph
// holds) must still be noticed at once: its last node counts the graphs that have run to their end in a host-mapped word
// the host reads next to the flag.  When the decision has been taken the host has long seen the flag: this launch is
// behind the critical path.
__global__ void cg_marker_kernel(int* state, int* host_state) {
  const int c = state[5] + 1;
  state[5] = c;
  __threadfence_system();
  host_state[4] = c;
}

// ---- Complex-shift solve of the (K + s I) system in precision form, symmetric normalisation, nu = 2 (round 5).
// A = I + c B^2 with B = tau I + L_sym and c = noise * scale factorises over the complex numbers: 1 + c b^2 =
// (1 + i sigma b)(1 - i sigma b), sigma = sqrt(c), and 1 / (1 + c b^2) = Re[1 / (1 + i sigma b)], so
//     x = Re[(I + i sigma B)^-1 y].
// M = I + i sigma B is complex SYMMETRIC (not Hermitian) with its spectrum on the segment {1 + i sigma b}: its condition is
// ~sqrt(cond(A)), and COCG -- the CG recurrences with the unconjugated bilinear form z . w = sum z_j w_j -- needs about the
// square root of CG's iterations on A.  Measured on the 1M-node swiss roll (cond(A) = 1.4e4): 58 iterations of ONE product with
// B against 688 iterations of two for CG on A, the same solution to 2e-7 (tools/lab/cocg_s5.py).  The reference's call site is the
// unpreconditioned linear_cg of precision_matern_operator.py:53; this is the north star's "preconditioned CG" taken to its
// end for the systems that factorise: an exact algebraic split instead of an approximate inverse.
//   * vectors z, r, p, s are [n] complex (float2); the product B u runs on the 4-column tile SpMM (spmm_tile_q_kernel) over
//     u4 = (u_re, u_im, u_re, u_im) with dot weights w4 = (u_re, u_im, u_im, u_re): its per-workgroup partials are exactly the
//     four real sums of u . B u = (d0 - d1) + i (d2 + d3); w = M u = u + i sigma B u is formed in the update;
//   * single-reduction (Chronopoulos-Gear) form as cg_update_kernel: gamma = r . r, delta = u . M u = gamma + i sigma u . B u
//     (u = r: no preconditioner), beta = gamma / gamma_old, alpha = gamma / (delta - beta gamma / alpha_old), all complex;
//   * stop: on the REAL system's residual, ||e||_2 <= tol ||b||_2 with e = b - A Re z = r_re + sigma B r_im.  The complex
//     residual r alone is no bound for it: e can be up to |I - i sigma B| ~ sqrt(cond A) times larger (dumbbell fixture,
//     tol 1e-2: complex residual 9.6e-3, real residual 2.5e-1).  The update already holds u = r_{k-1} and B u for every
//     row, so e_{k-1} costs no extra pass: it is summed into the fourth word of the gamma partials and the NEXT launch
//     decides on it, one step behind.  The solution therefore lags by one step too: the update of step k writes
//     x = Re z_{k-1}, so that a stop decided on e_{k-1} returns exactly the x it was decided on and `resid` is its
//     real relative residual.  `iters` reports the COCG steps of that x (the launch count less one: cg_plan_solve_body),
//     and the max_iter exit waits one launch longer, so that it returns x = Re z_{max_iter} with iters = max_iter;
////   * state words, host flags, skip / tick and the chunked hipGraph replay are those of the real solver.

struct CxArgs {
  float2 *z, *r, *p, *s;     // [n] complex
  mgp_cg_v4f *u4, *w4;       // SpMM input (u_re, u_im, u_re, u_im), dot weights (u_re, u_im, u_im, u_re)
  const mgp_cg_v4f* y4;      // B u4
  const float* pd4;          // [nbs4][4] partials of w4 . y4 per column
  int nbs4;
  float sigma;
  float* pd_g;               // [2][nbv][4]: gamma_re, gamma_im, ||r||^2 of r_k, ||e||^2 of the previous step (see above)
  float* sc;                 // [2][4] {gamma_old re, im, alpha_old re, im} per parity, then [8] = ||b||^2
};

__device__ __forceinline__ float2 cx_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cx_div(float2 a, float2 b) {
  const float d = b.x * b.x + b.y * b.y;
  if (!(d > 0.f)) return make_float2(0.f, 0.f);
  return make_float2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

__global__ __launch_bounds__(kBlock) void cx_init_kernel(CgArgs a, CxArgs c, const float* __restrict__ B) {
  __shared__ float sh_o[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lb = mgp_xcd_block(blockIdx.x, gridDim.x);
  const int64_t r0 = (int64_t)lb * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  if (blockIdx.x == 0 && tid == 0) { a.state[0] = 0; a.state[1] = 0; a.state[2] = 0; }   // the first product ticks it to 1
  float g = 0.f;
  for (int64_t r = r0 + tid; r < r1; r += kBlock) {
    const float b = B[r];
    c.z[r] = make_float2(0.f, 0.f);
    c.r[r] = make_float2(b, 0.f);
    c.p[r] = make_float2(0.f, 0.f);
    c.s[r] = make_float2(0.f, 0.f);
    c.u4[r] = mgp_cg_v4f{b, 0.f, b, 0.f};
    c.w4[r] = mgp_cg_v4f{b, 0.f, 0.f, b};
    a.x[r] = 0.f;
    g = fmaf(b, b, g);
  }
  g = mgp_wave_sum(g);
  if (lane == 0) sh_o[wave] = g;
  __syncthreads();
  if (tid == 0) {
    const float t = (sh_o[0] + sh_o[1]) + (sh_o[2] + sh_o[3]);
    float* dst = c.pd_g + 4 * (int64_t)lb;            // parity slot 0 = "previous" of iteration 1
    dst[0] = t; dst[1] = 0.f; dst[2] = t; dst[3] = t;     // e_0 = b
  }
}

__global__ __launch_bounds__(kBlock) void cx_update_kernel(CgArgs a, CxArgs c) {
  __shared__ float sh_w[kBlock / 64][8];
  __shared__ float sh_o[kBlock / 64][4];
  __shared__ int sh_state[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int st_it = a.state[0], st_done = a.state[1];
  const int lb = mgp_xcd_block(blockIdx.x, gridDim.x);
  const int64_t r0 = (int64_t)lb * a.rows_per_block;
  int64_t r1 = r0 + a.rows_per_block;
  if (r1 > a.n) r1 = a.n;
  // ---- one round trip: the partials of both parities, the four-column partials of u . B u, the scalars
  float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // gamma re/im, rr of the previous parity, u . B u (4), ee
  mgp_cg_v4f gv[2][kC1GammaSlots];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < kC1GammaSlots; ++q) {
      const int b = tid + q * kBlock;
      const int bc = b < a.nbv ? b : a.nbv - 1;
      gv[h][q] = *reinterpret_cast<const mgp_cg_v4f*>(c.pd_g + 4 * ((int64_t)h * a.nbv + bc));
    }
  }
  mgp_cg_v4f dv[kCxDeltaSlots];
#pragma unroll
  for (int q = 0; q < kCxDeltaSlots; ++q) {
    const int b = tid + q * kBlock;
    const int bc = b < c.nbs4 ? b : c.nbs4 - 1;
    dv[q] = *reinterpret_cast<const mgp_cg_v4f*>(c.pd4 + 4 * (int64_t)bc);
  }
  const float go_r0 = c.sc[0], go_i0 = c.sc[1], ao_r0 = c.sc[2], ao_i0 = c.sc[3];
  const float go_r1 = c.sc[4], go_i1 = c.sc[5], ao_r1 = c.sc[6], ao_i1 = c.sc[7];
  const float bb_old = c.sc[8];
  float g0[4] = {0.f, 0.f, 0.f, 0.f}, g1[4] = {0.f, 0.f, 0.f, 0.f}, d4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < kC1GammaSlots; ++q) {
    const bool on = tid + q * kBlock < a.nbv;
    g0[0] += on ? gv[0][q].x : 0.f; g0[1] += on ? gv[0][q].y : 0.f; g0[2] += on ? gv[0][q].z : 0.f; g0[3] += on ? gv[0][q].w : 0.f;
    g1[0] += on ? gv[1][q].x : 0.f; g1[1] += on ? gv[1][q].y : 0.f; g1[2] += on ? gv[1][q].z : 0.f; g1[3] += on ? gv[1][q].w : 0.f;
  }
#pragma unroll
  for (int q = 0; q < kCxDeltaSlots; ++q) {
    const bool on = tid + q * kBlock < c.nbs4;
    d4[0] += on ? dv[q].x : 0.f; d4[1] += on ? dv[q].y : 0.f; d4[2] += on ? dv[q].z : 0.f; d4[3] += on ? dv[q].w : 0.f;
  }
  if (tid == 0) { sh_state[0] = st_it; sh_state[1] = st_done; }
  __syncthreads();
  if (sh_state[1]) return;
  const int it = sh_state[0];
  const int par = it & 1, prev = par ^ 1;
  t[0] = prev ? g1[0] : g0[0]; t[1] = prev ? g1[1] : g0[1]; t[2] = prev ? g1[2] : g0[2];
  t[3] = d4[0]; t[4] = d4[1]; t[5] = d4[2]; t[6] = d4[3];
  t[7] = prev ? g1[3] : g0[3];
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k] = mgp_wave_sum(t[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) sh_w[wave][k] = t[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k] = (sh_w[0][k] + sh_w[1][k]) + (sh_w[2][k] + sh_w[3][k]);
  const float2 gamma = make_float2(t[0], t[1]);
  const float rr2 = t[2], ee = t[7];
  const float2 uBu = make_float2(t[3] - t[4], t[5] + t[6]);
  const float2 delta = make_float2(gamma.x - c.sigma * uBu.y, gamma.y + c.sigma * uBu.x);     // u . (u + i sigma B u)
  const float bb = (it == 1) ? rr2 : bb_old;
  const float rel = cg_rel(ee, bb);     // the real system's residual of x = Re z_{it-2}
  float2 alpha = make_float2(0.f, 0.f), beta = make_float2(0.f, 0.f);
  if (rel > a.tol) {
    if (it == 1) {
      alpha = cx_div(gamma, delta);
    } else {
      const float2 go = prev ? make_float2(go_r1, go_i1) : make_float2(go_r0, go_i0);
      const float2 ao = prev ? make_float2(ao_r1, ao_i1) : make_float2(ao_r0, ao_i0);
      beta = cx_div(gamma, go);
      const float2 corr = cx_div(cx_mul(beta, gamma), ao);
      alpha = cx_div(gamma, make_float2(delta.x - corr.x, delta.y - corr.y));
    }
    if (!isfinite(alpha.x) || !isfinite(alpha.y) || !isfinite(beta.x) || !isfinite(beta.y)) {
      alpha = make_float2(0.f, 0.f); beta = make_float2(0.f, 0.f);
    }
  }
  // stop_mode 1 only (plan_create_impl); max_iter + 1: decided on e_{it-2}, so that x = Re z_{max_iter}
  const CgStop st = cg_stop(1, 0, a.max_iter + 1, a.tol, it, rel);
  const int done = st.done;
  if (blockIdx.x == 0 && tid == 0) {
    c.sc[4 * par + 0] = gamma.x; c.sc[4 * par + 1] = gamma.y;
    c.sc[4 * par + 2] = alpha.x; c.sc[4 * par + 3] = alpha.y;
    if (it == 1) c.sc[8] = bb;
    a.resid[0] = rel;
    if (done) cg_publish(a.state, a.host_state, a.host_resid, &rel, 1, it, st.status);
  }
  if (done) return;
  // ---- vector update over this workgroup's rows, four rows per lane in flight
  float ngr = 0.f, ngi = 0.f, nrr = 0.f, nee = 0.f;
  constexpr int U = 4;
  const int64_t rf = r0 + tid;
  for (int64_t rb = rf; rb < r1; rb += (int64_t)U * kBlock) {
    float2 uo[U], po[U], so[U], zo[U];
    mgp_cg_v4f yo[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = rb + (int64_t)k * kBlock;
      const int64_t rc = r < r1 ? r : rf;
      uo[k] = c.r[rc]; po[k] = c.p[rc]; so[k] = c.s[rc]; zo[k] = c.z[rc]; yo[k] = c.y4[rc];
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t r = rb + (int64_t)k * kBlock;
      if (r < r1) {
        const float2 u = uo[k];
        const float2 w = make_float2(u.x - c.sigma * yo[k].y, u.y + c.sigma * yo[k].x);       // M u = u + i sigma B u
        const float e = u.x + c.sigma * yo[k].y;                   // b - A Re z_{it-1} = r_re + sigma B r_im
        const float2 bp = cx_mul(beta, po[k]), bs = cx_mul(beta, so[k]);
        const float2 pn = make_float2(u.x + bp.x, u.y + bp.y);
        const float2 sn = make_float2(w.x + bs.x, w.y + bs.y);
        const float2 ap = cx_mul(alpha, pn), as = cx_mul(alpha, sn);
        const float2 zn = make_float2(zo[k].x + ap.x, zo[k].y + ap.y);
        const float2 rn = make_float2(u.x - as.x, u.y - as.y);
        c.p[r] = pn; c.s[r] = sn; c.z[r] = zn; c.r[r] = rn;
        a.x[r] = zo[k].x;                                          // Re z_{it-1}: the x that e belongs to
        c.u4[r] = mgp_cg_v4f{rn.x, rn.y, rn.x, rn.y};
        c.w4[r] = mgp_cg_v4f{rn.x, rn.y, rn.y, rn.x};
        ngr += rn.x * rn.x - rn.y * rn.y;
        ngi += 2.f * rn.x * rn.y;
        nrr += rn.x * rn.x + rn.y * rn.y;
        nee = fmaf(e, e, nee);
      }
    }
  }
  ngr = mgp_wave_sum(ngr); ngi = mgp_wave_sum(ngi); nrr = mgp_wave_sum(nrr); nee = mgp_wave_sum(nee);
  if (lane == 0) { sh_o[wave][0] = ngr; sh_o[wave][1] = ngi; sh_o[wave][2] = nrr; sh_o[wave][3] = nee; }
  __syncthreads();
  if (tid == 0) {
    float* dst = c.pd_g + 4 * ((int64_t)par * a.nbv + lb);
    dst[0] = (sh_o[0][0] + sh_o[1][0]) + (sh_o[2][0] + sh_o[3][0]);
    dst[1] = (sh_o[0][1] + sh_o[1][1]) + (sh_o[2][1] + sh_o[3][1]);
    dst[2] = (sh_o[0][2] + sh_o[1][2]) + (sh_o[2][2] + sh_o[3][2]);
    dst[3] = (sh_o[0][3] + sh_o[1][3]) + (sh_o[2][3] + sh_o[3][3]);
  }
}

// ---- iterative refinement (stop_mode 1, max_refine > 0): the recurrence residual of a single-
// reduction CG drifts from the true residual on ill-conditioned systems in fp32; the true residual
// R = B - A x is formed explicitly and, if it misses the tolerance, A d = R is solved and x += d.
__global__ __launch_bounds__(kBlock) void refine_residual_kernel(const float* __restrict__ B, const float* __restrict__ T,
                                                                 float* __restrict__ R, int64_t n, int C,
                                                                 float* __restrict__ partial /*[grid][C][2]*/) {
  __shared__ float sh[2][kBlock];
  int TC = 1;
  while (TC < C) TC <<= 1;
  const int TS = kBlock / TC;
  const int tid = threadIdx.x, cc = tid % TC, sl = tid / TC;
  float rr = 0.f, bb = 0.f;
  if (cc < C) {
    for (int64_t r = (int64_t)blockIdx.x * TS + sl; r < n; r += (int64_t)gridDim.x * TS) {
      const int64_t i = r * C + cc;
      const float b = B[i], d = b - T[i];
      R[i] = d;
      rr = fmaf(d, d, rr);
      bb = fmaf(b, b, bb);
    }
  }
  sh[0][tid] = rr; sh[1][tid] = bb;
  reduce_slices<2>(sh, TC, TS, sl, cc);
  if (tid < TC && tid < C) {
    partial[((int64_t)blockIdx.x * C + tid) * 2 + 0] = sh[0][tid];
    partial[((int64_t)blockIdx.x * C + tid) * 2 + 1] = sh[1][tid];
  }
}

__global__ void refine_finalize_kernel(const float* __restrict__ partial, int nblk, int C, float* __restrict__ host_rel) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float rr = 0.f, bb = 0.f;
    for (int b = 0; b < nblk; ++b) { rr += partial[((int64_t)b * C + c) * 2]; bb += partial[((int64_t)b * C + c) * 2 + 1]; }
    host_rel[c] = cg_rel(rr, bb);
  }
}

__global__ void refine_accumulate_kernel(float* __restrict__ xacc, const float* __restrict__ x, int64_t total, int first) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    xacc[i] = first ? x[i] : xacc[i] + x[i];
}

// ---- fp64 refinement (single GPU): the accumulated solution and the true residual live in fp64
__global__ void refine_accumulate64_kernel(double* __restrict__ xacc, const float* __restrict__ x, int64_t total, int first) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    xacc[i] = first ? (double)x[i] : xacc[i] + (double)x[i];
}

// R = B - T (fp64) -> next right-hand side in fp32; partial[blk][c] = {sum R^2, sum B^2} in fp64
__global__ __launch_bounds__(kBlock) void refine_residual64_kernel(const float* __restrict__ B, const double* __restrict__ T,
                                                                   float* __restrict__ R, int64_t n, int C,
                                                                   double* __restrict__ partial) {
  __shared__ double sh[2][kBlock];
  int TC = 1;
  while (TC < C) TC <<= 1;
  const int TS = kBlock / TC;
  const int tid = threadIdx.x, cc = tid % TC, sl = tid / TC;
  double rr = 0.0, bb = 0.0;
  if (cc < C) {
    for (int64_t r = (int64_t)blockIdx.x * TS + sl; r < n; r += (int64_t)gridDim.x * TS) {
      const int64_t i = r * C + cc;
      const double b = (double)B[i], d = b - T[i];
      R[i] = (float)d;
      rr += d * d;
      bb += b * b;
    }
  }
  sh[0][tid] = rr; sh[1][tid] = bb;
  __syncthreads();
  if (tid < TC && tid < C) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < TS; ++k) { s0 += sh[0][k * TC + tid]; s1 += sh[1][k * TC + tid]; }
    partial[((int64_t)blockIdx.x * C + tid) * 2 + 0] = s0;
    partial[((int64_t)blockIdx.x * C + tid) * 2 + 1] = s1;
  }
}

__global__ void refine_finalize64_kernel(const double* __restrict__ partial, int nblk, int C, float* __restrict__ host_rel) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double rr = 0.0, bb = 0.0;
    for (int b = 0; b < nblk; ++b) { rr += partial[((int64_t)b * C + c) * 2]; bb += partial[((int64_t)b * C + c) * 2 + 1]; }
    host_rel[c] = bb > 0.0 ? (float)sqrt(rr / bb) : 0.f;
  }
}

__global__ void refine_publish64_kernel(const double* __restrict__ xacc, float* __restrict__ x, float* __restrict__ X2,
                                        int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = (float)xacc[i];
    x[i] = v;
    if (X2) X2[i] = v;
  }
}

// Host-mapped blocks of the plans (solve state, residuals), pooled: hipHostMalloc costs ~0.1 ms and hipHostFree waits for the
// device to go idle, and a training epoch creates and retires a dozen plans (every hyper-parameter step changes the operator).
// A retired plan's block goes back behind an event recorded on the plan's stream (its last graph's end-of-graph marker may
// still be on its way); it is handed out again only once that event has completed.
struct HostBlock {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
};
std::mutex g_host_pool_mu;
std::vector<HostBlock> g_host_pool;

bool host_block_acquire(size_t bytes, HostBlock* out) {
  {
    std::lock_guard<std::mutex> lk(g_host_pool_mu);
    for (size_t i = 0; i < g_host_pool.size(); ++i) {
      HostBlock& b = g_host_pool[i];
      if (b.bytes < bytes || b.bytes > 4 * bytes + 4096) continue;
      if (b.pending && hipEventQuery(b.ev) != hipSuccess) continue;
      *out = b;
      out->pending = false;
      g_host_pool.erase(g_host_pool.begin() + (long)i);
      return true;
    }
  }
  HostBlock b;
  b.bytes = (bytes + 4095) & ~size_t(4095);
  if (hipHostMalloc(&b.p, b.bytes, hipHostMallocMapped) != hipSuccess) return false;
  if (hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(b.p); return false; }
  *out = b;
  return true;
}

void host_block_release(HostBlock b, hipStream_t stream) {
  if (!b.p) return;
  if (hipEventRecord(b.ev, stream) != hipSuccess) {          // cannot tell when its last writer ends: do not reuse it
    (void)hipEventDestroy(b.ev);
    (void)hipHostFree(b.p);
    return;
  }
  b.pending = true;
  std::lock_guard<std::mutex> lk(g_host_pool_mu);
  if (g_host_pool.size() < 64) { g_host_pool.push_back(b); return; }
  (void)hipEventDestroy(b.ev);
  (void)hipHostFree(b.p);
}

struct CgPlan {
  bool poisoned = false;     // a solve ended in MGP_ERR_TIMEOUT: destroy leaks instead of waiting (mgp_cg_plan_solve)
  HostBlock host_block;
  mgp_operator_t op{};
  MgpDist dist{};           // row partition (is_dist): op.L holds the local rows only
  bool is_dist = false;
  int nb_loc = 0;           // SpMM workgroups per rank that write dot partials
  int C = 0;
  mgp_cg_params_t prm{};
  CgChoice ch{};            // kernel family and grid (cg_choose at creation)
  CgBuffers buf{};          // the workspace as carved (cg_carve)
  CgArgs args{};
  hipStream_t stream = nullptr;       // caller's stream: all work is enqueued here
  hipStream_t cap_stream = nullptr;   // private stream used only to capture the iteration graph
  hipGraphExec_t exec = nullptr;        // `chunk` x (apply, update): continuation replays
  hipGraph_t graph_first = nullptr;     // cg_init + `len_first` x (apply, update): a short solve is ONE graph launch
  hipGraphExec_t exec_first = nullptr;
  hipGraphNode_t init_node = nullptr;   // the cg_init node of graph_first (its rhs argument is patched per solve)
  bool has_graph = false, has_first = false;
  int chunk = 0, len_first = 0;
  int last_need = 0;                    // (apply, update) pairs the previous solve needed: len_first follows it
  const float* patched_rhs = nullptr;   // rhs the cg_init node currently points at
  int solves = 0;                       // run_cg calls so far (graphs are captured at the second one)
  int64_t last_solve_ns = 0;            // host time of the previous solve when it ended inside its first chunk (0: it did not)
  int marker_seq = 0;                   // first graphs launched so far = what cg_marker_kernel will have counted when the newest ends
  bool graphs_tried = false;
  bool rebound = false;                 // mgp_cg_plan_rebind since the last solve: the graphs are refreshed before they are launched again
  bool decide_in_update = false;        // the first graph's last update decides + marks (CgKnobs::decide_in_update at plan creation)
  CxArgs cxa{};                         // complex-shift solve (ch.cx)
  mgp_operator_t opB{};                 // B = tau I + L_sym (one launch of the 4-column SpMM per iteration)
  char first_record[MGP_SPMM_RECORD_BYTES] = {};   // launch arguments of the first graph's root SpMV (rhs patched per solve)
  int32_t* host_state = nullptr;        // pinned
  float* host_resid = nullptr;          // pinned
  float* host_true_rel = nullptr;       // host-mapped [C]: true relative residuals
  float* dev_true_rel = nullptr;
};

CgKnobs g_knobs;   // the lab switches (mgp_cg_set_*)

// What a plan on `op` is created from.  minv, stop_mode: whatever the caller has when only the workspace is sized (no buffer depends on them).
CgShape cg_shape(const mgp_operator_t* op, int C, int world, bool is_dist, bool has_minv, int stop_mode) {
  CgShape sh{};
  sh.n = op->L.n; sh.world = world; sh.is_dist = is_dist; sh.C = C;
  sh.nb_loc = mgp_spmm_dot_blocks_for(&op->L, C);
  sh.nb4 = (C == 1 && !is_dist) ? mgp_spmm_dot_blocks_for(&op->L, 4) : 0;
  sh.has_minv = has_minv; sh.has_pre = op->pre != nullptr; sh.has_post = op->post != nullptr;
  sh.form = op->form; sh.nu = op->nu; sh.noise_scale = op->noise * op->scale;
  sh.stop_mode = stop_mode;
  sh.tile_plan = C == 1 && mgp_tile_plan(&op->L) != 0;
  sh.pre_is_post = op->pre == op->post;
  sh.tile_rows = (C == 1 && mgp_spmm_cgstep_fits(&op->L)) ? op->L.tile_rows : 0;
  return sh;
}

size_t cg_bytes(const mgp_operator_t* op, int C, int world, bool is_dist) {
  const CgShape sh = cg_shape(op, C, world, is_dist, false, 0);
  return cg_workspace_bytes(sh, cg_choose(sh, g_knobs));
}

// The operator of the complex-shift solve's one product per step: B = tau I + L_sym, from the (K + s I) operator in precision form
mgp_operator_t cx_operator(const mgp_operator_t* op) {
  mgp_operator_t b = mgp_operator_copy(op);
  b.nu = 1;
  b.kappa = op->kappa / sqrtf(2.0f);       // tau_B = 2 / kappa_B^2 = 2 nu / kappa^2
  b.scale = 1.0f; b.form = 0; b.noise = 0.f;
  return b;
}

// one CG step = operator apply (w = A u, partials of u . w, ticks the iteration counter; skipped once
// converged) followed by the fused update kernel, which also takes the stopping decision: every
// graph therefore ends right behind a decision and a solve that needs k steps runs exactly k bodies.
void launch_update_c1(CgPlan* pl, hipStream_t st, bool decide_last) {
  const dim3 grid(pl->args.nbv), block(kBlock);
  if (pl->args.nbs <= 4 * kBlock) {
    if (decide_last) hipLaunchKernelGGL((cg_update_c1_kernel<true, 4>), grid, block, 0, st, pl->args);
    else hipLaunchKernelGGL((cg_update_c1_kernel<false, 4>), grid, block, 0, st, pl->args);
  } else {
    if (decide_last) hipLaunchKernelGGL((cg_update_c1_kernel<true, kC1DeltaSlots>), grid, block, 0, st, pl->args);
    else hipLaunchKernelGGL((cg_update_c1_kernel<false, kC1DeltaSlots>), grid, block, 0, st, pl->args);
  }
}

// What the folded step's kernel takes from the plan (CgChoice::fold).  Its ||r||^2 partials live in pd_rr, one per SpMV workgroup
// and nbs apart per parity; pd_gamma is not used (gamma = ||r||^2 without a preconditioner).
MgpCgStep fold_step(const CgPlan* pl) {
  const CgArgs& a = pl->args;
  MgpCgStep cs{};
  cs.r = a.r; cs.x = a.x; cs.p = a.p; cs.s = a.s; cs.us = a.us; cs.pre = a.pre;
  cs.pd_rr = a.pd_rr; cs.pd_delta = a.pd_delta; cs.nbs = a.nbs;
  cs.blk = a.gamma_old; cs.state = a.state; cs.host_state = a.host_state; cs.host_resid = a.host_resid; cs.arrive = a.arrive;
  cs.tol = a.tol; cs.max_iter = a.max_iter; cs.min_iter = a.min_iter; cs.stop_mode = a.stop_mode;
  return cs;
}

int enqueue_body(CgPlan* pl, hipStream_t st, bool decide_last = false) {
  if (pl->ch.fold)       // two launches: t = B P u with the partials of |t|^2 (ticks the iteration; skipped once decided), then the step
    return mgp_operator_apply_cgstep(&pl->op, pl->args.us ? pl->args.us : pl->args.r, false, nullptr, fold_step(pl), decide_last,
                                     pl->buf.op_work, pl->buf.op_work_bytes, st);
  if (pl->ch.cx) {
    // B u on the 4-column tile SpMM (partials of u . B u ride along; skipped once decided; ticks the iteration), then the
    // complex update
    MGP_TRY(mgp_operator_apply_dist(&pl->opB, nullptr, reinterpret_cast<const float*>(pl->cxa.u4), nullptr, 4,
                                    const_cast<float*>(reinterpret_cast<const float*>(pl->cxa.y4)),
                                    reinterpret_cast<const float*>(pl->cxa.w4), pl->buf.pd4, pl->cxa.nbs4, pl->args.state + 1,
                                    pl->args.state, pl->buf.op_work4, pl->buf.op_work4_bytes, st));
    hipLaunchKernelGGL(cx_update_kernel, dim3(pl->args.nbv), dim3(kBlock), 0, st, pl->args, pl->cxa);
    MGP_LAUNCH_CHECK();
    return MGP_OK;
  }
  MGP_TRY(mgp_operator_apply_dist(&pl->op, pl->is_dist ? &pl->dist : nullptr, pl->args.u, pl->args.us, pl->C,
                                  pl->args.w, pl->args.u, pl->buf.pd_delta, pl->nb_loc, pl->args.state + 1,
                                  pl->args.state, pl->buf.op_work, pl->buf.op_work_bytes, st));
  if (pl->ch.c1_family) {
    launch_update_c1(pl, st, decide_last);
  } else {
    if (pl->args.tot) {
      hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)mgp_cdiv(pl->C, 4), 3), dim3(kBlock), 0, st, pl->args);
      MGP_LAUNCH_CHECK();
    }
    if (pl->ch.upd_quads) hipLaunchKernelGGL(cg_update_q_kernel<kBlock>, dim3(pl->args.nbv), dim3(kBlock), 0, st, pl->args);
    else hipLaunchKernelGGL(cg_update_kernel, dim3(pl->args.nbv), dim3(kBlock), 0, st, pl->args);
  }
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// Init-free solve: the first (apply, update) pair.  The apply reads `rhs` directly (launch 0 scales it by op->pre,
// copies it to r), leaves the partials of r . A r and ||r||^2 and resets the iteration state; the update then runs
// as iteration 1 with p = s = x = 0.  One launch (cg_init, ~3.8 us at N = 60k) less per solve.
int enqueue_first_body(CgPlan* pl, hipStream_t st, const float* rhs, bool record, bool decide_last = false) {
  if (pl->ch.fold)
    return mgp_operator_apply_cgstep(&pl->op, rhs, true, record ? pl->first_record : nullptr, fold_step(pl), decide_last,
                                     pl->buf.op_work, pl->buf.op_work_bytes, st);
  MGP_TRY(mgp_operator_apply_first(&pl->op, rhs, pl->args.r, pl->args.w, pl->buf.pd_delta, pl->buf.pd_bb, pl->args.state,
                                   record ? pl->first_record : nullptr, pl->buf.op_work, pl->buf.op_work_bytes, st));
  launch_update_c1(pl, st, decide_last);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// stream-capture the first graph (cg_init / init-free first apply + len bodies) into *out; false on any failure
bool record_first(CgPlan* pl, int len, hipGraph_t* out) {
  *out = nullptr;
  if (!pl->cap_stream || len < 1) return false;
  if (hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
  int rc = MGP_OK;
  const bool decide = cg_last_step_decides(len, pl->is_dist, pl->ch.c1_family);
  const int bodies = decide ? len - 1 : len;
  int done_bodies = 0;
  // decide: the graph's LAST update also takes the next step's decision and leaves the end-of-graph mark (CgKnobs::decide_in_update;
  // 0: the separate cg_decide_c1_kernel + cg_marker_kernel launches of rounds 1-3)
  const bool in_update = decide && pl->decide_in_update;
  if (pl->ch.init_free) {
    // root node = launch 0 of the first apply, reading a placeholder rhs that is patched before every launch
    rc = enqueue_first_body(pl, pl->cap_stream, (const float*)pl->args.x, true, in_update && bodies == 1);
    done_bodies = 1;
  } else {
    hipLaunchKernelGGL(cg_init_kernel, dim3(pl->args.nbv), dim3(kBlock), 0, pl->cap_stream, pl->args,
                       (const float*)pl->args.x);   // placeholder rhs, patched before every launch
    rc = hipGetLastError() == hipSuccess ? MGP_OK : 1;
  }
  for (int i = done_bodies; i < bodies && rc == MGP_OK; ++i) rc = enqueue_body(pl, pl->cap_stream, in_update && i == bodies - 1);
  if (decide && !in_update && rc == MGP_OK) {
    if (pl->ch.fold) {
      CgArgs d = pl->args;          // the step kernel's partials: one per SpMV workgroup, nbs apart per parity
      d.nbv = d.nbs;
      if (d.nbs <= 4 * kBlock) hipLaunchKernelGGL(cg_decide_c1_kernel<4>, dim3(1), dim3(kBlock), 0, pl->cap_stream, d);
      else hipLaunchKernelGGL(cg_decide_c1_kernel<kC1DeltaSlots>, dim3(1), dim3(kBlock), 0, pl->cap_stream, d);
    } else hipLaunchKernelGGL(cg_decide_c1_kernel<kC1GammaSlots>, dim3(1), dim3(kBlock), 0, pl->cap_stream, pl->args);
    rc = hipGetLastError() == hipSuccess ? MGP_OK : 1;
  }
  if (!in_update && rc == MGP_OK) {
    hipLaunchKernelGGL(cg_marker_kernel, dim3(1), dim3(1), 0, pl->cap_stream, pl->args.state, pl->args.host_state);
    rc = hipGetLastError() == hipSuccess ? MGP_OK : 1;
  }
  hipGraph_t graph = nullptr;
  const hipError_t e2 = hipStreamEndCapture(pl->cap_stream, &graph);
  if (rc == MGP_OK && e2 == hipSuccess && graph != nullptr) { *out = graph; return true; }
  if (graph) (void)hipGraphDestroy(graph);
  return false;
}

// (re)build the first graph: cg_init + len bodies.  Leaves has_first = false on any failure (the
// solve then launches cg_init eagerly and replays the continuation graph).
void capture_first(CgPlan* pl, int len) {
  if (pl->exec_first) { (void)hipGraphExecDestroy(pl->exec_first); pl->exec_first = nullptr; }
  if (pl->graph_first) { (void)hipGraphDestroy(pl->graph_first); pl->graph_first = nullptr; }
  pl->has_first = false;
  pl->patched_rhs = nullptr;
  pl->len_first = len;
  bool ok = record_first(pl, len, &pl->graph_first);
  if (ok) {
    size_t nroot = 1;
    hipGraphNode_t root = nullptr;
    ok = hipGraphGetRootNodes(pl->graph_first, &root, &nroot) == hipSuccess && nroot == 1 && root != nullptr;
    hipGraphNodeType ty;
    if (ok) ok = hipGraphNodeGetType(root, &ty) == hipSuccess && ty == hipGraphNodeTypeKernel;
    pl->init_node = root;
  }
  if (ok) ok = hipGraphInstantiate(&pl->exec_first, pl->graph_first, nullptr, nullptr, 0) == hipSuccess;
  (void)hipGetLastError();
  pl->has_first = ok;
}

// point the cg_init node of the first graph at this solve's right-hand side
bool patch_first_rhs(CgPlan* pl, const float* rhs) {
  if (rhs == pl->patched_rhs) return true;
  if (pl->ch.init_free) {
    if (mgp_spmm_patch_node(pl->exec_first, pl->init_node, pl->first_record, (const float*)pl->args.x, rhs) != MGP_OK) {
      (void)hipGetLastError();
      return false;
    }
    pl->patched_rhs = rhs;
    return true;
  }
  hipKernelNodeParams np;
  memset(&np, 0, sizeof(np));
  if (hipGraphKernelNodeGetParams(pl->init_node, &np) != hipSuccess) return false;
  void* kp[2] = {(void*)&pl->args, (void*)&rhs};
  np.kernelParams = kp;
  np.extra = nullptr;
  if (hipGraphExecKernelNodeSetParams(pl->exec_first, pl->init_node, &np) != hipSuccess) return false;
  pl->patched_rhs = rhs;
  return true;
}

}  // namespace

extern "C" size_t mgp_cg_workspace_bytes(const mgp_operator_t* op, int C) {
  if (!op || C <= 0 || C > kMaxC || op->L.n <= 0 || !mgp_spmv_lanes_ok(op->L.spmv_lanes)) return 0;
  return cg_bytes(op, C, 1, false);
}

// stream-capture `chunk` bodies (the continuation graph) into *out
static bool record_chunk(CgPlan* pl, hipGraph_t* out) {
  *out = nullptr;
  if (hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
  int rc = MGP_OK;
  for (int i = 0; i < pl->chunk && rc == MGP_OK; ++i) rc = enqueue_body(pl, pl->cap_stream);
  hipGraph_t graph = nullptr;
  const hipError_t e2 = hipStreamEndCapture(pl->cap_stream, &graph);
  if (rc == MGP_OK && e2 == hipSuccess && graph != nullptr) { *out = graph; return true; }
  if (graph) (void)hipGraphDestroy(graph);
  return false;
}

// After mgp_cg_plan_rebind: the captured graphs still hold the OLD operator's pointers and scalars.  Record the same launches
// again with the new ones and update the executable graphs in place (hipGraphExecUpdate: same topology, same kernels, new
// arguments -- tools/lab/graph_update.hip: record 15 us + update 20 us for 30 nodes, against instantiate 40-50 + the 210 us a
// hipGraphExecDestroy costs); an update the runtime refuses falls back to destroy + instantiate.  The first graph keeps its ORIGINAL
// hipGraph_t: the root node patched per solve (patch_first_rhs) is addressed through it, and the launch record it is patched from
// was rewritten by the recording.
static void refresh_graphs(CgPlan* pl) {
  pl->rebound = false;
  if (!pl->graphs_tried) return;          // nothing captured yet: the first capture will see the new operator
  (void)hipGetLastError();
  if (pl->has_graph) {
    hipGraph_t g = nullptr;
    bool ok = record_chunk(pl, &g);
    if (ok) {
      hipGraphNode_t err_node = nullptr;
      hipGraphExecUpdateResult res;
      if (hipGraphExecUpdate(pl->exec, g, &err_node, &res) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphExecDestroy(pl->exec);
        pl->exec = nullptr;
        ok = hipGraphInstantiate(&pl->exec, g, nullptr, nullptr, 0) == hipSuccess;
      }
    }
    if (g) (void)hipGraphDestroy(g);
    if (!ok && pl->exec) { (void)hipGraphExecDestroy(pl->exec); pl->exec = nullptr; }
    pl->has_graph = ok;
    (void)hipGetLastError();
  }
  if (pl->has_first) {
    hipGraph_t g = nullptr;
    bool ok = record_first(pl, pl->len_first, &g);
    if (ok) {
      hipGraphNode_t err_node = nullptr;
      hipGraphExecUpdateResult res;
      ok = hipGraphExecUpdate(pl->exec_first, g, &err_node, &res) == hipSuccess;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    pl->patched_rhs = nullptr;            // the update reset the root node to the placeholder right-hand side
    if (!ok) capture_first(pl, pl->len_first);
  }
}

// Graphs are captured at the SECOND solve of a plan: capture + instantiate cost ~0.3 ms (7 ms the first time in a
// process; tools/lab/time_capture.py), as much as a short solve, and plans built for a one-off solve never earn it
// back.  The first solve runs the same launches eagerly.
static void capture_graphs(CgPlan* pl) {
  pl->graphs_tried = true;
  if (!pl->prm.use_graph || pl->is_dist) return;   // collectives are enqueued eagerly (no capture)
  hipError_t e = hipStreamCreateWithFlags(&pl->cap_stream, hipStreamNonBlocking);
  bool ok = (e == hipSuccess);
  if (ok) {
    hipGraph_t graph = nullptr;
    ok = record_chunk(pl, &graph);
    if (ok) ok = hipGraphInstantiate(&pl->exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
  }
  pl->has_graph = ok;
  (void)hipGetLastError();   // a failed capture falls back to eager launches
  // (the complex-shift solve runs tens of iterations: init launch + chunk graphs, no single-graph form)
  if (ok && !pl->ch.cx) capture_first(pl, cg_first_len(pl->last_need, pl->chunk));
}

static int plan_create_impl(const mgp_operator_t* op, int C, const float* minv, const mgp_cg_params_t* params,
                            const MgpDist* dist, void* work, size_t work_bytes, void* stream, void** plan_out) {
  if (!op || !params || !work || !plan_out || !mgp_spmv_lanes_ok(op->L.spmv_lanes)) return MGP_ERR_ARG;
  if (C <= 0 || C > kMaxC) return C > kMaxC ? MGP_ERR_UNSUPPORTED : MGP_ERR_ARG;
  const int world = dist ? dist->world : 1;
  if (dist && (dist->n_loc != op->L.n || dist->world < 1 || dist->rank < 0 || dist->rank >= dist->world))
    return MGP_ERR_ARG;
  if (dist && op->form == 3) return MGP_ERR_UNSUPPORTED;       // form 3: single-GPU plans only
  mgp_cg_params_t prm = *params;
  if (prm.max_iter <= 0) prm.max_iter = 1000;
  if (prm.min_iter < 0) prm.min_iter = 0;
  const CgKnobs knobs = g_knobs;      // (lab knobs: read once, at plan creation)
  const CgShape sh = cg_shape(op, C, world, dist != nullptr, minv != nullptr, prm.stop_mode);
  const CgChoice ch = cg_choose(sh, knobs);
  if (work_bytes < cg_workspace_bytes(sh, ch)) return MGP_ERR_WORKSPACE;
  CgPlan* pl = new (std::nothrow) CgPlan();
  if (!pl) return MGP_ERR_ARG;
  MgpArena ar(work, work_bytes);
  cg_carve(ar, sh, ch, &pl->buf);
  if (!ar.ok()) { delete pl; return MGP_ERR_WORKSPACE; }
  const CgBuffers& b = pl->buf;
  pl->op = mgp_operator_copy(op);
  pl->is_dist = dist != nullptr;
  if (dist) pl->dist = *dist;
  pl->C = C; pl->prm = prm; pl->ch = ch; pl->nb_loc = sh.nb_loc;
  pl->decide_in_update = knobs.decide_in_update != 0;
  pl->chunk = prm.check_every > 0 ? prm.check_every : 10;
  pl->stream = mgp_stream(stream);
  CgArgs& a = pl->args;
  a.n = sh.n * world; a.C = C; a.TC = ch.TC; a.TS = ch.TS; a.CQ = ch.CQ; a.TSQ = ch.TSQ;
  a.rows_per_block = ch.rows_per_block; a.nbv = ch.nbv; a.nbs = ch.nbs;
  a.x = b.x; a.r = b.r; a.w = b.w; a.p = b.p; a.s = b.s;
  a.minv = minv; a.u = minv ? b.ubuf : a.r;
  a.pre = op->pre; a.us = op->pre ? b.usbuf : nullptr;
  a.pd_gamma = b.pd_gamma; a.pd_rr = b.pd_rr; a.pd_delta = b.pd_delta;
  a.gamma_old = b.blk; a.alpha_old = b.blk + 2 * (size_t)C; a.bb = b.blk + 4 * (size_t)C; a.resid = b.blk + 5 * (size_t)C;
  a.state = reinterpret_cast<int*>(b.blk + 6 * (size_t)C);
  a.tot = ch.reduce_once ? b.tot : nullptr;
  a.pd_bb = ch.init_free ? b.pd_bb : nullptr;
  a.arrive = b.arrive;
  a.tol = prm.tol; a.max_iter = prm.max_iter; a.min_iter = prm.min_iter; a.stop_mode = prm.stop_mode;
  (void)hipMemsetAsync(a.state, 0, (16 + kStampWords) * sizeof(int), pl->stream);      // (state[5]: cg_marker_kernel's count)
  MGP_HIP_TRY(hipMemsetAsync(a.arrive, 0, 9 * 32 * sizeof(int), pl->stream));
  if (b.cz) {
    CxArgs& cx = pl->cxa;
    cx.z = reinterpret_cast<float2*>(b.cz); cx.r = reinterpret_cast<float2*>(b.cr);
    cx.p = reinterpret_cast<float2*>(b.cp); cx.s = reinterpret_cast<float2*>(b.cs);
    cx.u4 = reinterpret_cast<mgp_cg_v4f*>(b.u4); cx.w4 = reinterpret_cast<mgp_cg_v4f*>(b.w4);
    cx.y4 = reinterpret_cast<const mgp_cg_v4f*>(b.y4);
    cx.pd4 = b.pd4; cx.pd_g = b.pd_g; cx.sc = b.sc;
  }
  if (ch.cx) {
    pl->opB = cx_operator(op);
    pl->cxa.nbs4 = sh.nb4;
    pl->cxa.sigma = sqrtf(sh.noise_scale);
    MGP_HIP_TRY(hipMemsetAsync(pl->cxa.sc, 0, 64 * sizeof(float), pl->stream));
  }
  // one pooled host-mapped block: [16 int32 state | C resid | C true_rel], each part on its own 64-byte line
  const size_t rbytes = (((size_t)C * sizeof(float)) + 63) & ~size_t(63);
  if (!host_block_acquire(64 + 2 * rbytes, &pl->host_block)) { delete pl; return (int)hipErrorOutOfMemory; }
  char* hb = static_cast<char*>(pl->host_block.p);
  pl->host_state = reinterpret_cast<int32_t*>(hb);
  pl->host_resid = reinterpret_cast<float*>(hb + 64);
  pl->host_true_rel = reinterpret_cast<float*>(hb + 64 + rbytes);
  hipError_t e = hipHostGetDevicePointer((void**)&a.host_state, pl->host_state, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&a.host_resid, pl->host_resid, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&pl->dev_true_rel, pl->host_true_rel, 0);
  if (e != hipSuccess) { host_block_release(pl->host_block, pl->stream); delete pl; return (int)e; }
  memset(hb, 0, 64 + 2 * rbytes);

  *plan_out = pl;
  return MGP_OK;
}

// The lab switches (include/mgp_hip.h) write g_knobs; the last two return the previous setting.
extern "C" int mgp_cg_set_init_free(int on) { g_knobs.init_free = on ? 1 : 0; return MGP_OK; }
extern "C" int mgp_cg_set_poll_spin(int spins) { g_knobs.poll_spin = spins < 0 ? 0 : spins; return MGP_OK; }
extern "C" int mgp_cg_set_reduce_once(int on) { g_knobs.reduce_once = on == 2 ? 2 : (on ? 1 : 0); return MGP_OK; }   // 2: from two columns up (A/B runs)
extern "C" int mgp_cg_set_update_quads(int on) { g_knobs.update_quads = on ? 1 : 0; return MGP_OK; }
extern "C" int mgp_cg_set_complex_shift(int on) { const int prev = g_knobs.complex_shift; g_knobs.complex_shift = on ? 1 : 0; return prev; }
extern "C" int mgp_cg_set_decide_in_update(int on) { const int prev = g_knobs.decide_in_update; g_knobs.decide_in_update = on ? 1 : 0; return prev; }

extern "C" int mgp_cg_set_fold_update(int on) { const int prev = g_knobs.fold_update; g_knobs.fold_update = on == 2 ? 2 : (on ? 1 : 0); return prev; }   // 2: at any partial count

extern "C" int mgp_cg_plan_is_folded(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  return pl && pl->ch.fold ? 1 : 0;
}

extern "C" int mgp_cg_plan_is_complex_shift(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  return pl && pl->ch.cx ? 1 : 0;
}

extern "C" int mgp_cg_plan_create(const mgp_operator_t* op, int C, const float* minv,
                                  const mgp_cg_params_t* params, void* work, size_t work_bytes,
                                  void* stream, void** plan_out) {
  return plan_create_impl(op, C, minv, params, nullptr, work, work_bytes, stream, plan_out);
}

// see include/mgp_hip.h
extern "C" int mgp_cg_plan_rebind(void* plan, const mgp_operator_t* op, const float* minv) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl || !op) return MGP_ERR_ARG;
  if (pl->poisoned || pl->is_dist) return MGP_ERR_UNSUPPORTED;
  const mgp_operator_t& o = pl->op;
  // the same STRUCTURE: everything that chose kernels, grids and buffer sizes at creation
  // (form 3: obs_w is read for that form only -- present on both sides, as the form is the same)
  const bool same = op->L.n == o.L.n && op->L.ncols == o.L.ncols && op->nu == o.nu && op->form == o.form &&
                    (op->form != 3 || ((op->obs_w != nullptr) == (o.obs_w != nullptr))) &&
                    (op->pre != nullptr) == (o.pre != nullptr) && (op->post != nullptr) == (o.post != nullptr) &&
                    (minv != nullptr) == (pl->args.minv != nullptr) &&
                    (op->L.tile_ptr != nullptr) == (o.L.tile_ptr != nullptr) && op->L.tile_rows == o.L.tile_rows &&
                    op->L.tile_max_cols == o.L.tile_max_cols && op->L.tile_max_entries == o.L.tile_max_entries &&
                    (op->L.tile_rowptr != nullptr) == (o.L.tile_rowptr != nullptr) &&
                    (op->L.tile_vals != nullptr) == (o.L.tile_vals != nullptr) &&
                    (op->L.tile_rowid != nullptr) == (o.L.tile_rowid != nullptr) &&
                    (op->L.mt_img != nullptr) == (o.L.mt_img != nullptr) && op->L.mt_tiles == o.L.mt_tiles &&
                    op->L.mt_steps == o.L.mt_steps && op->L.spmv_lanes == o.L.spmv_lanes &&
                    // the entry-balanced tile set's count and maxima sized grids and LDS: the SAME descriptor or none (the plan's
                    // one is not read again: its owner may be gone)
                    op->L.c1_tiles == o.L.c1_tiles &&
                    mgp_spmm_dot_blocks_for(&op->L, pl->C) == pl->nb_loc &&
                    (!pl->ch.fold || op->pre == op->post);        // the folded step's identity needs ONE vector P
  if (!same) return MGP_ERR_UNSUPPORTED;
  if (pl->ch.cx) {
    const float cc = op->noise * op->scale;
    if (!(cc > 0.f)) return MGP_ERR_UNSUPPORTED;
    pl->opB = cx_operator(op);
    if (mgp_spmm_dot_blocks_for(&pl->opB.L, 4) != pl->cxa.nbs4) return MGP_ERR_UNSUPPORTED;
    pl->cxa.sigma = sqrtf(cc);
  }
  pl->op = mgp_operator_copy(op);
  pl->args.minv = minv;
  pl->args.pre = op->pre;
  pl->rebound = true;
  return MGP_OK;
}

extern "C" size_t mgp_cg_dist_workspace_bytes(const mgp_operator_t* op_local, int C, int world) {
  if (!op_local || C <= 0 || C > kMaxC || op_local->L.n <= 0 || world < 1 || !mgp_spmv_lanes_ok(op_local->L.spmv_lanes)) return 0;
  return cg_bytes(op_local, C, world, true);
}

extern "C" int mgp_cg_plan_create_dist(const mgp_operator_t* op_local, int C, const float* minv,
                                       const mgp_cg_params_t* params, void* comm, int rank, int world,
                                       void* work, size_t work_bytes, void* stream, void** plan_out) {
  if (!op_local || !comm) return MGP_ERR_ARG;
  MgpDist d{comm, rank, world, op_local->L.n, (int64_t)rank * op_local->L.n};
  return plan_create_impl(op_local, C, minv, params, &d, work, work_bytes, stream, plan_out);
}

// one CG run on `rhs` into the plan's x buffer; ends with the stream synchronised
static int run_cg(CgPlan* pl, const float* rhs, float* Xcopy) {
  hipStream_t st = pl->stream;
  const size_t nc = (size_t)pl->args.n * pl->C;
  pl->host_state[1] = 0;
  pl->host_state[3] = 0;
  *reinterpret_cast<volatile uint64_t*>(pl->host_state + 8) = 0;     // the deciding update's 8-byte record
  bool first = true;
  const auto t_begin = std::chrono::steady_clock::now();
  if (pl->rebound) refresh_graphs(pl);
  if (pl->solves++ >= 1 && !pl->graphs_tried) capture_graphs(pl);
  if (pl->has_first && !patch_first_rhs(pl, rhs)) pl->has_first = false;
  int eager_done = 0;           // bodies of the first eager chunk already enqueued
  if (!pl->has_first) {
    if (pl->ch.cx) {
      hipLaunchKernelGGL(cx_init_kernel, dim3(pl->args.nbv), dim3(kBlock), 0, st, pl->args, pl->cxa, rhs);
      MGP_LAUNCH_CHECK();
    } else if (pl->ch.init_free) {
      MGP_TRY(enqueue_first_body(pl, st, rhs, false));
      eager_done = 1;
    } else {
      hipLaunchKernelGGL(cg_init_kernel, dim3(pl->args.nbv), dim3(kBlock), 0, st, pl->args, rhs);
      MGP_LAUNCH_CHECK();
    }
  }
  int guard = 0;
  for (;;) {
    const bool launched_first = first && pl->has_first;
    if (launched_first) {
      ++pl->marker_seq;
      // (round 4, measured and removed: the first (apply, update) pair launched eagerly in front of a graph holding steps
      // 2 .. k, to hide the replay's launch latency behind it -- 59.9 us per 60k solve against 55.2 with the whole solve in
      // the graph, tools/lab/ab_decide.py: three eager launches and a graph launch behind them cost more than one replay)
      MGP_HIP_TRY(hipGraphLaunch(pl->exec_first, st));
    } else if (pl->has_graph) {
      MGP_HIP_TRY(hipGraphLaunch(pl->exec, st));
    } else {
      const int len = cg_eager_len(first, pl->chunk);
      for (int i = first ? eager_done : 0; i < len; ++i) MGP_TRY(enqueue_body(pl, st));
    }
    first = false;
    // the solution rides behind every chunk so that one synchronisation ends the solve; the
    // convergence flag / residuals arrive through host-mapped memory written by the update kernel
    if (Xcopy) MGP_HIP_TRY(hipMemcpyAsync(Xcopy, pl->args.x, nc * sizeof(float), hipMemcpyDeviceToDevice, st));
    // The stopping decision arrives in host-mapped memory (written behind a system-scope fence by the
    // update kernel): poll it instead of sleeping in hipStreamSynchronize -- at ~70 us per solve the
    // wake-up latency of a blocking wait is a visible fraction.  Work queued behind the solve on the
    // same stream (the X copy, the caller's kernels) stays ordered; a chunk that ends undecided is
    // detected by the stream going idle.
    // hipStreamQuery is only the guard against a chunk that ends undecided: the first graph of a plan is sized to end
    // in the stopping decision, so for about twice as long as the previous solve took the host reads nothing but the
    // flag (measured: 60.5 -> 58.4 us per 60k solve with no query during the solve -- the queries themselves, a
    // runtime lock each, delay the launch's progress); continuation chunks poll as before.
    volatile int32_t* flag = pl->host_state + 1;
    // the deciding update launch (cg_update_c1_kernel<true>) reports through one 8-byte record instead of the flag words:
    // unpack it into them, so that everything below reads one format
    volatile uint64_t* record = reinterpret_cast<volatile uint64_t*>(pl->host_state + 8);
    auto decided = [&]() -> bool {
      if (*flag) return true;
      const uint64_t rec = *record;
      if (!(rec >> 32 & 1)) return false;
      const uint32_t lo = (uint32_t)rec, hi = (uint32_t)(rec >> 32);
      memcpy(pl->host_resid, &lo, sizeof(float));
      pl->host_state[0] = (int32_t)(hi >> 8);
      pl->host_state[2] = (int32_t)((hi >> 4) & 15);
      pl->host_state[3] = (int32_t)((hi >> 1) & 1);
      pl->host_state[1] = 1;
      return true;
    };
    const int poll_spin = g_knobs.poll_spin;      // (lab knob: read once per chunk)
    if (launched_first && poll_spin > 0) {
      // (not even one query every 20 us: two or three of them during a 55 us solve took the whole gain back.)
      const int64_t budget = cg_poll_budget_ns(pl->last_solve_ns);
      const auto t_spin = std::chrono::steady_clock::now();
      volatile int32_t* marker = pl->host_state + 4;
      while (!decided() && *marker != pl->marker_seq) {
        for (int spin = 0; spin < poll_spin && !decided() && *marker != pl->marker_seq; ++spin) __builtin_ia32_pause();
        if (std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_spin).count() > budget) break;
      }
    }
    if (!decided() && pl->is_dist && pl->dist.world > 1) {
      MGP_TRY(mgp_stream_wait_bounded(st));      // collectives on the stream: a dead peer must not hang this rank
    }
    while (!decided()) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return (int)q;
    }
    if (decided()) break;
    if (++guard > cg_guard_chunks(pl->prm.max_iter, pl->chunk)) break;
  }
  pl->last_solve_ns = 0;
  if (pl->host_state[1]) {
    if (guard == 0)      // decided inside the first chunk: how long such a solve takes (the next one's flag-only poll window)
      pl->last_solve_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
    const int need = pl->host_state[0];
    if (pl->exec_first && cg_recapture_first(need, pl->len_first, pl->last_need)) {
      MGP_HIP_TRY(hipStreamSynchronize(st));   // the graph being replaced may still be draining
      capture_first(pl, need);
    }
    pl->last_need = need;
  }
  return MGP_OK;
}

static int cg_plan_solve_body(void* plan, const float* B, float* X, int32_t* iters, float* resid,
                                 int32_t* status) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl || !B) return MGP_ERR_ARG;   // X == NULL: leave the solution in the plan (mgp_cg_plan_x)
  hipStream_t st = pl->stream;
  const size_t nc = (size_t)pl->args.n * pl->C;
  const int max_refine = (pl->prm.stop_mode == 1) ? pl->prm.max_refine : 0;
  // COCG decides one step behind (cx_update_kernel): its x has one step fewer than the launches that ran
  const int lag = pl->ch.cx ? 1 : 0;
  if (max_refine <= 0) {
    MGP_TRY(run_cg(pl, B, X));
    if (iters) *iters = std::max(pl->host_state[0] - 1 - lag, 0);
    if (status) *status = pl->host_state[2];
    if (resid) memcpy(resid, pl->host_resid, (size_t)pl->C * sizeof(float));
    return MGP_OK;
  }
  int total_iters = 0, last_status = 0;
  const float* rhs = B;
  const int egrid = (int)(mgp_cdiv((int64_t)nc, kBlock) > 2048 ? 2048 : mgp_cdiv((int64_t)nc, kBlock));
  const bool f64 = !pl->is_dist;     // single GPU: accumulate x and form the true residual in fp64
  const int rgrid = 256;
  for (int ref = 0; ref <= max_refine; ++ref) {
    MGP_TRY(run_cg(pl, rhs, nullptr));
    total_iters += std::max(pl->host_state[0] - 1 - lag, 0);
    last_status = pl->host_state[2];
    if (f64) {
      hipLaunchKernelGGL(refine_accumulate64_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->buf.xacc64, pl->args.x, (int64_t)nc,
                         ref == 0 ? 1 : 0);
      MGP_LAUNCH_CHECK();
      MGP_TRY(mgp_operator_apply_f64(&pl->op, pl->buf.xacc64, pl->C, pl->buf.t64, pl->buf.work64, st));
      hipLaunchKernelGGL(refine_residual64_kernel, dim3(rgrid), dim3(kBlock), 0, st, B, pl->buf.t64, pl->buf.rbuf, pl->args.n, pl->C,
                         pl->buf.rpart64);
      MGP_LAUNCH_CHECK();
      hipLaunchKernelGGL(refine_finalize64_kernel, dim3(1), dim3(kBlock), 0, st, pl->buf.rpart64, rgrid, pl->C, pl->dev_true_rel);
      MGP_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(refine_accumulate_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->buf.xacc, pl->args.x, (int64_t)nc,
                         ref == 0 ? 1 : 0);
      MGP_LAUNCH_CHECK();
      // true residual R = B - A xacc
      MGP_TRY(mgp_operator_apply_dist(&pl->op, &pl->dist, pl->buf.xacc, nullptr, pl->C, pl->buf.tbuf, nullptr, nullptr, 0, nullptr,
                                      nullptr, pl->buf.op_work, pl->buf.op_work_bytes, st));
      hipLaunchKernelGGL(refine_residual_kernel, dim3(rgrid), dim3(kBlock), 0, st, B, pl->buf.tbuf, pl->buf.rbuf, pl->args.n,
                         pl->C, pl->buf.rpart);
      MGP_LAUNCH_CHECK();
      hipLaunchKernelGGL(refine_finalize_kernel, dim3(1), dim3(kBlock), 0, st, pl->buf.rpart, rgrid, pl->C, pl->dev_true_rel);
      MGP_LAUNCH_CHECK();
    }
    MGP_STREAM_WAIT(st, pl->is_dist && pl->dist.world > 1);
    bool ok = true;
    for (int c = 0; c < pl->C; ++c) ok = ok && (pl->host_true_rel[c] <= 2.0f * pl->prm.tol);
    if (ok || ref == max_refine || last_status == 3) break;
    rhs = pl->buf.rbuf;
  }
  // publish the accumulated solution in the plan buffer (mgp_cg_plan_x) and, if asked, in X
  if (f64) {
    hipLaunchKernelGGL(refine_publish64_kernel, dim3(egrid), dim3(kBlock), 0, st, pl->buf.xacc64, pl->args.x, X, (int64_t)nc);
    MGP_LAUNCH_CHECK();
  } else {
    MGP_HIP_TRY(hipMemcpyAsync(pl->args.x, pl->buf.xacc, nc * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (X) MGP_HIP_TRY(hipMemcpyAsync(X, pl->buf.xacc, nc * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  MGP_STREAM_WAIT(st, pl->is_dist && pl->dist.world > 1);
  if (iters) *iters = total_iters;
  if (status) *status = last_status;
  if (resid) memcpy(resid, pl->host_true_rel, (size_t)pl->C * sizeof(float));   // TRUE relative residuals
  return MGP_OK;
}

// operator applies the last (non-refined) solve actually ran: its step count, minus the detecting step when the
// stopping decision came from the decision-only launch at the end of the first graph
extern "C" int mgp_cg_plan_last_applies(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl) return MGP_ERR_ARG;
  return pl->host_state[0] - (pl->host_state[3] ? 1 : 0);
}

// device pointer of the plan's solution buffer [n, C] (valid until the plan is destroyed)
extern "C" float* mgp_cg_plan_x(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  return pl ? pl->args.x : nullptr;
}

#ifdef MGP_STAMP
// lab build: the stamp ring of the plan (256 x uint64: 8 * wall_clock64 + kind) and how many were written
extern "C" int mgp_cg_plan_debug_block_stamps(void* plan, unsigned long long* out, int nblocks) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl || !out || nblocks > 2048) return MGP_ERR_ARG;
  MGP_HIP_TRY(hipStreamSynchronize(pl->stream));
  MGP_HIP_TRY(hipMemcpy(out, reinterpret_cast<unsigned long long*>(pl->args.state + 16) + 256, (size_t)nblocks * 2 * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
  return MGP_OK;
}
extern "C" int mgp_cg_plan_debug_stamps(void* plan, unsigned long long* out256, int* count) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl || !out256 || !count) return MGP_ERR_ARG;
  MGP_HIP_TRY(hipStreamSynchronize(pl->stream));
  MGP_HIP_TRY(hipMemcpy(count, pl->args.state + 8, sizeof(int), hipMemcpyDeviceToHost));
  MGP_HIP_TRY(hipMemcpy(out256, pl->args.state + 16, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return MGP_OK;
}
#endif

extern "C" double* mgp_cg_plan_x64(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  return (pl && !pl->is_dist) ? pl->buf.xacc64 : nullptr;
}

// A solve that ends in MGP_ERR_TIMEOUT leaves kernels / collectives queued on the stream that still reference the plan's
// buffers, and the peer they wait for is gone: the plan is POISONED.  Destroying a poisoned plan frees nothing and
// synchronises nothing (hipFree / hipGraphExecDestroy / hipStreamDestroy would wait on the dead collective, which is the
// hang the timeout exists to avoid): the memory is leaked on purpose and the process is expected to exit non-zero.
extern "C" int mgp_cg_plan_solve(void* plan, const float* B, float* X, int32_t* iters, float* resid, int32_t* status) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (pl && pl->poisoned) return MGP_ERR_TIMEOUT;
  const int rc = cg_plan_solve_body(plan, B, X, iters, resid, status);
  if (rc == MGP_ERR_TIMEOUT && pl) pl->poisoned = true;
  return rc;
}

extern "C" int mgp_cg_plan_poisoned(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  return pl && pl->poisoned ? 1 : 0;
}

extern "C" int mgp_cg_plan_poison(void* plan) {      // a caller that learns by other means that a peer rank is gone
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl) return MGP_ERR_ARG;
  pl->poisoned = true;
  return MGP_OK;
}

extern "C" int mgp_cg_plan_destroy(void* plan) {
  CgPlan* pl = static_cast<CgPlan*>(plan);
  if (!pl) return MGP_ERR_ARG;
  if (pl->poisoned) return MGP_OK;      // leaked on purpose, see above
  if (pl->exec) (void)hipGraphExecDestroy(pl->exec);
  if (pl->exec_first) (void)hipGraphExecDestroy(pl->exec_first);
  if (pl->graph_first) (void)hipGraphDestroy(pl->graph_first);
  if (pl->cap_stream) (void)hipStreamDestroy(pl->cap_stream);
  host_block_release(pl->host_block, pl->stream);
  delete pl;
  return MGP_OK;
}

extern "C" int mgp_cg_solve(const mgp_operator_t* op, const float* B, int C, float* X, const float* minv,
                            const mgp_cg_params_t* params, int32_t* iters, float* resid, void* work,
                            size_t work_bytes, void* stream) {
  void* plan = nullptr;
  MGP_TRY(mgp_cg_plan_create(op, C, minv, params, work, work_bytes, stream, &plan));
  int32_t status = 0;
  int rc = mgp_cg_plan_solve(plan, B, X, iters, resid, &status);
  (void)mgp_cg_plan_destroy(plan);
  if (rc != MGP_OK) return rc;
  return status == 1 ? MGP_OK : MGP_ERR_NOT_CONVERGED;
}
