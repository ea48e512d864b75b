// Conjugate gradients on the Newton system of the C-class softmax Laplace fit (docs/kernels/classification.md):
//
//   A = Q2 (x) I_C + H(pi),      (H X)_i = pi_i o x_i - pi_i (pi_i . x_i),      X, B, pi row-major [n, C]
//
// ONE SPD system of size n C: the softmax ties the C latent functions together at every observed node, so the solve has one
// alpha and one beta, where the multi-column CG of cg.hip keeps a set per column.  The recurrence is the same single-reduction
// (Chronopoulos-Gear) one, its step rule is cg_rule.h applied to one "column" of length n C, and Q2 on the C columns is the
// operator chain (mgp_operator_apply_ex, with its skip flag).  One step is
//
//   W = Q2 R                                   the chain
//   W_i += pi_i o r_i - pi_i (pi_i . r_i)      softmax_hess_kernel: a group of TC lanes (least power of two >= C) per row, the
//                                              row's dot product by an xor tree in float32; float64 partials of gamma = R . R
//                                              and delta = R . W per workgroup
//   update                                     softmax_update_kernel: every workgroup adds the partials in the same fixed order
//                                              (thread t takes partials t, t + 256, ... in order, xor tree over the wave, the waves in order), forms
//                                              alpha and beta by the rule and runs P = R + beta P, S = W + beta S, X += alpha P,
//                                              R -= alpha S on its share; workgroup 0 takes the stopping decision
//                                              ||r||_2 <= tol ||b||_2 over all n C entries and publishes it
//
// No atomics: a repeated solve is bitwise equal, and so is one with another check_every.  Launches are eager; state[1] turns
// every launch behind the decision into a no-op, and the host copies the state back once per check_every steps.  The scalars
// of step k (gamma, alpha) go to slot k & 1 and are read from there by step k + 1: no launch reads a word that one of its own
// workgroups writes, except the flag, which every workgroup of that launch would set to the same value.
#include "mgp_common.h"
#include "mgp_internal.h"
#include "cg_rule.h"
#include "softmax_rows.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MGP_WAVE;
constexpr int kHessMaxBlocks = 1024;       // grid cap of the epilogue: 1024 x 256 / TC rows per step, one partial pair each
constexpr int kUpdateMaxBlocks = 1024;
constexpr int kDefaultCheckEvery = 8;

// device words of a solve
struct SolveState {
  int it, done, status;    // completed updates, the flag the launches skip on, the status word
  float rel;               // relative residual of the decision
  float bb;                // ||b||^2
  float gamma[2], alpha[2];
};

// the workgroup's two sums from its threads': xor tree over each wave, the waves in order; every thread gets them
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double s_part[kWaves][2];
  const int lane = threadIdx.x & (MGP_WAVE - 1), wave = threadIdx.x / MGP_WAVE;
  a = mgp_wave_sum_d(a);
  b = mgp_wave_sum_d(b);
  if (lane == 0) {
    s_part[wave][0] = a;
    s_part[wave][1] = b;
  }
  __syncthreads();
  a = s_part[0][0];
  b = s_part[0][1];
  for (int k = 1; k < kWaves; ++k) {
    a += s_part[k][0];
    b += s_part[k][1];
  }
}

// Y_i += pi_i o x_i - pi_i (pi_i . x_i); partials (nullable) [gridDim.x][2] = sum x . x, sum x . y of the workgroup's rows
template <int TC>
__global__ __launch_bounds__(kBlock) void softmax_hess_kernel(const float* __restrict__ pi, const float* __restrict__ X,
                                                              float* __restrict__ Y, int64_t n, int C,
                                                              double* __restrict__ partials, const int* __restrict__ skip) {
  if (skip && *skip) return;
  constexpr int kRows = kBlock / TC;
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  const int64_t steps = (n + stride - 1) / stride;
  double xx = 0.0, xy = 0.0;
  for (int64_t k = 0; k < steps; ++k) {
    const int64_t i = k * stride + (int64_t)blockIdx.x * kRows + g;
    const bool live = i < n && c < C;
    const int64_t at = i * C + c;
    const float p = live ? pi[at] : 0.f;
    const float x = live ? X[at] : 0.f;
    const float dot = mgp_group_sum<TC>(p * x);
    if (!live) continue;
    const float y = Y[at] + (p * x - p * dot);
    Y[at] = y;
    xx += (double)x * (double)x;
    xy += (double)x * (double)y;
  }
  if (partials) {
    block_sum2(xx, xy);
    if (threadIdx.x == 0) {
      partials[2 * (int64_t)blockIdx.x] = xx;
      partials[2 * (int64_t)blockIdx.x + 1] = xy;
    }
  }
}

__global__ __launch_bounds__(kBlock) void softmax_update_kernel(const double* __restrict__ partials, int nblk, int step,
                                                                float tol, int max_iter, int64_t len, float* __restrict__ X,
                                                                float* __restrict__ R, float* __restrict__ P,
                                                                float* __restrict__ S, const float* __restrict__ W,
                                                                SolveState* __restrict__ st) {
  if (st->done) return;
  double g64 = 0.0, d64 = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kBlock) {                    // thread t: partials t, t + 256, ... in order
    g64 += partials[2 * b];
    d64 += partials[2 * b + 1];
  }
  block_sum2(g64, d64);
  const float gamma = (float)g64, delta = (float)d64;
  const bool first = step == 1;
  const float bb = first ? gamma : st->bb;                              // r_0 = b
  const float rel = cg_rel(gamma, bb);
  const CgStop stop = cg_stop(1, 0, max_iter, tol, step, rel);
  const int prev = (step - 1) & 1, cur = step & 1;
  const CgCoef k = cg_coef(first, false, gamma, delta, first ? 0.f : st->gamma[prev], first ? 0.f : st->alpha[prev]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (first) st->bb = bb;
    st->rel = rel;
    if (stop.done) {
      st->status = stop.status;
      st->done = 1;
    } else {
      st->gamma[cur] = gamma;
      st->alpha[cur] = k.alpha;
      st->it = step;
    }
  }
  if (stop.done) return;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < len; j += stride) {
    const float r = R[j], w = W[j];
    const float p = first ? r : r + k.beta * P[j];                      // (P, S and X are not read at the first step)
    const float s = first ? w : w + k.beta * S[j];
    P[j] = p;
    S[j] = s;
    X[j] = first ? k.alpha * p : X[j] + k.alpha * p;
    R[j] = r - k.alpha * s;
  }
}

int hess_blocks(int64_t n, int C) { return mgp_softmax_blocks(n, C, kBlock, kHessMaxBlocks); }

int hess_add(const float* pi, const float* X, float* Y, int64_t n, int C, double* partials, const int* skip, hipStream_t st) {
  const int blocks = hess_blocks(n, C);
  mgp_softmax_dispatch(C, [&](auto tc) {
    hipLaunchKernelGGL(softmax_hess_kernel<decltype(tc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, pi, X, Y, n, C,
                       partials, skip);
  });
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

struct Carve {
  float *R, *P, *S, *W;
  double* partials;
  SolveState* state;
  void* opwork;
  size_t opbytes;
};

// the one statement of the workspace layout: a counting arena sizes it, a real one hands it out
bool carve(MgpArena& ar, const mgp_operator_t* op, int C, Carve* cv) {
  const size_t nc = (size_t)op->L.n * C;
  cv->R = ar.take<float>(nc);
  cv->P = ar.take<float>(nc);
  cv->S = ar.take<float>(nc);
  cv->W = ar.take<float>(nc);
  cv->partials = ar.take<double>(2 * (size_t)kHessMaxBlocks);
  cv->state = ar.take<SolveState>(1);
  cv->opbytes = mgp_operator_workspace_bytes(op, C);
  cv->opwork = ar.take<char>(cv->opbytes);
  return ar.ok();
}

bool args_ok(const mgp_operator_t* op, int C) {
  return op && C >= 2 && C <= 64 && op->form >= 0 && op->form <= 3 && mgp_operator_workspace_bytes(op, C) != 0;
}

}  // namespace

extern "C" int mgp_softmax_hessian_add(const float* pi, const float* X, int64_t n, int C, float* Y, void* stream) {
  if (!pi || !X || !Y || X == Y || n < 1 || C < 2 || C > 64) return MGP_ERR_ARG;
  return hess_add(pi, X, Y, n, C, nullptr, nullptr, mgp_stream(stream));
}

extern "C" size_t mgp_softmax_cg_workspace_bytes(const mgp_operator_t* op, int C) {
  if (!op) return 0;
  const mgp_operator_t o = mgp_operator_copy(op);
  if (!args_ok(&o, C) || o.form != 0) return 0;
  MgpArena count;
  Carve cv;
  carve(count, &o, C, &cv);
  return count.off;
}

extern "C" int mgp_softmax_cg(const mgp_operator_t* op, const float* pi, int C, const float* B, float* X, float tol,
                              int max_iter, int check_every, int32_t* iters, float* resid, int32_t* status, void* work,
                              size_t work_bytes, void* stream) {
  if (!op || !pi || !B || !X || B == X) return MGP_ERR_ARG;
  const mgp_operator_t o = mgp_operator_copy(op);
  if (!args_ok(&o, C) || !(tol >= 0.f) || max_iter < 1 || check_every < 0) return MGP_ERR_ARG;
  if (o.form != 0) return MGP_ERR_UNSUPPORTED;
  if (!work || (reinterpret_cast<uintptr_t>(work) & 15) != 0 || work_bytes < mgp_softmax_cg_workspace_bytes(op, C))
    return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  Carve cv;
  if (!carve(ar, &o, C, &cv)) return MGP_ERR_WORKSPACE;
  if (check_every == 0) check_every = kDefaultCheckEvery;
  hipStream_t st = mgp_stream(stream);
  const int64_t n = o.L.n, len = n * C;
  const int nblk = hess_blocks(n, C);
  int64_t ub = mgp_cdiv(len, (int64_t)kBlock);
  if (ub > kUpdateMaxBlocks) ub = kUpdateMaxBlocks;

  MGP_HIP_TRY(hipMemsetAsync(cv.state, 0, sizeof(SolveState), st));
  MGP_HIP_TRY(hipMemsetAsync(X, 0, (size_t)len * sizeof(float), st));                  // the answer when B = 0
  MGP_HIP_TRY(hipMemcpyAsync(cv.R, B, (size_t)len * sizeof(float), hipMemcpyDeviceToDevice, st));
  SolveState host = {};
  for (int step = 1; step <= max_iter + 1; ++step) {                                   // step max_iter + 1 only decides
    MGP_TRY(mgp_operator_apply_ex(&o, cv.R, C, cv.W, nullptr, nullptr, &cv.state->done, nullptr, cv.opwork, cv.opbytes,
                                  stream));
    MGP_TRY(hess_add(pi, cv.R, cv.W, n, C, cv.partials, &cv.state->done, st));
    hipLaunchKernelGGL(softmax_update_kernel, dim3((unsigned)ub), dim3(kBlock), 0, st, cv.partials, nblk, step, tol, max_iter,
                       len, X, cv.R, cv.P, cv.S, cv.W, cv.state);
    MGP_LAUNCH_CHECK();
    if (step % check_every == 0 || step == max_iter + 1) {
      MGP_HIP_TRY(hipMemcpyAsync(&host, cv.state, sizeof(SolveState), hipMemcpyDeviceToHost, st));
      MGP_HIP_TRY(hipStreamSynchronize(st));
      if (host.done) break;
    }
  }
  if (iters) *iters = host.it;
  if (resid) *resid = host.rel;
  if (status) *status = host.status;
  return MGP_OK;
}
