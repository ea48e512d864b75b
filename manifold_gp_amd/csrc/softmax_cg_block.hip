// S right-hand sides of the softmax Newton system at once (docs/kernels/classification.md, "Samples in blocks"):
//
//   A X_s = B_s,  s = 0 .. S - 1,      A = Q2 (x) I_C + H(pi),      X, B row-major [n, S, C],  pi [n, C] shared
//
// The samples of a Laplace fit share the matrix and differ in the right-hand side, so the operator chain runs once per step on
// the S C columns of the block, where softmax_cg.hip runs it once per sample on C.  Each sample keeps the scalar set of its own
// CG: gamma_s = R_s . R_s, delta_s = R_s . W_s, alpha_s, beta_s, ||b_s||^2, rel_s; the rule is cg_rule.h with a sample in the
// place of a column.  One step is
//
//   W = Q2 R                                   the chain on S C columns
//   W_is += pi_i o r_is - pi_i (pi_i . r_is)   sblk_hess_kernel: a group of TC lanes per (node, sample) row; a group keeps one
//                                              sample for the whole launch; float64 partials of gamma_s and delta_s, one pair
//                                              per (sample, workgroup), the workgroup's groups added in ascending order
//   sums_s = the partials of s in order        sblk_reduce_kernel: one workgroup per sample, thread t takes the partials
//                                              t, t + 256, ..., xor tree over the wave, the waves in order
//   update                                     sblk_update_kernel: alpha_s, beta_s by the rule; P = R + beta_s P,
//                                              S = W + beta_s S, X += alpha_s P, R -= alpha_s S; a thread keeps one sample for
//                                              the whole launch.  A sample with rel_s <= tol is frozen: its threads write
//                                              nothing, so X_s and R_s keep their bits and gamma_s repeats: it stays frozen.
//                                              Workgroup 0 publishes the scalars and the block's decision.
//
// softmax_block.h holds the layout (which rows a group takes, the grids, the partial slots, the carve).  No atomics; every
// float64 sum has a fixed order, and a sample's sums hold its own rows alone: sample s does not see the other right-hand
// sides, check_every or a repetition.  The scalars of step k go to slot k & 1 and step k + 1 reads them there: no launch
// reads a word that one of its own workgroups writes, except the flag, which every workgroup would set alike.
#include "mgp_common.h"
#include "mgp_internal.h"
#include "cg_rule.h"
#include "softmax_rows.h"
#include "softmax_block.h"

namespace {

constexpr int kWaves = kBlkThreads / MGP_WAVE;
constexpr int kMaxSamples = kBlkMaxCols / 2;      // C >= 2
constexpr int kDefaultCheckEvery = 8;

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

// Y_q += pi_i o x_q - pi_i (pi_i . x_q) for the rows q = i S + s; partials (nullable) [S][gridDim.x][2] = sum x . x and
// sum x . y over the workgroup's rows of each sample
template <int TC>
__global__ __launch_bounds__(kBlkThreads) void sblk_hess_kernel(const float* __restrict__ pi, const float* __restrict__ X,
                                                                float* __restrict__ Y, int64_t n, int C, int S, SblkHess h,
                                                                double* __restrict__ partials, const int* __restrict__ skip) {
  if (skip && *skip) return;
  constexpr int kRows = kBlkThreads / TC;
  __shared__ double s_grp[kRows][2];
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t j = sblk_group(h, (int)blockIdx.x, g);
  const int s = (int)(j % S);
  const int64_t i0 = j / S;
  double xx = 0.0, xy = 0.0;
  for (int64_t k = 0; k < h.passes; ++k) {
    const int64_t i = i0 + k * h.node_step;
    const bool live = i < n && c < C;
    const int64_t at = (i * S + s) * C + c;
    const float p = live ? pi[i * C + c] : 0.f;
    const float x = live ? X[at] : 0.f;
    const float dot = mgp_group_sum<TC>(p * x);
    if (!live) continue;
    const float y = Y[at] + (p * x - p * dot);
    Y[at] = y;
    xx += (double)x * (double)x;
    xy += (double)x * (double)y;
  }
  if (!partials) return;
  xx = mgp_group_sum_d<TC>(xx);
  xy = mgp_group_sum_d<TC>(xy);
  if (c == 0) {
    s_grp[g][0] = xx;
    s_grp[g][1] = xy;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < S; t += kBlkThreads) {
    double a = 0.0, b = 0.0;
    for (int gg = sblk_first_group(h, S, (int)blockIdx.x, t); gg < kRows; gg += S) {
      a += s_grp[gg][0];
      b += s_grp[gg][1];
    }
    const size_t at = sblk_slot(t, (int)blockIdx.x, (int)gridDim.x);
    partials[at] = a;
    partials[at + 1] = b;
  }
}

// sums[s] = the nblk partial pairs of sample s = blockIdx.x, in a fixed order
__global__ __launch_bounds__(kBlkThreads) void sblk_reduce_kernel(const double* __restrict__ partials, int nblk,
                                                                  double* __restrict__ sums, const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int s = (int)blockIdx.x;
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < nblk; k += kBlkThreads) {               // thread t: partials t, t + 256, ... in order
    const size_t at = sblk_slot(s, k, nblk);
    a += partials[at];
    b += partials[at + 1];
  }
  block_sum2(a, b);
  if (threadIdx.x == 0) {
    sums[2 * s] = a;
    sums[2 * s + 1] = b;
  }
}

struct SampleStep {
  float gamma, bb, rel;
  bool frozen;
  CgCoef k;
};

// the scalars of sample s at this step, from its sums and the previous step's slot: every thread that asks gets the same bits
__device__ __forceinline__ SampleStep sample_step(const double* __restrict__ sums, const SblkSample* __restrict__ smp, int s,
                                                  int step, float tol) {
  const bool first = step == 1;
  const int prev = (step - 1) & 1;
  SampleStep r;
  r.gamma = (float)sums[2 * s];
  const float delta = (float)sums[2 * s + 1];
  r.bb = first ? r.gamma : smp[s].bb;                                   // r_0 = b
  r.rel = cg_rel(r.gamma, r.bb);
  r.frozen = cg_frozen(1, tol, r.rel);
  r.k = cg_coef(first, r.frozen, r.gamma, delta, first ? 0.f : smp[s].gamma[prev], first ? 0.f : smp[s].alpha[prev]);
  return r;
}

__global__ __launch_bounds__(kBlkThreads) void sblk_update_kernel(const double* __restrict__ sums, int C, int S, int step,
                                                                  float tol, int max_iter, int64_t len, float* __restrict__ X,
                                                                  float* __restrict__ R, float* __restrict__ P,
                                                                  float* __restrict__ Sv, const float* __restrict__ W,
                                                                  SblkHead* __restrict__ head, SblkSample* __restrict__ smp) {
  __shared__ float s_rel[kMaxSamples];
  __shared__ int s_stop[2], s_skip;
  if (threadIdx.x == 0) s_skip = head->done;       // one read per workgroup: workgroup 0 of this launch may be setting the flag
  __syncthreads();
  if (s_skip) return;
  const bool first = step == 1;
  const int prev = (step - 1) & 1, cur = step & 1;
  for (int t = threadIdx.x; t < S; t += kBlkThreads) s_rel[t] = sample_step(sums, smp, t, step, tol).rel;
  __syncthreads();
  if (threadIdx.x == 0) {
    const CgStop stop = cg_stop_columns(1, 0, max_iter, tol, step, s_rel, S);
    s_stop[0] = stop.done;
    s_stop[1] = stop.status;
  }
  __syncthreads();
  const bool done = s_stop[0] != 0;
  if (blockIdx.x == 0) {
    for (int t = threadIdx.x; t < S; t += kBlkThreads) {
      const SampleStep q = sample_step(sums, smp, t, step, tol);
      if (first) smp[t].bb = q.bb;
      smp[t].rel = q.rel;
      if (!done) {
        smp[t].gamma[cur] = q.gamma;
        smp[t].alpha[cur] = q.k.alpha;
        smp[t].it[cur] = (first ? 0 : smp[t].it[prev]) + (q.frozen ? 0 : 1);
      }
    }
    if (threadIdx.x == 0 && done) {
      head->status = s_stop[1];
      head->step = step;
      head->done = 1;
    }
  }
  if (done) return;
  const int64_t e0 = (int64_t)blockIdx.x * kBlkThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlkThreads;               // a multiple of S C: the sample below holds for every j
  if (e0 >= len) return;
  const int s = (int)((e0 / C) % S);
  const SampleStep q = sample_step(sums, smp, s, step, tol);
  if (q.frozen) return;                                                  // X_s, R_s, P_s, S_s keep their bits
  for (int64_t j = e0; j < len; j += stride) {
    const float r = R[j], w = W[j];
    const float p = first ? r : r + q.k.beta * P[j];                     // (P, S and X are not read at the first step)
    const float sv = first ? w : w + q.k.beta * Sv[j];
    P[j] = p;
    Sv[j] = sv;
    X[j] = first ? q.k.alpha * p : X[j] + q.k.alpha * p;
    R[j] = r - q.k.alpha * sv;
  }
}

int hess_add(const float* pi, const float* X, float* Y, int64_t n, int C, int S, double* partials, const int* skip,
             hipStream_t st) {
  const SblkHess h = sblk_hess(n, C, S);
  mgp_softmax_dispatch(C, [&](auto tc) {
    hipLaunchKernelGGL(sblk_hess_kernel<decltype(tc)::value>, dim3((unsigned)h.grid), dim3(kBlkThreads), 0, st, pi, X, Y, n, C,
                       S, h, partials, skip);
  });
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

int reduce(const double* partials, int64_t n, int C, int S, double* sums, const int* skip, hipStream_t st) {
  hipLaunchKernelGGL(sblk_reduce_kernel, dim3((unsigned)S), dim3(kBlkThreads), 0, st, partials, sblk_hess(n, C, S).grid, sums,
                     skip);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

bool args_ok(const mgp_operator_t* op, int C, int S) {
  return op && sblk_shape_ok(C, S) && op->form >= 0 && op->form <= 3 && mgp_operator_workspace_bytes(op, S * C) != 0;
}

}  // namespace

extern "C" size_t mgp_softmax_hessian_add_block_workspace_bytes(int64_t n, int C, int S) {
  if (n < 1 || !sblk_shape_ok(C, S)) return 0;
  MgpArena count;
  double* partials;
  sblk_carve_hess(count, S, &partials);
  return count.off;
}

extern "C" int mgp_softmax_hessian_add_block(const float* pi, const float* X, int64_t n, int C, int S, float* Y, double* sums,
                                             void* work, size_t work_bytes, void* stream) {
  if (!pi || !X || !Y || X == Y || n < 1 || !sblk_shape_ok(C, S)) return MGP_ERR_ARG;
  double* partials = nullptr;
  if (sums) {
    if (!work || (reinterpret_cast<uintptr_t>(work) & 15) != 0) return MGP_ERR_WORKSPACE;
    MgpArena ar(work, work_bytes);
    if (!sblk_carve_hess(ar, S, &partials)) return MGP_ERR_WORKSPACE;
  }
  hipStream_t st = mgp_stream(stream);
  MGP_TRY(hess_add(pi, X, Y, n, C, S, partials, nullptr, st));
  if (sums) MGP_TRY(reduce(partials, n, C, S, sums, nullptr, st));
  return MGP_OK;
}

extern "C" size_t mgp_softmax_cg_block_workspace_bytes(const mgp_operator_t* op, int C, int S) {
  if (!op) return 0;
  const mgp_operator_t o = mgp_operator_copy(op);
  if (!args_ok(&o, C, S) || o.form != 0) return 0;
  MgpArena count;
  SblkCarve cv;
  sblk_carve(count, o.L.n, C, S, mgp_operator_workspace_bytes(&o, S * C), &cv);
  return count.off;
}

extern "C" int mgp_softmax_cg_block(const mgp_operator_t* op, const float* pi, int C, int S, const float* B, float* X,
                                    float tol, int max_iter, int check_every, int32_t* iters, float* resid, int32_t* status,
                                    void* work, size_t work_bytes, void* stream) {
  if (!op || !pi || !B || !X || B == X) return MGP_ERR_ARG;
  const mgp_operator_t o = mgp_operator_copy(op);
  if (!args_ok(&o, C, S) || !(tol >= 0.f) || max_iter < 1 || check_every < 0) return MGP_ERR_ARG;
  if (o.form != 0) return MGP_ERR_UNSUPPORTED;
  if (!work || (reinterpret_cast<uintptr_t>(work) & 15) != 0 || work_bytes < mgp_softmax_cg_block_workspace_bytes(op, C, S))
    return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  SblkCarve cv;
  if (!sblk_carve(ar, o.L.n, C, S, mgp_operator_workspace_bytes(&o, S * C), &cv)) return MGP_ERR_WORKSPACE;
  if (check_every == 0) check_every = kDefaultCheckEvery;
  hipStream_t st = mgp_stream(stream);
  const int64_t n = o.L.n, len = n * S * C;
  const SblkUpdate up = sblk_update(n, C, S);
  SblkHead* head = reinterpret_cast<SblkHead*>(cv.state);
  SblkSample* smp = reinterpret_cast<SblkSample*>(cv.state + sizeof(SblkHead));
  const size_t state_bytes = sblk_state_bytes(S);

  MGP_HIP_TRY(hipMemsetAsync(cv.state, 0, state_bytes, st));
  MGP_HIP_TRY(hipMemsetAsync(X, 0, (size_t)len * sizeof(float), st));                  // the answer where B_s = 0
  MGP_HIP_TRY(hipMemcpyAsync(cv.R, B, (size_t)len * sizeof(float), hipMemcpyDeviceToDevice, st));
  std::vector<char> host(state_bytes, 0);
  const SblkHead* hh = reinterpret_cast<const SblkHead*>(host.data());
  const SblkSample* hs = reinterpret_cast<const SblkSample*>(host.data() + sizeof(SblkHead));
  for (int step = 1; step <= max_iter + 1; ++step) {                                   // step max_iter + 1 only decides
    MGP_TRY(mgp_operator_apply_ex(&o, cv.R, S * C, cv.W, nullptr, nullptr, &head->done, nullptr, cv.opwork, cv.opbytes, stream));
    MGP_TRY(hess_add(pi, cv.R, cv.W, n, C, S, cv.partials, &head->done, st));
    MGP_TRY(reduce(cv.partials, n, C, S, cv.sums, &head->done, st));
    hipLaunchKernelGGL(sblk_update_kernel, dim3((unsigned)up.grid), dim3(kBlkThreads), 0, st, cv.sums, C, S, step, tol, max_iter,
                       len, X, cv.R, cv.P, cv.Sv, cv.W, head, smp);
    MGP_LAUNCH_CHECK();
    if (step % check_every == 0 || step == max_iter + 1) {
      MGP_HIP_TRY(hipMemcpyAsync(host.data(), cv.state, state_bytes, hipMemcpyDeviceToHost, st));
      MGP_HIP_TRY(hipStreamSynchronize(st));
      if (hh->done) break;
    }
  }
  const int last = (hh->step - 1) & 1;                                                 // the slot of the last update made
  for (int s = 0; s < S; ++s) {
    if (iters) iters[s] = hh->step >= 1 ? hs[s].it[last] : 0;
    if (resid) resid[s] = hs[s].rel;
  }
  if (status) *status = hh->status;
  return MGP_OK;
}
