// Marginal posterior variances in precision form (docs/kernels/sampling.md, "Marginal variances"): the two kernels the
// single-site Rao-Blackwell estimator adds to the sampler.  Neither is on an iteration path.
//
// 1. mgp_operator_diag_exact: the diagonal of operator forms 0 / 2 / 3 for nu = 1, 2, 3 in float64.  With
//    A = tau I + L_sym = diag(a) - S (a_i = tau + diag_i, S the stored off-diagonal values, S_ji = S_ij):
//      diag(A)_i   = a_i
//      diag(A^2)_i = a_i^2 + sum_j S_ij^2
//      diag(A^3)_i = a_i^3 + 2 a_i sum_j S_ij^2 + sum_j a_j S_ij^2 - sum_j S_ij sum_k S_jk S_ik     (k != i, j: triangles)
//    and (Q2)_ii = scale pre_i post_i diag(A^nu)_i.  A wave per row i: lanes over the neighbours j; for nu = 3 a lane walks
//    row j and looks every k up in row i's (column, value) list, which the wave holds in LDS.  Entries with col == row or
//    S == 0 (padding) are skipped as in gmrf_noise_kernel.  The graph builders write a row's columns ascending with the
//    padding at its end (graph.hip), but a caller's CSR need not: the wave checks its LDS copy (padding rewritten to the
//    largest column id) and looks up by binary search only when the copy ascends strictly, by a linear scan that adds
//    every match otherwise.  A row longer than the LDS list is scanned in global memory the same way.  Every lane sums
//    its own terms in CSR order, the lanes are added by a fixed xor tree: no atomics, repeated calls are bitwise equal.
//
// 2. mgp_row_moments: acc[i] += (sum_c u v, sum_c (u v)^2) over the columns of a sample block, u = U - Pm rdiag,
//    v likewise from V, in float64.  A group of lanes per row, a float4 per lane and step where the rows are whole
//    aligned quads, scalar loads otherwise; xor tree over the group; lane 0 adds to the caller's state.
#include <limits.h>
#include "mgp_common.h"
#include "mgp_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MGP_WAVE;
constexpr int kList = 512;   // (column, value) pairs of row i a wave keeps in LDS: 4 KiB per wave, 16 KiB per workgroup

// S_ik from row i's list; 0 when i and k are not neighbours
__device__ __forceinline__ double list_value(const int32_t* lc, const float* lv, int len, bool ascending, int k) {
  if (ascending) {
    int lo = 0, hi = len;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lc[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    return (lo < len && lc[lo] == k) ? (double)lv[lo] : 0.0;
  }
  double s = 0.0;
  for (int e = 0; e < len; ++e)
    if (lc[e] == k) s += (double)lv[e];
  return s;
}

__global__ __launch_bounds__(kBlock) void diag_exact_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, const float* __restrict__ vals,
                                                            const float* __restrict__ diag, const float* __restrict__ pre,
                                                            const float* __restrict__ post, const float* __restrict__ obs_w,
                                                            int nu, double tau, double scale, int form, double noise,
                                                            double* __restrict__ out) {
  __shared__ int32_t s_col[kWaves][kList];
  __shared__ float s_val[kWaves][kList];
  const int lane = threadIdx.x & (MGP_WAVE - 1), wave = threadIdx.x / MGP_WAVE;
  // workgroup-uniform trip count: the barriers below are reached by all four waves
  for (int64_t base = (int64_t)blockIdx.x * kWaves; base < n; base += (int64_t)gridDim.x * kWaves) {
    const int64_t r = base + wave;
    const bool live = r < n;
    const int s0 = live ? rowptr[r] : 0, s1 = live ? rowptr[r + 1] : 0;
    const int len = s1 - s0;
    const bool in_lds = nu == 3 && len <= kList;
    if (in_lds) {
      for (int e = lane; e < len; e += MGP_WAVE) {
        const int c = col[s0 + e];
        const float v = vals[s0 + e];
        const bool pad = c == (int)r || v == 0.0f;
        s_col[wave][e] = pad ? INT_MAX : c;
        s_val[wave][e] = pad ? 0.0f : v;
      }
    }
    __syncthreads();
    bool ascending = false;
    if (in_lds) {
      bool bad = false;
      for (int e = 1 + lane; e < len; e += MGP_WAVE) {
        const int p = s_col[wave][e - 1], c = s_col[wave][e];
        bad = bad || !(p < c || (p == INT_MAX && c == INT_MAX));
      }
      ascending = __ballot(bad) == 0ull;
    }
    const int32_t* lc = in_lds ? s_col[wave] : col + s0;
    const float* lv = in_lds ? s_val[wave] : vals + s0;
    double s2 = 0.0, s2a = 0.0, tri = 0.0;
    if (nu >= 2) {
      for (int e = s0 + lane; e < s1; e += MGP_WAVE) {
        const int j = col[e];
        const double sij = (double)vals[e];
        if (j == (int)r || sij == 0.0) continue;                       // padding (col == row, S = 0)
        s2 += sij * sij;
        if (nu == 3) {
          double t = 0.0;
          const int j1 = rowptr[j + 1];
          for (int f = rowptr[j]; f < j1; ++f) {
            const int k = col[f];
            const double sjk = (double)vals[f];
            if (k == j || k == (int)r || sjk == 0.0) continue;
            t += sjk * list_value(lc, lv, len, ascending, k);
          }
          s2a += (tau + (double)diag[j]) * (sij * sij);
          tri += sij * t;
        }
      }
      s2 = mgp_wave_sum_d(s2);
      if (nu == 3) {
        s2a = mgp_wave_sum_d(s2a);
        tri = mgp_wave_sum_d(tri);
      }
    }
    if (live && lane == 0) {
      const double a = tau + (double)diag[r];
      double p = a;
      if (nu == 2) p = a * a + s2;
      if (nu == 3) p = a * a * a + 2.0 * a * s2 + s2a - tri;
      double q = scale * p;
      if (pre) q *= (double)pre[r];
      if (post) q *= (double)post[r];
      out[r] = form == 0 ? q : (form == 2 ? 1.0 : (double)obs_w[r]) + noise * q;
    }
    __syncthreads();                                                   // the lists are rewritten by the next round
  }
}

__device__ __forceinline__ void add_moment(double u, double v, double& m1, double& m2) {
  const double p = u * v;
  m1 += p;
  m2 += p * p;
}

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void row_moments_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                             const double* __restrict__ rdiag, const float* __restrict__ Pm,
                                                             int64_t n, int C, int G, double* __restrict__ acc) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t g0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int64_t ng = ((int64_t)gridDim.x * blockDim.x) / G;
  for (int64_t r = g0; r < n; r += ng) {                               // group-uniform: the shuffles below are converged
    const float* ur = U + r * (int64_t)C;
    const float* vr = V ? V + r * (int64_t)C : nullptr;
    const float* pr = Pm ? Pm + r * (int64_t)C : nullptr;
    const double rd = Pm ? rdiag[r] : 0.0;
    double m1 = 0.0, m2 = 0.0;
    if (VEC4) {
      for (int c = 4 * lane; c < C; c += 4 * G) {
        const float4 uf = *reinterpret_cast<const float4*>(ur + c);
        double u[4] = {(double)uf.x, (double)uf.y, (double)uf.z, (double)uf.w};
        double v[4] = {u[0], u[1], u[2], u[3]};
        if (vr) {
          const float4 vf = *reinterpret_cast<const float4*>(vr + c);
          v[0] = (double)vf.x, v[1] = (double)vf.y, v[2] = (double)vf.z, v[3] = (double)vf.w;
        }
        if (pr) {
          const float4 pf = *reinterpret_cast<const float4*>(pr + c);
          const double s[4] = {(double)pf.x * rd, (double)pf.y * rd, (double)pf.z * rd, (double)pf.w * rd};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            u[t] -= s[t];
            v[t] -= s[t];
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) add_moment(u[t], v[t], m1, m2);
      }
    } else {
      for (int c = lane; c < C; c += G) {
        const double s = pr ? (double)pr[c] * rd : 0.0;
        const double u = (double)ur[c] - s;
        add_moment(u, vr ? (double)vr[c] - s : u, m1, m2);
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {                             // fixed tree over the group
      m1 += __shfl_xor(m1, o, 64);
      m2 += __shfl_xor(m2, o, 64);
    }
    if (lane == 0) {
      acc[2 * r] += m1;
      acc[2 * r + 1] += m2;
    }
  }
}

int pow2_ceil64(int v) {
  int p = 1;
  while (p < v && p < MGP_WAVE) p <<= 1;
  return p;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" size_t mgp_operator_diag_exact_workspace_bytes(const mgp_operator_t* op) {
  (void)op;
  return 0;   // row i's list lives in LDS: no scratch in memory
}

extern "C" int mgp_operator_diag_exact(const mgp_operator_t* op_in, double* diag_out, void* work, size_t work_bytes,
                                       void* stream) {
  (void)work;
  (void)work_bytes;
  if (!op_in || !diag_out) return MGP_ERR_ARG;
  const mgp_operator_t op = mgp_operator_copy(op_in);
  if (!op.L.rowptr || !op.L.col || !op.L.vals || !op.L.diag) return MGP_ERR_ARG;
  if (op.L.n < 1 || op.L.n >= ((int64_t)1 << 31) || op.nu < 1 || !(op.kappa > 0.f)) return MGP_ERR_ARG;
  if (op.form < 0 || op.form > 3 || (op.form == 3 && !op.obs_w)) return MGP_ERR_ARG;
  if (op.form == 1 || op.nu > 3) return MGP_ERR_UNSUPPORTED;
  // tau, scale and s as the float64 operator of the refined solves takes them (operator.hip, q2_chain_f64)
  const double tau = 2.0 * (double)op.nu / ((double)op.kappa * (double)op.kappa);
  int64_t blocks = mgp_cdiv(op.L.n, kWaves);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(diag_exact_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), op.L.n, op.L.rowptr,
                     op.L.col, op.L.vals, op.L.diag, op.pre, op.post, op.obs_w, op.nu, tau, (double)op.scale, op.form,
                     (double)op.noise, diag_out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_row_moments(const float* U, const float* V, const double* rdiag, const float* Pm, int64_t n, int C,
                               double* acc, void* stream) {
  if (!U || !acc || n < 1 || C < 1 || C > 256 || (Pm && !rdiag)) return MGP_ERR_ARG;
  if (V == U) V = nullptr;
  const bool vec4 = (C & 3) == 0 && aligned16(U) && aligned16(V) && aligned16(Pm);
  const int G = pow2_ceil64(vec4 ? C / 4 : C);
  int64_t blocks = mgp_cdiv(n, kBlock / G);
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (vec4)
    hipLaunchKernelGGL(row_moments_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), U, V, rdiag, Pm,
                       n, C, G, acc);
  else
    hipLaunchKernelGGL(row_moments_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), U, V, rdiag,
                       Pm, n, C, G, acc);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
