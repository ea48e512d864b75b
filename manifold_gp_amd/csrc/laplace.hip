// The per-node kernels of the Laplace fits on the graph nodes: Bernoulli-logit and softmax (docs/kernels/classification.md),
// Poisson / binomial / negative binomial (docs/kernels/counts.md), ordered categories (docs/kernels/ordinal.md), and of their
// evidence (docs/kernels/evidence.md).  All float64 arithmetic from float32 inputs, one rounding at the store.
//
// The node loop (site_kernel, evidence_kernel).  Every family of the two per-node stages runs one loop: a thread takes quads of
// nodes at a grid stride (256 threads, at most 1024 workgroups), a float4 / uchar4 (var: two double2) per array and step where
// every array is 16-byte (obs 4-byte) aligned, scalar otherwise and for the last n % 4 nodes.  The family -- a struct passed by
// value, its scalars as members and operator() the formulas of one node -- is the template argument.  Its two input
// arrays (a, b) are (y, -) for Bernoulli, (y, aux) for the counts and (lo, hi) for ordinal; they are read only where a node of
// the quad is observed (they may be NaN elsewhere) and b may be NULL (zeros).  qf NULL: zeros; obs NULL: every node.
//
// The sums.  A thread adds its nodes in index order into a SiteAcc {lp, fq, mx, sq}; block_reduce takes an xor tree over each
// wave and the waves in order; store_partials leaves the workgroup's four float64 numbers in the workspace (32 bytes per
// workgroup) and a second single-workgroup launch, site_sum_kernel, adds the partials in a fixed order into sums[4].  No atomics:
// repeated calls are bitwise equal.  Newton stage: sums = { sum_obs log p, sum f qf, max |g - qf|, sum (g - qf)^2 }; evidence
// stage: { sum_obs log p, nodes kept, sum corr, max |corr| } (sum_first: the sum slot leaves before the max slot).
//
// Newton stage (mgp_bernoulli_site, mgp_count_site, mgp_nb_site, mgp_ordinal_site): from the family's log p, g = d log p / df and
// h = -d g / df on observed nodes (g = h = 0 elsewhere), w = s_ref h and rhs = s_ref (g - qf) leave as float32.
//   Bernoulli, t = (y > 0.5), a = (2 t - 1) f, e = exp(-|f|):  log p = min(a, 0) - log1p(e), pi = f >= 0 ? 1 / (1 + e) : e / (1 + e),
//     g = t - pi, h = e / (1 + e)^2  (no overflow, h without cancellation).
//   Poisson, eta = f + mean + log-exposure:  mu = exp(min(eta, 700)), log p = y eta - mu, g = y - mu, h = mu.
//   Binomial with N trials, eta = f + mean, e = exp(-|eta|):  log p = -(N - y)(max(eta, 0) + log1p(e)) - y (max(-eta, 0) + log1p(e)),
//     g = y (1 - pi) - (N - y) pi with 1 - pi formed without the subtraction, h = N e / (1 + e)^2.
//   Negative binomial with dispersion r:  the binomial arithmetic with y + r trials and r failures at eta = f + mean +
//     log-exposure - log r, so 0 < h <= (y + r) / 4.
//   h of the counts is unbounded: their w and rhs saturate at +-FLT_MAX instead of leaving as inf (site_tail<true>).
//   Ordinal, the node's interval of cutpoints (lo, hi], u = hi - f, l = lo - f:  log p = log sigma(u) + log sigma(-l) (the product
//     form of sigma(u) - sigma(l), its f-independent factor left to the caller), g = sigma(l) - sigma(-u),
//     h = sigma(u) sigma(-u) + sigma(l) sigma(-l) in (0, 1/2].  The ends may be infinite.
//
// Evidence stage at the mode (mgp_laplace_evidence_site, mgp_nb_evidence_site, mgp_ordinal_evidence_site): root_h = sqrt(h) and
// corr = var h' (h' = dh / df; var NULL: no corr) on the observed nodes with h >= h_floor, 0 elsewhere.  h as above (Bernoulli:
// the binomial with one trial); h' = mu (Poisson), h (1 - 2 pi) (binomial kind), -(a_u (sigma(-u) - sigma(u)) + a_l (sigma(-l) -
// sigma(l))) with a_x = sigma(x) sigma(-x) (ordinal), the differences formed as -+(1 - e) / (1 + e) from e = exp(-|x|).
//
// mgp_nb_dispersion_sums runs the same loop with another node (DispersionNode: nothing is stored, a second float64 array u is
// read beside var): the three rows of d log Z / dr of a negative-binomial fit, r its dispersion (docs/kernels/counts.md,
// "Learning the dispersion"), in the slots lp, fq and sq:
//   row 0 = sum_obs psi(y + r) - psi(r) + log(1 - pi) + pi - y (1 - pi) / r,  log(1 - pi) = -softplus(z),
//   row 1 = -1/2 sum_eff var (pi (1 - pi) - h' / r),   row 2 = -1/2 sum_eff u (h / r - pi),   eff: observed and h >= h_floor;
// psi(y + r) - psi(r) from positive terms no larger than itself (psi_diff).
//
// The other kernels:
//   mgp_softmax_site: the Newton stage of a C-class fit.  F, Q2 F, pi and rhs are row-major [n, C]; a group of TC lanes owns a row
//     (softmax_rows.h).  Per row: m = max_c f_c, e_c = exp(f_c - m), Z = sum e_c (xor trees inside the group), pi_c = e_c / Z,
//     log p = f_t - m - log Z; G = onehot(t) - pi on observed rows (G_t = sum_{c != t} e_c / Z, a second xor tree: 1 - pi_t cancels
//     where pi_t -> 1), 0 elsewhere, rhs = G - qf.  The label is only compared with the lane's class, never used as an index.
//     The four sums leave as above.
//   mgp_bernoulli_predict: p_i = sum_k D phi(u_k) sigma(m_i + sqrt(v_i) u_k), u_k = -8 + k D, D = 16 / (K - 1): the K-point
//     trapezoid rule on [-8, 8].  The workgroup fills (u_k, D phi(u_k)) in LDS once (trapezoid_table); a thread per node sums k in
//     ascending order.
//   mgp_ordinal_predict: out_ik = int P(y = k | f) N(f; eta_i, var_i) df for the K ordered categories by the same rule, the
//     integrand in the product form (every term positive: a tail category keeps its relative accuracy), the sum divided by the
//     sum of the weights (rows sum to 1).  A group of TK lanes per node, lane k its category: one exp per lane and point, the
//     lower cut's factor from lane k - 1 by a shuffle.
//   mgp_ordinal_cut_sums: the three rows of d log Z / d b_k for the K - 1 cutpoints (likelihood, curvature at fixed f, through the
//     mode), a per-cutpoint float64 reduction over the nodes: a node of category c adds to its upper cut b_{c+1} and to its lower
//     cut b_c.  A workgroup stages a step's contributions in LDS and one lane per (row, cut) adds them in node order; one partial
//     [3, K - 1] per workgroup, a second launch adds the partials in workgroup order.  No atomics, no shuffles.
//   mgp_scale_rows: out = s_i V_ij or fmaf(s_i, X_ij, V_ij) on row-major [n, P] blocks: the two row scalings around the solve in a
//     product with B = I + S Q2^-1 S.  Bandwidth-trivial and launch-bound at 60k nodes.
//   mgp_softmax_root_apply: the factor R of the softmax Hessian, R_i = diag(s_i)(I - s_i s_i^T) with s_i = sqrt(pi_i), so that
//     R_i R_i^T = H_i: out = R V or out = V + R^T X on S vectors of [n, C] in either order of class and sample inside a row (the
//     strides are arguments), a row per (node, sample).  The two launches around the solve in a product with
//     B = I + R^T (Q2^-1 (x) I) R (docs/kernels/evidence.md, "The softmax family").
//   mgp_softmax_curvature: g_ic = tr(V_i dH_i / df_ic) of the same evidence as an expectation over latent deviations, accumulated
//     block by block in float64 with its sum of squares: a group per node adds its S samples in order, one writer per entry.
#include <cfloat>
#include <cmath>
#include <utility>

#include "mgp_common.h"
#include "mgp_internal.h"
#include "site_formulas.h"
#include "softmax_rows.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MGP_WAVE;
constexpr int kSiteMaxBlocks = 1024;      // grid cap of the site kernels: 1024 x 256 threads x 4 nodes per step (the node loop),
                                          // 1024 x 256 / TC rows per step (softmax)
constexpr int kPredictMaxBlocks = 2048;   // grid cap of the predict kernel: 2048 x 256 threads x 1 node per step
constexpr int kMaxPoints = 1025;

struct SiteAcc {
  double lp, fq, mx, sq;
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// the workgroup's four numbers from its threads': xor tree over each wave, the waves in order.  Valid in thread 0.
__device__ __forceinline__ SiteAcc block_reduce(SiteAcc a) {
  __shared__ double s_part[kWaves][4];
  const int lane = threadIdx.x & (MGP_WAVE - 1), wave = threadIdx.x / MGP_WAVE;
  a.lp = mgp_wave_sum_d(a.lp);
  a.fq = mgp_wave_sum_d(a.fq);
  a.mx = wave_max_d(a.mx);
  a.sq = mgp_wave_sum_d(a.sq);
  if (lane == 0) {
    s_part[wave][0] = a.lp;
    s_part[wave][1] = a.fq;
    s_part[wave][2] = a.mx;
    s_part[wave][3] = a.sq;
  }
  __syncthreads();
  SiteAcc r = {s_part[0][0], s_part[0][1], s_part[0][2], s_part[0][3]};
  for (int k = 1; k < kWaves; ++k) {
    r.lp += s_part[k][0];
    r.fq += s_part[k][1];
    r.mx = s_part[k][2] > r.mx ? s_part[k][2] : r.mx;
    r.sq += s_part[k][3];
  }
  return r;
}

// the workgroup's partial {lp, fq, mx, sq} from its threads' sums; every thread of the workgroup calls it
__device__ __forceinline__ void store_partials(const SiteAcc& acc, double* __restrict__ partials) {
  const SiteAcc r = block_reduce(acc);
  if (threadIdx.x == 0) {
    double* p = partials + 4 * (int64_t)blockIdx.x;
    p[0] = r.lp;
    p[1] = r.fq;
    p[2] = r.mx;
    p[3] = r.sq;
  }
}

// sums[4] from the partials of `nblk` workgroups: thread t takes partials t, t + 256, ... in order, then the same tree.
// sum_first: the sum slot leaves before the max slot (the evidence stage: { .., sum corr, max |corr| }); nout < 4: only the
// first nout slots leave (mgp_nb_dispersion_sums: three sums, sums has three entries)
__global__ __launch_bounds__(kBlock) void site_sum_kernel(const double* __restrict__ partials, int nblk,
                                                          double* __restrict__ sums, bool sum_first = false, int nout = 4) {
  SiteAcc acc = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += kBlock) {
    const double* p = partials + 4 * (int64_t)b;
    acc.lp += p[0];
    acc.fq += p[1];
    acc.mx = p[2] > acc.mx ? p[2] : acc.mx;
    acc.sq += p[3];
  }
  const SiteAcc r = block_reduce(acc);
  if (threadIdx.x == 0) {
    sums[0] = r.lp;
    sums[1] = r.fq;
    sums[2] = sum_first ? r.sq : r.mx;
    if (nout > 3) sums[3] = sum_first ? r.mx : r.sq;
  }
}

// a float64 result as float32, +-FLT_MAX where the cast would leave as inf (NaN stays NaN)
__device__ __forceinline__ float sat_f32(double v) {
  const double m = (double)FLT_MAX;
  return (float)(v > m ? m : (v < -m ? -m : v));
}

// ---- Newton stage.  A family: its scalars, kReadsB (it reads the second array) and operator(): one node, observed or not --
// log p into acc.lp, g and h (site_formulas.h, shared with spectral_laplace.hip), then site_tail.

// w, rhs and the three sums of a node from its g and h (0 at an unobserved node).  SATURATE: the counts, whose h is unbounded
template <bool SATURATE>
__device__ __forceinline__ void site_tail(double s_ref, double f, double qf, double g, double h, float& w, float& rhs,
                                          SiteAcc& acc) {
  const double r = g - qf;
  w = SATURATE ? sat_f32(s_ref * h) : (float)(s_ref * h);
  rhs = SATURATE ? sat_f32(s_ref * r) : (float)(s_ref * r);
  acc.fq += f * qf;
  const double ar = fabs(r);
  acc.mx = ar > acc.mx ? ar : acc.mx;
  acc.sq += r * r;
}

struct BernoulliSite {
  static constexpr bool kReadsB = false;
  double s_ref;
  __device__ __forceinline__ void operator()(float f32, float qf32, float y32, float, bool obs, float& w, float& rhs,
                                             SiteAcc& acc) const {
    const double f = (double)f32;
    double g = 0.0, h = 0.0;
    if (obs) {
      double lp;
      mgp_bernoulli_lgh(f, y32, lp, g, h);
      acc.lp += lp;
    }
    site_tail<false>(s_ref, f, (double)qf32, g, h, w, rhs, acc);
  }
};

// FAMILY 0: Poisson, a32 the log-exposure; FAMILY 1: binomial, a32 the trials; FAMILY 2: negative binomial with the dispersion
// r_nb (log_r = log r), a32 the log-exposure (mgp_count_lgh)
template <int FAMILY>
struct CountSite {
  static constexpr bool kReadsB = true;
  double s_ref, mean, r_nb, log_r;
  __device__ __forceinline__ void operator()(float f32, float qf32, float y32, float a32, bool obs, float& w, float& rhs,
                                             SiteAcc& acc) const {
    const double f = (double)f32;
    double g = 0.0, h = 0.0;
    if (obs) {
      double lp;
      mgp_count_lgh<FAMILY>(f, mean, r_nb, log_r, y32, a32, lp, g, h);
      acc.lp += lp;
    }
    site_tail<true>(s_ref, f, (double)qf32, g, h, w, rhs, acc);
  }
};

// the category is the interval (lo32, hi32] of cutpoints, -inf / +inf at the end categories (mgp_ordinal_lgh)
struct OrdinalSite {
  static constexpr bool kReadsB = true;
  double s_ref;
  __device__ __forceinline__ void operator()(float f32, float qf32, float lo32, float hi32, bool obs, float& w, float& rhs,
                                             SiteAcc& acc) const {
    const double f = (double)f32;
    double g = 0.0, h = 0.0;
    if (obs) {
      double lp;
      mgp_ordinal_lgh(f, lo32, hi32, lp, g, h);
      acc.lp += lp;
    }
    site_tail<false>(s_ref, f, (double)qf32, g, h, w, rhs, acc);
  }
};

template <bool VEC4, typename Family>
__global__ __launch_bounds__(kBlock) void site_kernel(const float* __restrict__ f, const float* __restrict__ qf,
                                                      const float* __restrict__ a, const float* __restrict__ b,
                                                      const uint8_t* __restrict__ obs, int64_t n, Family fam,
                                                      float* __restrict__ w, float* __restrict__ rhs,
                                                      double* __restrict__ partials) {
  SiteAcc acc = {0.0, 0.0, 0.0, 0.0};
  const int64_t nq = (n + 3) >> 2;                                     // quads of nodes, the last one may be short
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q << 2;
    if (VEC4 && i0 + 4 <= n) {
      const float4 fv = *reinterpret_cast<const float4*>(f + i0);
      const float4 qv = qf ? *reinterpret_cast<const float4*>(qf + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
      const uchar4 ov = obs ? *reinterpret_cast<const uchar4*>(obs + i0) : make_uchar4(1, 1, 1, 1);
      // a and b are read where a node of the quad is observed (they may be NaN elsewhere: never compared).  The zeros are written
      // out at each use: with one named float4 the compiler splits these float4 loads into four dependent dword loads
      const bool any = ov.x | ov.y | ov.z | ov.w;
      const float4 av = any ? *reinterpret_cast<const float4*>(a + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 bv =
          (Family::kReadsB && any && b) ? *reinterpret_cast<const float4*>(b + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 wv, rv;
      fam(fv.x, qv.x, av.x, bv.x, ov.x != 0, wv.x, rv.x, acc);
      fam(fv.y, qv.y, av.y, bv.y, ov.y != 0, wv.y, rv.y, acc);
      fam(fv.z, qv.z, av.z, bv.z, ov.z != 0, wv.z, rv.z, acc);
      fam(fv.w, qv.w, av.w, bv.w, ov.w != 0, wv.w, rv.w, acc);
      *reinterpret_cast<float4*>(w + i0) = wv;
      *reinterpret_cast<float4*>(rhs + i0) = rv;
    } else {
      const int64_t i1 = i0 + 4 < n ? i0 + 4 : n;
      for (int64_t i = i0; i < i1; ++i) {
        const bool o = obs ? obs[i] != 0 : true;
        float wi, ri;
        fam(f[i], qf ? qf[i] : 0.f, o ? a[i] : 0.f, (Family::kReadsB && o && b) ? b[i] : 0.f, o, wi, ri, acc);
        w[i] = wi;
        rhs[i] = ri;
      }
    }
  }
  store_partials(acc, partials);
}

// (u_k, D phi(u_k)), k < K, of the K-point trapezoid rule on [-8, 8] in the workgroup's LDS, ready after the call
__device__ __forceinline__ void trapezoid_table(int K, double* s_u, double* s_wt) {
  const double step = 16.0 / (double)(K - 1);
  for (int k = threadIdx.x; k < K; k += kBlock) {
    const double u = -8.0 + (double)k * step;
    s_u[k] = u;
    s_wt[k] = step * (0.3989422804014327 * exp(-0.5 * u * u));        // D phi(u_k), 1 / sqrt(2 pi)
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void bernoulli_predict_kernel(const float* __restrict__ mean,
                                                                   const double* __restrict__ var, int64_t n, int K,
                                                                   double* __restrict__ prob) {
  __shared__ double s_u[kMaxPoints];
  __shared__ double s_wt[kMaxPoints];
  trapezoid_table(K, s_u, s_wt);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const double m = (double)mean[i];
    const double v = var[i];
    const double sd = sqrt(v < 0.0 ? 0.0 : v);                         // (a NaN variance stays NaN)
    double p = 0.0;
    for (int k = 0; k < K; ++k) {
      const double x = m + sd * s_u[k];
      const double e = exp(-fabs(x));
      p += s_wt[k] * (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
    }
    prob[i] = p > 1.0 ? 1.0 : p;                                       // the weights sum to 1 up to rounding
  }
}

constexpr double kOrdinalVMin = 0x1p-76;  // below it the rule and the plain probability at eta agree to 2^-77 relative

// sigma(up - f) sigma(f - b_k) of lane k's category at the latent value f: the lane forms e = exp(-|up - f|) once, keeps
// sigma(up - f) and hands sigma(f - up), the lower factor of category k + 1, to the next lane of its group.  up = +inf (the last
// category, idle lanes) gives the factor 1; lane 0 has no lower cut.  Every lane of the wave calls it.
template <int TK>
__device__ __forceinline__ double ordinal_term(double up, double f, int k) {
  const double x = up - f;
  const double e = exp(-fabs(x));
  const double d = 1.0 + e;
  const double below = x >= 0.0 ? 1.0 / d : e / d;                     // sigma(up - f)
  const double above = x >= 0.0 ? e / d : 1.0 / d;                     // sigma(f - up)
  const double lower = __shfl_up(above, 1, TK);
  return k == 0 ? below : below * lower;
}

// a group of TK lanes per node, lane k its category (softmax_rows.h)
template <int TK>
__global__ __launch_bounds__(kBlock) void ordinal_predict_kernel(const double* __restrict__ eta, const double* __restrict__ var,
                                                                 const double* __restrict__ cuts, int64_t n, int K, int points,
                                                                 int log_out, double* __restrict__ out) {
  __shared__ double s_u[kMaxPoints];
  __shared__ double s_wt[kMaxPoints];
  trapezoid_table(points, s_u, s_wt);
  double total = 0.0;                                                  // the sum of the weights, j ascending
  for (int j = 0; j < points; ++j) total += s_wt[j];
  constexpr int kRows = kBlock / TK;                                   // nodes a workgroup takes per step
  const int k = threadIdx.x & (TK - 1), g = threadIdx.x / TK;
  const double up = k < K - 1 ? cuts[k] : INFINITY;
  const double c = (k >= 1 && k < K - 1) ? -expm1(-(up - cuts[k - 1])) : 1.0;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  const int64_t steps = (n + stride - 1) / stride;                     // the same for every lane: the shuffles stay convergent
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t i = s * stride + (int64_t)blockIdx.x * kRows + g;
    const bool node = i < n;
    const double m = node ? eta[i] : 0.0;
    const double v = node ? var[i] : 0.0;
    const bool plain = v <= kOrdinalVMin;                              // (a NaN variance is not: sqrt keeps it)
    const double sd = plain ? 0.0 : sqrt(v);
    double p = 0.0;
    for (int j = 0; j < points; ++j) p += s_wt[j] * ordinal_term<TK>(up, m + sd * s_u[j], k);
    const double at_eta = ordinal_term<TK>(up, m, k);
    if (!node || k >= K) continue;                                     // (after the group's shuffles)
    const double r = c * (plain ? at_eta : p / total);
    out[i * (int64_t)K + k] = log_out ? log(r) : r;
  }
}

// ---- Evidence stage.  A family: its scalars, kReadsB, kSaturate (sqrt(h) may leave the float32 range) and
// operator()(f, a, b, h, hp): h and h' = dh / df of one observed node at the mode, its log p returned.

// FAMILY 0: Poisson (a32 the log-exposure), 1: binomial (a32 the trials), 2: Bernoulli-logit (one trial, y the label), 3: negative
// binomial (a32 the log-exposure, r_nb the dispersion, log_r its log: y + r trials and r failures at z = f + mean + a - log r, as
// CountSite)
template <int FAMILY>
struct CountEvidence {
  static constexpr bool kReadsB = FAMILY != 2, kSaturate = true;
  double mean, r_nb, log_r;
  __device__ __forceinline__ double operator()(double f, float y32, float a32, double& h, double& hp) const {
    if (FAMILY == 0) {
      const double y = (double)y32;
      const double eta = f + mean + (double)a32;
      const double mu = exp(eta < 700.0 ? eta : 700.0);
      h = mu;
      hp = mu;
      return y * eta - mu;
    }
    const double eta = FAMILY == 3 ? f + mean + (double)a32 - log_r : f + mean;
    const double y = FAMILY == 2 ? (y32 > 0.5f ? 1.0 : 0.0) : (double)y32;
    const double N = FAMILY == 1 ? (double)a32 : (FAMILY == 3 ? y + r_nb : 1.0);
    const double m = FAMILY == 3 ? r_nb : N - y;
    const double e = exp(-fabs(eta));
    const double d = 1.0 + e;
    const double l1 = log1p(e);
    h = N * e / (d * d);
    const double gap = -expm1(-fabs(eta)) / d;                         // |(1 - pi) - pi| = (1 - e) / (1 + e), no cancellation
    hp = h * (eta >= 0.0 ? -gap : gap);
    return -m * ((eta > 0.0 ? eta : 0.0) + l1) - y * ((eta < 0.0 ? -eta : 0.0) + l1);
  }
};

// sigma(x), sigma(-x), a = sigma(x) sigma(-x) and gap = sigma(-x) - sigma(x) = -+ (1 - e) / (1 + e) from one e = exp(-|x|): the gap
// as CountEvidence forms (1 - pi) - pi, no cancellation near 0.  x = +-inf: e = 0, a = 0, gap = -+1, every product with a is 0
struct OrdinalEnd {
  double e, sig, sigm, a, gap;
};

__device__ __forceinline__ OrdinalEnd ordinal_end(double x) {
  const double ax = fabs(x);
  const double e = exp(-ax);
  const double d = 1.0 + e;
  const double big = 1.0 / d, small = e / d;
  const double gap = -expm1(-ax) / d;
  OrdinalEnd r;
  r.e = e;
  r.sig = x >= 0.0 ? big : small;
  r.sigm = x >= 0.0 ? small : big;
  r.a = e / (d * d);
  r.gap = x >= 0.0 ? -gap : gap;
  return r;
}

// the interval of OrdinalSite, h' = -(a_u gap_u + a_l gap_l)
struct OrdinalEvidence {
  static constexpr bool kReadsB = true, kSaturate = false;                             // h <= 1/2
  __device__ __forceinline__ double operator()(double f, float lo32, float hi32, double& h, double& hp) const {
    const double u = (double)hi32 - f, l = (double)lo32 - f;
    const OrdinalEnd eu = ordinal_end(u), el = ordinal_end(l);
    h = eu.a + el.a;
    hp = -(eu.a * eu.gap + el.a * el.gap);
    return -((u < 0.0 ? -u : 0.0) + log1p(eu.e)) - ((l > 0.0 ? l : 0.0) + log1p(el.e));   // log p as OrdinalSite forms it
  }
};

// root and corr of an observed node from its h and h'; acc: fq = nodes kept, sq = sum corr, mx = max |corr|
template <bool SATURATE>
__device__ __forceinline__ void evidence_tail(double h, double hp, double var, bool has_var, double h_floor, float& root,
                                              float& corr, SiteAcc& acc) {
  if (!(h >= h_floor)) return;
  acc.fq += 1.0;
  root = SATURATE ? sat_f32(sqrt(h)) : (float)sqrt(h);
  if (has_var) {
    const double m = (double)FLT_MAX;
    double c = var * hp;
    c = c > m ? m : (c < -m ? -m : c);
    corr = (float)c;
    acc.sq += c;
    const double ac = fabs(c);
    acc.mx = ac > acc.mx ? ac : acc.mx;
  }
}

// A node of the evidence stage's loop: kReadsB (it reads the second array), kReadsU (the second float64 array), kWrites (root_h
// and corr leave) and operator(): one node, observed or not; var and u are 0 where they are not read.
template <typename Family>
struct EvidenceNode {
  static constexpr bool kReadsB = Family::kReadsB, kReadsU = false, kWrites = true;
  Family fam;
  double h_floor;
  __device__ __forceinline__ void operator()(float f32, float a32, float b32, bool obs, double var, double, bool has_var, bool,
                                             float& root, float& corr, SiteAcc& acc) const {
    root = 0.f;
    corr = 0.f;
    if (!obs) return;
    double h, hp;
    acc.lp += fam((double)f32, a32, b32, h, hp);
    evidence_tail<Family::kSaturate>(h, hp, var, has_var, h_floor, root, corr, acc);
  }
};

constexpr int kPsiLift = 32;              // psi_diff: the sum of reciprocals up to here, the asymptotic series at arguments from here

// psi(x) - (log x - 1 / (2 x)) = -(1/12 x^-2 - 1/120 x^-4 + 1/252 x^-6 - 1/240 x^-8 + 1/132 x^-10 - 691/32760 x^-12) for x >= 32
// (the next term is below 2^-67), returned with the sign turned: t(x) > 0, decreasing
__device__ __forceinline__ double psi_tail(double x) {
  const double x2 = 1.0 / (x * x);
  return x2 * (1.0 / 12 - x2 * (1.0 / 120 - x2 * (1.0 / 252 - x2 * (1.0 / 240 - x2 * (1.0 / 132 - x2 * (691.0 / 32760))))));
}

// sum_{j < 32} 1 / (r + j), j ascending: the recurrence that lifts psi(r) to psi(r + 32).  It depends on r alone: the entry point
// forms it once on the host, in the arithmetic of the device (correctly rounded divisions and sums, no contraction)
inline double psi_lift(double r) {
  double s = 0.0;
  for (int j = 0; j < kPsiLift; ++j) s += 1.0 / (r + (double)j);
  return s;
}

// psi(y + r) - psi(r) for a count y (an integer 0 .. 2^24) and r in [2^-10, 2^20], every term positive and no larger than the
// result: y <= 32: sum_{j < y} 1 / (r + j), j ascending.  Beyond it, with k = 32 for r < 32 and 0 otherwise, b = r + k, a = y + r:
//   sum_{j < k} 1 / (r + j)  +  log1p((y - k) / b)  +  (y - k) / (2 a b)  +  (t(b) - t(a))
// (the recurrence psi(r) = psi(r + k) - sum_{j < k} 1 / (r + j), then psi(a) - psi(b) from the asymptotic series with the
// logarithms as one log1p of the ratio and the 1 / (2 x) terms as one quotient).  lift: psi_lift(r) for r < 32, 0 otherwise.
// y = 0 gives exactly 0.
__device__ __forceinline__ double psi_diff(double y, double r, double lift) {
  if (y <= (double)kPsiLift) {
    double s = 0.0;
    for (int j = 0; j < kPsiLift && (double)j < y; ++j) s += 1.0 / (r + (double)j);
    return s;
  }
  const bool lifted = r < (double)kPsiLift;
  const double b = lifted ? r + (double)kPsiLift : r;
  const double d = lifted ? y - (double)kPsiLift : y;
  const double a = y + r;
  return lift + log1p(d / b) + d / (2.0 * a * b) + (psi_tail(b) - psi_tail(a));
}

// The integrands of d log Z / dr of a negative-binomial fit at the mode (mgp_nb_dispersion_sums): acc.lp the likelihood's term
// on every observed node, acc.fq the curvature's at fixed f and acc.sq the one through the mode on the nodes with h >= h_floor.
// z, pi, 1 - pi, h and h' as CountEvidence<3> forms them.
struct DispersionNode {
  static constexpr bool kReadsB = true, kReadsU = true, kWrites = false;
  double mean, r_nb, log_r, lift, h_floor;
  __device__ __forceinline__ void operator()(float f32, float y32, float a32, bool obs, double var, double u, bool has_var,
                                             bool has_u, float&, float&, SiteAcc& acc) const {
    if (!obs) return;
    const double y = (double)y32;
    const double z = (double)f32 + mean + (double)a32 - log_r;
    const double az = fabs(z);
    const double e = exp(-az);
    const double d = 1.0 + e;
    const double pi = z >= 0.0 ? 1.0 / d : e / d;
    const double pib = z >= 0.0 ? e / d : 1.0 / d;                     // 1 - pi without the subtraction
    const double softplus = (z > 0.0 ? z : 0.0) + log1p(e);            // -log(1 - pi)
    acc.lp += ((psi_diff(y, r_nb, lift) - softplus) + pi) - y * pib / r_nb;
    const double pq = e / (d * d);                                     // pi (1 - pi)
    const double h = (y + r_nb) * pq;
    if (!(h >= h_floor)) return;
    const double gap = -expm1(-az) / d;
    const double hp = h * (z >= 0.0 ? -gap : gap);
    if (has_var) acc.fq += -0.5 * (var * (pq - hp / r_nb));
    if (has_u) acc.sq += -0.5 * (u * (h / r_nb - pi));
  }
};

// the node loop of site_kernel; var (NULL: no corr) and u (read by a node with kReadsU only) are float64, two double2 per quad
// on the vector path
template <bool VEC4, typename Node>
__global__ __launch_bounds__(kBlock) void evidence_kernel(const float* __restrict__ f, const float* __restrict__ a,
                                                          const float* __restrict__ b, const uint8_t* __restrict__ obs,
                                                          const double* __restrict__ var, const double* __restrict__ usol,
                                                          int64_t n, Node node, float* __restrict__ root_h,
                                                          float* __restrict__ corr, double* __restrict__ partials) {
  SiteAcc acc = {0.0, 0.0, 0.0, 0.0};
  const bool has_var = var != nullptr;
  const bool has_u = Node::kReadsU && usol != nullptr;
  const int64_t nq = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
    const int64_t i0 = q << 2;
    if (VEC4 && i0 + 4 <= n) {
      const float4 fv = *reinterpret_cast<const float4*>(f + i0);
      const uchar4 ov = obs ? *reinterpret_cast<const uchar4*>(obs + i0) : make_uchar4(1, 1, 1, 1);
      const bool any = ov.x | ov.y | ov.z | ov.w;
      const float4 av = any ? *reinterpret_cast<const float4*>(a + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 bv =
          (Node::kReadsB && any && b) ? *reinterpret_cast<const float4*>(b + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
      double2 v0 = make_double2(0.0, 0.0), v1 = v0, u0 = v0, u1 = v0;
      if (has_var && any) {
        v0 = *reinterpret_cast<const double2*>(var + i0);
        v1 = *reinterpret_cast<const double2*>(var + i0 + 2);
      }
      if (has_u && any) {
        u0 = *reinterpret_cast<const double2*>(usol + i0);
        u1 = *reinterpret_cast<const double2*>(usol + i0 + 2);
      }
      float4 rv, cv;
      node(fv.x, av.x, bv.x, ov.x != 0, v0.x, u0.x, has_var, has_u, rv.x, cv.x, acc);
      node(fv.y, av.y, bv.y, ov.y != 0, v0.y, u0.y, has_var, has_u, rv.y, cv.y, acc);
      node(fv.z, av.z, bv.z, ov.z != 0, v1.x, u1.x, has_var, has_u, rv.z, cv.z, acc);
      node(fv.w, av.w, bv.w, ov.w != 0, v1.y, u1.y, has_var, has_u, rv.w, cv.w, acc);
      if (Node::kWrites) {
        *reinterpret_cast<float4*>(root_h + i0) = rv;
        if (has_var) *reinterpret_cast<float4*>(corr + i0) = cv;
      }
    } else {
      const int64_t i1 = i0 + 4 < n ? i0 + 4 : n;
      for (int64_t i = i0; i < i1; ++i) {
        const bool o = obs ? obs[i] != 0 : true;
        float ri, ci;
        node(f[i], o ? a[i] : 0.f, (Node::kReadsB && o && b) ? b[i] : 0.f, o, (o && has_var) ? var[i] : 0.0,
             (o && has_u) ? usol[i] : 0.0, has_var, has_u, ri, ci, acc);
        if (Node::kWrites) {
          root_h[i] = ri;
          if (has_var) corr[i] = ci;
        }
      }
    }
  }
  store_partials(acc, partials);
}

constexpr int kCutMaxBlocks = 1024;       // grid cap of mgp_ordinal_cut_sums: 1024 x 256 threads x 1 node per step
constexpr int kCutRows = 3;               // likelihood, curvature, through the mode

// The three rows of d log Z / d b_k, k = 1 .. K - 1, as one partial [3, K - 1] per workgroup.  A step: thread t stages the six
// contributions of its node in LDS -- three to its upper cut b_{c+1} and three to its lower cut b_c -- with its category c (-1: no
// contribution), then lane t < 3 (K - 1), the owner of (row, cut) = (t / (K - 1), 1 + t % (K - 1)), scans the 256 staged nodes in
// thread order (every lane reads the same address: a broadcast) and adds the ones that touch its cut.  The sum of a (row, cut) is
// therefore taken in node order inside the workgroup's stripe, by one lane: no shuffles, no atomics, the same trip count for
// every thread (the barriers stay convergent).
__global__ __launch_bounds__(kBlock) void ordinal_cut_sums_kernel(const float* __restrict__ f, const float* __restrict__ lo,
                                                                  const float* __restrict__ hi, const uint8_t* __restrict__ cat,
                                                                  const uint8_t* __restrict__ obs, const double* __restrict__ var,
                                                                  const double* __restrict__ usol, int64_t n, int K, double h_floor,
                                                                  double* __restrict__ partials) {
  __shared__ double s_val[kBlock][2 * kCutRows];
  __shared__ int s_cat[kBlock];
  const int cuts = K - 1;
  const int t = threadIdx.x;
  const bool owner = t < kCutRows * cuts;
  const int row = owner ? t / cuts : 0;
  const int cut = owner ? 1 + t % cuts : 0;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t steps = (n + stride - 1) / stride;                     // the same for every thread of the grid
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t i = s * stride + (int64_t)blockIdx.x * kBlock + t;
    int c = -1;
    double up0 = 0.0, up1 = 0.0, up2 = 0.0, dn0 = 0.0, dn1 = 0.0, dn2 = 0.0;
    if (i < n && (obs ? obs[i] != 0 : true)) {
      const int ci = (int)cat[i];
      if (ci < K) {                                                    // compared before it selects a cut: no table is indexed
        c = ci;
        const double fi = (double)f[i];
        const double lo_i = (double)lo[i], hi_i = (double)hi[i];
        const OrdinalEnd eu = ordinal_end(hi_i - fi), el = ordinal_end(lo_i - fi);
        const double width = 1.0 / expm1(hi_i - lo_i);                 // 0 at an infinite end
        up0 = eu.sigm + width;
        dn0 = -(el.sig + width);
        if (eu.a + el.a >= h_floor) {
          if (var) {
            const double v = var[i];
            up1 = -0.5 * (v * (eu.a * eu.gap));
            dn1 = -0.5 * (v * (el.a * el.gap));
          }
          if (usol) {
            const double ui = usol[i];
            up2 = -0.5 * (ui * eu.a);
            dn2 = -0.5 * (ui * el.a);
          }
        }
      }
    }
    s_cat[t] = c;
    s_val[t][0] = up0;
    s_val[t][1] = up1;
    s_val[t][2] = up2;
    s_val[t][3] = dn0;
    s_val[t][4] = dn1;
    s_val[t][5] = dn2;
    __syncthreads();
    if (owner) {
      // both candidates are read whatever the category, so the reads of the next nodes do not wait for a branch; a node that does
      // not touch the cut adds 0.0, which changes nothing
#pragma unroll 8
      for (int j = 0; j < kBlock; ++j) {
        const int cj = s_cat[j];
        const double up = s_val[j][row], dn = s_val[j][kCutRows + row];    // the node's upper cut, its lower cut
        acc += cj == cut - 1 ? up : (cj == cut ? dn : 0.0);
      }
    }
    __syncthreads();
  }
  if (owner) partials[(int64_t)blockIdx.x * (kCutRows * cuts) + t] = acc;
}

// out [3, K - 1] from the partials of `nblk` workgroups: lane t adds its entry over the workgroups in order
__global__ __launch_bounds__(kBlock) void ordinal_cut_sums_add_kernel(const double* __restrict__ partials, int nblk, int entries,
                                                                      double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= entries) return;
  double acc = 0.0;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) acc += partials[(int64_t)b * entries + t];          // (the loads run ahead, the adds stay in order)
  out[t] = acc;
}

constexpr int kScaleMaxBlocks = 2048;     // grid cap of mgp_scale_rows: 2048 x 256 threads x 4 (or 1) entries per step

// out = s_i V_ij, or fmaf(s_i, X_ij, V_ij): one entry (or one float4 inside a row, P % 4 == 0) per thread and step.  out may be
// V or X: an entry is read before it is written, by the same thread.
template <bool VEC4>
__global__ __launch_bounds__(kBlock) void scale_rows_kernel(const float* __restrict__ s, const float* V, const float* X,
                                                            int64_t n, int P, float* out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t start = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (VEC4) {
    const int P4 = P >> 2;
    const int64_t total = n * P4;
    for (int64_t q = start; q < total; q += stride) {
      const float si = s[q / P4];
      const float4 v = reinterpret_cast<const float4*>(V)[q];
      float4 o;
      if (X) {
        const float4 x = reinterpret_cast<const float4*>(X)[q];
        o = make_float4(fmaf(si, x.x, v.x), fmaf(si, x.y, v.y), fmaf(si, x.z, v.z), fmaf(si, x.w, v.w));
      } else {
        o = make_float4(si * v.x, si * v.y, si * v.z, si * v.w);
      }
      reinterpret_cast<float4*>(out)[q] = o;
    }
  } else {
    const int64_t total = n * P;
    for (int64_t e = start; e < total; e += stride) {
      const float si = s[e / P];
      const float v = V[e];
      out[e] = X ? fmaf(si, X[e], v) : si * v;
    }
  }
}

template <int TC>
__global__ __launch_bounds__(kBlock) void softmax_site_kernel(const float* __restrict__ f, const float* __restrict__ qf,
                                                              const int32_t* __restrict__ labels,
                                                              const uint8_t* __restrict__ obs, int64_t n, int C,
                                                              float* __restrict__ pi, float* __restrict__ rhs,
                                                              double* __restrict__ partials) {
  constexpr int kRows = kBlock / TC;                                   // rows a workgroup takes per step
  SiteAcc acc = {0.0, 0.0, 0.0, 0.0};
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  const int64_t steps = (n + stride - 1) / stride;                           // the same for every lane: the shuffles stay convergent
  for (int64_t k = 0; k < steps; ++k) {
    const int64_t i = k * stride + (int64_t)blockIdx.x * kRows + g;
    const bool live = i < n && c < C;
    const int64_t at = i * C + c;
    const bool o = live && (obs ? obs[i] != 0 : true);
    const bool mine = o && labels[i] == c;                             // compared, never an index
    const double fv = live ? (double)f[at] : -INFINITY;
    const double m = mgp_group_max_d<TC>(fv);
    const double e = live ? exp(fv - m) : 0.0;
    const double Z = mgp_group_sum_d<TC>(e);
    const double rest = mgp_group_sum_d<TC>(mine ? 0.0 : e);               // Z without the label's term
    if (!live) continue;                                               // (after the group's shuffles)
    const double q = qf ? (double)qf[at] : 0.0;
    double p = 0.0, gr = 0.0;
    if (o) {
      p = e / Z;
      gr = mine ? rest / Z : -p;                                       // 1 - pi_t = rest / Z: no cancellation where pi_t -> 1
      if (mine) acc.lp += fv - m - log(Z);
    }
    const double r = gr - q;
    pi[at] = (float)p;
    rhs[at] = (float)r;
    acc.fq += fv * q;
    const double ar = fabs(r);
    acc.mx = ar > acc.mx ? ar : acc.mx;
    acc.sq += r * r;
  }
  store_partials(acc, partials);
}

// out = R V (forward) or V + R^T X (transposed; V nullable) on S vectors of [n, C]: entry (i, c, s) lies at i C S + c cstride +
// s sstride.  A group of TC lanes owns the row q = i S + s, lane c its class.  sqrt(pi), the row's dot product (an xor tree over
// the group) and the combination in float64, one rounding at the store.  Where pi_ic = 0 the lane's terms are exactly 0 whatever
// V and X hold.  out may be V or X: every lane loads its entry before the group's shuffles and stores after them.
template <int TC>
__global__ __launch_bounds__(kBlock) void softmax_root_kernel(const float* __restrict__ pi, const float* V, const float* X,
                                                              int64_t n, int C, int S, int64_t cstride, int64_t sstride,
                                                              bool transpose, float* out) {
  constexpr int kRows = kBlock / TC;
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t rows = n * S;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  const int64_t steps = (rows + stride - 1) / stride;                   // the same for every lane: the shuffles stay convergent
  for (int64_t k = 0; k < steps; ++k) {
    const int64_t q = k * stride + (int64_t)blockIdx.x * kRows + g;
    const bool live = q < rows && c < C;
    const int64_t i = q / S;
    const int64_t at = i * C * S + c * cstride + (q - i * S) * sstride;
    const double p = live ? (double)pi[i * C + c] : 0.0;
    const bool on = p > 0.0;
    const double root = on ? sqrt(p) : 0.0;
    double r;
    if (!transpose) {
      const double t = on ? root * (double)V[at] : 0.0;
      const double dot = mgp_group_sum_d<TC>(t);
      r = on ? t - p * dot : 0.0;
    } else {
      const double x = on ? (double)X[at] : 0.0;
      const double dot = mgp_group_sum_d<TC>(p * x);
      const double v = (live && V) ? (double)V[at] : 0.0;
      r = on ? v + root * (x - dot) : v;
    }
    if (live) out[at] = (float)r;
  }
}

// acc_ic += sum_s g_s, acc2_ic += sum_s g_s^2 with g_s = pi_c (d_c^2 - sum_a pi_a d_a^2), d = delta_s - (pi . delta_s), over the
// S deviations delta [n, S, C] of a block: a group of TC lanes owns node i for all its samples, which it adds in the order
// s = 0 .. S - 1.  float64 from the float32 inputs; one writer per entry.  A row of zeros in pi is not written.
template <int TC>
__global__ __launch_bounds__(kBlock) void softmax_curvature_kernel(const float* __restrict__ pi, const float* __restrict__ delta,
                                                                   int64_t n, int C, int S, double* __restrict__ acc,
                                                                   double* __restrict__ acc2) {
  constexpr int kRows = kBlock / TC;
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  const int64_t steps = (n + stride - 1) / stride;
  for (int64_t k = 0; k < steps; ++k) {
    const int64_t i = k * stride + (int64_t)blockIdx.x * kRows + g;
    const bool live = i < n && c < C;
    const double p = live ? (double)pi[i * C + c] : 0.0;
    const bool row_on = mgp_group_max_d<TC>(p) > 0.0;                    // (no early exit: the groups of a wave stay in step)
    double sum = 0.0, sum2 = 0.0;
    for (int s = 0; s < S; ++s) {
      const double x = p > 0.0 ? (double)delta[(i * S + s) * C + c] : 0.0;
      const double d = x - mgp_group_sum_d<TC>(p * x);
      const double d2 = d * d;
      const double gs = p * (d2 - mgp_group_sum_d<TC>(p * d2));
      sum += gs;
      sum2 += gs * gs;
    }
    if (live && row_on) {
      acc[i * C + c] += sum;
      acc2[i * C + c] += sum2;
    }
  }
}

// the strides of a dense [C, S] or [S, C] image of a row: positive, no two entries at one offset, every offset below C S
bool root_strides_ok(int C, int S, int64_t cstride, int64_t sstride) {
  if (cstride < 1 || sstride < 1) return false;
  int64_t s1 = cstride, e1 = C, s2 = sstride, e2 = S;
  if (s1 > s2 || (s1 == s2 && e1 < e2)) { std::swap(s1, s2); std::swap(e1, e2); }     // (s1, e1): the inner dimension
  if (e2 > 1 && s2 < s1 * e1) return false;                                            // the outer dimension steps over the inner
  return (e1 - 1) * s1 + (e2 - 1) * s2 < (int64_t)C * S;
}

int softmax_site_blocks(int64_t n, int C) { return mgp_softmax_blocks(n, C, kBlock, kSiteMaxBlocks); }

int site_blocks(int64_t n) {
  const int64_t b = mgp_cdiv((n + 3) >> 2, (int64_t)kBlock);
  return (int)(b > kSiteMaxBlocks ? kSiteMaxBlocks : b);
}

int cut_blocks(int64_t n) {
  const int64_t b = mgp_cdiv(n, (int64_t)kBlock);
  return (int)(b > kCutMaxBlocks ? kCutMaxBlocks : b);
}

// the workspace of the node loop's entry points: one partial per workgroup
size_t site_workspace_bytes(int64_t n) { return n < 1 ? 0 : (size_t)site_blocks(n) * 4 * sizeof(double); }

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the second launch of every site entry point: sums[4] from the partials of `blocks` workgroups
int sum_partials(const double* partials, int blocks, double* sums, bool sum_first, hipStream_t st, int nout = 4) {
  hipLaunchKernelGGL(site_sum_kernel, dim3(1), dim3(kBlock), 0, st, partials, blocks, sums, sum_first, nout);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// The Newton stage of one family on validated arguments: the workspace check, the vector instantiation where every array
// allows it (a NULL pointer does), the sums.
template <typename Family>
int launch_site(const float* f, const float* qf, const float* a, const float* b, const uint8_t* obs, int64_t n, const Family& fam,
                float* w, float* rhs, double* sums, void* work, size_t work_bytes, void* stream) {
  if (!work || !aligned_to(work, 8) || work_bytes < site_workspace_bytes(n)) return MGP_ERR_WORKSPACE;
  const int blocks = site_blocks(n);
  double* partials = static_cast<double*>(work);
  const bool vec4 = aligned_to(f, 16) && aligned_to(qf, 16) && aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(obs, 4) &&
                    aligned_to(w, 16) && aligned_to(rhs, 16);
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t st = mgp_stream(stream);
  if (vec4)
    hipLaunchKernelGGL((site_kernel<true, Family>), grid, block, 0, st, f, qf, a, b, obs, n, fam, w, rhs, partials);
  else
    hipLaunchKernelGGL((site_kernel<false, Family>), grid, block, 0, st, f, qf, a, b, obs, n, fam, w, rhs, partials);
  MGP_LAUNCH_CHECK();
  return sum_partials(partials, blocks, sums, false, st);
}

// The evidence stage's loop over one kind of node, as launch_site: the first nout of { lp, fq, sq, mx } leave in sums.
template <typename Node>
int launch_evidence_nodes(const float* f, const float* a, const float* b, const uint8_t* obs, const double* var, const double* u,
                          int64_t n, const Node& node, float* root_h, float* corr, double* sums, int nout, void* work,
                          size_t work_bytes, void* stream) {
  if (!work || !aligned_to(work, 8) || work_bytes < site_workspace_bytes(n)) return MGP_ERR_WORKSPACE;
  const int blocks = site_blocks(n);
  double* partials = static_cast<double*>(work);
  const bool vec4 = aligned_to(f, 16) && aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(obs, 4) && aligned_to(var, 16) &&
                    aligned_to(u, 16) && aligned_to(root_h, 16) && aligned_to(corr, 16);
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t st = mgp_stream(stream);
  if (vec4)
    hipLaunchKernelGGL((evidence_kernel<true, Node>), grid, block, 0, st, f, a, b, obs, var, u, n, node, root_h, corr, partials);
  else
    hipLaunchKernelGGL((evidence_kernel<false, Node>), grid, block, 0, st, f, a, b, obs, var, u, n, node, root_h, corr, partials);
  MGP_LAUNCH_CHECK();
  return sum_partials(partials, blocks, sums, true, st, nout);
}

// The evidence stage of one family.  corr is written only where var is given too.
template <typename Family>
int launch_evidence(const float* f, const float* a, const float* b, const uint8_t* obs, const double* var, int64_t n,
                    const Family& fam, double h_floor, float* root_h, float* corr, double* sums, void* work, size_t work_bytes,
                    void* stream) {
  if (!var || !corr) var = nullptr, corr = nullptr;
  return launch_evidence_nodes(f, a, b, obs, var, nullptr, n, EvidenceNode<Family>{fam, h_floor}, root_h, corr, sums, 4, work,
                               work_bytes, stream);
}

// the dispersion of the negative-binomial entry points: one finite scalar in [2^-10, 2^20] (NaN fails the comparison)
bool nb_dispersion_ok(double r) { return r >= 0x1p-10 && r <= 0x1p20; }

}  // namespace

extern "C" size_t mgp_bernoulli_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_bernoulli_site(const float* f, const float* qf, const float* y, const uint8_t* obs, int64_t n,
                                  double s_ref, int link, float* w, float* rhs, double* sums, void* work,
                                  size_t work_bytes, void* stream) {
  if (!f || !y || !w || !rhs || !sums || n < 1) return MGP_ERR_ARG;
  if (link != 0) return MGP_ERR_UNSUPPORTED;
  return launch_site(f, qf, y, nullptr, obs, n, BernoulliSite{s_ref}, w, rhs, sums, work, work_bytes, stream);
}

extern "C" size_t mgp_count_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_count_site(const float* f, const float* qf, const float* y, const float* aux, const uint8_t* obs, int64_t n,
                              double s_ref, double mean, int family, float* w, float* rhs, double* sums, void* work,
                              size_t work_bytes, void* stream) {
  if (!f || !y || !w || !rhs || !sums || n < 1) return MGP_ERR_ARG;
  if (family != 0 && family != 1) return MGP_ERR_UNSUPPORTED;
  if (family == 1 && !aux) return MGP_ERR_ARG;                         // the trials have no default
  if (family == 0)
    return launch_site(f, qf, y, aux, obs, n, CountSite<0>{s_ref, mean, 0.0, 0.0}, w, rhs, sums, work, work_bytes, stream);
  return launch_site(f, qf, y, aux, obs, n, CountSite<1>{s_ref, mean, 0.0, 0.0}, w, rhs, sums, work, work_bytes, stream);
}

extern "C" size_t mgp_nb_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_nb_site(const float* f, const float* qf, const float* y, const float* aux, const uint8_t* obs, int64_t n,
                           double s_ref, double mean, double dispersion, float* w, float* rhs, double* sums, void* work,
                           size_t work_bytes, void* stream) {
  if (!f || !y || !w || !rhs || !sums || n < 1 || !nb_dispersion_ok(dispersion)) return MGP_ERR_ARG;
  return launch_site(f, qf, y, aux, obs, n, CountSite<2>{s_ref, mean, dispersion, std::log(dispersion)}, w, rhs, sums, work,
                     work_bytes, stream);
}

extern "C" size_t mgp_ordinal_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_ordinal_site(const float* f, const float* qf, const float* lo, const float* hi, const uint8_t* obs, int64_t n,
                                double s_ref, float* w, float* rhs, double* sums, void* work, size_t work_bytes, void* stream) {
  if (!f || !lo || !hi || !w || !rhs || !sums || n < 1) return MGP_ERR_ARG;
  return launch_site(f, qf, lo, hi, obs, n, OrdinalSite{s_ref}, w, rhs, sums, work, work_bytes, stream);
}

extern "C" int mgp_ordinal_predict(const double* eta, const double* var, const double* cuts, int64_t n, int K, int points,
                                   int log_out, double* out, void* stream) {
  if (!eta || !var || !cuts || !out || n < 1 || K < 2 || K > 64) return MGP_ERR_ARG;
  if (points < 9 || points > kMaxPoints || (points & 1) == 0) return MGP_ERR_ARG;
  const int blocks = mgp_softmax_blocks(n, K, kBlock, kPredictMaxBlocks);
  hipStream_t st = mgp_stream(stream);
  mgp_softmax_dispatch(K, [&](auto tk) {
    hipLaunchKernelGGL(ordinal_predict_kernel<decltype(tk)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, cuts, n,
                       K, points, log_out, out);
  });
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" size_t mgp_laplace_evidence_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_laplace_evidence_site(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var,
                                         int64_t n, double mean, int family, double h_floor, float* root_h, float* corr,
                                         double* sums, void* work, size_t work_bytes, void* stream) {
  if (!f || !y || !root_h || !sums || n < 1 || !(h_floor >= 0.0)) return MGP_ERR_ARG;
  if (family < 0 || family > 2) return MGP_ERR_UNSUPPORTED;
  if (family == 1 && !aux) return MGP_ERR_ARG;                         // the trials have no default
  if (family == 0)
    return launch_evidence(f, y, aux, obs, var, n, CountEvidence<0>{mean, 0.0, 0.0}, h_floor, root_h, corr, sums, work, work_bytes,
                           stream);
  if (family == 1)
    return launch_evidence(f, y, aux, obs, var, n, CountEvidence<1>{mean, 0.0, 0.0}, h_floor, root_h, corr, sums, work, work_bytes,
                           stream);
  return launch_evidence(f, y, nullptr, obs, var, n, CountEvidence<2>{mean, 0.0, 0.0}, h_floor, root_h, corr, sums, work,
                         work_bytes, stream);                          // the Bernoulli family takes no aux
}

extern "C" size_t mgp_nb_evidence_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_nb_evidence_site(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var,
                                    int64_t n, double mean, double dispersion, double h_floor, float* root_h, float* corr,
                                    double* sums, void* work, size_t work_bytes, void* stream) {
  if (!f || !y || !root_h || !sums || n < 1 || !(h_floor >= 0.0) || !nb_dispersion_ok(dispersion)) return MGP_ERR_ARG;
  return launch_evidence(f, y, aux, obs, var, n, CountEvidence<3>{mean, dispersion, std::log(dispersion)}, h_floor, root_h, corr,
                         sums, work, work_bytes, stream);
}

extern "C" size_t mgp_nb_dispersion_sums_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_nb_dispersion_sums(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var,
                                      const double* u, int64_t n, double mean, double dispersion, double h_floor, double* out,
                                      void* work, size_t work_bytes, void* stream) {
  if (!f || !y || !out || n < 1 || !(h_floor >= 0.0) || !nb_dispersion_ok(dispersion)) return MGP_ERR_ARG;
  const double lift = dispersion < (double)kPsiLift ? psi_lift(dispersion) : 0.0;
  return launch_evidence_nodes(f, y, aux, obs, var, u, n, DispersionNode{mean, dispersion, std::log(dispersion), lift, h_floor},
                               nullptr, nullptr, out, 3, work, work_bytes, stream);
}

extern "C" size_t mgp_ordinal_evidence_site_workspace_bytes(int64_t n) { return site_workspace_bytes(n); }

extern "C" int mgp_ordinal_evidence_site(const float* f, const float* lo, const float* hi, const uint8_t* obs, const double* var,
                                         int64_t n, double h_floor, float* root_h, float* corr, double* sums, void* work,
                                         size_t work_bytes, void* stream) {
  if (!f || !lo || !hi || !root_h || !sums || n < 1 || !(h_floor >= 0.0)) return MGP_ERR_ARG;
  return launch_evidence(f, lo, hi, obs, var, n, OrdinalEvidence{}, h_floor, root_h, corr, sums, work, work_bytes, stream);
}

extern "C" size_t mgp_ordinal_cut_sums_workspace_bytes(int64_t n, int K) {
  return (n < 1 || K < 2 || K > 64) ? 0 : (size_t)cut_blocks(n) * kCutRows * (size_t)(K - 1) * sizeof(double);
}

extern "C" int mgp_ordinal_cut_sums(const float* f, const float* lo, const float* hi, const uint8_t* cat, const uint8_t* obs,
                                    const double* var, const double* u, int64_t n, int K, double h_floor, double* out, void* work,
                                    size_t work_bytes, void* stream) {
  if (!f || !lo || !hi || !cat || !out || n < 1 || K < 2 || K > 64 || !(h_floor >= 0.0)) return MGP_ERR_ARG;
  if (!work || !aligned_to(work, 8) || work_bytes < mgp_ordinal_cut_sums_workspace_bytes(n, K)) return MGP_ERR_WORKSPACE;
  const int blocks = cut_blocks(n);
  double* partials = static_cast<double*>(work);
  hipStream_t st = mgp_stream(stream);
  hipLaunchKernelGGL(ordinal_cut_sums_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, f, lo, hi, cat, obs, var, u, n, K,
                     h_floor, partials);
  MGP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ordinal_cut_sums_add_kernel, dim3(1), dim3(kBlock), 0, st, partials, blocks, kCutRows * (K - 1), out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_scale_rows(const float* s, const float* V, const float* X, int64_t n, int P, float* out, void* stream) {
  if (!s || !V || !out || n < 1 || P < 1 || P > 256) return MGP_ERR_ARG;
  const bool vec4 = (P & 3) == 0 && aligned_to(V, 16) && aligned_to(X, 16) && aligned_to(out, 16);
  const int64_t work = vec4 ? n * (P >> 2) : n * (int64_t)P;
  int64_t blocks = mgp_cdiv(work, (int64_t)kBlock);
  if (blocks > kScaleMaxBlocks) blocks = kScaleMaxBlocks;
  if (vec4)
    hipLaunchKernelGGL(scale_rows_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), s, V, X, n, P, out);
  else
    hipLaunchKernelGGL(scale_rows_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), s, V, X, n, P, out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_softmax_root_apply(const float* pi, const float* V, const float* X, int64_t n, int C, int S,
                                      int64_t class_stride, int64_t sample_stride, int transpose, float* out, void* stream) {
  if (!pi || !out || n < 1 || C < 2 || C > 64 || S < 1 || (int64_t)C * S > 256) return MGP_ERR_ARG;
  if (transpose ? !X : (!V || X)) return MGP_ERR_ARG;
  if (!root_strides_ok(C, S, class_stride, sample_stride)) return MGP_ERR_ARG;
  const int blocks = mgp_softmax_blocks(n * S, C, kBlock, kSiteMaxBlocks);
  hipStream_t st = mgp_stream(stream);
  mgp_softmax_dispatch(C, [&](auto tc) {
    hipLaunchKernelGGL(softmax_root_kernel<decltype(tc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, pi, V, X, n, C, S,
                       class_stride, sample_stride, transpose != 0, out);
  });
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_softmax_curvature(const float* pi, const float* delta, int64_t n, int C, int S, double* acc, double* acc2,
                                     void* stream) {
  if (!pi || !delta || !acc || !acc2 || acc == acc2 || n < 1 || C < 2 || C > 64 || S < 1 || (int64_t)C * S > 256)
    return MGP_ERR_ARG;
  const int blocks = softmax_site_blocks(n, C);
  hipStream_t st = mgp_stream(stream);
  mgp_softmax_dispatch(C, [&](auto tc) {
    hipLaunchKernelGGL(softmax_curvature_kernel<decltype(tc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, pi, delta, n,
                       C, S, acc, acc2);
  });
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" size_t mgp_softmax_site_workspace_bytes(int64_t n, int C) {
  return (n < 1 || C < 2 || C > 64) ? 0 : (size_t)softmax_site_blocks(n, C) * 4 * sizeof(double);
}

extern "C" int mgp_softmax_site(const float* f, const float* qf, const int32_t* labels, const uint8_t* obs, int64_t n, int C,
                                float* pi, float* rhs, double* sums, void* work, size_t work_bytes, void* stream) {
  if (!f || !labels || !pi || !rhs || !sums || n < 1 || C < 2 || C > 64) return MGP_ERR_ARG;
  if (!work || !aligned_to(work, 8) || work_bytes < mgp_softmax_site_workspace_bytes(n, C)) return MGP_ERR_WORKSPACE;
  const int blocks = softmax_site_blocks(n, C);
  double* partials = static_cast<double*>(work);
  hipStream_t st = mgp_stream(stream);
  mgp_softmax_dispatch(C, [&](auto tc) {
    hipLaunchKernelGGL(softmax_site_kernel<decltype(tc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, f, qf, labels, obs,
                       n, C, pi, rhs, partials);
  });
  MGP_LAUNCH_CHECK();
  return sum_partials(partials, blocks, sums, false, st);
}

extern "C" int mgp_bernoulli_predict(const float* mean, const double* var, int64_t n, int points, double* prob,
                                     void* stream) {
  if (!mean || !var || !prob || n < 1) return MGP_ERR_ARG;
  if (points < 9 || points > kMaxPoints || (points & 1) == 0) return MGP_ERR_ARG;
  int64_t blocks = mgp_cdiv(n, (int64_t)kBlock);
  if (blocks > kPredictMaxBlocks) blocks = kPredictMaxBlocks;
  hipLaunchKernelGGL(bernoulli_predict_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), mean, var, n,
                     points, prob);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
