// The predictive pmf of a count fit (docs/kernels/count_predict.md): with m the linear predictor at the mode (without the
// exposure), v the latent marginal variance and a the log-exposure (Poisson) or the trials N (binomial),
//
//   pmf(k) = (2 pi v)^-1/2 int exp(g(eta)) d eta,
//   Poisson:   g = k (eta + a) - exp(eta + a) - lgamma(k + 1) - (eta - m)^2 / 2v
//   binomial:  g = log C(N, k) - k softplus(-eta) - (N - k) softplus(eta) - (eta - m)^2 / 2v
//
// by a quadrature of its own per (node, k), all in float64 (count_logpmf below; tests/_count_pmf_ref.py restates it operation
// by operation):
//   1. the mode eta* of g by Newton's method inside a bracket (between m and log(k / E) or logit(k / N); m - v E e^m, m -+ v N at
//      the ends of the count range), bisection where a step leaves the bracket or (binomial) is more than half the last one; it
//      ends on a step below 1e-8 sigma_hat,
//      sigma_hat = (-g''(eta*))^-1/2;
//   2. t_L, t_R with g(eta* -+ t) - g(eta*) <= -40: doubling from sigma_hat, then six bisections;
//   3. the P-point trapezoid rule on [eta* - t_L, eta* + t_R] of exp(g(eta* + t) - g(eta*)), the difference formed without
//      cancellation (drop()): an identity at any centre, so the accuracy of eta* only places the window;
//   log pmf = g(eta*) + log(h sum / sqrt(2 pi v)): one logarithm of a quantity of order 1.
// v <= V_MIN (zero and negative variances included) is the plain log pmf at eta = m; k > N gives -inf; NaN in m, v or k gives NaN.
//
// mgp_count_predict_pmf: a wave per (node, 64 consecutive counts), lane = count, so a wave stores 64 consecutive doubles and
// m, v, a are wave-uniform (the wave index goes through readfirstlane: scalar loads).  mgp_count_predict_logpmf: a lane per
// node.  In both the Newton and the window loops run while any lane of the wave needs another step (a ballot per step), up to a
// fixed bound; a lane that is done keeps its values.  No LDS, no atomics: repeated calls are bitwise equal.  8-byte and 4-byte
// accesses only: no alignment beyond the element's.
#include <cfloat>
#include <cmath>

#include "mgp_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MGP_WAVE;
constexpr int kPmfMaxBlocks = 2048;       // grid cap of the pmf kernel: 2048 x 4 waves x 64 counts per step
constexpr int kLogpmfMaxBlocks = 2048;    // grid cap of the logpmf kernel: 2048 x 256 threads x 1 node per step
constexpr int kMinPoints = 17, kMaxPoints = 257;
constexpr int kMaxK = 65536;
constexpr int64_t kMaxCount = (int64_t)1 << 24;
constexpr double kVMin = 0x1p-76;         // v D^2 / 2 <= 2^-53 D for counts and means D <= 2^24 (count_predict.md)
constexpr double kDrop = 40.0;
constexpr int kNewtonMax = 100;
constexpr int kDoubleMax = 40;
constexpr int kBisect = 6;
constexpr double kStepTol = 1e-8;
constexpr double kEtaMax = 700.0;         // exp(min(eta + a, 700)) stays finite, as in mgp_count_site
constexpr double kTwoPi = 6.283185307179586;

struct Site {
  double l1, l2;   // dl / d eta, d2l / d eta2
  double q, qb;    // Poisson: mu (qb unused); binomial: pi, 1 - pi
};

template <int FAM>
__device__ __forceinline__ Site site(double eta, double a, double k) {
  Site s;
  if (FAM == 0) {
    const double mu = exp(fmin(eta + a, kEtaMax));
    s.l1 = k - mu;
    s.l2 = -mu;
    s.q = mu;
    s.qb = 0.0;
  } else {
    const double e = exp(-fabs(eta));
    const double d = 1.0 + e;
    s.q = eta >= 0.0 ? 1.0 / d : e / d;
    s.qb = eta >= 0.0 ? e / d : 1.0 / d;
    s.l1 = k * s.qb - (a - k) * s.q;
    s.l2 = -(a * e / (d * d));
  }
  return s;
}

__device__ __forceinline__ double softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// log p(k | eta) with its constant
template <int FAM>
__device__ __forceinline__ double loglik(double eta, double a, double k) {
  if (FAM == 0) {
    const double mu = exp(fmin(eta + a, kEtaMax));
    return k * (eta + a) - mu + -lgamma(k + 1.0);
  }
  const double c = lgamma(a + 1.0) - lgamma(k + 1.0) - lgamma(a - k + 1.0);
  return c - k * softplus(-eta) - (a - k) * softplus(eta);
}

// g(eta* + t) - g(eta*).  Binomial: softplus(eta + t) - softplus(eta) = log1p(pi expm1(t)) = t + log1p((1 - pi) expm1(-t)), the
// form with the smaller of pi and 1 - pi
template <int FAM>
__device__ __forceinline__ double drop(double t, double k, double a, const Site& s, bool pos, double dm, double v) {
  const double quad = t * (2.0 * dm + t) / (2.0 * v);
  if (FAM == 0) return k * t - s.q * expm1(t) - quad;
  const double lg = log1p((pos ? s.qb : s.q) * expm1(pos ? -t : t));
  return (pos ? -(a - k) * t : k * t) - a * lg - quad;
}

template <int FAM>
__device__ double count_logpmf(double m, double v, double a, double k, int points) {
  if (isnan(m) || isnan(v) || isnan(k)) return NAN;
  if (FAM == 1 && k > a) return -INFINITY;
  if (v <= kVMin) return loglik<FAM>(m, a, k);
  // 1. the mode
  double x, lo, hi;
  if (FAM == 0) {
    const double lk = log(k) - a;
    x = k > 0.0 ? fmax(m, lk) : m;
    lo = k > 0.0 ? fmin(m, lk) : m - v * exp(fmin(m + a, kEtaMax));
    hi = x;
  } else {
    const bool inner = k > 0.0 && k < a;
    const double lg = log(k) - log(a - k);
    x = inner ? lg : m;
    lo = inner ? fmin(m, lg) : (k > 0.0 ? m : m - v * a);
    hi = inner ? fmax(m, lg) : (k > 0.0 ? m + v * a : m);
  }
  bool done = false;
  double dxold = hi - lo;
  for (int it = 0; it < kNewtonMax; ++it) {
    if (!__any(!done)) break;
    const Site s = site<FAM>(x, a, k);
    const double g1 = s.l1 - (x - m) / v;
    const double g2 = s.l2 - 1.0 / v;
    lo = g1 > 0.0 ? x : lo;
    hi = g1 < 0.0 ? x : hi;
    const double step = g1 / g2;
    const bool conv = fabs(step) <= kStepTol / sqrt(-g2) + 4.0 * DBL_EPSILON * fabs(x);
    double xn = x - step;
    // binomial: g' is not concave, and a step that does not halve the last one is not trusted either (from eta = m with k = 0 of
    // 65535 trials the plain iteration cycles between m and m - v N pi inside the bracket)
    const bool ok = xn > lo && xn < hi && (FAM == 0 || fabs(step) <= 0.5 * dxold);
    xn = (conv || ok) ? xn : 0.5 * (lo + hi);
    dxold = done ? dxold : fabs(xn - x);
    x = done ? x : xn;
    done = done || conv;
  }
  // 2. the window
  const Site s = site<FAM>(x, a, k);
  const bool pos = x >= 0.0;
  const double dm = x - m;
  const double sig = 1.0 / sqrt(-(s.l2 - 1.0 / v));
  double side[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double sign = r == 0 ? -1.0 : 1.0;
    double wl = 0.0, wh = sig;
    for (int it = 0; it < kDoubleMax; ++it) {
      const bool need = drop<FAM>(sign * wh, k, a, s, pos, dm, v) > -kDrop;
      if (!__any(need)) break;
      wl = need ? wh : wl;
      wh = need ? 2.0 * wh : wh;
    }
    for (int it = 0; it < kBisect; ++it) {
      const double mid = 0.5 * (wl + wh);
      const bool reached = drop<FAM>(sign * mid, k, a, s, pos, dm, v) <= -kDrop;
      wh = reached ? mid : wh;
      wl = reached ? wl : mid;
    }
    side[r] = wh;
  }
  // 3. the sum, j ascending
  const double tl = side[0], tr = side[1];
  const double h = (tl + tr) / (double)(points - 1);
  double sum = 0.0;
  for (int j = 0; j < points; ++j) {
    const double t = -tl + (double)j * h;
    const double w = (j == 0 || j == points - 1) ? 0.5 : 1.0;
    sum = sum + w * exp(drop<FAM>(t, k, a, s, pos, dm, v));
  }
  const double quad = dm * dm / (2.0 * v);
  return loglik<FAM>(x, a, k) - quad + log(h * sum / sqrt(kTwoPi * v));
}

template <int FAM>
__global__ __launch_bounds__(kBlock) void count_predict_pmf_kernel(const double* __restrict__ eta, const double* __restrict__ var,
                                                                   const float* __restrict__ aux, int64_t n, int64_t k0, int K,
                                                                   int points, int log_out, double* __restrict__ out) {
  const int lane = threadIdx.x & (MGP_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / MGP_WAVE));
  const int chunks = (K + MGP_WAVE - 1) / MGP_WAVE;
  const int64_t tasks = n * (int64_t)chunks;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  for (int64_t task = (int64_t)blockIdx.x * kWaves + wave; task < tasks; task += stride) {
    const int64_t node = task / chunks;
    const int j = (int)(task - node * chunks) * MGP_WAVE + lane;
    if (j >= K) continue;                                                // (the last chunk of a row: the other lanes go on)
    const double m = eta[node], v = var[node];
    const double a = aux ? (double)aux[node] : 0.0;
    const double lp = count_logpmf<FAM>(m, v, a, (double)(k0 + j), points);
    out[node * (int64_t)K + j] = log_out ? lp : exp(lp);
  }
}

template <int FAM>
__global__ __launch_bounds__(kBlock) void count_predict_logpmf_kernel(const double* __restrict__ eta, const double* __restrict__ var,
                                                                      const float* __restrict__ aux, const float* __restrict__ y,
                                                                      const uint8_t* __restrict__ at, int64_t n, int points,
                                                                      double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    double lp = NAN;
    if (!at || at[i]) {
      const double a = aux ? (double)aux[i] : 0.0;
      lp = count_logpmf<FAM>(eta[i], var[i], a, (double)y[i], points);
    }
    out[i] = lp;
  }
}

int check_common(const double* eta, const double* var, const float* aux, int64_t n, int family, int points, const double* out) {
  if (!eta || !var || !out || n < 1) return MGP_ERR_ARG;
  if (points < kMinPoints || points > kMaxPoints || (points & 1) == 0) return MGP_ERR_ARG;
  if (family != 0 && family != 1) return MGP_ERR_UNSUPPORTED;
  if (family == 1 && !aux) return MGP_ERR_ARG;
  return MGP_OK;
}

}  // namespace

extern "C" int mgp_count_predict_pmf(const double* eta, const double* var, const float* aux, int64_t n, int family, int64_t k0,
                                     int K, int points, int log_out, double* out, void* stream) {
  if (K < 1 || K > kMaxK || k0 < 0 || k0 + K - 1 > kMaxCount) return MGP_ERR_ARG;
  MGP_TRY(check_common(eta, var, aux, n, family, points, out));
  const int64_t tasks = n * (int64_t)((K + MGP_WAVE - 1) / MGP_WAVE);
  int64_t blocks = mgp_cdiv(tasks, (int64_t)kWaves);
  if (blocks > kPmfMaxBlocks) blocks = kPmfMaxBlocks;
  hipStream_t st = mgp_stream(stream);
  if (family == 0)
    hipLaunchKernelGGL(count_predict_pmf_kernel<0>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, n, k0, K, points,
                       log_out, out);
  else
    hipLaunchKernelGGL(count_predict_pmf_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, n, k0, K, points,
                       log_out, out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_count_predict_logpmf(const double* eta, const double* var, const float* aux, const float* y, const uint8_t* at,
                                        int64_t n, int family, int points, double* out, void* stream) {
  if (!y) return MGP_ERR_ARG;
  MGP_TRY(check_common(eta, var, aux, n, family, points, out));
  int64_t blocks = mgp_cdiv(n, (int64_t)kBlock);
  if (blocks > kLogpmfMaxBlocks) blocks = kLogpmfMaxBlocks;
  hipStream_t st = mgp_stream(stream);
  if (family == 0)
    hipLaunchKernelGGL(count_predict_logpmf_kernel<0>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, y, at, n, points,
                       out);
  else
    hipLaunchKernelGGL(count_predict_logpmf_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, y, at, n, points,
                       out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
