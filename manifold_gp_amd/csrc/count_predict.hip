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
// Negative binomial with the dispersion r (mgp_nb_predict_pmf / mgp_nb_predict_logpmf, FAM 2), a the log-exposure:
//   g = c(k, r) - k softplus(-z) - r softplus(z) - (eta - m)^2 / 2v,   z = eta + a - log r,   c = lgamma(k + r) - lgamma(r) - lgamma(k + 1).
// In the variable z this is the binomial integrand with k + r in the place of N, r in the place of N - k and m + a - log r in the
// place of m, so the rule above runs unchanged on those; only the constant differs (nb_const: no term larger than the result's
// scale) and no count is out of range.
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

constexpr double kNbSmallK = 32.0;         // c(k, r): the sum of k logarithms below, Stirling differences from here

struct Site {
  double l1, l2;   // dl / d eta, d2l / d eta2
  double q, qb;    // Poisson: mu (qb unused); binomial: pi, 1 - pi
};

// the failures N - k: the binomial's difference of two integers, the negative binomial's r itself ((k + r) - k is not r)
template <int FAM>
__device__ __forceinline__ double fails(double a, double k, double r) {
  return FAM == 2 ? r : a - k;
}

// S(x) = lgamma(x) - ((x - 1/2) log x - x + log(2 pi) / 2) for x >= 32: six terms of Stirling's series (the seventh is below 1e-21)
__device__ __forceinline__ double stirling_s(double x) {
  const double zi = 1.0 / x;
  const double z2 = zi * zi;
  return zi * (1.0 / 12 + z2 * (-1.0 / 360 + z2 * (1.0 / 1260 + z2 * (-1.0 / 1680 + z2 * (1.0 / 1188 + z2 * (-691.0 / 360360))))));
}

// c(k, r) = lgamma(k + r) - lgamma(r) - lgamma(k + 1) = log C(k + r - 1, k) from terms of the size of the result
// (count_predict.md).  k < 32: sum_{j < k} log((r + j) / (j + 1)), j ascending.  Beyond, lgamma(k + r) is paired with the larger
// of the other two arguments through Stirling's formula, the two leading terms combined by log1p:
//   r >= k + 1:  (k + r - 1/2) log1p(k / r) + k log r - k + S(k + r) - S(r) - lgamma(k + 1)
//   r <  k + 1:  (k + r - 1/2) log1p((r - 1) / (k + 1)) + (r - 1) log(k + 1) - (r - 1) + S(k + r) - S(k + 1) - lgamma(r)
// lr = log r and lgr = lgamma(r) come from the host: r is one scalar per fit.
__device__ __forceinline__ double nb_const(double k, double r, double lr, double lgr) {
  if (k < kNbSmallK) {
    double c = 0.0;
    for (double j = 0.0; j < k; j += 1.0) c = c + log((r + j) / (j + 1.0));
    return c;
  }
  const double x = k + r;
  if (r >= k + 1.0) return (x - 0.5) * log1p(k / r) + k * lr - k + (stirling_s(x) - stirling_s(r)) - lgamma(k + 1.0);
  const double y = k + 1.0, d = r - 1.0;
  return (x - 0.5) * log1p(d / y) + d * log(y) - d + (stirling_s(x) - stirling_s(y)) - lgr;
}

// what the negative-binomial family needs beside (m, v, a, k): the dispersion, its logarithm and lgamma of it
struct Nb {
  double r, lr, lgr;
};

template <int FAM>
__device__ __forceinline__ Site site(double eta, double a, double k, double r = 0.0) {
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
    s.l1 = k * s.qb - fails<FAM>(a, k, r) * s.q;
    s.l2 = -(a * e / (d * d));
  }
  return s;
}

__device__ __forceinline__ double softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// log p(k | eta) with its constant
template <int FAM>
__device__ __forceinline__ double loglik(double eta, double a, double k, const Nb& nb) {
  if (FAM == 0) {
    const double mu = exp(fmin(eta + a, kEtaMax));
    return k * (eta + a) - mu + -lgamma(k + 1.0);
  }
  const double c = FAM == 2 ? nb_const(k, nb.r, nb.lr, nb.lgr) : lgamma(a + 1.0) - lgamma(k + 1.0) - lgamma(a - k + 1.0);
  return c - k * softplus(-eta) - fails<FAM>(a, k, nb.r) * softplus(eta);
}

// g(eta* + t) - g(eta*).  Binomial: softplus(eta + t) - softplus(eta) = log1p(pi expm1(t)) = t + log1p((1 - pi) expm1(-t)), the
// form with the smaller of pi and 1 - pi
template <int FAM>
__device__ __forceinline__ double drop(double t, double k, double a, const Site& s, bool pos, double dm, double v,
                                       double r = 0.0) {
  const double quad = t * (2.0 * dm + t) / (2.0 * v);
  if (FAM == 0) return k * t - s.q * expm1(t) - quad;
  const double lg = log1p((pos ? s.qb : s.q) * expm1(pos ? -t : t));
  return (pos ? -fails<FAM>(a, k, r) * t : k * t) - a * lg - quad;
}

template <int FAM>
__device__ double count_logpmf(double m, double v, double a, double k, int points, const Nb& nb) {
  if (isnan(m) || isnan(v) || isnan(k)) return NAN;
  if (FAM == 1 && k > a) return -INFINITY;
  const double disp = nb.r;                                            // (r names a side of the window below)
  if (FAM == 2) {                                                      // the binomial problem in z = eta + a - log r
    m = m + a - nb.lr;
    a = k + disp;
  }
  if (v <= kVMin) return loglik<FAM>(m, a, k, nb);
  // 1. the mode
  double x, lo, hi;
  if (FAM == 0) {
    const double lk = log(k) - a;
    x = k > 0.0 ? fmax(m, lk) : m;
    lo = k > 0.0 ? fmin(m, lk) : m - v * exp(fmin(m + a, kEtaMax));
    hi = x;
  } else {
    const bool inner = k > 0.0 && (FAM == 2 || k < a);
    const double lg = FAM == 2 ? log(k) - nb.lr : log(k) - log(a - k);
    x = inner ? lg : m;
    lo = inner ? fmin(m, lg) : (k > 0.0 ? m : m - v * a);                 // (negative binomial, k = 0: a = r)
    hi = inner ? fmax(m, lg) : (k > 0.0 ? m + v * a : m);
  }
  bool done = false;
  double dxold = hi - lo;
  for (int it = 0; it < kNewtonMax; ++it) {
    if (!__any(!done)) break;
    const Site s = site<FAM>(x, a, k, disp);
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
  const Site s = site<FAM>(x, a, k, disp);
  const bool pos = x >= 0.0;
  const double dm = x - m;
  const double sig = 1.0 / sqrt(-(s.l2 - 1.0 / v));
  double side[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double sign = r == 0 ? -1.0 : 1.0;
    double wl = 0.0, wh = sig;
    for (int it = 0; it < kDoubleMax; ++it) {
      const bool need = drop<FAM>(sign * wh, k, a, s, pos, dm, v, disp) > -kDrop;
      if (!__any(need)) break;
      wl = need ? wh : wl;
      wh = need ? 2.0 * wh : wh;
    }
    for (int it = 0; it < kBisect; ++it) {
      const double mid = 0.5 * (wl + wh);
      const bool reached = drop<FAM>(sign * mid, k, a, s, pos, dm, v, disp) <= -kDrop;
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
    sum = sum + w * exp(drop<FAM>(t, k, a, s, pos, dm, v, disp));
  }
  const double quad = dm * dm / (2.0 * v);
  return loglik<FAM>(x, a, k, nb) - quad + log(h * sum / sqrt(kTwoPi * v));
}

template <int FAM>
__global__ __launch_bounds__(kBlock) void count_predict_pmf_kernel(const double* __restrict__ eta, const double* __restrict__ var,
                                                                   const float* __restrict__ aux, int64_t n, int64_t k0, int K,
                                                                   int points, int log_out, Nb nb, double* __restrict__ out) {
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
    const double lp = count_logpmf<FAM>(m, v, a, (double)(k0 + j), points, nb);
    out[node * (int64_t)K + j] = log_out ? lp : exp(lp);
  }
}

template <int FAM>
__global__ __launch_bounds__(kBlock) void count_predict_logpmf_kernel(const double* __restrict__ eta, const double* __restrict__ var,
                                                                      const float* __restrict__ aux, const float* __restrict__ y,
                                                                      const uint8_t* __restrict__ at, int64_t n, int points,
                                                                      Nb nb, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    double lp = NAN;
    if (!at || at[i]) {
      const double a = aux ? (double)aux[i] : 0.0;
      lp = count_logpmf<FAM>(eta[i], var[i], a, (double)y[i], points, nb);
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
                       log_out, Nb{0.0, 0.0, 0.0}, out);
  else
    hipLaunchKernelGGL(count_predict_pmf_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, n, k0, K, points,
                       log_out, Nb{0.0, 0.0, 0.0}, out);
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
                       Nb{0.0, 0.0, 0.0}, out);
  else
    hipLaunchKernelGGL(count_predict_logpmf_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, eta, var, aux, y, at, n, points,
                       Nb{0.0, 0.0, 0.0}, out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

namespace {

int check_nb(const double* eta, const double* var, int64_t n, double dispersion, int points, const double* out) {
  if (!eta || !var || !out || n < 1) return MGP_ERR_ARG;
  if (points < kMinPoints || points > kMaxPoints || (points & 1) == 0) return MGP_ERR_ARG;
  if (!(dispersion >= 0x1p-10 && dispersion <= 0x1p20)) return MGP_ERR_ARG;      // (NaN fails the comparison)
  return MGP_OK;
}

Nb nb_of(double dispersion) { return Nb{dispersion, std::log(dispersion), std::lgamma(dispersion)}; }

}  // namespace

extern "C" int mgp_nb_predict_pmf(const double* eta, const double* var, const float* aux, int64_t n, double dispersion, int64_t k0,
                                  int K, int points, int log_out, double* out, void* stream) {
  if (K < 1 || K > kMaxK || k0 < 0 || k0 + K - 1 > kMaxCount) return MGP_ERR_ARG;
  MGP_TRY(check_nb(eta, var, n, dispersion, points, out));
  const int64_t tasks = n * (int64_t)((K + MGP_WAVE - 1) / MGP_WAVE);
  int64_t blocks = mgp_cdiv(tasks, (int64_t)kWaves);
  if (blocks > kPmfMaxBlocks) blocks = kPmfMaxBlocks;
  hipLaunchKernelGGL(count_predict_pmf_kernel<2>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), eta, var, aux, n, k0,
                     K, points, log_out, nb_of(dispersion), out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

extern "C" int mgp_nb_predict_logpmf(const double* eta, const double* var, const float* aux, const float* y, const uint8_t* at,
                                     int64_t n, double dispersion, int points, double* out, void* stream) {
  if (!y) return MGP_ERR_ARG;
  MGP_TRY(check_nb(eta, var, n, dispersion, points, out));
  int64_t blocks = mgp_cdiv(n, (int64_t)kBlock);
  if (blocks > kLogpmfMaxBlocks) blocks = kLogpmfMaxBlocks;
  hipLaunchKernelGGL(count_predict_logpmf_kernel<2>, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), eta, var, aux, y,
                     at, n, points, nb_of(dispersion), out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
