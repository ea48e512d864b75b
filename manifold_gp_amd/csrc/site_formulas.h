// The per-node likelihood arithmetic of the Laplace fits, stated once: log p, g = d log p / df and h = -d g / df of one observed
// node, float64 from the float32 data.  laplace.hip (the fits on the graph nodes, f a float32 iterate) and spectral_laplace.hip
// (the fits on the spectral features, f = z . w in float64) both include it; the formulas are the ones laplace.hip's head comment
// derives.  Every function takes f as a double and leaves through references; none reads memory.
#pragma once
#include <hip/hip_runtime.h>

// Bernoulli-logit, class 1 where y32 > 0.5
__device__ __forceinline__ void mgp_bernoulli_lgh(double f, float y32, double& lp, double& g, double& h) {
  const bool t = y32 > 0.5f;
  const double a = t ? f : -f;
  const double e = exp(-fabs(f));
  const double d = 1.0 + e;
  const double pi = f >= 0.0 ? 1.0 / d : e / d;
  lp = (a < 0.0 ? a : 0.0) - log1p(e);
  g = (t ? 1.0 : 0.0) - pi;
  h = e / (d * d);
}

// FAMILY 0: Poisson, a32 the log-exposure; FAMILY 1: binomial, a32 the trials; FAMILY 2: negative binomial with the dispersion
// r_nb (log_r = log r), a32 the log-exposure: the binomial arithmetic with y + r "trials" and r "failures" at the predictor
// z = f + mean + a - log r (pi = mu / (r + mu))
template <int FAMILY>
__device__ __forceinline__ void mgp_count_lgh(double f, double mean, double r_nb, double log_r, float y32, float a32, double& lp,
                                              double& g, double& h) {
  const double y = (double)y32;
  if (FAMILY == 0) {
    const double eta = f + mean + (double)a32;
    const double mu = exp(eta < 700.0 ? eta : 700.0);
    lp = y * eta - mu;
    g = y - mu;
    h = mu;
  } else {
    const double eta = FAMILY == 1 ? f + mean : f + mean + (double)a32 - log_r;
    const double N = FAMILY == 1 ? (double)a32 : y + r_nb;
    const double m = FAMILY == 1 ? N - y : r_nb;                     // failures (binomial: exact, both are integers <= 2^24)
    const double e = exp(-fabs(eta));
    const double d = 1.0 + e;
    const double l1 = log1p(e);
    const double pi = eta >= 0.0 ? 1.0 / d : e / d;
    const double pib = eta >= 0.0 ? e / d : 1.0 / d;                 // 1 - pi without the subtraction
    lp = -m * ((eta > 0.0 ? eta : 0.0) + l1) - y * ((eta < 0.0 ? -eta : 0.0) + l1);
    g = y * pib - m * pi;
    h = N * e / (d * d);
  }
}

// the category is the interval (lo32, hi32] of cutpoints, -inf / +inf at the end categories.  exp(-|x|) is 0 at an infinite end,
// so sigma, log sigma and sigma (1 - sigma) need no special case there
__device__ __forceinline__ void mgp_ordinal_lgh(double f, float lo32, float hi32, double& lp, double& g, double& h) {
  const double u = (double)hi32 - f, l = (double)lo32 - f;
  const double eu = exp(-fabs(u)), el = exp(-fabs(l));
  const double du = 1.0 + eu, dl = 1.0 + el;
  lp = -((u < 0.0 ? -u : 0.0) + log1p(eu)) - ((l > 0.0 ? l : 0.0) + log1p(el));           // log sigma(u) + log sigma(-l)
  g = (l >= 0.0 ? 1.0 / dl : el / dl) - (u >= 0.0 ? eu / du : 1.0 / du);                 // sigma(l) - sigma(-u)
  h = eu / (du * du) + el / (dl * dl);
}
