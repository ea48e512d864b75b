// The CG step rule: how the dot products of one step become alpha, beta, a stopping decision and a status.
// This header is the single statement of it; every update / decide kernel of cg.hip and pcg.hip calls it.  The kernels own
// what differs between them: their loads, the order of their reductions and their vector passes.
// Scalars in, small structs out, no pointers into kernel arguments: the header also compiles with a host compiler alone
// (tests/test_cg_rule_cpu.py runs the recurrence through it on the CPU).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MGP_RULE __host__ __device__ __forceinline__
#else
#define MGP_RULE static inline
#endif

// status words of a solve (include/mgp_hip.h); 4 is the partitioned solver's stagnation guard (pcg.hip)
enum { kCgConverged = 1, kCgMaxIter = 2, kCgNotFinite = 3, kCgStagnated = 4 };

struct CgCoef { float alpha, beta; };
struct CgStop { int done, status; };

// relative residual ||r|| / ||b|| from the two squared norms; a zero right-hand side has residual 0.  The test is
// bb != 0, not bb > 0: a NaN in the right-hand side (bb is NaN) then gives a NaN residual, which the decision reports
// (kCgNotFinite), where 0 would pass for convergence.
MGP_RULE float cg_rel(float rr, float bb) { return (bb != 0.f) ? sqrtf(rr / bb) : 0.f; }

// a frozen column takes alpha = beta = 0 from here on: linear_cg's threshold (stop_mode 0) or the column's own tolerance (1)
MGP_RULE bool cg_frozen(int stop_mode, float tol, float rel) { return (stop_mode == 0) ? (rel < 1e-10f) : (rel <= tol); }

// Chronopoulos-Gear coefficients of one column: beta = gamma / gamma_old, alpha = gamma / (delta - beta gamma / alpha_old);
// the first step has no history (alpha = gamma / delta).  A zero denominator gives 0, a non-finite result resets both.
MGP_RULE CgCoef cg_coef(bool first, bool frozen, float gamma, float delta, float gamma_old, float alpha_old) {
  CgCoef c = {0.f, 0.f};
  if (!frozen) {
    if (first) {
      c.alpha = (delta != 0.f) ? gamma / delta : 0.f;
    } else {
      c.beta = (gamma_old != 0.f) ? gamma / gamma_old : 0.f;
      const float den = delta - ((alpha_old != 0.f) ? c.beta * gamma / alpha_old : 0.f);
      c.alpha = (den != 0.f) ? gamma / den : 0.f;
    }
    if (!isfinite(c.alpha) || !isfinite(c.beta)) { c.alpha = 0.f; c.beta = 0.f; }
  }
  return c;
}

// What follows the convergence test of either decision below: `status` is kCgConverged or 0; a non-finite residual
// overrides it, max_iter comes last.  `step` is 1-based: the update of step k decides on r_{k-1}, so `step > min_iter`
// means min_iter steps are done and `step > max_iter` that max_iter are.
MGP_RULE CgStop cg_stop_rest(int status, bool finite, int max_iter, int step) {
  if (!finite) status = kCgNotFinite;
  if (status == 0 && step > max_iter) status = kCgMaxIter;
  const CgStop s = {status != 0, status};
  return s;
}

// stopping decision of a single column
MGP_RULE CgStop cg_stop(int stop_mode, int min_iter, int max_iter, float tol, int step, float rel) {
  int status = 0;
  if (stop_mode == 0) {
    if (step > min_iter && rel < tol) status = kCgConverged;
  } else if (rel <= tol) status = kCgConverged;
  return cg_stop_rest(status, isfinite(rel), max_iter, step);
}

// stopping decision of a block of C columns: stop_mode 0 the mean residual against tol once min_iter steps are done
// (linear_cg), stop_mode 1 every column <= tol; one non-finite column ends the solve.  The mean is a float sum in column order.
MGP_RULE CgStop cg_stop_columns(int stop_mode, int min_iter, int max_iter, float tol, int step, const float* rel, int C) {
  bool conv;
  if (stop_mode == 0) {
    float m = 0.f;
    for (int c = 0; c < C; ++c) m += rel[c];
    m /= (float)C;
    conv = step > min_iter && m < tol;
  } else {
    conv = true;
    for (int c = 0; c < C; ++c) conv &= rel[c] <= tol;
  }
  bool finite = true;
  for (int c = 0; c < C; ++c) if (!isfinite(rel[c])) finite = false;
  return cg_stop_rest(conv ? kCgConverged : 0, finite, max_iter, step);
}

#if defined(__HIPCC__)
// Publication of a decision, by the one thread that took it: the device flags for the launches behind it, then the
// zero-copy results for the host (no blit kernels behind the solve) -- residuals, step and status first, the flag the
// host polls last, behind a system-scope fence.
__device__ __forceinline__ void cg_publish(int* state, int* host_state, float* host_resid, const float* rel, int C, int it,
                                           int status) {
  state[2] = status; state[1] = 1;
  for (int c = 0; c < C; ++c) host_resid[c] = rel[c];
  host_state[0] = it; host_state[2] = status;
  __threadfence_system();
  host_state[1] = 1;
}
#endif
