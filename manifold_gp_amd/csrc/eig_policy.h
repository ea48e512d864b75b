// The round policy of the filtered block eigensolver (mgp_lanczos_smallest): where the filter starts, what a warm start
// changes, when the estimated upper end of the spectrum has fallen short, and -- after every Rayleigh-Ritz round -- whether the
// solve has converged, has reached the fp32 floor, or runs another round and with which interval, degree and locked columns.
// Plain structs and pure functions over <math.h> / <algorithm>: no HIP, no I/O, no environment.  eigen.hip drives the GPU with
// it; tests/test_eig_policy_cpu.py drives a dense float iteration on the CPU with the same functions.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>

// ub: the Gershgorin bound (rigorous; the norm of L the residual test is relative to); ubf: the filter's upper end (the Krylov
// estimate of lambda_max where there is one, else ub); kCap: the degree cap.  The next round damps [a, ubf], normalised at a0, at
// degree deg, and does not filter the leading nlock columns.  top_prev: the largest Ritz value of the previous round's block (they
// only come down); rmax_prev / nconv_prev: its largest wanted residual and pairs under tol (the observed floor exit).
struct EigPolicy {
  double ub, ubf;
  int kCap;
  double a, a0;
  int deg;
  double top_prev, rmax_prev;
  int nconv_prev, nlock;
  bool whole;       // the block spans the whole space (b = n): no filter, see eig_whole_space
};

// Cold start on the bounds (ub, ubf); user_degree > 0 fixes the degree of every round.
// Degree cap: 200 was tuned with the Gershgorin bound as the filter's upper end (80: 8 rounds / 497 applies at m = 100, 200:
// 4 / 343, 300: 4 / 443).  What a degree buys goes with 1 / sqrt(ub - a), so under a tighter bound the same filter strength
// is degree 200 sqrt(ubf / ub) (146 when lambda_max is half of Gershgorin); more only over-solves the last round (60k graph,
// cap 120 / 146 / 200 / 240: 247 / 273 / 327 / 367 applies for residuals 2.7 / 2.6 / 1.9 / 1.9e-4, tolerance 3.0e-4).
inline EigPolicy eig_cold_start(double ub, double ubf, int user_degree) {
  const int kCap = std::max(100, std::min(200, (int)lround(200.0 * sqrt(ubf / ub))));
  return EigPolicy{ub, ubf, kCap, ubf / 4.0, 0.0, user_degree > 0 ? user_degree : 10, 1e300, 1e300, 0, 0, false};
}

// A block as wide as the whole space (b = n) needs no filter: Rayleigh-Ritz on it is exact, and there is nothing outside the block to
// damp -- the interval [a, ubf] above the block's largest Ritz value is then empty of eigenvalues, and a polynomial that is small
// on that sliver grows over the WHOLE spectrum, so even the minimum degree lifts the lowest modes over mode m by more than float32
// columns survive (n = 300, m = 250: the rounds never converged).  Such a solve runs rounds of degree 0 -- L V, Gram blocks,
// Rayleigh-Ritz, rotation -- on all columns: the first on the random block, the second on its orthonormalised rotation, where the
// fp32 rotation is accurate.  Set after eig_cold_start / eig_warm_start (a cold start clears it); a user degree is kept instead.
inline void eig_whole_space(EigPolicy& s) { s.whole = true; s.deg = 0; s.nlock = 0; }

// Warm start: the warm block's own Ritz values (warm_evals [b], ascending) stand in for a first Rayleigh-Ritz round (a little
// margin on the interval's lower end: the matrix has moved since they were computed).  Values that cannot be used leave the
// cold state as it is.
inline void eig_warm_start(EigPolicy& s, const float* warm_evals, int b, int m, int user_degree) {
  if (b <= m) return;
  const double top = (double)warm_evals[b - 1], thm = (double)warm_evals[m - 1];
  if (std::isfinite(top) && top > 0.0 && top < s.ubf && std::isfinite(thm) && thm < top) {
    s.a = std::min(0.5 * (top + s.ubf), 1.02 * top);
    s.a0 = std::min((double)warm_evals[0], 0.0);
    const double gap = std::max(s.a - thm, 1e-12 * s.ub);
    const int dnew = (int)ceil(3.0 / (2.0 * sqrt(gap / (s.ubf - s.a))));
    if (!(user_degree > 0)) s.deg = std::min(std::max(dnew, 8), s.kCap);
  }
}

// The estimated upper end fell short if a Ritz value lies above it (proof: Ritz values never exceed lambda_max), or if
// the block's largest Ritz value (top), which only comes down from round to round, jumps up towards the top of the spectrum
// (the filter amplified what it should have damped).  The answer is eig_cold_start(ub, ub, ...) and a fresh block.
inline bool eig_bound_short(const EigPolicy& s, double top) {
  return s.ubf < s.ub && (top > s.ubf * (1.0 + 1e-3) || (top > 2.0 * s.top_prev && top > 0.25 * s.ubf));
}

// Block width.  One fused SpMM launch serves at most kEigChunkMax columns; a block of up to kEigMaxBlock columns runs its products
// in column chunks (the Gram blocks, the rotation and the residuals take the whole width).
constexpr int kEigChunkMax = 256;
constexpr int kEigMaxBlock = 512;

// The chunk rule of a block product on `ba` active columns: ceil(ba / 256) chunks of equal width rounded up to a multiple of 4,
// the last one taking what is left -- 320 runs as 160 + 160, 300 as 152 + 148, never 256 + 64: with more than one chunk every
// chunk has at least 125 columns (257 runs as 132 + 125), so none falls under the 48 the matrix-core SpMM needs, and every chunk
// starts on a multiple of 4 (16-byte aligned rows in its own [n, width] buffer).  Every width is a multiple of 4 except that
// the LAST chunk carries ba mod 4 (a block as wide as the whole space, b = n, need not be a multiple of 4).  ba <= 256 is one
// chunk of ba columns: the launch there has always been.
inline int eig_chunk_count(int ba) { return std::max(1, (ba + kEigChunkMax - 1) / kEigChunkMax); }
// first column of chunk k (k = eig_chunk_count(ba): ba)
inline int eig_chunk_start(int ba, int k) {
  const int nc = eig_chunk_count(ba);
  const int w = ((ba + nc - 1) / nc + 3) / 4 * 4;
  return std::min(ba, k * w);
}

enum EigVerdict { EIG_CONTINUE = 0, EIG_CONVERGED = 1, EIG_FLOOR = 2 };

// nconv / lead: wanted pairs under tol ub and the leading run of them; rmx: the largest wanted residual; ruled: the exponent
// rule ran and left what the trace prints in the remaining fields
struct EigStep {
  EigVerdict verdict;
  int nconv, lead, dask, dnew;
  double rmx, gap, target, t_fin, t_safe;
  bool ruled;
};

// The step after a Rayleigh-Ritz round that was not answered by eig_bound_short: th [kept] the Ritz values, res [b] the
// residuals of the rotated block, deg_used the degree of the round just run, tiles: the CSR carries the matrix-core tile image,
// lab_target (nullable): a fixed damping exponent in place of the rule (lab builds).  EIG_CONTINUE leaves the next round's
// a, a0, deg and nlock in s.
inline EigStep eig_round_step(EigPolicy& s, const double* th, const double* res, int m, int b, int kept, double tol, int64_t n,
                              int deg_used, bool tiles, int user_degree, const double* lab_target) {
  EigStep r{};                 // verdict: EIG_CONTINUE
  s.top_prev = th[kept - 1];
  s.nlock = 0;
  if (kept < m) return r;      // the wanted block is not even spanned: same filter again (dropped directions were refilled)
  const double ub = s.ub;
  for (int j = 0; j < m; ++j) {
    r.nconv += (res[j] <= tol * ub) ? 1 : 0;
    r.rmx = std::max(r.rmx, res[j]);
  }
  while (r.lead < m && res[r.lead] <= tol * ub) ++r.lead;
  if (r.nconv == m) { r.verdict = EIG_CONVERGED; return r; }
  // the two early exits below hand the block back with MGP_OK and info[2] < m; they apply only once the largest residual
  // is within 50 x the tolerance asked for, or within 10 x the measured fp32 floor (1.8e-6 ub, see there) for tolerances
  // below it -- a block further out than that is NOT "at the floor" and keeps iterating / ends as MGP_ERR_NOT_CONVERGED
  const double floor_guard = std::max(50.0 * tol, 2e-5);
  // The attainable residual of an fp32 iteration is a few ulp of |L| (the SpMM's own rounding: measured 1.8e-6 ub on
  // the 60k RMNIST-like graph, 7e-8 ub on the smooth modes of the dumbbell): a tolerance under that floor can never
  // be met, and the rounds past it only shuffle round-off (60 rounds / 1.3 s where 5 reach the floor).  With the
  // filter at its degree cap a round multiplies the error of the slowest wanted pair by <= e^-3 unless the gap
  // behind the block is tiny; a round at the cap that does not even halve the largest residual, with no further
  // pair converging, is therefore taken as the floor: the caller gets the block as it stands, the true residuals in
  // `resid`, info[2] = pairs under tol (< m) and MGP_OK.
  if ((deg_used >= s.kCap || s.whole) && r.rmx > 0.5 * s.rmax_prev && r.nconv <= s.nconv_prev && r.rmx <= floor_guard * ub) { r.verdict = EIG_FLOOR; return r; }
  s.rmax_prev = r.rmx;
  s.nconv_prev = r.nconv;
  if (s.whole) return r;       // the next round is another unfiltered one on all columns (deg 0, nlock 0 stay)
  // Soft locking: the leading run of converged Ritz vectors (a multiple of 4 columns) is no longer filtered -- the Chebyshev
  // recurrence and the L apply run on the remaining columns -- but stays in the Rayleigh-Ritz basis.  Per chunk of the block
  // products (eig_chunk_start) the same holds: the locked run is a multiple of 4, so every chunk of the b - nlock active columns
  // starts on a multiple of 4, and the minimum of 8 (or 48) active columns below is a minimum per chunk, since more than one
  // chunk means at least 125 columns in each.
  s.nlock = r.lead / 4 * 4;
  if (b - s.nlock < 8) s.nlock = 0;
  // the matrix-core tile SpMM serves 48 columns and more: a block locked down to fewer active columns falls back to the gather
  // kernel, whose 28 columns cost MORE per product than 64 on the tiles (1M nodes, b = 64: 0.48 against 0.38 ms) -- keep 48
  if (tiles && b >= 48 && b - s.nlock < 48) s.nlock = (b - 48) / 4 * 4;
  s.a = th[kept - 1];
  s.a0 = std::min(th[0], 0.0);
  r.ruled = true;
  r.gap = std::max(s.a - th[m - 1], 1e-12 * ub);
  // dunit: the filter degree per unit of damping exponent at the measured gap; dnew: the degree of an e^-3 round (rounds 1-4
  // ran every round at it; the exits below are written in it).
  const double dunit = 1.0 / (2.0 * sqrt(r.gap / (s.ubf - s.a)));
  r.dnew = (int)ceil(3.0 * dunit);
  // Round 5: a Rayleigh-Ritz round costs ~2 ms of host + Gram + rotation at b = 128 -- as much as 57 block products at 60k -- so
  // a round should do what the arithmetic allows, and the last one no more than is left to do.  The largest wanted residual falls
  // by ~exp(-t / 2) in a round of exponent t (measured: t = 3 / 4.5 / 9 -> x 0.22 / 0.1 / 0.01), so t_fin = 2 ln(r_max / (0.3 tol
  // ub)) would finish; inside the wanted block the filter lifts mode 1 over mode m by exp(t (sqrt(a - th_1) - sqrt(gap)) /
  // sqrt(gap)), which float32 columns survive up to ~1e4 (t_safe; more and mode m drops under the round-off of mode 1), and 9
  // at most (t_cap, below).  Never less than the e^-3 round.  Conditioned 60k swiss roll: 7 rounds / 105 products / 18.3 ms -> 4 / ~120 /
  // ~13.5 ms; RMNIST-like 60k (ends at the fp32 floor): 4 / 280 / 18.4 ms -> 3 / ~220 / ~14 ms.
  r.t_fin = 2.0 * log(std::max(r.rmx, 1e-300) / (0.3 * tol * ub));
  const double s1 = sqrt(std::max(s.a - th[0], 0.0)), sm = sqrt(r.gap);
  r.t_safe = s1 > sm ? log(1e4) * sm / (s1 - sm) : 9.0;
  // ... where rounds are expensive against block products: a round is ~57 products at n b = 7.7e6 (60k x 128) but ~5 at
  // 6.4e7 (1M x 64), where the stronger rounds only add products (530 against 438, 229 against 225 ms): the cap goes from 9
  // under n b = 1.6e7 to the e^-3 round at 6.4e7 (logarithmically in between; deterministic, no timing involved).
  const double nb = (double)n * (double)b;
  const double t_cap = nb <= 1.6e7 ? 9.0 : nb >= 6.4e7 ? 3.0 : 9.0 - 6.0 * log(nb / 1.6e7) / log(4.0);
  r.target = std::min(std::max(r.t_fin, 3.0), std::min(t_cap, std::max(r.t_safe, 3.0)));
  if (lab_target) r.target = *lab_target;       // lab: fixed per-round damping exponent
  r.dask = (int)ceil(r.target * dunit);
  // degree cap 200 (80 until late in round 1: 8 rounds / 497 applies at m = 100 where 200 needs 4 / 343; the
  // scaled three-term recurrence is normalised at a0, so the block does not overflow at these degrees)
  s.deg = std::min(std::max(r.dask, 8), s.kCap);
  if (user_degree > 0) s.deg = user_degree;
  // The same exit, predicted instead of observed.  A round of degree d multiplies the slowest wanted pair's error by
  // about exp(-3 d / dnew) (dnew = the degree that gives e^-3 at the measured gap between the wanted block and its
  // last guard).  When a round at the cap has been run and the gap asks for more than ~4.3 caps (predicted factor
  // > 0.5: the wanted modes sit in a cluster with their guards -- on the 60k RMNIST-like graph 128 Ritz values lie
  // within 1e-6 lambda_max), every further 200-apply round would buy less than a factor 2: stop before running it
  // (C3 at tol 1e-6: 4 rounds / 50 ms instead of 5 / 67 ms, same residual 2.5e-4 as tol 1e-5 reaches).
  // (Round 5: 0.5 -> 0.36.  The largest RESIDUAL follows the square root of that factor -- see the exponent rule above -- so a
  // cap round predicted at 0.36 improves it by less than 1.7 x for ~7 ms at 60k; and with the stronger early rounds the first
  // cap round is reached a round sooner, at a gap that asks for ~3.8 caps instead of ~5.8: the same block quality -- RMNIST-like
  // 60k: 2.4e-4 after 3 rounds / 249 products against 2.2e-4 after 4 / 280 -- must end the same way.)
  if (!(user_degree > 0) && deg_used >= s.kCap && r.dnew > s.kCap && exp(-3.0 * s.kCap / (double)r.dnew) > 0.36 &&
      r.rmx <= floor_guard * ub)
    r.verdict = EIG_FLOOR;
  return r;
}
