// Host dense algebra of the eigensolver (fp64, standard C++ and the Linux affinity mask only: a host compiler builds this header alone, which is how
// tests/test_eig_policy_cpu.py runs it): the small symmetric eigensolver, the worker pool, the whitening and the
// Rayleigh-Ritz step of a round.  eigen.hip holds the kernels and the driver, eig_policy.h the round policy.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef __linux__
#include <sched.h>
#endif
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// ---------------------------------------------------------------- host: symmetric eigensolver (fp64)
// Householder tridiagonalisation + implicit-shift QL, restated so that every O(n^3) loop walks a ROW of a row-major
// array and the eigenvector update runs on host threads:
//   1. T = Q^T A Q on the lower triangle (symmetric rank-2 updates, 4/3 n^3 flops);
//   2. Z^T = Q^T accumulated by right multiplications (4/3 n^3);
//   3. QL on (d, e) alone -- its plane rotations are RECORDED (they do not depend on the vectors);
//   4. the ~n^2 recorded rotations are applied to Z^T, rows i / i+1, over column slices of 32: a slice is an
//      L1-resident private copy owned by one host thread (3 n^3 flops, the largest part, now parallel).
// Round 3: the b = 128 Rayleigh-Ritz problem took 2.0 ms per round in the column-walking EISPACK form this replaces
// (4 rounds = 8 of the 48 ms of the 60k eigensolve).  Dot products use four interleaved partial sums in a fixed
// order and -ffp-contract=off holds for the host pass too, so the result does not depend on the thread count or on
// whether the AVX2 clones run.  A [n x n] row-major symmetric; evals ascending; eigenvectors = columns of V.
#define MGP_HOST_INLINE static inline __attribute__((always_inline))

MGP_HOST_INLINE double dot4(const double* __restrict__ a, const double* __restrict__ b, int n) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    s0 += a[i] * b[i];
    s1 += a[i + 1] * b[i + 1];
    s2 += a[i + 2] * b[i + 2];
    s3 += a[i + 3] * b[i + 3];
  }
  double s = (s0 + s2) + (s1 + s3);
  for (; i < n; ++i) s += a[i] * b[i];
  return s;
}

struct PlaneRot { int i; double c, s; };

// T = Q^T A Q, Q = H_0 H_1 ... H_{n-3}, H_k = I - tau_k v_k v_k^T with v_k in indices k+1 .. n-1 (v_k[k+1] = 1; row k
// of hv).  Only the LOWER triangle of W is read and written.  d = diagonal of T, e[i] = T[i+1, i].
MGP_HOST_INLINE void householder_tridiag_impl(int n, int ld, double* W, double* d, double* e, double* hv, double* tau,
                                              double* p, double* w) {
  for (int k = 0; k + 2 < n; ++k) {
    const int s = n - k - 1;
    double* v = hv + (size_t)k * ld + (k + 1);
    double scale = 0.0, tail = 0.0;
    for (int j = 0; j < s; ++j) {
      v[j] = W[(size_t)(k + 1 + j) * ld + k];
      scale = std::max(scale, fabs(v[j]));
      if (j) tail = std::max(tail, fabs(v[j]));
    }
    d[k] = W[(size_t)k * ld + k];
    const double alpha = v[0];
    if (tail == 0.0) { tau[k] = 0.0; e[k] = alpha; continue; }   // the column is tridiagonal already: H_k = I
    double ss = 0.0;
    for (int j = 0; j < s; ++j) { const double t = v[j] / scale; ss += t * t; }
    const double nrm = scale * sqrt(ss);
    const double beta = alpha > 0.0 ? -nrm : nrm;
    const double tk = (beta - alpha) / beta;
    const double inv = 1.0 / (alpha - beta);
    v[0] = 1.0;
    for (int j = 1; j < s; ++j) v[j] *= inv;
    tau[k] = tk;
    e[k] = beta;
    double* B = W + (size_t)(k + 1) * ld + (k + 1);
    // p = tau B v: row j of the lower triangle gives its own dot product and its share of the entries above it
    for (int j = 0; j < s; ++j) {
      const double* __restrict__ row = B + (size_t)j * ld;
      const double vj = v[j];
      const double t = dot4(row, v, j);
      for (int i = 0; i < j; ++i) p[i] += row[i] * vj;
      p[j] = t + row[j] * vj;
    }
    for (int j = 0; j < s; ++j) p[j] *= tk;
    const double hh = 0.5 * tk * dot4(p, v, s);
    for (int j = 0; j < s; ++j) w[j] = p[j] - hh * v[j];
    for (int j = 0; j < s; ++j) {          // B -= v w^T + w v^T
      double* __restrict__ row = B + (size_t)j * ld;
      const double vj = v[j], wj = w[j];
      for (int i = 0; i <= j; ++i) row[i] -= vj * w[i] + wj * v[i];
    }
  }
  if (n >= 2) { d[n - 2] = W[(size_t)(n - 2) * ld + (n - 2)]; e[n - 2] = W[(size_t)(n - 1) * ld + (n - 2)]; }
  d[n - 1] = W[(size_t)(n - 1) * ld + (n - 1)];
  e[n - 1] = 0.0;
}

// Zt = Q^T = H_{n-3} ... H_0 as ((I H_{n-3}) H_{n-4}) ... H_0: M <- M - tau (M v) v^T touches rows and columns
// k+1 .. n-1 only (the rows above are still rows of the identity).
MGP_HOST_INLINE void householder_accumulate_impl(int n, int ld, const double* hv, const double* tau, double* Zt, int r0, int r1) {
  // rows [r0, r1) only: a row of M runs through all the H_k on its own, so row ranges are independent jobs
  for (int r = r0; r < r1; ++r) {
    for (int c = 0; c < n; ++c) Zt[(size_t)r * ld + c] = 0.0;
    Zt[(size_t)r * ld + r] = 1.0;
  }
  for (int k = std::min(n - 3, r1 - 2); k >= 0; --k) {
    if (tau[k] == 0.0) continue;
    const int s = n - k - 1;
    const double* __restrict__ v = hv + (size_t)k * ld + (k + 1);
    for (int r = std::max(r0, k + 1); r < r1; ++r) {
      double* __restrict__ row = Zt + (size_t)r * ld + (k + 1);
      const double g = tau[k] * dot4(row, v, s);
      for (int i = 0; i < s; ++i) row[i] -= g * v[i];
    }
  }
}

// rows i, i+1 of Zt <- the recorded rotations, columns [k0, k1): worked on in a compact private copy (n x len: 32 KB
// at n = 128 and 32 columns), so no cache line is shared with the neighbouring slices' threads
MGP_HOST_INLINE void apply_rots_impl(int n, int ld, double* Zt, const std::vector<PlaneRot>& rots, int k0, int k1) {
  const int len = k1 - k0;
  if (len <= 0) return;
  std::vector<double> loc((size_t)n * len);
  for (int r = 0; r < n; ++r) memcpy(&loc[(size_t)r * len], Zt + (size_t)r * ld + k0, len * sizeof(double));
  for (const PlaneRot& q : rots) {
    double* __restrict__ r0 = &loc[(size_t)q.i * len];
    double* __restrict__ r1 = r0 + len;
    const double c = q.c, s = q.s;
    for (int k = 0; k < len; ++k) {
      const double h = r1[k], g = r0[k];
      r1[k] = s * g + c * h;
      r0[k] = c * g - s * h;
    }
  }
  for (int r = 0; r < n; ++r) memcpy(Zt + (size_t)r * ld + k0, &loc[(size_t)r * len], len * sizeof(double));
}

// the same three loops compiled twice: baseline x86-64 and AVX2 (picked at run time; identical arithmetic)
inline void householder_tridiag_base(int n, int ld, double* W, double* d, double* e, double* hv, double* tau, double* p, double* w) {
  householder_tridiag_impl(n, ld, W, d, e, hv, tau, p, w);
}
__attribute__((target("avx2"))) inline void householder_tridiag_avx2(int n, int ld, double* W, double* d, double* e, double* hv,
                                                              double* tau, double* p, double* w) {
  householder_tridiag_impl(n, ld, W, d, e, hv, tau, p, w);
}
inline void householder_accumulate_base(int n, int ld, const double* hv, const double* tau, double* Zt, int r0, int r1) {
  householder_accumulate_impl(n, ld, hv, tau, Zt, r0, r1);
}
__attribute__((target("avx2"))) inline void householder_accumulate_avx2(int n, int ld, const double* hv, const double* tau, double* Zt, int r0,
                                                                 int r1) {
  householder_accumulate_impl(n, ld, hv, tau, Zt, r0, r1);
}
inline void apply_rots_base(int n, int ld, double* Zt, const std::vector<PlaneRot>& rots, int k0, int k1) {
  apply_rots_impl(n, ld, Zt, rots, k0, k1);
}
__attribute__((target("avx2"))) inline void apply_rots_avx2(int n, int ld, double* Zt, const std::vector<PlaneRot>& rots, int k0, int k1) {
  apply_rots_impl(n, ld, Zt, rots, k0, k1);
}

inline double pythag(double a, double b) {
  const double r2 = a * a + b * b;
  if (r2 > 1e-280 && r2 < 1e280) return sqrt(r2);
  return hypot(a, b);
}

// implicit-shift QL on the symmetric tridiagonal (d, e[i] = T[i+1, i]): eigenvalues into d (unsorted), the plane
// rotations (acting on vector indices i, i+1) appended to `rots` in the order they have to be applied
inline void tridiag_ql(int n, double* d, double* e, std::vector<PlaneRot>& rots) {
  double f = 0.0, tst1 = 0.0;
  const double eps = 2.220446049250313e-16;
  e[n - 1] = 0.0;
  for (int l = 0; l < n; ++l) {
    tst1 = std::max(tst1, fabs(d[l]) + fabs(e[l]));
    int m = l;
    while (m < n) {
      if (fabs(e[m]) <= eps * tst1) break;
      ++m;
    }
    if (m > l) {
      int iter = 0;
      do {
        ++iter;
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = pythag(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c;
        const double el1 = e[l + 1];
        double s = 0.0, s2 = 0.0;
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = pythag(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          rots.push_back(PlaneRot{i, c, s});
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (fabs(e[l]) > eps * tst1 && iter < 200);
    }
    d[l] = d[l] + f;
    e[l] = 0.0;
  }
}

// Host worker pool of one eigensolve: the Rayleigh-Ritz step has four short parallel sections per round (two b^3
// products, the eigenvector rotations, W = T S); starting fresh threads for each cost as much as their arithmetic.
// run(njobs, fn) calls fn(job) once per job on the workers and the calling thread and returns when all are done.  Which
// thread takes which job varies, the arithmetic of a job does not: every output element belongs to exactly one job.
class HostPool {
 public:
  explicit HostPool(int workers) {
    for (int t = 0; t < workers; ++t) th_.emplace_back([this]() { work(); });
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& x : th_) x.join();
  }
  HostPool(const HostPool&) = delete;
  HostPool& operator=(const HostPool&) = delete;
  int threads() const { return (int)th_.size() + 1; }
  void run(int njobs, const std::function<void(int)>& fn) {
    if (njobs <= 0) return;
    std::unique_lock<std::mutex> lk(mu_);
    job_ = &fn; njobs_ = njobs; next_ = 0; pending_ = njobs; ++gen_;
    lk.unlock();
    cv_.notify_all();
    lk.lock();
    take(lk);
    done_.wait(lk, [&]() { return pending_ == 0; });
    job_ = nullptr;
  }
  // fn(i) for i in [0, n): contiguous chunks of `chunk` rows as jobs
  void rows(int n, int chunk, const std::function<void(int)>& fn) {
    const int nj = (n + chunk - 1) / chunk;
    const std::function<void(int)> job = [&](int j) {
      const int i1 = std::min(n, (j + 1) * chunk);
      for (int i = j * chunk; i < i1; ++i) fn(i);
    };
    run(nj, job);
  }

 private:
  void take(std::unique_lock<std::mutex>& lk) {      // called with the lock held
    while (next_ < njobs_) {
      const int j = next_++;
      const std::function<void(int)>* f = job_;
      lk.unlock();
      (*f)(j);
      lk.lock();
      if (--pending_ == 0) done_.notify_all();
    }
  }
  void work() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&]() { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      take(lk);
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* job_ = nullptr;
  int njobs_ = 0, next_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// CPUs this process may run on: its affinity mask (what a container or a batch system grants; hardware_concurrency may
// report the whole machine), and no more than OMP_NUM_THREADS where the launcher sets it.
inline int host_cpus_granted() {
  unsigned cpus = std::thread::hardware_concurrency();
#ifdef __linux__
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) cpus = (unsigned)CPU_COUNT(&set);
#endif
  if (const char* e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) cpus = std::min<unsigned>(cpus ? cpus : (unsigned)v, (unsigned)v);
  }
  return (int)std::max(1u, cpus);
}

// Workers beside the calling thread for a b x b host step: up to 8 threads for b <= 256 (the sections are short: more threads
// cost more to wake than they do), up to 16 for the wider blocks, whose b^3 sections are 8 x longer.  The result does not
// depend on the count.
inline int host_pool_workers(int b = 0) {
  return std::min(host_cpus_granted(), b > 256 ? 16 : 8) - 1;
}

// Gn (b x b, unit diagonal, symmetric positive definite) = C C^T; T = D C^-T (b x b) so that
// T^T (D^-1 Gn D^-1) T = I.  False when a pivot falls under 1e-10 (relative to the unit diagonal): the caller
// then needs the rank-revealing path.
inline bool cholesky_whiten(int b, const std::vector<double>& Gn, const std::vector<double>& dg, std::vector<double>& T) {
  // every inner loop walks rows: the dot products with four interleaved partial sums (a single running sum is a chain of
  // dependent adds), the inverse row by row as axpys
  std::vector<double> C((size_t)b * b, 0.0);
  for (int i = 0; i < b; ++i) {
    double* ci = &C[(size_t)i * b];
    for (int j = 0; j < i; ++j) {
      const double* cj = &C[(size_t)j * b];
      ci[j] = (Gn[(size_t)i * b + j] - dot4(ci, cj, j)) / cj[j];
    }
    const double s = Gn[(size_t)i * b + i] - dot4(ci, ci, i);
    if (!(s > 1e-10)) return false;
    ci[i] = sqrt(s);
  }
  // Ci = C^-1 (lower): row i = (e_i - sum_{k < i} C[i][k] Ci[k][:]) / C[i][i]
  std::vector<double> Ci((size_t)b * b, 0.0);
  for (int i = 0; i < b; ++i) {
    double* __restrict__ ri = &Ci[(size_t)i * b];
    const double* ci = &C[(size_t)i * b];
    for (int k = 0; k < i; ++k) {
      const double c = ci[k];
      const double* __restrict__ rk = &Ci[(size_t)k * b];
      for (int j = 0; j <= k; ++j) ri[j] -= c * rk[j];
    }
    const double inv = 1.0 / ci[i];
    for (int j = 0; j < i; ++j) ri[j] *= inv;
    ri[i] = inv;
  }
  // T = D C^-T (upper triangular): T[i][j] = dg[i] * Ci[j][i]
  T.assign((size_t)b * b, 0.0);
  for (int i = 0; i < b; ++i)
    for (int j = i; j < b; ++j) T[(size_t)i * b + j] = dg[i] * Ci[(size_t)j * b + i];
  return true;
}

inline void host_symeigh(int n, std::vector<double>& A, std::vector<double>& evals, std::vector<double>& V, HostPool* pool = nullptr) {
  // Padded leading dimension: with ld = n a power-of-two n (block sizes 128, 256) maps the rows of a column slice onto
  // a handful of L1 sets of the host CPU.
  evals.resize(n);
  V.assign((size_t)n * n, 0.0);
  if (n == 1) { evals[0] = A[0]; V[0] = 1.0; return; }
  const int ld = (n + 7) / 8 * 8 + 8;
  std::vector<double> W((size_t)n * ld), hv((size_t)n * ld, 0.0), Zt((size_t)n * ld), d(n), e(n), tau(n, 0.0), p(n, 0.0), w(n);
  for (int i = 0; i < n; ++i)      // use the symmetric part
    for (int j = 0; j <= i; ++j) W[(size_t)i * ld + j] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
  const bool avx2 = __builtin_cpu_supports("avx2");
  (avx2 ? householder_tridiag_avx2 : householder_tridiag_base)(n, ld, W.data(), d.data(), e.data(), hv.data(), tau.data(),
                                                               p.data(), w.data());
  auto accumulate = avx2 ? householder_accumulate_avx2 : householder_accumulate_base;
  if (pool && n >= 64) {
    // later rows pass through more reflectors: jobs of 8 rows, taken in turn by whoever is free
    const int nj = (n + 7) / 8;
    pool->run(nj, [&](int j) { accumulate(n, ld, hv.data(), tau.data(), Zt.data(), j * 8, std::min(n, j * 8 + 8)); });
  } else {
    accumulate(n, ld, hv.data(), tau.data(), Zt.data(), 0, n);
  }
  std::vector<PlaneRot> rots;
  rots.reserve((size_t)n * n);
  tridiag_ql(n, d.data(), e.data(), rots);
  auto apply = avx2 ? apply_rots_avx2 : apply_rots_base;
  // column slices of 32 (the last one takes the remainder); on the caller's pool when there is one
  const int nsl = std::max(1, n / 32);
  auto slice = [&](int t) {
    const int k0 = t * 32, k1 = t + 1 == nsl ? n : (t + 1) * 32;
    apply(n, ld, Zt.data(), rots, k0, k1);
  };
  if (nsl == 1) {
    slice(0);
  } else if (pool) {
    pool->run(nsl, slice);
  } else {
    for (int q = 0; q < nsl; ++q) slice(q);
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
  for (int j = 0; j < n; ++j) {
    evals[j] = d[order[j]];
    const double* z = &Zt[(size_t)order[j] * ld];
    for (int k = 0; k < n; ++k) V[(size_t)k * n + j] = z[k];
  }
}

// symmetric tridiagonal (alpha[k], beta[k-1]) eigenvalues + first components of eigenvectors
inline void tridiag_eigh(int k, const std::vector<double>& alpha, const std::vector<double>& beta, std::vector<double>& evals,
                  std::vector<double>& evecs) {
  std::vector<double> T((size_t)k * k, 0.0);
  for (int i = 0; i < k; ++i) {
    T[(size_t)i * k + i] = alpha[i];
    if (i + 1 < k) { T[(size_t)i * k + i + 1] = beta[i]; T[(size_t)(i + 1) * k + i] = beta[i]; }
  }
  host_symeigh(k, T, evals, evecs);
}

using HostClock = std::chrono::steady_clock;
inline double host_ms(HostClock::time_point t0, HostClock::time_point t1) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); }

// The host step of a Rayleigh-Ritz round.  In: G = V^T V and H = V^T L V (b x b, fp64, as the Gram kernels leave them).
// Out: kept (the block's numerical rank), the Ritz values th [kept] ascending, and W^T as the rotation kernel takes it
// (float [b x b]: row j = Ritz direction j over the b block columns, rows kept .. b-1 zero) with theta [b] beside it; ms: the
// four phases (whitening, the two products, eigh, W) for the trace.  rank_tol: directions of the Gram block under rank_tol of
// its largest eigenvalue are dropped; cholesky: try the triangular whitening first.  False on a non-positive or non-finite
// Gram diagonal: the block is unusable.
struct RitzStep {
  int kept = 0;
  std::vector<double> th;
  std::vector<float> wt, thf;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
};

inline bool rayleigh_ritz_host(int b, const std::vector<double>& G, const std::vector<double>& H, HostPool& pool, RitzStep& out,
                               double rank_tol = 1e-10, bool cholesky = true) {
  const auto tp0 = HostClock::now();
  std::vector<double> dg(b);
  for (int i = 0; i < b; ++i) {
    const double g = G[(size_t)i * b + i];
    if (!(g > 0.0) || !std::isfinite(g)) return false;
    dg[i] = 1.0 / sqrt(g);
  }
  std::vector<double> Gn((size_t)b * b);
  for (int i = 0; i < b; ++i)
    for (int j = 0; j < b; ++j) Gn[(size_t)i * b + j] = 0.5 * (G[(size_t)i * b + j] + G[(size_t)j * b + i]) * dg[i] * dg[j];
  // whitening T (b x kept) with T^T G T = I: Cholesky Gn = C C^T, T = D C^-T (0.2 ms); a block that has
  // (nearly) dependent columns -- pivot ratio under 1e-5, i.e. cond(Gn) ~ 1e10 -- takes the rank-revealing
  // eigendecomposition instead (3 ms) and drops the dependent directions
  std::vector<double> T, lam, U, S;
  bool tri = true;
  int kept = b;
  if (!cholesky || !cholesky_whiten(b, Gn, dg, T)) {
    tri = false;
    host_symeigh(b, Gn, lam, U, &pool);
    const double lmax = lam[b - 1];
    int k0 = 0;
    while (k0 < b && lam[k0] <= rank_tol * lmax) ++k0;
    kept = b - k0;
    if (kept < 1) return false;
    // T = D U[:, k0:] Lambda^-1/2   (b x kept)
    T.assign((size_t)b * kept, 0.0);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < kept; ++j) T[(size_t)i * kept + j] = dg[i] * U[(size_t)i * b + k0 + j] / sqrt(lam[k0 + j]);
  }
  const auto tp1 = HostClock::now();
  // Hp = T^T Hs T   (rows of the outputs are independent: jobs of 8 rows on the pool, fixed order inside).  After the
  // Cholesky whitening T is upper triangular (tri): T[l][j] = 0 for j < l, which leaves 1/2 and 1/3 of the two products.
  std::vector<double> HT((size_t)b * kept, 0.0), Hp((size_t)kept * kept, 0.0);
  pool.rows(b, 8, [&](int i) {
    double* __restrict__ o = &HT[(size_t)i * kept];
    for (int l = 0; l < b; ++l) {
      const double h = 0.5 * (H[(size_t)i * b + l] + H[(size_t)l * b + i]);
      if (h == 0.0) continue;
      const double* __restrict__ t = &T[(size_t)l * kept];
      for (int j = tri ? l : 0; j < kept; ++j) o[j] += h * t[j];
    }
  });
  pool.rows(kept, 8, [&](int j) {
    double* __restrict__ o = &Hp[(size_t)j * kept];
    const int i1 = tri ? j + 1 : b;
    for (int i = 0; i < i1; ++i) {
      const double t = T[(size_t)i * kept + j];
      const double* __restrict__ h = &HT[(size_t)i * kept];
      for (int l = 0; l < kept; ++l) o[l] += t * h[l];
    }
  });
  const auto tp2 = HostClock::now();
  host_symeigh(kept, Hp, out.th, S, &pool);
  const auto tp3 = HostClock::now();
  // W = T S (b x kept); W^T rows = Ritz directions, zero-padded to b
  out.wt.assign((size_t)b * b, 0.f);
  std::vector<float>& wt = out.wt;
  pool.rows(b, 8, [&](int i) {
    std::vector<double> acc(kept, 0.0);
    for (int l = tri ? i : 0; l < kept; ++l) {
      const double t = T[(size_t)i * kept + l];
      const double* __restrict__ sr = &S[(size_t)l * kept];
      for (int j = 0; j < kept; ++j) acc[j] += t * sr[j];
    }
    for (int j = 0; j < kept; ++j) wt[(size_t)j * b + i] = (float)acc[j];
  });
  out.thf.resize(b);
  for (int j = 0; j < b; ++j) out.thf[j] = j < kept ? (float)out.th[j] : 0.f;
  out.kept = kept;
  out.ms[0] = host_ms(tp0, tp1); out.ms[1] = host_ms(tp1, tp2); out.ms[2] = host_ms(tp2, tp3); out.ms[3] = host_ms(tp3, HostClock::now());
  return true;
}

// largest Ritz value of (H, G) on the leading k of kfull basis vectors (G = K^T K, H = K^T L K, fp64): the same step serially,
// always by the rank-revealing whitening (directions under 1e-6 of the largest Gram eigenvalue are rounding of the fp32
// vectors).  NaN when the Gram block is unusable.
inline double top_ritz(int kfull, int k, const std::vector<double>& G, const std::vector<double>& H) {
  std::vector<double> g((size_t)k * k), h((size_t)k * k);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) { g[(size_t)i * k + j] = G[(size_t)i * kfull + j]; h[(size_t)i * k + j] = H[(size_t)i * kfull + j]; }
  HostPool serial(0);
  RitzStep r;
  return rayleigh_ritz_host(k, g, h, serial, r, 1e-6, false) ? r.th[r.kept - 1] : NAN;
}
