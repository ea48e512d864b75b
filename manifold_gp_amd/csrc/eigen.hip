// Eigensolve for the m smallest eigenpairs of the symmetric graph Laplacian, and the k-step
// Lanczos tridiagonalisation of a precision-family operator.
//
// Replaces torch.linalg.eigh on the densified N x N matrix (manifold_gp/kernels/riemann_kernel.py:
// 121-125, O(N^3) and 14 GB at N = 60k) and GraphLaplacianOperator.diagonalization
// (manifold_gp/operators/graph_laplacian_operator.py:132-144; its Lanczos branch is
// linear_operator's lanczos_tridiag with full re-orthogonalisation).
//
// mgp_lanczos_smallest: Chebyshev-filtered block Krylov iteration with Rayleigh-Ritz
//   The low end of a graph-Laplacian spectrum is clustered and, for a k-NN graph with several
//   connected components, degenerate; single-vector Lanczos needs thousands of steps there and
//   misses multiplicities (the reference itself abandoned its Lanczos call for dense eigh,
//   riemann_kernel.py:120).  So: (1) Gershgorin gives a safe upper bound ub of the spectrum (the norm the
//   residual test is relative to) and a 32-dimensional Krylov space a tight one, ubf ~ 1.03 lambda_max -- about half
//   of Gershgorin on k-NN graph Laplacians, checked against the Ritz values of every round, Gershgorin as fallback,
//   (2) a block of b = m + pad vectors is filtered by a scaled Chebyshev polynomial of L that
//   damps [a, ubf] (a = largest Ritz value of the previous round) -- d fused SpMM launches, the
//   matrix is streamed once per launch for all b columns, (3) Rayleigh-Ritz in the filtered
//   block: Gram matrices V^T V, V^T L V accumulated in fp64 on device, b x b generalized
//   eigenproblem in fp64 on the host (Householder + QL on a worker pool), rotation V <- V W on the fp32
//   MFMA kernel, (4) residuals ||L v - theta v|| <= tol ub decide convergence.
//
// mgp_lanczos_tridiag: q_{j+1} beta_j = A q_j - alpha_j q_j - beta_{j-1} q_{j-1} with classical
//   Gram-Schmidt against ALL previous vectors, twice; alpha/beta stay on device until the end.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <cstdio>
#include <atomic>
#include "mgp_common.h"
#include "mgp_internal.h"
#include "eig_host.h"
#include "eig_policy.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------- small kernels
__global__ void gershgorin_kernel(int64_t n, const int32_t* __restrict__ rowptr, const float* __restrict__ vals,
                                  const float* __restrict__ diag, float* __restrict__ block_max) {
  __shared__ float sh[kBlock];
  float mx = 0.f;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    float s = fabsf(diag[r]);
    for (int i = rowptr[r]; i < rowptr[r + 1]; ++i) s += fabsf(vals[i]);
    mx = fmaxf(mx, s);
  }
  sh[threadIdx.x] = mx;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) block_max[blockIdx.x] = sh[0];
}

__device__ __forceinline__ uint32_t hash32(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
  return (uint32_t)x;
}

// V[r, c0:c1) = uniform(-1, 1), counter-based (reproducible for a seed)
__global__ void random_cols_kernel(float* __restrict__ V, int64_t n, int ld, int c0, int c1, uint64_t seed) {
  const int w = c1 - c0;
  const int64_t total = n * w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / w;
    const int c = c0 + (int)(i % w);
    const uint32_t h = hash32(seed * 0x9E3779B97F4A7C15ULL + (uint64_t)r * 1315423911ULL + (uint64_t)c * 2654435761ULL + 12345);
    V[r * ld + c] = (float)h * (2.0f / 4294967296.0f) - 1.0f;
  }
}

// partial[chunk][i][j] = sum_{r in chunk} A[r,i] * B[r,j], fp64 accumulation, 64 x 64 tile per block
__global__ __launch_bounds__(kBlock) void gram_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                      int64_t n, int b, int64_t rows_per_chunk,
                                                      double* __restrict__ partial) {
  __shared__ float As[16][64 + 1];
  __shared__ float Bs[16][64 + 1];
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.z * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;   // outputs i = ti*64 + ty*4 + a, j = tj*64 + tx*4 + c
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  for (int64_t rr = r0; rr < r1; rr += 16) {
    for (int e = threadIdx.x; e < 16 * 64; e += kBlock) {
      const int lr = e >> 6, lc = e & 63;
      const int64_t r = rr + lr;
      const int ci = ti * 64 + lc, cj = tj * 64 + lc;
      As[lr][lc] = (r < r1 && ci < b) ? A[r * b + ci] : 0.f;
      Bs[lr][lc] = (r < r1 && cj < b) ? B[r * b + cj] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int lr = 0; lr < 16; ++lr) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = (double)As[lr][ty * 4 + a];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = (double)Bs[lr][tx * 4 + c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fma(av[a], bv[c], acc[a][c]);
    }
    __syncthreads();
  }
  double* out = partial + (int64_t)blockIdx.z * b * b;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = ti * 64 + ty * 4 + a, j = tj * 64 + tx * 4 + c;
      if (i < b && j < b) out[(int64_t)i * b + j] = acc[a][c];
    }
}

// The same partial Gram blocks on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: exact products of the converted fp32 entries,
// fp64 accumulation): same 64 x 64 tile per block and 16-row LDS stages as gram_kernel; a wave owns 32 x 32 of the tile as
// 2 x 2 MFMA tiles and per four rows reads two A^T and two B operands from LDS (lane (i, k) = As[row k][col i]: conflict
// free), converts them and issues four MFMAs -- 16 MFMAs per stage where the vector form issues 256 DFMAs and 128 converts.
using f64x4 = __attribute__((ext_vector_type(4))) double;
__global__ __launch_bounds__(kBlock) void gram_mfma_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                           int64_t n, int b, int64_t rows_per_chunk,
                                                           double* __restrict__ partial) {
  // Staging (round 5, second half): 32 rows x 64 columns of A and of B per stage, one 16-byte global load per thread, item and
  // matrix (8 scalar loads per stage of 16 rows before), requested a stage ahead into registers and written to LDS behind the
  // barrier; rows padded to 80 floats: the four k-groups of a ds_read_b32 (lanes 16 apart read rows one apart) then fall 16 banks
  // apart (65 floats: one bank apart, SQ_LDS_BANK_CONFLICT 40 % of the LDS cycles).  Half the barriers per row of the chunk.
  constexpr int kGR = 32, kGP = 64 + 16;
  __shared__ __attribute__((aligned(16))) float As[kGR][kGP];
  __shared__ __attribute__((aligned(16))) float Bs[kGR][kGP];
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.z * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, kq = lane >> 4;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = f64x4{0.0, 0.0, 0.0, 0.0};
  // thread -> (row lr, 4 columns from lc) of the stage, two such items per thread and matrix (32 x 64 floats = 512 float4)
  const bool vec = (b & 3) == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
  float4 pa[2], pb[2];
  auto fetch = [&](int64_t rr) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = threadIdx.x + u * kBlock;
      const int lr = e >> 4, lc = (e & 15) * 4;
      const int64_t r = rr + lr;
      const int ci = ti * 64 + lc, cj = tj * 64 + lc;
      pa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      pb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < r1) {
        if (vec && ci + 3 < b) pa[u] = *reinterpret_cast<const float4*>(A + r * b + ci);
        else {
          if (ci < b) pa[u].x = A[r * b + ci];
          if (ci + 1 < b) pa[u].y = A[r * b + ci + 1];
          if (ci + 2 < b) pa[u].z = A[r * b + ci + 2];
          if (ci + 3 < b) pa[u].w = A[r * b + ci + 3];
        }
        if (vec && cj + 3 < b) pb[u] = *reinterpret_cast<const float4*>(B + r * b + cj);
        else {
          if (cj < b) pb[u].x = B[r * b + cj];
          if (cj + 1 < b) pb[u].y = B[r * b + cj + 1];
          if (cj + 2 < b) pb[u].z = B[r * b + cj + 2];
          if (cj + 3 < b) pb[u].w = B[r * b + cj + 3];
        }
      }
    }
  };
  if (r0 < r1) fetch(r0);
  for (int64_t rr = r0; rr < r1; rr += kGR) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = threadIdx.x + u * kBlock;
      const int lr = e >> 4, lc = (e & 15) * 4;
      *reinterpret_cast<float4*>(&As[lr][lc]) = pa[u];
      *reinterpret_cast<float4*>(&Bs[lr][lc]) = pb[u];
    }
    __syncthreads();
    if (rr + kGR < r1) fetch(rr + kGR);            // the next stage's rows are in flight during this stage's MFMAs
#pragma unroll
    for (int k0 = 0; k0 < kGR; k0 += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) av[a] = (double)As[k0 + kq][wi + 16 * a + l16];
#pragma unroll
      for (int c = 0; c < 2; ++c) bv[c] = (double)Bs[k0 + kq][wj + 16 * c + l16];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[c], acc[a][c], 0, 0, 0);
    }
    __syncthreads();
  }
  // acc[a][c][r]: row i = wi + 16 a + 4 r + kq, column j = wj + 16 c + l16 of the tile (the f64 16x16x4 result interleaves the
  // four k-groups of lanes over the rows: register r of lane group kq is row 4 r + kq -- not the f32 layout's 4 kq + r;
  // found with tools/lab/dbg_gram.py)
  double* out = partial + (int64_t)blockIdx.z * b * b;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 64 + wi + 16 * a + 4 * r + kq, j = tj * 64 + wj + 16 * c + l16;
        if (i < b && j < b) out[(int64_t)i * b + j] = acc[a][c][r];
      }
}

__global__ void gram_reduce_kernel(const double* __restrict__ partial, int chunks, int bb, double* __restrict__ G) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < bb; i += gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[(int64_t)c * bb + i];
    G[i] = s;
  }
}

// column partial sums of (LV[r,c] - theta[c] * V[r,c])^2 in fp64.  blockIdx.y: the group of kBlock columns (one group up to
// b = 256; a wider block's last group may be narrower and then takes several row slices per column, like a narrow block)
__global__ __launch_bounds__(kBlock) void residual_kernel(const float* __restrict__ LV, const float* __restrict__ V,
                                                          const float* __restrict__ theta, int64_t n, int b,
                                                          int64_t rows_per_chunk, double* __restrict__ partial) {
  __shared__ double sh[kBlock];
  const int cb = blockIdx.y * kBlock, bw = min(b - cb, kBlock);
  int TC = 1;
  while (TC < bw && TC < kBlock) TC <<= 1;
  const int TS = kBlock / TC;
  const int cc = threadIdx.x % TC, sl = threadIdx.x / TC;
  const int64_t r0 = blockIdx.x * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  double acc = 0.0;
  if (cc < bw) {
    const float th = theta[cb + cc];
    for (int64_t r = r0 + sl; r < r1; r += TS) {
      const float d = LV[r * b + cb + cc] - th * V[r * b + cb + cc];
      acc += (double)d * (double)d;
    }
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (sl == 0 && cc < bw) {
    double t = 0.0;
    for (int s = 0; s < TS; ++s) t += sh[s * TC + cc];
    partial[(int64_t)blockIdx.x * b + cb + cc] = t;
  }
}

// dst[r, dc0 + j] = src[r, sc0 + j], j < m  (column sub-blocks between row-major blocks of different widths)
__global__ void move_cols_kernel(const float* __restrict__ src, int64_t n, int sld, int sc0, int m, float* __restrict__ dst,
                                 int dld, int dc0) {
  const int64_t total = n * m;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    dst[(i / m) * dld + dc0 + (i % m)] = src[(i / m) * sld + sc0 + (i % m)];
}

__global__ void copy_cols_kernel(const float* __restrict__ V, int64_t n, int ld, int m, float* __restrict__ out) {
  const int64_t total = n * m;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = V[(i / m) * ld + (i % m)];
}

// K[r, j] = KT[j, r] for kk <= 64 vectors of length n kept one after the other (the Krylov vectors of the lambda_max estimate: each is
// written in place by its SpMV launch; one transpose instead of a strided column copy behind every launch)
__global__ __launch_bounds__(256) void vecs_to_cols_kernel(const float* __restrict__ KT, int64_t n, int kk, float* __restrict__ K) {
  __shared__ float tile[64][64 + 1];
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  for (int e = threadIdx.x; e < 64 * kk; e += 256) {
    const int j = e >> 6, lr = e & 63;
    tile[j][lr] = r0 + lr < n ? KT[(int64_t)j * n + r0 + lr] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * kk; e += 256) {
    const int lr = e / kk, j = e - lr * kk;
    if (r0 + lr < n) K[(r0 + lr) * kk + j] = tile[j][lr];
  }
}

std::atomic<int> g_eig_bound_mode{1};   // 1: the filter's upper end from a Krylov estimate of lambda_max; 0: Gershgorin;
                            // 2 (tests): HALF the estimate, a bound that is certainly short -- the fallback must catch it

struct EigWork {
  float* buf[5];
  double* gpart;
  double* G;
  double* H;
  double* rpart;
  float* wt;        // W^T upload [b x b]
  float* theta;     // [b]
  float* bmax;      // gershgorin partials
  void* opwork;
  size_t opwork_bytes;
  int chunks;
  int64_t rows_per_chunk;
  int rchunks;
  int64_t rrows;
};

int block_size_for(int m, const mgp_lanczos_params_t* p) {
  // The SpMM's cost steps with every 64 columns (one more accumulator per lane), the host side grows with b^3 and,
  // with filter degrees up to 200, a handful of guard vectors is enough: the next multiple of 64 above
  // m + max(m / 8, 12).  Measured at N = 60k, m = 100 (degree cap 200): 112 columns 47 ms, 128: 49 ms, 136: 67 ms,
  // 160: 65 ms, 192: 94 ms; N = 1M, m = 50: 64 columns 0.69 s, 96: 0.82 s, 128: 0.94 s.  (With the degree capped
  // at 80 the same sweep preferred ~2 m columns and took 138 ms / 0.84 s.)
  int b = (p && p->max_basis > 0) ? p->max_basis : m + std::max(m / 8, 12);
  if (b < m + 2) b = m + 2;
  // (Until blocks wider than one SpMM launch ran in column chunks, m = 229 .. 254 was clamped to 256 columns -- fewer guards than
  // the rule asks for -- so as to run at all; such m now gets its 320 columns.  Blocks above kEigMaxBlock are refused by the solve.)
  if (!(p && p->max_basis > 0)) b = (b + 63) / 64 * 64;
  return b;
}

void chunking(int64_t n, int* chunks, int64_t* rpc, int max_chunks, int64_t min_rows) {
  int64_t r = std::max<int64_t>(min_rows, mgp_cdiv(mgp_cdiv(n, max_chunks), 16) * 16);
  *rpc = r;
  *chunks = (int)mgp_cdiv(n, r);
}

size_t eig_bytes(int64_t n, int m, const mgp_lanczos_params_t* p) {
  const int b = block_size_for(m, p);
  int chunks, rch; int64_t rpc, rr;
  chunking(n, &chunks, &rpc, 96, 512);
  chunking(n, &rch, &rr, 256, 256);
  size_t s = 5 * mgp_align((size_t)n * b * sizeof(float));
  s += mgp_align((size_t)chunks * b * b * sizeof(double));
  s += 2 * mgp_align((size_t)b * b * sizeof(double));
  s += mgp_align((size_t)rch * b * sizeof(double));
  s += mgp_align((size_t)b * b * sizeof(float)) + mgp_align(b * sizeof(float)) + mgp_align(1024 * sizeof(float));
  return s + 4096;
}

// 1 (default): the partial Gram blocks on the fp64 matrix cores; 0: fp64 vector FMAs (mgp_gram_set_mfma: A/B, tests)
std::atomic<int> g_gram_mfma{1};

int launch_gram(const float* A, const float* B, int64_t n, int b, EigWork& w, double* out, hipStream_t st) {
  dim3 grid((unsigned)mgp_cdiv(b, 64), (unsigned)mgp_cdiv(b, 64), (unsigned)w.chunks);
  if (g_gram_mfma) hipLaunchKernelGGL(gram_mfma_kernel, grid, dim3(kBlock), 0, st, A, B, n, b, w.rows_per_chunk, w.gpart);
  else hipLaunchKernelGGL(gram_kernel, grid, dim3(kBlock), 0, st, A, B, n, b, w.rows_per_chunk, w.gpart);
  MGP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)mgp_cdiv((int64_t)b * b, kBlock)), dim3(kBlock), 0, st, w.gpart,
                     w.chunks, b * b, out);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

}  // namespace

// ================================================================= the driver of mgp_lanczos_smallest
// validate -> carve the workspace -> spectrum bounds -> start block -> rounds { filter, Rayleigh-Ritz + rotation, policy step }
// -> outputs.  The host algebra of a round is eig_host.h, every decision between the launches eig_policy.h.
namespace {

// One call's state.  user_degree > 0: every round runs at it; trace: MGP_EIG_TIMING, read once per call; lab: lab builds
// (-DMGP_LAB_EIG) take a fixed damping exponent for every round from MGP_EIG_TARGET.  bV / bLV: the buffers that hold the current
// block V and L V (full width b); c0 .. c2: the three more that serve the filter.  rr: kept, Ritz values and W^T of the last
// Rayleigh-Ritz step; tr0 / tr1: start of the round / everything of it queued.
struct EigCtx {
  const mgp_csr_t* L;
  void* stream;
  hipStream_t st;
  int64_t n;
  int m, b, user_degree;
  uint64_t seed;
  double tol, lab_target;
  bool trace, lab, floor_hit;
  EigWork w;
  int bV, bLV, c0, c1, c2, rounds, nspmm, nconv, deg_used;
  EigPolicy pol;
  HostPool* pool;
  std::vector<double> G, H, rp, res;
  RitzStep rr;
  HostClock::time_point tr0, tr1;
  float *evals, *evecs, *resid, *block_evals, *block_evecs, *block_resid;     // the caller's outputs
};

int eig_setup(EigCtx& cx, const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, void* work, size_t work_bytes, void* stream) {
  if (!L || !L->rowptr || !L->col || !L->vals || !L->diag || !cx.evals || !cx.evecs || !work) return MGP_ERR_ARG;
  if (!mgp_spmv_lanes_ok(L->spmv_lanes)) return MGP_ERR_ARG;
  const int64_t n = L->n;
  if (n <= 0 || m <= 0 || m > n) return MGP_ERR_ARG;
  int b = block_size_for(m, p);
  if (b > n) b = (int)n;
  if (b > kEigMaxBlock) return MGP_ERR_UNSUPPORTED;   // block products run in chunks of <= 256 columns up to this width; beyond it:
                                                      // hard-locked sweeps (docs/kernels/eigen.md), not built
  if (work_bytes < eig_bytes(n, m, p)) return MGP_ERR_WORKSPACE;
  cx.L = L; cx.stream = stream; cx.st = mgp_stream(stream); cx.n = n; cx.m = m; cx.b = b;
  cx.seed = p ? p->seed : 1337;
  cx.tol = (p && p->tol > 0.f) ? p->tol : 1e-5f;
  cx.user_degree = (p && p->degree > 0) ? p->degree : 0;
  cx.trace = getenv("MGP_EIG_TIMING") != nullptr;
  cx.lab = false;
#ifdef MGP_LAB_EIG
  if (const char* e = getenv("MGP_EIG_TARGET")) { cx.lab = true; cx.lab_target = atof(e); }
#endif
  EigWork& w = cx.w;
  MgpArena ar(work, work_bytes);
  for (int i = 0; i < 5; ++i) w.buf[i] = ar.take<float>((size_t)n * b);
  chunking(n, &w.chunks, &w.rows_per_chunk, 96, 512);
  chunking(n, &w.rchunks, &w.rrows, 256, 256);
  w.gpart = ar.take<double>((size_t)w.chunks * b * b);
  w.G = ar.take<double>((size_t)b * b);
  w.H = ar.take<double>((size_t)b * b);
  w.rpart = ar.take<double>((size_t)w.rchunks * b);
  w.wt = ar.take<float>((size_t)b * b);
  w.theta = ar.take<float>(b);
  w.bmax = ar.take<float>(1024);
  if (!ar.ok()) return MGP_ERR_WORKSPACE;
  cx.G.resize((size_t)b * b); cx.H.resize((size_t)b * b); cx.rp.resize((size_t)w.rchunks * b);
  return MGP_OK;
}

// Y = ca X + cl L X (+ cz Z) on C <= 256 columns: one fused SpMM launch
int eig_apply(EigCtx& cx, const float* X, int C, float* Y, double ca, double cl, const float* Z = nullptr, double cz = 0.0) {
  return mgp_spmm_fused(cx.L, X, C, Y, (float)ca, (float)cl, nullptr, nullptr, Z, (float)cz, 1.f, nullptr, nullptr, cx.stream);
}

// Spectrum bounds -- ub: Gershgorin, always >= lambda_max; ubf: the filter's upper end -- and the cold policy on them.
int eig_bounds(EigCtx& cx) {
  const mgp_csr_t* L = cx.L;
  const int64_t n = cx.n;
  EigWork& w = cx.w;
  hipStream_t st = cx.st;
  const int gb = (int)std::min<int64_t>(1024, mgp_cdiv(n, kBlock));
  hipLaunchKernelGGL(gershgorin_kernel, dim3(gb), dim3(kBlock), 0, st, n, L->rowptr, L->vals, L->diag, w.bmax);
  MGP_LAUNCH_CHECK();
  std::vector<float> hb(gb);
  MGP_HIP_TRY(hipMemcpyAsync(hb.data(), w.bmax, gb * sizeof(float), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipStreamSynchronize(st));
  double ub = 0.0;
  for (float v : hb) ub = std::max(ub, (double)v);
  ub *= 1.0 + 1e-6;
  if (!(ub > 0.0)) return MGP_ERR_ARG;

  // ---- the filter's upper end.  Gershgorin is rigorous and loose: on the k-NN graph Laplacians of this package lambda_max
  // is about HALF of it (60k RMNIST-like graph: 15.4 of 29.7; 1M swiss roll: 649 of 1239), and the degree a Chebyshev filter
  // needs grows with sqrt(ub - a) -- a bound twice too large costs 40 % more applies.  So: a 32-dimensional Krylov space of
  // one random vector in the Chebyshev basis of [0, ub] (the same fused three-term SpMV launches as the filter, C = 1; the
  // basis stays bounded and well conditioned, unlike the monomials), Rayleigh-Ritz with the Gram kernels, the largest
  // Ritz value theta_32 <= lambda_max; the filter gets theta_32 + max(3 %, twice what the last 16 dimensions still moved).
  // The residual test keeps the Gershgorin bound as its norm of L, so `tol` means what it meant.  An estimate that fell
  // short would let the filter AMPLIFY the top of the spectrum; that shows as a Ritz value above the supposed bound in
  // the next Rayleigh-Ritz step and is answered there (Gershgorin, fresh block).
  double ubf = ub;
  const int kk = 32;
  const int bound_mode = g_eig_bound_mode;      // (lab switch: read once per call)
  if (bound_mode && cx.b >= kk && n >= 8 * kk) {
    float* K = w.buf[0];
    float* LK = w.buf[1];
    float* KT = w.buf[2];          // the kk Krylov vectors one after the other (b >= kk columns of room): vector j at KT + j n
    const int g1 = (int)std::min<int64_t>(4096, mgp_cdiv(n, kBlock));
    hipLaunchKernelGGL(random_cols_kernel, dim3(g1), dim3(kBlock), 0, st, KT, n, 1, 0, 1, cx.seed ^ 0x5bd1e995ULL);
    MGP_LAUNCH_CHECK();
    const double ce = ub / 2.0;     // centre = half width of [0, ub]
    // T_1 = (L - c) / e
    MGP_TRY(eig_apply(cx, KT, 1, KT + n, -1.0, 1.0 / ce));
    for (int j = 2; j < kk; ++j) {
      // T_j = 2 (L - c) / e T_{j-1} - T_{j-2}, written where it stays (round 5: no column copy behind every launch)
      MGP_TRY(eig_apply(cx, KT + (int64_t)(j - 1) * n, 1, KT + (int64_t)j * n, -2.0, 2.0 / ce, KT + (int64_t)(j - 2) * n, -1.0));
    }
    hipLaunchKernelGGL(vecs_to_cols_kernel, dim3((unsigned)mgp_cdiv(n, 64)), dim3(256), 0, st, KT, n, kk, K);
    MGP_LAUNCH_CHECK();
    MGP_TRY(eig_apply(cx, K, kk, LK, 0.0, 1.0));
    MGP_TRY(launch_gram(K, K, n, kk, w, w.G, st));
    MGP_TRY(launch_gram(K, LK, n, kk, w, w.H, st));
    std::vector<double> Gk((size_t)kk * kk), Hk((size_t)kk * kk);
    MGP_HIP_TRY(hipMemcpyAsync(Gk.data(), w.G, (size_t)kk * kk * sizeof(double), hipMemcpyDeviceToHost, st));
    MGP_HIP_TRY(hipMemcpyAsync(Hk.data(), w.H, (size_t)kk * kk * sizeof(double), hipMemcpyDeviceToHost, st));
    MGP_HIP_TRY(hipStreamSynchronize(st));
    const double th_full = top_ritz(kk, kk, Gk, Hk), th_half = top_ritz(kk, kk / 2, Gk, Hk);
    if (std::isfinite(th_full) && std::isfinite(th_half) && th_full > 0.0) {
      const double cand = th_full + std::max(0.03 * th_full, 2.0 * fabs(th_full - th_half));
      if (cand < ub) ubf = cand;
      if (bound_mode == 2) ubf = 0.5 * th_full;
    }
    if (cx.trace)
      fprintf(stderr, "[eig] upper end: Gershgorin %.5g, Krylov(32) theta %.5g (16: %.5g) -> filter bound %.5g\n", ub, th_full, th_half, ubf);
  }
  cx.pol = eig_cold_start(ub, ubf, cx.user_degree);
  return MGP_OK;
}

// V[:, c0:c1) <- fresh random columns
int eig_random_cols(EigCtx& cx, float* V, int c0, int c1, uint64_t seed) {
  const int rgrid = (int)std::min<int64_t>(4096, mgp_cdiv(cx.n * cx.b, kBlock));
  hipLaunchKernelGGL(random_cols_kernel, dim3(rgrid), dim3(kBlock), 0, cx.st, V, cx.n, cx.b, c0, c1, seed);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

void eig_move_cols(EigCtx& cx, const float* src, int sld, int sc0, int mcols, float* dst, int dld, int dc0) {
  const int grid = (int)std::min<int64_t>(4096, mgp_cdiv(cx.n * mcols, kBlock));
  hipLaunchKernelGGL(move_cols_kernel, dim3(grid), dim3(kBlock), 0, cx.st, src, cx.n, sld, sc0, mcols, dst, dld, dc0);
}

// Scaled Chebyshev filter of degree pol.deg damping [a, ubf], normalised at a0, on the active columns; then the Gram blocks.
// Soft locking: the leading pol.nlock columns are not filtered -- the recurrence and the L apply run on the remaining `ba`
// columns, compacted to an [n, ba] block -- but stay in the Rayleigh-Ritz basis, so they keep being refined and the block
// stays orthogonal.
// Wide blocks: ba > 256 active columns run as the column chunks of eig_chunk_start, each compacted to its own [n, width] block at
// column offset c0 of the three filter buffers (element offset n c0: 16-byte aligned, c0 is a multiple of 4).  The three-term
// recurrence is column-independent, and each chunk runs its WHOLE degree before the next one starts: the matrix is streamed once
// per launch either way, but the three vector blocks a chunk's recurrence cycles through are half the size of the whole block's
// (60k x 192 x 3: 138 MB against 276 MB), so more of them is still in the last-level cache when the next launch asks for them.
// One chunk (ba <= 256) is the launch sequence there has always been.
int eig_filter_round(EigCtx& cx) {
  EigWork& w = cx.w;
  const int b = cx.b, nlock = cx.pol.nlock, deg = cx.pol.deg;
  cx.tr0 = HostClock::now();
  const int ba = b - nlock;
  cx.deg_used = deg;
  const double e = (cx.pol.ubf - cx.pol.a) / 2.0, c = (cx.pol.ubf + cx.pol.a) / 2.0;
  const int nch = eig_chunk_count(ba);
  for (int k = 0; k < nch; ++k) {
    const int c0 = eig_chunk_start(ba, k), cw = eig_chunk_start(ba, k + 1) - c0;
    const size_t off = (size_t)cx.n * c0;
    double sig = e / (cx.pol.a0 - c);
    const double tau = 2.0 / sig;
    int iX = cx.c0, iY = cx.c1, iN = cx.c2;
    eig_move_cols(cx, w.buf[cx.bV], b, nlock + c0, cw, w.buf[iX] + off, cw, 0);
    MGP_LAUNCH_CHECK();
    if (deg == 0) {      // a block that spans the whole space (eig_whole_space): no filter, only L V behind the unchanged columns
      MGP_TRY(eig_apply(cx, w.buf[iX] + off, cw, w.buf[iN] + off, 0.0, 1.0));
      ++cx.nspmm;
      eig_move_cols(cx, w.buf[iN] + off, cw, 0, cw, w.buf[cx.bLV], b, nlock + c0);
      MGP_LAUNCH_CHECK();
      continue;
    }
    // Y = (sig/e) (L X - c X)
    MGP_TRY(eig_apply(cx, w.buf[iX] + off, cw, w.buf[iY] + off, -c * sig / e, sig / e));
    ++cx.nspmm;
    for (int i = 2; i <= deg; ++i) {
      const double sn = 1.0 / (tau - sig);
      // Ynew = (2 sn / e) (L Y - c Y) - (sig sn) X
      MGP_TRY(eig_apply(cx, w.buf[iY] + off, cw, w.buf[iN] + off, -c * 2.0 * sn / e, 2.0 * sn / e, w.buf[iX] + off, -sig * sn));
      ++cx.nspmm;
      const int t = iX; iX = iY; iY = iN; iN = t;
      sig = sn;
    }
    // filtered active chunk in iY; L (filtered) into iN; both back into the active columns of V / L V
    MGP_TRY(eig_apply(cx, w.buf[iY] + off, cw, w.buf[iN] + off, 0.0, 1.0));
    ++cx.nspmm;
    eig_move_cols(cx, w.buf[iY] + off, cw, 0, cw, w.buf[cx.bV], b, nlock + c0);
    eig_move_cols(cx, w.buf[iN] + off, cw, 0, cw, w.buf[cx.bLV], b, nlock + c0);
    MGP_LAUNCH_CHECK();
  }
  // ---- Rayleigh-Ritz: G = V^T V, H = V^T L V (fp64), generalized eigenproblem on the host
  MGP_TRY(launch_gram(w.buf[cx.bV], w.buf[cx.bV], cx.n, b, w, w.G, cx.st));
  MGP_TRY(launch_gram(w.buf[cx.bV], w.buf[cx.bLV], cx.n, b, w, w.H, cx.st));
  cx.tr1 = HostClock::now();   // everything of this round is queued; the copies of the Rayleigh-Ritz step wait for it
  return MGP_OK;
}

// The Rayleigh-Ritz step on the filtered block: Gram blocks to the host, rayleigh_ritz_host, rotation V <- V W and L V <- L V W
// on the MFMA kernel, residuals into cx.res.  *fresh: the Ritz values proved the estimated bound short -- the policy is back on
// Gershgorin, the block is a fresh random one and nothing was rotated.
int eig_ritz_rotate(EigCtx& cx, bool* fresh) {
  EigWork& w = cx.w;
  const int64_t n = cx.n;
  const int b = cx.b, outer = cx.rounds;
  hipStream_t st = cx.st;
  *fresh = false;
  MGP_HIP_TRY(hipMemcpyAsync(cx.G.data(), w.G, (size_t)b * b * sizeof(double), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipMemcpyAsync(cx.H.data(), w.H, (size_t)b * b * sizeof(double), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipStreamSynchronize(st));
  const auto tp0 = HostClock::now();
  if (!rayleigh_ritz_host(b, cx.G, cx.H, *cx.pool, cx.rr)) return MGP_ERR_NOT_CONVERGED;
  const auto tp4 = HostClock::now();
  const int kept = cx.rr.kept;
  const double top = cx.rr.th[kept - 1];
  if (!cx.pol.whole && eig_bound_short(cx.pol, top)) {      // (an unfiltered round does not use the bound)
    if (cx.trace)
      fprintf(stderr, "[eig] round %d: largest Ritz value %.5g against the estimated bound %.5g: back to Gershgorin %.5g\n", outer,
              top, cx.pol.ubf, cx.pol.ub);
    MGP_TRY(eig_random_cols(cx, w.buf[cx.bV], 0, b, cx.seed + 104729ULL * (outer + 1)));
    cx.pol = eig_cold_start(cx.pol.ub, cx.pol.ub, cx.user_degree);
    *fresh = true;
    return MGP_OK;
  }
  if (cx.trace)
    fprintf(stderr, "[eig] round %d: whiten %.2f  HT/Hp %.2f  eigh(Hp) %.2f  W %.2f ms\n", outer, cx.rr.ms[0], cx.rr.ms[1], cx.rr.ms[2],
            cx.rr.ms[3]);
  MGP_HIP_TRY(hipMemcpyAsync(w.wt, cx.rr.wt.data(), (size_t)b * b * sizeof(float), hipMemcpyHostToDevice, st));
  MGP_HIP_TRY(hipMemcpyAsync(w.theta, cx.rr.thf.data(), b * sizeof(float), hipMemcpyHostToDevice, st));
  // ---- rotate on the MFMA: Vn = V W, LVn = LV W   (K = Z1 Z2^T with Z2 = W^T)
  const int iVn = cx.c0, iLVn = cx.c1;
  MGP_TRY(mgp_kernel_block_ld(w.buf[cx.bV], n, w.wt, b, b, 1.f, w.buf[iVn], b, cx.stream));
  MGP_TRY(mgp_kernel_block_ld(w.buf[cx.bLV], n, w.wt, b, b, 1.f, w.buf[iLVn], b, cx.stream));
  hipLaunchKernelGGL(residual_kernel, dim3(w.rchunks, (unsigned)mgp_cdiv(b, kBlock)), dim3(kBlock), 0, st, w.buf[iLVn], w.buf[iVn],
                     w.theta, n, b, w.rrows, w.rpart);
  MGP_LAUNCH_CHECK();
  MGP_HIP_TRY(hipMemcpyAsync(cx.rp.data(), w.rpart, (size_t)w.rchunks * b * sizeof(double), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipStreamSynchronize(st));
  if (cx.trace)
    fprintf(stderr, "[eig] round %d: enqueue %.2f  filter + Gram on the GPU (wait) %.2f  host %.2f  rotate + residual %.2f ms\n", outer,
            host_ms(cx.tr0, cx.tr1), host_ms(cx.tr1, tp0), host_ms(tp0, tp4), host_ms(tp4, HostClock::now()));
  for (int j = 0; j < b; ++j) {
    double s = 0.0;
    for (int cch = 0; cch < w.rchunks; ++cch) s += cx.rp[(size_t)cch * b + j];
    cx.res[j] = sqrt(s);
  }
  if (kept < b)     // refill dropped directions with fresh random vectors (their L V column is rebuilt by
                    // the next round's filter: dropped directions sit at the end, locked ones at the start)
    MGP_TRY(eig_random_cols(cx, w.buf[iVn], kept, b, cx.seed + 7919ULL * (outer + 1)));
  { const int ov = cx.bV, olv = cx.bLV; cx.bV = iVn; cx.bLV = iLVn; cx.c0 = ov; cx.c1 = olv; }
  return MGP_OK;
}

void eig_trace_step(const EigCtx& cx, const EigStep& s) {
  const int outer = cx.rounds, m = cx.m;
  fprintf(stderr, "[eig] round %d: deg %d, converged %d of %d (leading run %d), max resid %.3e (tol*ub %.3e)\n", outer,
          cx.deg_used, s.nconv, m, s.lead, s.rmx, cx.tol * cx.pol.ub);
  if (s.ruled)
    fprintf(stderr, "[eig] round %d: a %.4e  theta_m %.4e  gap %.3e  exponent %.2f (finish %.2f, safe %.2f)  degree asked %d (e^-3: %d)\n",
            outer, cx.pol.a, cx.rr.th[m - 1], s.gap, s.target, s.t_fin, s.t_safe, s.dask, s.dnew);
}

int eig_write_outputs(EigCtx& cx) {
  const int64_t n = cx.n;
  const int m = cx.m, b = cx.b, kept = cx.rr.kept;
  const float* V = cx.w.buf[cx.bV];
  const int cgrid = (int)std::min<int64_t>(4096, mgp_cdiv(n * m, kBlock));
  hipLaunchKernelGGL(copy_cols_kernel, dim3(cgrid), dim3(kBlock), 0, cx.st, V, n, b, m, cx.evecs);
  MGP_LAUNCH_CHECK();
  if (cx.block_evecs) {     // the whole Rayleigh-Ritz block, guard columns included: [n, b] row-major
    const int bgrid = (int)std::min<int64_t>(4096, mgp_cdiv(n * b, kBlock));
    hipLaunchKernelGGL(copy_cols_kernel, dim3(bgrid), dim3(kBlock), 0, cx.st, V, n, b, b, cx.block_evecs);
    MGP_LAUNCH_CHECK();
  }
  MGP_HIP_TRY(hipStreamSynchronize(cx.st));
  for (int j = 0; j < m; ++j) {
    cx.evals[j] = (kept >= m) ? (float)cx.rr.th[j] : 0.f;
    if (cx.resid) cx.resid[j] = (float)cx.res[j];
  }
  for (int j = 0; j < b; ++j) {
    if (cx.block_evals) cx.block_evals[j] = j < kept ? (float)cx.rr.th[j] : 0.f;
    if (cx.block_resid) cx.block_resid[j] = (float)cx.res[j];
  }
  return MGP_OK;
}

// One solve of at most max_outer rounds on the carved workspace, from the warm block (nullable: random start) to the outputs.
// Leaves rounds, nspmm, nconv and floor_hit in cx.
int eig_solve(EigCtx& cx, const float* warm_block, const float* warm_evals, int max_outer) {
  MGP_TRY(eig_bounds(cx));
  cx.bV = 0; cx.bLV = 1; cx.c0 = 2; cx.c1 = 3; cx.c2 = 4;
  if (warm_block) MGP_HIP_TRY(hipMemcpyAsync(cx.w.buf[0], warm_block, (size_t)cx.n * cx.b * sizeof(float), hipMemcpyDeviceToDevice, cx.st));
  else MGP_TRY(eig_random_cols(cx, cx.w.buf[0], 0, cx.b, cx.seed));
  if (warm_block && warm_evals) eig_warm_start(cx.pol, warm_evals, cx.b, cx.m, cx.user_degree);
  if (cx.b >= cx.n && !(cx.user_degree > 0)) eig_whole_space(cx.pol);
  cx.nspmm = 0; cx.nconv = 0; cx.deg_used = 0; cx.floor_hit = false;
  cx.res.assign(cx.b, 1e300);
  cx.rr.kept = cx.b;
  for (cx.rounds = 0; cx.rounds < max_outer; ++cx.rounds) {
    bool fresh;
    MGP_TRY(eig_filter_round(cx));
    MGP_TRY(eig_ritz_rotate(cx, &fresh));
    cx.nconv = 0;
    if (fresh) continue;
    const EigStep s = eig_round_step(cx.pol, cx.rr.th.data(), cx.res.data(), cx.m, cx.b, cx.rr.kept, cx.tol, cx.n, cx.deg_used,
                                     !!cx.L->mt_img, cx.user_degree, cx.lab ? &cx.lab_target : nullptr);
    cx.nconv = s.nconv;
    if (cx.trace && cx.rr.kept >= cx.m) eig_trace_step(cx, s);
    if (s.verdict != EIG_CONTINUE) { cx.floor_hit = s.verdict == EIG_FLOOR; ++cx.rounds; break; }
  }
  return eig_write_outputs(cx);
}

}  // namespace

static int lanczos_smallest_impl(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals, float* evecs, float* resid,
                                 int32_t* info, float* block_evals, float* block_evecs, float* block_resid, const float* warm_block,
                                 const float* warm_evals, void* work, size_t work_bytes, void* stream) {
  EigCtx cx;
  cx.evals = evals; cx.evecs = evecs; cx.resid = resid;
  cx.block_evals = block_evals; cx.block_evecs = block_evecs; cx.block_resid = block_resid;
  MGP_TRY(eig_setup(cx, L, m, p, work, work_bytes, stream));
  HostPool pool(host_pool_workers(cx.b));      // lives for this call: joined on every return path
  cx.pool = &pool;
  const int max_outer = (p && p->max_restarts > 0) ? p->max_restarts : 40;
  int warm_rounds = 0, warm_nspmm = 0;
  if (warm_block) {
    // a warm start that has not converged within four rounds was not close enough (the matrix moved too far, or the wanted block
    // sits in a cluster that no start resolves): the solve is then repeated from a cold start, with its own floor exits, and the
    // rounds / block products of the abandoned warm attempt are added to the report
    MGP_TRY(eig_solve(cx, warm_block, warm_evals, 4));
    if (cx.nconv != m) { warm_rounds = cx.rounds; warm_nspmm = cx.nspmm; }
  }
  if (!warm_block || cx.nconv != m) MGP_TRY(eig_solve(cx, nullptr, nullptr, max_outer));
  if (info) { info[0] = cx.rounds + warm_rounds; info[1] = cx.nspmm + warm_nspmm; info[2] = cx.nconv; info[3] = cx.b; }
  if (cx.nconv == m) return MGP_OK;
  return cx.floor_hit ? MGP_OK : MGP_ERR_NOT_CONVERGED;
}

// G = A^T A (b x b, fp64 accumulation of the fp32 entries' exact products) for a tall block A [n, b]:
// the Gram kernel of the eigensolver behind the C-ABI.  rocBLAS' dgemm takes 53 ms for this shape at
// n = 1M, b = 50 (one long K loop per output tile); here the rows are split over up to 512 chunks.
extern "C" size_t mgp_gram_workspace_bytes(int64_t n, int b) {
  if (n <= 0 || b <= 0 || b > 512) return 0;
  int chunks; int64_t rpc;
  chunking(n, &chunks, &rpc, 512, 512);
  return mgp_align((size_t)chunks * b * b * sizeof(double)) + 256;
}

extern "C" int mgp_gram_f64(const float* A, int64_t n, int b, double* G, void* work, size_t work_bytes, void* stream) {
  if (!A || !G || !work || n <= 0 || b <= 0 || b > 512) return MGP_ERR_ARG;
  if (work_bytes < mgp_gram_workspace_bytes(n, b)) return MGP_ERR_WORKSPACE;
  EigWork w{};
  chunking(n, &w.chunks, &w.rows_per_chunk, 512, 512);
  MgpArena ar(work, work_bytes);
  w.gpart = ar.take<double>((size_t)w.chunks * b * b);
  if (!ar.ok()) return MGP_ERR_WORKSPACE;
  return launch_gram(A, A, n, b, w, G, mgp_stream(stream));
}

extern "C" int mgp_gram_set_mfma(int on) {
  const int prev = g_gram_mfma;
  g_gram_mfma = on ? 1 : 0;
  return prev;
}

// host-only: the small dense symmetric eigensolver used inside the block eigensolver (exported so that
// the CPU test suite can pin it against LAPACK).  A [n x n] row-major; evals [n]; V [n x n] columns.
extern "C" int mgp_host_symeig(int n, const double* A, double* evals, double* V) {
  if (n <= 0 || !A || !evals || !V) return MGP_ERR_ARG;
  std::vector<double> a(A, A + (size_t)n * n), ev, vv;
  HostPool pool(n >= 64 ? host_pool_workers(n) : 0);      // as inside the block eigensolver
  host_symeigh(n, a, ev, vv, &pool);
  memcpy(evals, ev.data(), (size_t)n * sizeof(double));
  memcpy(V, vv.data(), (size_t)n * n * sizeof(double));
  return MGP_OK;
}

extern "C" size_t mgp_lanczos_workspace_bytes(int64_t n, int m, const mgp_lanczos_params_t* p) {
  if (n <= 0 || m <= 0) return 0;
  return eig_bytes(n, m, p);
}

extern "C" int mgp_lanczos_set_bound_mode(int mode) {
  g_eig_bound_mode = mode == 2 ? 2 : (mode ? 1 : 0);
  return MGP_OK;
}

extern "C" int mgp_lanczos_block_size(int m, const mgp_lanczos_params_t* p) { return m > 0 ? block_size_for(m, p) : 0; }

extern "C" int mgp_lanczos_smallest(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals,
                                    float* evecs, float* resid, int32_t* info, void* work, size_t work_bytes,
                                    void* stream) {
  return mgp_lanczos_smallest_ex(L, m, p, evals, evecs, resid, info, nullptr, nullptr, nullptr, work, work_bytes, stream);
}

extern "C" int mgp_lanczos_smallest_ex(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals,
                                       float* evecs, float* resid, int32_t* info, float* block_evals, float* block_evecs,
                                       float* block_resid, void* work, size_t work_bytes, void* stream) {
  return lanczos_smallest_impl(L, m, p, evals, evecs, resid, info, block_evals, block_evecs, block_resid, nullptr, nullptr, work,
                               work_bytes, stream);
}

// Warm start (round 5): the reference re-runs the whole eigendecomposition on every eval() (riemann_kernel.py:117-130); while the
// hyper-parameters move a little per step the previous Rayleigh-Ritz block is already close.  warm_block [n, b] (device, the
// block_evecs of an earlier call on the SAME sparsity pattern and row order, b = mgp_lanczos_block_size) replaces the random
// start, warm_evals [b] (host, its Ritz values, ascending) set the first round's filter: damping interval from the block's
// largest Ritz value, degree from the gap behind mode m -- i.e. the first round is already a full-strength round.
extern "C" int mgp_lanczos_smallest_warm(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals, float* evecs,
                                         float* resid, int32_t* info, float* block_evals, float* block_evecs, float* block_resid,
                                         const float* warm_block, const float* warm_evals, void* work, size_t work_bytes,
                                         void* stream) {
  if (!warm_block || !warm_evals) return MGP_ERR_ARG;
  return lanczos_smallest_impl(L, m, p, evals, evecs, resid, info, block_evals, block_evecs, block_resid, warm_block, warm_evals, work,
                               work_bytes, stream);
}

// ================================================================= Lanczos tridiagonalisation
namespace {

// partial[blk][j] = sum_{r in chunk} w[r] * Q[j][r],  j = 0..nq-1   (Q column vectors contiguous)
__global__ __launch_bounds__(kBlock) void lz_dots_kernel(const float* __restrict__ w, const float* __restrict__ Q,
                                                         int64_t n, int nq, int64_t rows_per_block,
                                                         float* __restrict__ partial) {
  __shared__ float sh[kBlock / 64];
  const int64_t r0 = blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  for (int j = 0; j < nq; ++j) {
    const float* q = Q + (int64_t)j * n;
    float acc = 0.f;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) acc = fmaf(w[r], q[r], acc);
    acc = mgp_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * nq + j] = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
  }
}

// h[j] = sum_blk partial[blk][j]; w -= sum_j h[j] Q[j]; alpha_acc += h[nq-1] (block 0); norm partials of new w
__global__ __launch_bounds__(kBlock) void lz_update_kernel(float* __restrict__ w, const float* __restrict__ Q, int64_t n,
                                                           int nq, int64_t rows_per_block, const float* __restrict__ partial,
                                                           int nblk, float* __restrict__ alpha_slot, int accumulate,
                                                           float* __restrict__ norm_partial) {
  extern __shared__ float hs[];   // [nq] + reduction scratch [4]
  float* red = hs + nq;
  for (int j = threadIdx.x; j < nq; j += kBlock) {
    float s = 0.f;
    for (int bI = 0; bI < nblk; ++bI) s += partial[(int64_t)bI * nq + j];
    hs[j] = s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (accumulate) *alpha_slot += hs[nq - 1]; else *alpha_slot = hs[nq - 1];
  }
  const int64_t r0 = blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  float nn = 0.f;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
    float v = w[r];
    for (int j = 0; j < nq; ++j) v = fmaf(-hs[j], Q[(int64_t)j * n + r], v);
    w[r] = v;
    nn = fmaf(v, v, nn);
  }
  nn = mgp_wave_sum(nn);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nn;
  __syncthreads();
  if (threadIdx.x == 0) norm_partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// beta = sqrt(sum norm_partial); qnext = w / beta
__global__ __launch_bounds__(kBlock) void lz_normalize_kernel(const float* __restrict__ w, float* __restrict__ qnext,
                                                              int64_t n, const float* __restrict__ norm_partial, int nblk,
                                                              float* __restrict__ beta_slot) {
  __shared__ float sh_beta;
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int bI = 0; bI < nblk; ++bI) s += norm_partial[bI];
    sh_beta = sqrtf(s);
    if (blockIdx.x == 0) *beta_slot = sh_beta;
  }
  __syncthreads();
  const float inv = sh_beta > 0.f ? 1.0f / sh_beta : 0.f;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    qnext[r] = w[r] * inv;
}

}  // namespace

// ---------------------------------------------------------------- block of independent Lanczos runs
// P start vectors at once (the probes of the stochastic log-determinant): every vector is an [n, P]
// row-major block, every coefficient a P-vector, the operator apply is ONE P-column SpMM chain.  The runs
// stay independent (no coupling between columns) -- this is batching, not block Lanczos: it divides the
// launch count by P, and the single-vector version is launch-bound (11 launches per step).
namespace {

constexpr int kBlzMaxNq = 48;    // basis vectors kept for re-orthogonalisation (steps + 1 <= this; 48 KB of LDS)
constexpr int kBlzMaxP = 16;

// partial[blk][i][p] = sum_{r in chunk} W[r,p] * Q_i[r,p],  i < nq
__global__ __launch_bounds__(kBlock) void blz_dots_kernel(const float* __restrict__ W, const float* __restrict__ Q,
                                                          int64_t n, int P, int nq, int64_t rows_per_block,
                                                          float* __restrict__ partial) {
  extern __shared__ float sh[];                 // [nq][RL][P]
  const int RL = kBlock / P;
  const int p = threadIdx.x % P, rl = threadIdx.x / P;
  const bool on = rl < RL;
  const int64_t r0 = blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  const int64_t stride = n * P;
  for (int i0 = 0; i0 < nq; i0 += 8) {          // 8 basis vectors per sweep over the chunk (registers)
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
      // two rows x (1 + 8) loads in flight per pass (clamped rows, masked products): with one row per pass the chunk was
      // a chain of dependent round trips (34 us per launch at 60k x 12; the data is 3-60 MB)
      const int nb = nq - i0 < 8 ? nq - i0 : 8;
      for (int64_t rb = r0 + rl; rb < r1; rb += 2 * RL) {
        float w[2], q[2][8];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int64_t r = rb + v * RL < r1 ? rb + v * RL : rb;
          w[v] = W[r * P + p];
#pragma unroll
          for (int u = 0; u < 8; ++u) q[v][u] = Q[(int64_t)(i0 + (u < nb ? u : 0)) * stride + r * P + p];
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const float wv = rb + v * RL < r1 ? w[v] : 0.f;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (u < nb) acc[u] = fmaf(wv, q[v][u], acc[u]);
        }
      }
    }
    if (on)
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u < nq) sh[((i0 + u) * RL + rl) * P + p] = acc[u];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nq * P; e += kBlock) {
    const int i = e / P, pp = e % P;
    float t = 0.f;
    for (int k = 0; k < RL; ++k) t += sh[(i * RL + k) * P + pp];
    partial[((int64_t)blockIdx.x * nq + i) * P + pp] = t;
  }
}

// out[e] = sum_blk partial[blk][e], e < count: four lanes per element (blocks part, part + 4, ...; eight loads in flight
// each), quad xor-sum -- a fixed order.  Every workgroup of blz_update / blz_normalize used to re-reduce all nblk partials
// itself, one serial chain of nblk loads per thread: 71 / 34 us per launch at 60k x 12.
__global__ __launch_bounds__(kBlock) void blz_reduce_kernel(const float* __restrict__ partial, int nblk, int count,
                                                            float* __restrict__ out) {
  const int e = blockIdx.x * (kBlock / 4) + (threadIdx.x >> 2), part = threadIdx.x & 3;
  const int ec = e < count ? e : count - 1;
  float t = 0.f;
  for (int b0 = part; b0 < nblk; b0 += 32) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int b = b0 + 4 * k;
      v[k] = partial[(int64_t)(b < nblk ? b : nblk - 1) * count + ec];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) t += (b0 + 4 * k < nblk) ? v[k] : 0.f;
  }
  t += __shfl_xor(t, 1, 64);
  t += __shfl_xor(t, 2, 64);
  if (part == 0 && e < count) out[e] = t;
}

// h[i][p] (reduced by blz_reduce_kernel); W -= sum_i h[i][p] Q_i; alpha[p] (+)= h[nq-1][p]; norm partials of the new W
__global__ __launch_bounds__(kBlock) void blz_update_kernel(float* __restrict__ W, const float* __restrict__ Q, int64_t n,
                                                            int P, int nq, int64_t rows_per_block,
                                                            const float* __restrict__ hsum,
                                                            float* __restrict__ alpha_row, int accumulate,
                                                            float* __restrict__ norm_partial) {
  extern __shared__ float sh[];                 // h [nq][P], then reduction scratch [RL][P]
  float* h = sh;
  float* red = sh + nq * P;
  const int RL = kBlock / P;
  for (int e = threadIdx.x; e < nq * P; e += kBlock) h[e] = hsum[e];
  __syncthreads();
  if (blockIdx.x == 0 && (int)threadIdx.x < P) {
    const float a = h[(nq - 1) * P + threadIdx.x];
    alpha_row[threadIdx.x] = accumulate ? alpha_row[threadIdx.x] + a : a;
  }
  const int p = threadIdx.x % P, rl = threadIdx.x / P;
  const bool on = rl < RL;
  const int64_t r0 = blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  const int64_t stride = n * P;
  float nn = 0.f;
  if (on)
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      float v = W[r * P + p];
      // eight basis vectors' loads in flight per batch (one at a time: nq dependent round trips per row)
      for (int i0 = 0; i0 < nq; i0 += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = Q[(int64_t)(i0 + u < nq ? i0 + u : i0) * stride + r * P + p];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < nq) v = fmaf(-h[(i0 + u) * P + p], q[u], v);
      }
      W[r * P + p] = v;
      nn = fmaf(v, v, nn);
    }
  if (on) red[rl * P + p] = nn;
  __syncthreads();
  if ((int)threadIdx.x < P) {
    float t = 0.f;
    for (int k = 0; k < RL; ++k) t += red[k * P + threadIdx.x];
    norm_partial[(int64_t)blockIdx.x * P + threadIdx.x] = t;
  }
}

// beta[p] = sqrt(sum_blk norm_partial[blk][p]); Qnext = W / beta  (a zero column stays zero)
__global__ __launch_bounds__(kBlock) void blz_normalize_kernel(const float* __restrict__ W, float* __restrict__ Qnext,
                                                               int64_t n, int P, const float* __restrict__ norm_sum,
                                                               float* __restrict__ beta_row) {
  __shared__ float inv[kBlzMaxP];
  if ((int)threadIdx.x < P) {
    const float t = norm_sum[threadIdx.x];
    const float b = sqrtf(t);
    inv[threadIdx.x] = b > 0.f ? 1.0f / b : 0.f;
    if (blockIdx.x == 0) beta_row[threadIdx.x] = b;
  }
  __syncthreads();
  const int64_t total = n * P;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    Qnext[e] = W[e] * inv[e % P];
}

}  // namespace

namespace {

// Buffers of P independent Lanczos runs of `steps` steps on vectors of length n, laid out in one workspace the same way at
// every call (the external-operator form below is stateless: begin / step / end recompute this layout).
struct Blz {
  int64_t n, blockf, nblk, rpb;
  int P, steps, RL, egrid;
  float *Q, *W, *dpart, *npart, *hsum, *nsum, *d_alpha, *d_beta;
  bool ok;
};

size_t blz_bytes(int64_t n, int P, int steps) {
  size_t s = mgp_align((size_t)(steps + 1) * n * P * sizeof(float));   // Q
  s += mgp_align((size_t)n * P * sizeof(float));                       // W
  s += mgp_align((size_t)256 * (steps + 1) * P * sizeof(float));        // dot partials
  s += mgp_align((size_t)256 * P * sizeof(float));                      // norm partials
  s += 2 * mgp_align((size_t)(steps + 1) * P * sizeof(float));          // alpha, beta
  s += mgp_align((size_t)(steps + 1) * P * sizeof(float)) + mgp_align(kBlzMaxP * sizeof(float));   // reduced dots / norms
  return s + 2048;
}

Blz blz_layout(MgpArena& ar, int64_t n, int P, int steps) {
  Blz b;
  b.n = n; b.P = P; b.steps = steps;
  b.Q = ar.take<float>((size_t)(steps + 1) * n * P);
  b.W = ar.take<float>((size_t)n * P);
  b.dpart = ar.take<float>((size_t)256 * (steps + 1) * P);
  b.npart = ar.take<float>((size_t)256 * P);
  b.hsum = ar.take<float>((size_t)(steps + 1) * P);
  b.nsum = ar.take<float>((size_t)kBlzMaxP);
  b.d_alpha = ar.take<float>((size_t)(steps + 1) * P);
  b.d_beta = ar.take<float>((size_t)(steps + 1) * P);
  b.ok = ar.ok();
  b.RL = kBlock / P;
  b.nblk = std::min<int64_t>(256, mgp_cdiv(n, 4 * b.RL));
  if (b.nblk < 1) b.nblk = 1;
  b.rpb = mgp_cdiv(n, b.nblk);
  b.nblk = mgp_cdiv(n, b.rpb);
  b.egrid = (int)std::min<int64_t>(2048, mgp_cdiv(n * P, kBlock));
  b.blockf = n * P;
  return b;
}

void blz_reduce(const Blz& b, const float* part, int count, float* out, hipStream_t st) {
  hipLaunchKernelGGL(blz_reduce_kernel, dim3((unsigned)mgp_cdiv(count, kBlock / 4)), dim3(kBlock), 0, st, part, (int)b.nblk, count, out);
}

// q_0 = Q0 / column norms: one update launch with a zero coefficient gives the norm partials
int blz_begin(const Blz& b, const float* Q0, hipStream_t st) {
  const int P = b.P, steps = b.steps;
  MGP_HIP_TRY(hipMemcpyAsync(b.W, Q0, b.blockf * sizeof(float), hipMemcpyDeviceToDevice, st));
  MGP_HIP_TRY(hipMemcpyAsync(b.Q, Q0, b.blockf * sizeof(float), hipMemcpyDeviceToDevice, st));
  MGP_HIP_TRY(hipMemsetAsync(b.dpart, 0, (size_t)256 * P * sizeof(float), st));
  MGP_HIP_TRY(hipMemsetAsync(b.d_alpha, 0, (size_t)(steps + 1) * P * sizeof(float), st));
  MGP_HIP_TRY(hipMemsetAsync(b.hsum, 0, (size_t)P * sizeof(float), st));
  hipLaunchKernelGGL(blz_update_kernel, dim3((int)b.nblk), dim3(kBlock), (size_t)(P + b.RL * P) * sizeof(float), st, b.W, b.Q, b.n, P, 1,
                     b.rpb, b.hsum, b.d_alpha + (size_t)steps * P, 0, b.npart);
  MGP_LAUNCH_CHECK();
  blz_reduce(b, b.npart, P, b.nsum, st);
  MGP_LAUNCH_CHECK();
  hipLaunchKernelGGL(blz_normalize_kernel, dim3(b.egrid), dim3(kBlock), 0, st, b.W, b.Q, b.n, P, b.nsum, b.d_beta + (size_t)steps * P);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

// step j on W = A q_j (overwritten): classical Gram-Schmidt against q_0..q_j, twice; alpha_j, beta_j; q_{j+1}
int blz_step(const Blz& b, float* W, int j, hipStream_t st) {
  const int P = b.P, nq = j + 1;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(blz_dots_kernel, dim3((int)b.nblk), dim3(kBlock), (size_t)nq * b.RL * P * sizeof(float), st, W, b.Q, b.n, P,
                       nq, b.rpb, b.dpart);
    MGP_LAUNCH_CHECK();
    blz_reduce(b, b.dpart, nq * P, b.hsum, st);
    MGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(blz_update_kernel, dim3((int)b.nblk), dim3(kBlock), (size_t)(nq * P + b.RL * P) * sizeof(float), st, W,
                       b.Q, b.n, P, nq, b.rpb, b.hsum, b.d_alpha + (size_t)j * P, pass, b.npart);
    MGP_LAUNCH_CHECK();
  }
  blz_reduce(b, b.npart, P, b.nsum, st);
  MGP_LAUNCH_CHECK();
  hipLaunchKernelGGL(blz_normalize_kernel, dim3(b.egrid), dim3(kBlock), 0, st, W, b.Q + (int64_t)(j + 1) * b.blockf, b.n, P, b.nsum,
                     b.d_beta + (size_t)j * P);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}

int blz_end(const Blz& b, float* alpha, float* beta, hipStream_t st) {
  MGP_HIP_TRY(hipMemcpyAsync(alpha, b.d_alpha, (size_t)b.steps * b.P * sizeof(float), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipMemcpyAsync(beta, b.d_beta, (size_t)b.steps * b.P * sizeof(float), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipStreamSynchronize(st));
  return MGP_OK;
}

bool blz_shape_ok(int64_t n, int P, int steps) {
  return n > 0 && steps > 0 && steps + 1 <= kBlzMaxNq && P > 0 && P <= kBlzMaxP;
}

}  // namespace

extern "C" size_t mgp_lanczos_tridiag_block_workspace_bytes(const mgp_operator_t* op, int P, int steps) {
  if (!op || !blz_shape_ok(op->L.n, P, steps)) return 0;
  return blz_bytes(op->L.n, P, steps) + mgp_operator_workspace_bytes(op, P) + 2048;
}

// Q0 [n, P] start vectors (columns need not be normalised).  alpha / beta: host [steps][P].
extern "C" int mgp_lanczos_tridiag_block(const mgp_operator_t* op, const float* Q0, int P, int steps, float* alpha,
                                         float* beta, void* work, size_t work_bytes, void* stream) {
  if (!op || !Q0 || !alpha || !beta || !work || steps <= 0 || P <= 0) return MGP_ERR_ARG;
  if (P > kBlzMaxP || steps + 1 > kBlzMaxNq) return MGP_ERR_UNSUPPORTED;
  if (work_bytes < mgp_lanczos_tridiag_block_workspace_bytes(op, P, steps)) return MGP_ERR_WORKSPACE;
  hipStream_t st = mgp_stream(stream);
  MgpArena ar(work, work_bytes);
  const Blz b = blz_layout(ar, op->L.n, P, steps);
  const size_t owb = mgp_operator_workspace_bytes(op, P);
  void* ow = ar.take<char>(owb);
  if (!b.ok || !ar.ok()) return MGP_ERR_WORKSPACE;
  MGP_TRY(blz_begin(b, Q0, st));
  for (int j = 0; j < steps; ++j) {
    MGP_TRY(mgp_operator_apply_ex(op, b.Q + (int64_t)j * b.blockf, P, b.W, nullptr, nullptr, nullptr, nullptr, ow, owb, stream));
    MGP_TRY(blz_step(b, b.W, j, st));
  }
  return blz_end(b, alpha, beta, st);
}

// ---- the same P Lanczos runs for an operator the CALLER applies (a wrapper around a Schur complement: every product is a
// CG solve of its own): begin normalises the start block, the caller reads q_j (mgp_blz_q), applies its operator and hands
// W = A q_j to mgp_blz_step (W is overwritten), mgp_blz_end copies alpha / beta [steps][P] to the host and synchronises.
// Nothing in between synchronises or reads anything back.  The workspace is laid out identically at every call.
extern "C" size_t mgp_blz_workspace_bytes(int64_t n, int P, int steps) {
  return blz_shape_ok(n, P, steps) ? blz_bytes(n, P, steps) : 0;
}

extern "C" int mgp_blz_begin(const float* Q0, int64_t n, int P, int steps, void* work, size_t work_bytes, void* stream) {
  if (!Q0 || !work) return MGP_ERR_ARG;
  if (!blz_shape_ok(n, P, steps)) return MGP_ERR_UNSUPPORTED;
  if (work_bytes < blz_bytes(n, P, steps)) return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  const Blz b = blz_layout(ar, n, P, steps);
  if (!b.ok) return MGP_ERR_WORKSPACE;
  return blz_begin(b, Q0, mgp_stream(stream));
}

extern "C" float* mgp_blz_q(int64_t n, int P, int steps, int j, void* work, size_t work_bytes) {
  if (!work || !blz_shape_ok(n, P, steps) || j < 0 || j > steps || work_bytes < blz_bytes(n, P, steps)) return nullptr;
  MgpArena ar(work, work_bytes);
  const Blz b = blz_layout(ar, n, P, steps);
  return b.ok ? b.Q + (int64_t)j * b.blockf : nullptr;
}

extern "C" int mgp_blz_step(float* W, int64_t n, int P, int steps, int j, void* work, size_t work_bytes, void* stream) {
  if (!W || !work || j < 0 || j >= steps) return MGP_ERR_ARG;
  if (!blz_shape_ok(n, P, steps)) return MGP_ERR_UNSUPPORTED;
  if (work_bytes < blz_bytes(n, P, steps)) return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  const Blz b = blz_layout(ar, n, P, steps);
  if (!b.ok) return MGP_ERR_WORKSPACE;
  return blz_step(b, W, j, mgp_stream(stream));
}

extern "C" int mgp_blz_end(int64_t n, int P, int steps, float* alpha, float* beta, void* work, size_t work_bytes, void* stream) {
  if (!alpha || !beta || !work) return MGP_ERR_ARG;
  if (!blz_shape_ok(n, P, steps)) return MGP_ERR_UNSUPPORTED;
  if (work_bytes < blz_bytes(n, P, steps)) return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  const Blz b = blz_layout(ar, n, P, steps);
  if (!b.ok) return MGP_ERR_WORKSPACE;
  return blz_end(b, alpha, beta, mgp_stream(stream));
}

extern "C" size_t mgp_lanczos_tridiag_workspace_bytes(const mgp_operator_t* op, int steps) {
  if (!op || steps <= 0 || op->L.n <= 0) return 0;
  const int64_t n = op->L.n;
  size_t s = mgp_align((size_t)(steps + 1) * n * sizeof(float));   // Q
  s += mgp_align((size_t)n * sizeof(float));                      // w
  s += mgp_operator_workspace_bytes(op, 1);
  s += mgp_align((size_t)512 * (steps + 1) * sizeof(float));       // dot partials
  s += mgp_align(512 * sizeof(float));                            // norm partials
  s += 2 * mgp_align((size_t)(steps + 1) * sizeof(float));         // alpha, beta
  return s + 4096;
}

// q0 [n] start vector (need not be normalised).  alpha[steps], beta[steps] on the host;
// Q_out (nullable, device [steps, n]) receives the orthonormal Lanczos vectors (row j = q_j).
extern "C" int mgp_lanczos_tridiag(const mgp_operator_t* op, const float* q0, int steps, float* alpha, float* beta,
                                   float* Q_out, void* work, size_t work_bytes, void* stream) {
  if (!op || !q0 || !alpha || !beta || !work || steps <= 0) return MGP_ERR_ARG;
  if (work_bytes < mgp_lanczos_tridiag_workspace_bytes(op, steps)) return MGP_ERR_WORKSPACE;
  const int64_t n = op->L.n;
  hipStream_t st = mgp_stream(stream);
  MgpArena ar(work, work_bytes);
  float* Q = ar.take<float>((size_t)(steps + 1) * n);
  float* w = ar.take<float>(n);
  const size_t owb = mgp_operator_workspace_bytes(op, 1);
  void* ow = ar.take<char>(owb);
  float* dpart = ar.take<float>((size_t)512 * (steps + 1));
  float* npart = ar.take<float>(512);
  float* d_alpha = ar.take<float>(steps + 1);
  float* d_beta = ar.take<float>(steps + 1);
  if (!ar.ok()) return MGP_ERR_WORKSPACE;
  int64_t nblk = std::min<int64_t>(512, mgp_cdiv(n, 1024));
  if (nblk < 1) nblk = 1;
  const int64_t rpb = mgp_cdiv(n, nblk);
  nblk = mgp_cdiv(n, rpb);
  const int egrid = (int)std::min<int64_t>(2048, mgp_cdiv(n, kBlock));

  // q_0 = q0 / ||q0||: reuse the update kernel with nq = 0 to get the norm partials
  MGP_HIP_TRY(hipMemcpyAsync(w, q0, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  MGP_HIP_TRY(hipMemsetAsync(d_alpha, 0, (steps + 1) * sizeof(float), st));
  {
    // norm of w without subtraction: nq = 1 with a zero coefficient is simpler than a new kernel
    MGP_HIP_TRY(hipMemsetAsync(dpart, 0, (size_t)512 * sizeof(float), st));
    MGP_HIP_TRY(hipMemcpyAsync(Q, w, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(lz_update_kernel, dim3((int)nblk), dim3(kBlock), (1 + 4) * sizeof(float), st, w, Q, n, 1, rpb,
                       dpart, (int)nblk, d_alpha + steps, 0, npart);
    MGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(lz_normalize_kernel, dim3(egrid), dim3(kBlock), 0, st, w, Q, n, npart, (int)nblk, d_beta + steps);
    MGP_LAUNCH_CHECK();
  }
  for (int j = 0; j < steps; ++j) {
    float* qj = Q + (int64_t)j * n;
    MGP_TRY(mgp_operator_apply_ex(op, qj, 1, w, nullptr, nullptr, nullptr, nullptr, ow, owb, stream));
    for (int pass = 0; pass < 2; ++pass) {   // classical Gram-Schmidt against q_0..q_j, twice
      hipLaunchKernelGGL(lz_dots_kernel, dim3((int)nblk), dim3(kBlock), 0, st, w, Q, n, j + 1, rpb, dpart);
      MGP_LAUNCH_CHECK();
      hipLaunchKernelGGL(lz_update_kernel, dim3((int)nblk), dim3(kBlock), (j + 1 + 4) * sizeof(float), st, w, Q, n,
                         j + 1, rpb, dpart, (int)nblk, d_alpha + j, pass, npart);
      MGP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lz_normalize_kernel, dim3(egrid), dim3(kBlock), 0, st, w, Q + (int64_t)(j + 1) * n, n, npart,
                       (int)nblk, d_beta + j);
    MGP_LAUNCH_CHECK();
  }
  MGP_HIP_TRY(hipMemcpyAsync(alpha, d_alpha, steps * sizeof(float), hipMemcpyDeviceToHost, st));
  MGP_HIP_TRY(hipMemcpyAsync(beta, d_beta, steps * sizeof(float), hipMemcpyDeviceToHost, st));
  if (Q_out) MGP_HIP_TRY(hipMemcpyAsync(Q_out, Q, (size_t)steps * n * sizeof(float), hipMemcpyDeviceToDevice, st));
  MGP_HIP_TRY(hipStreamSynchronize(st));
  return MGP_OK;
}
