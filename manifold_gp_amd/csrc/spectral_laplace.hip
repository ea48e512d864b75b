// One Newton evaluation of a Laplace fit on the spectral features (docs/kernels/spectral_laplace.md): with Z [n, m] the float32
// feature rows, w [m] the float64 weights, f_i = z_i . w and (l_i, g_i, h_i) the family's log p, d log p / df and -d2 log p / df2
// at f_i + mean on the observed rows (0 elsewhere; site_formulas.h, the arithmetic of the fits on the graph nodes),
//
//   f [n],   grad = Z^T g [m],   hess = Z^T diag(h) Z [m, m],   sums = { sum_obs l_i, max_i |f_i| }          all float64.
//
// Two kernels, a first one that leaves h as float64 [n] in the workspace and the weighted Gram after it -- not one fused
// kernel: the Gram's grid is (tile pairs x row chunks) and every tile pair would form the row dots and the exp / log1p of the
// family again (3 times at m = 100, 36 times at m = 512), while h costs 8 n bytes against the 4 n m of a pass over Z; and a
// line-search evaluation (hess == NULL) is the first kernel alone, so its f, grad and sums are the same bits either way.
//
// spectral_site_kernel (pass 1 over Z).  A wave owns a row per step, rows at a grid stride of 4 waves x at most kSpecMaxBlocks
// workgroups, the next row's loads in flight behind the current row's arithmetic.  Lane l holds the columns 4 (64 k + l) .. + 3
// (one 16-byte load per k < 2; m % 4 == 0 and Z 16-byte aligned) or 64 k + l (k < 8, scalar loads) with the matching w in
// registers; the row dot is fma's in float64 and an xor tree over the wave, which leaves the same bits in every lane; every lane
// forms (l, g, h) from it and adds g z_ij to its columns' float64 accumulators, rows in ascending order.  The workgroup's four
// waves are added in wave order through LDS: one partial [m + 2] per workgroup (grad, sum l, max |f|).
// spectral_sum_kernel adds the partials: 16 columns x 16 slices of workgroups per launch block, a slice in workgroup order, the
// slices in order.  No atomics anywhere: repeated calls are bitwise equal.
//
// spectral_gram_kernel (pass 2, with a Hessian only): the tile, LDS staging and register prefetch of gram_mfma_kernel
// (eigen.hip) -- 64 x 64 output tile per workgroup, 32-row stages, rows padded to 80 floats, v_mfma_f64_16x16x4_f64 with the
// result layout row 4 r + kq -- with the B operand scaled by h_r as it is converted, only the tile pairs ti <= tj, and the
// diagonal pairs staging one operand.  A stage's 32 values of h are loaded a stage before its rows; a stage whose h are all zero
// (unobserved rows) is skipped whole -- no loads of Z, no barrier: the decision is a ballot over values every wave reads alike.
// One partial [m, m] per row chunk (upper tile pairs written); spectral_gram_sum_kernel adds the chunks in order for i <= j and
// writes both (i, j) and (j, i): hess is bitwise symmetric.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): docs/kernels/spectral_laplace.md.
#include <cmath>

#include "mgp_common.h"
#include "mgp_arena.h"
#include "site_formulas.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MGP_WAVE;
constexpr int kMaxModes = 512;            // the cap of mgp_gram_f64
constexpr int kSpecMaxBlocks = 512;       // grid cap of spectral_site_kernel: 512 workgroups x 4 rows per step
constexpr int kLaneCols = kMaxModes / MGP_WAVE;   // 8 columns per lane
constexpr int kSumCols = 16, kSumSlices = 16;     // spectral_sum_kernel: columns x slices of workgroups per launch block
constexpr int kGR = 32, kGP = 64 + 16;    // spectral_gram_kernel: rows per stage, padded row of the staged 64 columns
constexpr int kGramMinRows = 128;         // rows per chunk at least (a multiple of kGR)
constexpr int kGramMaxChunks = 128;       // row chunks at most
constexpr int kGramTargetBlocks = 1024;   // tile pairs x chunks aimed at (at least 8 chunks)

struct SpecParams {
  double mean, r_nb, log_r;
};

// FAM 0 Bernoulli-logit, 1 Poisson, 2 binomial, 3 negative binomial, 4 ordinal; f without the mean
template <int FAM>
__device__ __forceinline__ void spec_lgh(const SpecParams& p, double f, float a32, float b32, double& lp, double& g, double& h) {
  if (FAM == 0) mgp_bernoulli_lgh(f + p.mean, a32, lp, g, h);
  else if (FAM == 1) mgp_count_lgh<0>(f, p.mean, 0.0, 0.0, a32, b32, lp, g, h);
  else if (FAM == 2) mgp_count_lgh<1>(f, p.mean, 0.0, 0.0, a32, b32, lp, g, h);
  else if (FAM == 3) mgp_count_lgh<2>(f, p.mean, p.r_nb, p.log_r, a32, b32, lp, g, h);
  else mgp_ordinal_lgh(f + p.mean, a32, b32, lp, g, h);
}

// the columns of lane `lane`: item k, entry e -> column; VEC: 4 (64 k + lane) + e, e < 4, k < 2; scalar: 64 k + lane, k < 8
template <bool VEC>
__device__ __forceinline__ int spec_col(int lane, int k, int e) {
  return VEC ? 4 * (MGP_WAVE * k + lane) + e : MGP_WAVE * k + lane;
}

template <bool VEC>
__device__ __forceinline__ void spec_load_row(const float* __restrict__ Z, int64_t row, int m, int lane, float (&z)[kLaneCols]) {
  const float* zr = Z + row * (int64_t)m;
  if (VEC) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = 4 * (MGP_WAVE * k + lane);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < m) v = *reinterpret_cast<const float4*>(zr + c);          // m % 4 == 0: the whole float4 is inside the row
      z[4 * k] = v.x;
      z[4 * k + 1] = v.y;
      z[4 * k + 2] = v.z;
      z[4 * k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kLaneCols; ++k) {
      const int c = MGP_WAVE * k + lane;
      z[k] = c < m ? zr[c] : 0.f;
    }
  }
}

template <bool VEC, int FAM>
__global__ __launch_bounds__(kBlock) void spectral_site_kernel(const float* __restrict__ Z, int64_t n, int m,
                                                               const double* __restrict__ w, const float* __restrict__ a,
                                                               const float* __restrict__ b, const uint8_t* __restrict__ obs,
                                                               SpecParams prm, double* __restrict__ f, double* __restrict__ hout,
                                                               double* __restrict__ partials) {
  __shared__ double s_g[kWaves][kMaxModes];
  __shared__ double s_s[kWaves][2];
  const int lane = threadIdx.x & (MGP_WAVE - 1), wave = threadIdx.x / MGP_WAVE;
  double wv[kLaneCols], ga[kLaneCols];
#pragma unroll
  for (int j = 0; j < kLaneCols; ++j) {
    const int c = VEC ? spec_col<true>(lane, j >> 2, j & 3) : spec_col<false>(lane, j, 0);
    wv[j] = c < m ? w[c] : 0.0;
    ga[j] = 0.0;
  }
  double lp_sum = 0.0, f_max = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  int64_t row = (int64_t)blockIdx.x * kWaves + wave;
  float z[kLaneCols], zn[kLaneCols];
  if (row < n) spec_load_row<VEC>(Z, row, m, lane, z);
  for (; row < n; row += stride) {
    const int64_t next = row + stride;
    if (next < n) spec_load_row<VEC>(Z, next, m, lane, zn);             // in flight behind this row's arithmetic
    double p = 0.0;
#pragma unroll
    for (int j = 0; j < kLaneCols; ++j) p = fma((double)z[j], wv[j], p);
    const double fi = mgp_wave_sum_d(p);                                // the same bits in every lane
    const bool o = obs ? obs[row] != 0 : true;
    double lp = 0.0, g = 0.0, h = 0.0;
    if (o) {                                                            // (a and b are read at observed rows only)
      spec_lgh<FAM>(prm, fi, a[row], b ? b[row] : 0.f, lp, g, h);
#pragma unroll
      for (int j = 0; j < kLaneCols; ++j) ga[j] = fma(g, (double)z[j], ga[j]);
    }
    lp_sum += lp;
    const double af = fabs(fi);
    f_max = af > f_max ? af : f_max;
    if (lane == 0) {
      if (f) f[row] = fi;
      if (hout) hout[row] = h;
    }
#pragma unroll
    for (int j = 0; j < kLaneCols; ++j) z[j] = zn[j];
  }
#pragma unroll
  for (int j = 0; j < kLaneCols; ++j) {
    const int c = VEC ? spec_col<true>(lane, j >> 2, j & 3) : spec_col<false>(lane, j, 0);
    if (c < m) s_g[wave][c] = ga[j];
  }
  if (lane == 0) {
    s_s[wave][0] = lp_sum;
    s_s[wave][1] = f_max;
  }
  __syncthreads();
  double* out = partials + (int64_t)blockIdx.x * (m + 2);
  for (int c = threadIdx.x; c < m; c += kBlock) {
    double s = s_g[0][c];
    for (int k = 1; k < kWaves; ++k) s += s_g[k][c];
    out[c] = s;
  }
  if (threadIdx.x == 0) {
    double s = s_s[0][0], mx = s_s[0][1];
    for (int k = 1; k < kWaves; ++k) {
      s += s_s[k][0];
      mx = s_s[k][1] > mx ? s_s[k][1] : mx;
    }
    out[m] = s;
    out[m + 1] = mx;
  }
}

// grad [m] and sums [2] from the partials [nblk, m + 2]: thread (column c, slice s) adds the workgroups of its slice in order
// (column m + 1: their maximum), then the slices are added in order
__global__ __launch_bounds__(kBlock) void spectral_sum_kernel(const double* __restrict__ partials, int nblk, int m,
                                                              double* __restrict__ grad, double* __restrict__ sums) {
  __shared__ double s_p[kSumSlices][kSumCols];
  const int cl = threadIdx.x % kSumCols, sl = threadIdx.x / kSumCols;
  const int c = blockIdx.x * kSumCols + cl;
  const int ld = m + 2;
  const bool is_max = c == m + 1;
  const int per = (nblk + kSumSlices - 1) / kSumSlices;
  const int b0 = sl * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  double acc = 0.0;
  if (c < ld) {
#pragma unroll 8
    for (int k = b0; k < b1; ++k) {
      const double v = partials[(int64_t)k * ld + c];
      acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
  }
  s_p[sl][cl] = acc;
  __syncthreads();
  if (sl == 0 && c < ld) {
    double r = s_p[0][cl];
    for (int k = 1; k < kSumSlices; ++k) r = is_max ? (s_p[k][cl] > r ? s_p[k][cl] : r) : r + s_p[k][cl];
    if (c < m) grad[c] = r;
    else sums[c - m] = r;
  }
}

using f64x4 = __attribute__((ext_vector_type(4))) double;

// partial[chunk][i][j] = sum_{r in chunk} Z[r, i] h_r Z[r, j] on the tile pair blockIdx.x = (ti <= tj), chunk blockIdx.y
__global__ __launch_bounds__(kBlock) void spectral_gram_kernel(const float* __restrict__ Z, const double* __restrict__ h, int64_t n,
                                                               int m, int64_t rows_per_chunk, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float As[kGR][kGP];
  __shared__ __attribute__((aligned(16))) float Bs[kGR][kGP];
  __shared__ double Hs[kGR];
  const int nt = (m + 63) >> 6;
  int ti = 0, t = blockIdx.x;
  while (t >= nt - ti) {                                               // row ti of the upper triangle holds nt - ti pairs
    t -= nt - ti;
    ++ti;
  }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, kq = lane >> 4;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  f64x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[x][c] = f64x4{0.0, 0.0, 0.0, 0.0};
  const bool vec = (m & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0;
  // h of the rows rr + lane (lanes 0 .. 31; 0 past the chunk), every wave the same 32 values
  auto load_h = [&](int64_t rr) { return (lane < kGR && rr + lane < r1) ? h[rr + lane] : 0.0; };
  auto load4 = [&](int64_t r, int c0) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* zr = Z + r * (int64_t)m;
    if (vec && c0 + 3 < m) v = *reinterpret_cast<const float4*>(zr + c0);
    else {
      if (c0 < m) v.x = zr[c0];
      if (c0 + 1 < m) v.y = zr[c0 + 1];
      if (c0 + 2 < m) v.z = zr[c0 + 2];
      if (c0 + 3 < m) v.w = zr[c0 + 3];
    }
    return v;
  };
  float4 pa[2], pb[2];
  double hq = r0 < r1 ? load_h(r0) : 0.0;                              // h of the stage that fetch() takes next
  double hf = 0.0;                                                     // h of the fetched stage
  bool livef = false;                                                  // the fetched stage has a row with h != 0
  // thread -> (row lr, 4 columns from lc) of the stage, two such items per thread and operand (32 x 64 floats = 512 float4)
  auto fetch = [&](int64_t rr) {
    hf = hq;
    livef = __ballot(hf != 0.0) != 0;
    hq = rr + kGR < r1 ? load_h(rr + kGR) : 0.0;
    if (!livef) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = threadIdx.x + u * kBlock;
      const int lr = e >> 4, lc = (e & 15) * 4;
      const int64_t r = rr + lr;
      pa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      pb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < r1) {
        pa[u] = load4(r, ti * 64 + lc);
        if (!diag) pb[u] = load4(r, tj * 64 + lc);
      }
    }
  };
  const float(*Bp)[kGP] = diag ? As : Bs;
  if (r0 < r1) fetch(r0);
  for (int64_t rr = r0; rr < r1; rr += kGR) {
    const bool live = livef;                                           // the same in every wave: the barriers stay convergent
    if (live) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = threadIdx.x + u * kBlock;
        const int lr = e >> 4, lc = (e & 15) * 4;
        *reinterpret_cast<float4*>(&As[lr][lc]) = pa[u];
        if (!diag) *reinterpret_cast<float4*>(&Bs[lr][lc]) = pb[u];
      }
      if (wave == 0 && lane < kGR) Hs[lane] = hf;
      __syncthreads();
    }
    if (rr + kGR < r1) fetch(rr + kGR);                                // the next stage's rows are in flight during the MFMAs
    if (live) {
#pragma unroll
      for (int k0 = 0; k0 < kGR; k0 += 4) {
        const double hk = Hs[k0 + kq];
        double av[2], bv[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) av[x] = (double)As[k0 + kq][wi + 16 * x + l16];
#pragma unroll
        for (int c = 0; c < 2; ++c) bv[c] = (double)Bp[k0 + kq][wj + 16 * c + l16] * hk;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[x][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[c], acc[x][c], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  // acc[x][c][r]: row i = wi + 16 x + 4 r + kq, column j = wj + 16 c + l16 of the tile (gram_mfma_kernel)
  double* out = partial + (int64_t)blockIdx.y * m * m;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 64 + wi + 16 * x + 4 * r + kq, j = tj * 64 + wj + 16 * c + l16;
        if (i < m && j < m) out[(int64_t)i * m + j] = acc[x][c][r];
      }
}

// hess[i][j] = hess[j][i] = sum_chunks partial[chunk][i][j] for i <= j (an entry of a tile pair ti <= tj), chunks in order
__global__ __launch_bounds__(kBlock) void spectral_gram_sum_kernel(const double* __restrict__ partial, int chunks, int m,
                                                                   double* __restrict__ hess) {
  const int mm = m * m;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < mm; e += gridDim.x * kBlock) {
    const int i = e / m, j = e - i * m;
    if (i > j) continue;
    double s = 0.0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) s += partial[(int64_t)c * mm + e];
    hess[e] = s;
    hess[j * m + i] = s;
  }
}

int spec_blocks(int64_t n) {
  const int64_t b = mgp_cdiv(n, (int64_t)kWaves);
  return (int)(b > kSpecMaxBlocks ? kSpecMaxBlocks : b);
}

int gram_pairs(int m) {
  const int nt = (m + 63) / 64;
  return nt * (nt + 1) / 2;
}

void gram_chunking(int64_t n, int m, int* chunks, int64_t* rows_per_chunk) {
  int maxc = kGramTargetBlocks / gram_pairs(m);
  if (maxc < 8) maxc = 8;
  if (maxc > kGramMaxChunks) maxc = kGramMaxChunks;
  int64_t r = mgp_cdiv(mgp_cdiv(n, (int64_t)maxc), (int64_t)kGR) * kGR;
  if (r < kGramMinRows) r = kGramMinRows;
  *rows_per_chunk = r;
  *chunks = (int)mgp_cdiv(n, r);
}

struct SpecWork {
  double *partials, *h, *gpart;
  int blocks, chunks;
  int64_t rows_per_chunk;
};

// the workspace of one call, carved from `ar` (a counting arena: the bytes it needs)
void spec_carve(MgpArena& ar, int64_t n, int m, bool with_hessian, SpecWork& sw) {
  sw.blocks = spec_blocks(n);
  sw.partials = ar.take<double>((size_t)sw.blocks * (size_t)(m + 2));
  sw.h = sw.gpart = nullptr;
  sw.chunks = 0;
  sw.rows_per_chunk = 0;
  if (with_hessian) {
    gram_chunking(n, m, &sw.chunks, &sw.rows_per_chunk);
    sw.h = ar.take<double>((size_t)n);
    sw.gpart = ar.take<double>((size_t)sw.chunks * m * m);
  }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int FAM>
void launch_spec_site(bool vec, dim3 grid, hipStream_t st, const float* Z, int64_t n, int m, const double* w, const float* a,
                      const float* b, const uint8_t* obs, const SpecParams& prm, double* f, double* hout, double* partials) {
  if (vec)
    hipLaunchKernelGGL((spectral_site_kernel<true, FAM>), grid, dim3(kBlock), 0, st, Z, n, m, w, a, b, obs, prm, f, hout, partials);
  else
    hipLaunchKernelGGL((spectral_site_kernel<false, FAM>), grid, dim3(kBlock), 0, st, Z, n, m, w, a, b, obs, prm, f, hout, partials);
}

}  // namespace

extern "C" size_t mgp_spectral_site_workspace_bytes(int64_t n, int m, int with_hessian) {
  if (n < 1 || m < 1 || m > kMaxModes) return 0;
  MgpArena ar;
  SpecWork sw;
  spec_carve(ar, n, m, with_hessian != 0, sw);
  return ar.off;
}

extern "C" int mgp_spectral_site(const float* Z, int64_t n, int m, const double* w, int family, const float* a, const float* b,
                                 const uint8_t* obs, double mean, double dispersion, double* f, double* grad, double* hess,
                                 double* sums, void* work, size_t work_bytes, void* stream) {
  if (!Z || !w || !a || !grad || !sums || n < 1 || m < 1 || m > kMaxModes) return MGP_ERR_ARG;
  if (family < 0 || family > 4) return MGP_ERR_UNSUPPORTED;
  if ((family == 2 || family == 4) && !b) return MGP_ERR_ARG;          // the trials and the upper cutpoints have no default
  if (family == 3 && !(dispersion >= 0x1p-10 && dispersion <= 0x1p20)) return MGP_ERR_ARG;   // (NaN fails the comparison)
  if (!aligned_to(Z, 4) || !aligned_to(w, 8) || !aligned_to(f, 8) || !aligned_to(grad, 8) || !aligned_to(hess, 8) ||
      !aligned_to(sums, 8))
    return MGP_ERR_ARG;
  const bool with_hessian = hess != nullptr;
  if (!work || !aligned_to(work, 8) || work_bytes < mgp_spectral_site_workspace_bytes(n, m, with_hessian ? 1 : 0))
    return MGP_ERR_WORKSPACE;
  MgpArena ar(work, work_bytes);
  SpecWork sw;
  spec_carve(ar, n, m, with_hessian, sw);
  if (!ar.ok()) return MGP_ERR_WORKSPACE;
  SpecParams prm = {mean, family == 3 ? dispersion : 0.0, family == 3 ? std::log(dispersion) : 0.0};
  hipStream_t st = mgp_stream(stream);
  const bool vec = (m & 3) == 0 && aligned_to(Z, 16);
  const dim3 grid((unsigned)sw.blocks);
  switch (family) {
    case 0: launch_spec_site<0>(vec, grid, st, Z, n, m, w, a, b, obs, prm, f, sw.h, sw.partials); break;
    case 1: launch_spec_site<1>(vec, grid, st, Z, n, m, w, a, b, obs, prm, f, sw.h, sw.partials); break;
    case 2: launch_spec_site<2>(vec, grid, st, Z, n, m, w, a, b, obs, prm, f, sw.h, sw.partials); break;
    case 3: launch_spec_site<3>(vec, grid, st, Z, n, m, w, a, b, obs, prm, f, sw.h, sw.partials); break;
    default: launch_spec_site<4>(vec, grid, st, Z, n, m, w, a, b, obs, prm, f, sw.h, sw.partials); break;
  }
  MGP_LAUNCH_CHECK();
  hipLaunchKernelGGL(spectral_sum_kernel, dim3((unsigned)mgp_cdiv(m + 2, kSumCols)), dim3(kBlock), 0, st, sw.partials, sw.blocks, m,
                     grad, sums);
  MGP_LAUNCH_CHECK();
  if (!with_hessian) return MGP_OK;
  hipLaunchKernelGGL(spectral_gram_kernel, dim3((unsigned)gram_pairs(m), (unsigned)sw.chunks), dim3(kBlock), 0, st, Z, sw.h, n, m,
                     sw.rows_per_chunk, sw.gpart);
  MGP_LAUNCH_CHECK();
  int sum_blocks = (int)mgp_cdiv((int64_t)m * m, kBlock);
  if (sum_blocks > 1024) sum_blocks = 1024;
  hipLaunchKernelGGL(spectral_gram_sum_kernel, dim3((unsigned)sum_blocks), dim3(kBlock), 0, st, sw.gpart, sw.chunks, m, hess);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
