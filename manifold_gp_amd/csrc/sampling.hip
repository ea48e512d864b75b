// GMRF noise for exact sampling of the Matern precision (docs/kernels/sampling.md).
//
//   tau I + L_sym = G G^T,  G = [sqrt(tau) I | E]   (n x (n + M)),  for the undirected edge e = (a, b), a < b:
//     E[a, e] = + sqrt(S_ab dsqrt_b / dsqrt_a),   E[b, e] = - sqrt(S_ab dsqrt_a / dsqrt_b)
// so  Y = node_coef w_tag + E w_edge  is one row-parallel pass over the padded symmetric CSR: every edge sits in both of
// its rows, and both rows REGENERATE its noise from the counter-based generator keyed on the unordered pair -- no noise
// is stored, no atomics, no communication between rows.  Each row sums its own entries in a fixed order (lanes over
// entries in CSR order, then a fixed xor tree over those lanes), so repeated calls are bitwise equal.
//
// Generator (bit for bit what tests/_sampling_ref.py restates): Philox4x32-10, key (seed lo, seed hi); global sample
// index s = sample_offset + column, quad q = s >> 2; node counter (i, 0, q, tag), edge counter (min, max, q, 1); normal
// s & 3 from Box-Muller on the word pair p = (s & 3) >> 1: u, v = ((x >> 8) + 0.5) 2^-24, r = sqrt(-2 ln u),
// even s r cos(2 pi v), odd s r sin(2 pi v).
//
// Layout: a group of G lanes per row, QL lanes over sample quads x EL = G / QL lanes over the row's entries.  The
// QL lanes of one entry read the same (col, S, dsqrt[col]) (one address per entry lane: broadcast), each computes its
// own Philox quad.  With the edge term EL = 16 always (the reduction tree must not depend on S) and QL <= 4: S = 1..4 is
// one quad on a 16-lane group (the lap_pass form), S >= 13 a whole wave per row whose quad lanes loop over their quads.
#include <math.h>
#include "mgp_common.h"
#include "mgp_internal.h"

namespace {

constexpr int kBlock = 256;

struct Quad {
  float x, y, z, w;
};

__device__ __forceinline__ uint4 philox10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;   // one v_mad_u64_u32 each: high and low word together
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// u = (m + 1/2) 2^-24, m = x >> 8, has 25 significant bits: a float only for m < 2^23.  The rounding of u costs nothing
// where ln u is away from 0 (|error| <= 2^-25 / u); near u = 1 the series of ln(1 - t) in t = 1 - u (exact there, and its
// truncation error t^4 / 4 <= 2^-42) replaces logf.  One logf per pair and selects, no divergent branch.
// 2v = (2m + 1) 2^-24 is exact below 1; above, sincospi takes the exact 2v - 2 = -(2 (2^24 - m) - 1) 2^-24 (one period off).
constexpr float kTwoM24 = 5.9604644775390625e-8f;

__device__ __forceinline__ float box_muller_r(uint32_t x) {
  const uint32_t m = x >> 8;
  const float t = ((float)((1u << 24) - m) - 0.5f) * kTwoM24;
  const float lg = logf(((float)m + 0.5f) * kTwoM24);
  const float series = -(t + t * t * (0.5f + t * (1.0f / 3.0f)));
  return sqrtf(-2.0f * (t < 0.0009765625f ? series : lg));
}

__device__ __forceinline__ float box_muller_turns(uint32_t x) {
  const uint32_t m = x >> 8;
  return m < (1u << 23) ? (float)(2u * m + 1u) * kTwoM24 : -(float)(2u * ((1u << 24) - m) - 1u) * kTwoM24;
}

// the four normals of one Philox quad (samples 4q .. 4q + 3)
__device__ __forceinline__ Quad normals4(uint4 x) {
  Quad o;
  float s, c;
  float r = box_muller_r(x.x);
  sincospif(box_muller_turns(x.y), &s, &c);
  o.x = r * c;
  o.y = r * s;
  r = box_muller_r(x.z);
  sincospif(box_muller_turns(x.w), &s, &c);
  o.z = r * c;
  o.w = r * s;
  return o;
}

__device__ __forceinline__ float xor_sum(float v, int o) { return v + __shfl_xor(v, o, 64); }

__global__ __launch_bounds__(kBlock) void gmrf_noise_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, const float* __restrict__ vals,
                                                            const float* __restrict__ dsqrt, float node_coef, uint32_t tag,
                                                            int with_edges, uint32_t k0, uint32_t k1, int64_t offset, int S,
                                                            int G, int QL, float* __restrict__ Y) {
  const int lane = threadIdx.x & (G - 1);
  const int ql = lane % QL, el = lane / QL, EL = G / QL;
  const int64_t g0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G;
  const int64_t ng = ((int64_t)gridDim.x * blockDim.x) / G;
  const int64_t qfirst = offset >> 2, qlast = (offset + S - 1) >> 2;   // global quads this call touches
  const bool vec4 = ((offset | S) & 3) == 0;                           // whole quads, 16-byte aligned row slices
  for (int64_t r = g0; r < n; r += ng) {                               // group-uniform: the shuffles below are converged
    const int s0 = rowptr[r], s1 = rowptr[r + 1];
    const float dr = with_edges ? dsqrt[r] : 1.0f;
    for (int64_t qb = qfirst; qb <= qlast; qb += QL) {                 // group-uniform trip count
      const int64_t q = qb + ql;
      const bool live = q <= qlast;
      Quad acc = {0.f, 0.f, 0.f, 0.f};
      if (with_edges && live) {
        for (int i = s0 + el; i < s1; i += EL) {
          const int c = col[i];
          const float v = vals[i];
          if (c == (int)r || v == 0.0f) continue;                      // padding (col == row, S = 0)
          const float coef = sqrtf(v * dsqrt[c] / dr);
          const bool lo = (int)r < c;
          const Quad z = normals4(philox10(lo ? (uint32_t)r : (uint32_t)c, lo ? (uint32_t)c : (uint32_t)r, (uint32_t)q, 1u, k0, k1));
          const float e = lo ? coef : -coef;
          acc.x += e * z.x;
          acc.y += e * z.y;
          acc.z += e * z.z;
          acc.w += e * z.w;
        }
      }
      if (with_edges) {
        for (int o = QL; o < G; o <<= 1) {                             // fixed tree over the entry lanes
          acc.x = xor_sum(acc.x, o);
          acc.y = xor_sum(acc.y, o);
          acc.z = xor_sum(acc.z, o);
          acc.w = xor_sum(acc.w, o);
        }
      }
      if (el == 0 && live) {
        const Quad w = normals4(philox10((uint32_t)r, 0u, (uint32_t)q, tag, k0, k1));
        Quad y;
        y.x = node_coef * w.x + acc.x;
        y.y = node_coef * w.y + acc.y;
        y.z = node_coef * w.z + acc.z;
        y.w = node_coef * w.w + acc.w;
        const int64_t j0 = 4 * q - offset;                             // column of sample 4q (may be < 0 or the last quad may overrun S)
        float* yr = Y + r * (int64_t)S;
        if (vec4) {
          *reinterpret_cast<float4*>(yr + j0) = make_float4(y.x, y.y, y.z, y.w);
        } else {
          const float yy[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int64_t j = j0 + t;
            if (j >= 0 && j < S) yr[j] = yy[t];
          }
        }
      }
    }
  }
}

int pow2_ceil(int v) {
  int p = 1;
  while (p < v && p < 64) p <<= 1;
  return p;
}

}  // namespace

extern "C" int mgp_gmrf_noise(const mgp_csr_t* L, const float* dsqrt, float node_coef, int tag, int with_edges,
                              uint64_t seed, int64_t sample_offset, int S, float* Y, void* stream) {
  if (!L || !L->rowptr || !L->col || !L->vals || !dsqrt || !Y || !mgp_spmv_lanes_ok(L->spmv_lanes)) return MGP_ERR_ARG;
  if (S < 1 || L->n < 1 || L->n >= ((int64_t)1 << 31) || tag < 0 || sample_offset < 0) return MGP_ERR_ARG;
  if (with_edges != 0 && with_edges != 1) return MGP_ERR_ARG;
  if (((sample_offset + S) >> 2) >= ((int64_t)1 << 32)) return MGP_ERR_ARG;        // the quad index is one 32-bit word
  const int64_t n = L->n;
  const int nq = (int)(((sample_offset + S - 1) >> 2) - (sample_offset >> 2) + 1);
  // with edges: 16 entry lanes (the lap_pass group: ~4 entries each on rows of ~60) for EVERY S, so that a row's sum runs
  // through the same tree whatever the batch: column j of a call is bitwise the same in any chunking; up to 4 quad lanes,
  // each looping over its quads.  Without edges: lanes over quads only.
  const int EL = with_edges ? 16 : 1;
  const int QL = with_edges ? (pow2_ceil(nq) < 4 ? pow2_ceil(nq) : 4) : pow2_ceil(nq);
  const int G = QL * EL;
  const int64_t groups_per_block = kBlock / G;
  int64_t blocks = mgp_cdiv(n, groups_per_block);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(gmrf_noise_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, mgp_stream(stream), n, L->rowptr, L->col,
                     L->vals, dsqrt, node_coef, (uint32_t)tag, with_edges, (uint32_t)(seed & 0xffffffffu),
                     (uint32_t)(seed >> 32), sample_offset, S, G, QL, Y);
  MGP_LAUNCH_CHECK();
  return MGP_OK;
}
