// The row layout of the softmax kernels (laplace.hip: softmax_site_kernel; softmax_cg.hip: softmax_hess_kernel), stated once:
// a row of a row-major [n, C] block, 2 <= C <= 64, belongs to a group of TC lanes, TC the least power of two >= C, lane c of
// the group holding class c (lanes c >= C idle).  TC divides the wave, so a group never straddles two waves and its xor trees
// stay inside it; a workgroup of B threads takes B / TC rows per step.
#pragma once
#include <type_traits>
#include "mgp_common.h"

static inline int mgp_softmax_lanes(int C) {
  int tc = 2;
  while (tc < C) tc <<= 1;
  return tc;
}

// workgroups of `block` threads that cover n rows of C classes once, at most `cap` (the kernels stride beyond)
static inline int mgp_softmax_blocks(int64_t n, int C, int block, int cap) {
  const int64_t b = mgp_cdiv(n, (int64_t)(block / mgp_softmax_lanes(C)));
  return (int)(b > cap ? cap : b);
}

// fn(std::integral_constant<int, TC>) for the TC of C: the one switch over the six lane counts
template <typename Fn>
static inline void mgp_softmax_dispatch(int C, Fn&& fn) {
  switch (mgp_softmax_lanes(C)) {
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 8: fn(std::integral_constant<int, 8>{}); break;
    case 16: fn(std::integral_constant<int, 16>{}); break;
    case 32: fn(std::integral_constant<int, 32>{}); break;
    default: fn(std::integral_constant<int, 64>{}); break;
  }
}

// the group's value from its TC lanes'; every lane gets the same bits (the float sum is mgp_group_sum of mgp_common.h)
template <int TC>
__device__ __forceinline__ double mgp_group_max_d(double v) {
#pragma unroll
  for (int o = TC / 2; o > 0; o >>= 1) {
    const double other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}
template <int TC>
__device__ __forceinline__ double mgp_group_sum_d(double v) {
#pragma unroll
  for (int o = TC / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
