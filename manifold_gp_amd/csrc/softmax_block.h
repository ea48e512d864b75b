// The layout of the block softmax solver (softmax_cg_block.hip; docs/kernels/classification.md, "Samples in blocks"), stated
// once.  Host arithmetic only: this header compiles with a host compiler alone (tests/test_softmax_block_cpu.py).
//
// S systems share A = Q2 (x) I_C + H(pi).  Their vectors are row-major [n, S, C]: node i, sample s, class c at (i S + s) C + c,
// so the operator chain sees one block of S C columns and the epilogue sees n S rows of C floats, row q = i S + s, whose
// pi row is q / S and whose sample is q % S.
//
// Epilogue.  A group of TC lanes (softmax_rows.h) owns a row; a workgroup of kBlkThreads threads has kBlkThreads / TC groups.
// Group g of workgroup b has the launch-wide index j = b rows_per_block + g and takes the rows j, j + stride, j + 2 stride ...
// with stride = grid rows_per_block.  The grid is a multiple of S / gcd(S, rows_per_block), so S divides the stride: a group
// keeps the sample j % S for the whole launch (its per-sample sums stay in two registers) and its node advances by stride / S
// per pass, while a workgroup's groups still cover consecutive rows of every pass.  The workgroup adds its groups' sums
// per sample, groups in ascending order, and writes one pair per sample: slot (s, b) of [S][grid][2].
//
// Update.  Thread t of workgroup b starts at element e = b kBlkThreads + t and strides by grid kBlkThreads.  The grid is a
// multiple of S C / gcd(S C, kBlkThreads), so S C divides the stride and the thread keeps the sample (e / C) % S.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "mgp_arena.h"

#if defined(__HIPCC__)
#define SBLK_FN __host__ __device__ __forceinline__
#else
#define SBLK_FN static inline
#endif

enum {
  kBlkThreads = 256,          // threads of every workgroup of the three kernels
  kBlkMaxCols = 256,          // S C <= 256: the operator path's column cap
  kBlkMaxClasses = 64,
  kBlkHessMaxBlocks = 1024,   // grid caps (the kernels stride beyond)
  kBlkUpdateMaxBlocks = 1024,
};

static inline bool sblk_shape_ok(int C, int S) {
  return C >= 2 && C <= kBlkMaxClasses && S >= 1 && (int64_t)S * C <= kBlkMaxCols;
}

static inline int sblk_lanes(int C) {       // mgp_softmax_lanes, restated without the HIP include of softmax_rows.h
  int tc = 2;
  while (tc < C) tc <<= 1;
  return tc;
}

static inline int64_t sblk_gcd(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

// the largest grid <= cap that is a multiple of `unit` and no larger than `want` rounded up to one
static inline int sblk_grid(int64_t want, int unit, int cap) {
  const int64_t top = (int64_t)(cap / unit) * unit;
  const int64_t g = mgp_cdiv(want, (int64_t)unit) * unit;
  return (int)(g > top ? top : g);
}

struct SblkHess {
  int tc;                  // lanes per row
  int rows_per_block;      // lane groups of a workgroup
  int grid;
  int64_t stride;          // rows between two passes of a group: grid rows_per_block, a multiple of S
  int64_t node_step;       // stride / S
  int64_t passes;          // ceil(n S / stride)
};

static inline SblkHess sblk_hess(int64_t n, int C, int S) {
  SblkHess h;
  h.tc = sblk_lanes(C);
  h.rows_per_block = kBlkThreads / h.tc;
  const int unit = (int)(S / sblk_gcd(S, h.rows_per_block));
  h.grid = sblk_grid(mgp_cdiv(n * S, (int64_t)h.rows_per_block), unit, kBlkHessMaxBlocks);
  h.stride = (int64_t)h.grid * h.rows_per_block;
  h.node_step = h.stride / S;
  h.passes = mgp_cdiv(n * S, h.stride);
  return h;
}

// launch-wide index j of group g of workgroup b: its sample is j % S, its first node j / S
SBLK_FN int64_t sblk_group(const SblkHess& h, int b, int g) { return (int64_t)b * h.rows_per_block + g; }

// the first group of workgroup b that holds sample s (the others follow at g + S, g + 2 S ...); >= rows_per_block: none
SBLK_FN int sblk_first_group(const SblkHess& h, int S, int b, int s) {
  const int at = (int)(((int64_t)b * h.rows_per_block) % S);
  return (s - at + S) % S;
}

// partial pair of (sample s, workgroup b) in doubles, for a launch of `grid` workgroups
SBLK_FN size_t sblk_slot(int s, int b, int grid) { return 2 * ((size_t)s * grid + b); }
static inline size_t sblk_partial_doubles(int S) { return 2 * (size_t)S * kBlkHessMaxBlocks; }

struct SblkUpdate {
  int grid;
  int64_t stride;          // elements between two passes of a thread: grid kBlkThreads, a multiple of S C
};

static inline SblkUpdate sblk_update(int64_t n, int C, int S) {
  SblkUpdate u;
  const int cols = S * C;
  const int unit = (int)(cols / sblk_gcd(cols, kBlkThreads));
  u.grid = sblk_grid(mgp_cdiv(n * cols, (int64_t)kBlkThreads), unit, kBlkUpdateMaxBlocks);
  u.stride = (int64_t)u.grid * kBlkThreads;
  return u;
}

// device words of a block solve: one header and one entry per sample
struct SblkHead {
  int done, status, step;   // the flag the launches skip on, the status word, the step of the decision
  int pad;
};
struct SblkSample {
  float gamma[2], alpha[2]; // slot k & 1 holds the scalars of step k
  int it[2];                // updates applied after step k
  float bb, rel;            // ||b_s||^2, the relative residual of the last decision
};

static inline size_t sblk_state_bytes(int S) { return sizeof(SblkHead) + (size_t)S * sizeof(SblkSample); }

struct SblkCarve {
  float *R, *P, *Sv, *W;    // [n, S, C] each
  double* partials;         // [S][grid][2]
  double* sums;             // [S][2]: gamma_s, delta_s
  char* state;              // SblkHead, then SblkSample[S]
  char* opwork;
  size_t opbytes;
};

// the one statement of the solver's workspace: a counting arena sizes it, a real one hands it out
static inline bool sblk_carve(MgpArena& ar, int64_t n, int C, int S, size_t opbytes, SblkCarve* cv) {
  const size_t len = (size_t)n * S * C;
  cv->R = ar.take<float>(len);
  cv->P = ar.take<float>(len);
  cv->Sv = ar.take<float>(len);
  cv->W = ar.take<float>(len);
  cv->partials = ar.take<double>(sblk_partial_doubles(S));
  cv->sums = ar.take<double>(2 * (size_t)S);
  cv->state = ar.take<char>(sblk_state_bytes(S));
  cv->opbytes = opbytes;
  cv->opwork = ar.take<char>(opbytes);
  return ar.ok();
}

// ... and of the epilogue's test entry: the partials alone
static inline bool sblk_carve_hess(MgpArena& ar, int S, double** partials) {
  *partials = ar.take<double>(sblk_partial_doubles(S));
  return ar.ok();
}
