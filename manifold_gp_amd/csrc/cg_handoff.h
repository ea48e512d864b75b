// Device code shared by the two kernels that can end a plan's first graph with the stopping decision: cg_update_c1_kernel<true>
// (cg.hip) and spmv_tile_cgstep_kernel<.., true> (spmm.hip).  The scalar block of a single-column solve and the hand-off of the
// deciding launch are written once, here.
#pragma once
#include "mgp_common.h"
#include "cg_rule.h"

// C == 1 layout of the scalar block (cg_carve: blk): fetched as one s_load_dwordx8.  Separate scalar
// loads are not batched by hipcc (each is followed by lgkmcnt(0)): five of them cost five round trips.
struct alignas(32) CgScalars {
  float go0, go1, ao0, ao1, bb, resid;
  int it, done;
};

// What the hand-off needs of a plan (CgArgs / MgpCgStep carry the same words)
struct CgHandoff {
  int* arrive;        // [9][32] arrival counters (8 groups + top, a 128-byte line each), zero between launches
  int* state;         // [1] done, [2] status, [5] graphs that ran to their end
  int* host_state;    // host-mapped: [4] end-of-graph mark, [8..9] the 8-byte decision record
  float* resid;
  float tol;
  int max_iter, min_iter, stop_mode;
};

// End-of-graph mark of a deciding launch whose workgroups all left before the hand-off (decided earlier, or deciding now)
__device__ __forceinline__ void cg_mark_end_of_graph(int* state, int* host_state) {
  const int c = state[5] + 1;
  state[5] = c;
  __threadfence_system();
  host_state[4] = c;
}

// The hand-off inside a deciding launch, called by EVERY thread of EVERY workgroup of the launch, behind the barrier that
// gave thread 0 its workgroup's ||r||^2 partial `o_r` (other threads pass anything).  Lane 0 of every workgroup
// stores the partial write-through (sc1) to rr_par[slot], drains its stores (s_waitcnt vmcnt(0)), makes one returning agent-scope
// atomic add on its group's arrival counter; the lane that completes the count joins the workgroup barrier, then all lanes of
// that workgroup read the `npart` partials with sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility, table of sc1
// hand-offs: "one lane of each storing workgroup ... the workgroup whose add came last, told by the value its add returned")
// and take the stopping decision of step it + 1 through cg_rule.h, the sums in cg_decide_c1_kernel<SLOTS>'s order.  The counter
// needs no reset between solves: in a launch either every workgroup arrives or none does, and the last arriver puts it back
// to zero.  No workgroup waits for another.  sh4: 4 floats of LDS, free for reuse once every thread is here; sh_last: one int.
template <int SLOTS>
__device__ __forceinline__ void cg_handoff_decide(const CgHandoff& h, float* rr_par, int npart, int slot, float o_r, int it, float bb,
                                                  float* sh4, int* sh_last) {
  constexpr int BS = 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    // write-through (sc1) store, drained, then the arrive; the last arriver reads the partials with sc1 loads below.
    // (An agent-scope release fence here writes back every dirty L2 line of the vectors this launch has just stored:
    // measured +3.4 us per solve against the separate decision launch it was meant to save.)
    __hip_atomic_store(&rr_par[slot], o_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // two levels (one word takes ~88 arrivals per us: 235 workgroups on it were 3 us of the launch): the workgroups
    // with equal blockIdx % 8 -- one XCD under round-robin placement, which only speed depends on -- count on a line of
    // their own, the last of each group counts on the top word
    const int grp = blockIdx.x & 7, members = ((int)gridDim.x - grp + 7) >> 3, groups = (int)gridDim.x < 8 ? (int)gridDim.x : 8;
    int last = 0;
    if (__hip_atomic_fetch_add(h.arrive + 32 * grp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
      __hip_atomic_store(h.arrive + 32 * grp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_fetch_add(h.arrive + 32 * 8, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1) {
        __hip_atomic_store(h.arrive + 32 * 8, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = 1;
      }
    }
    *sh_last = last;
  }
  __syncthreads();
  if (!*sh_last) return;
  // ---- the last arriver: stopping decision of step it + 1
  const int itn = it + 1;
  float t2 = 0.f;
#pragma unroll
  for (int q = 0; q < SLOTS; ++q) {
    const int b = tid + q * BS;
    const float v = __hip_atomic_load(&rr_par[b < npart ? b : npart - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t2 += (b < npart) ? v : 0.f;
  }
  t2 = mgp_wave_sum(t2);
  __syncthreads();                          // sh4 may have held the caller's wave sums: everyone has read sh_last / is done with them
  if (lane == 0) sh4[wave] = t2;
  __syncthreads();
  if (tid != 0) return;
  const float rr2n = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  const float reln = cg_rel(rr2n, bb);
  const CgStop stn = cg_stop(h.stop_mode, h.min_iter, h.max_iter, h.tol, itn, reln);
  // The host reads nothing but host-mapped words (the solution stays in stream order).  The decision travels as ONE
  // naturally aligned 8-byte record {residual bits, step << 8 | status << 4 | 3} at host_state[8..9], written by one store
  // instruction (one PCIe write, observed whole by the host's 8-byte read): no drain between "the details" and "the
  // flag" -- that wait for a host-memory write to be acknowledged was ~1 us of every solve -- and no
  // __threadfence_system(), which would also write back every dirty L2 line of the vectors this launch has just stored.
  // run_cg clears the record before every solve and unpacks it into the words the other deciding kernels write.
  const int c = h.state[5] + 1;
  h.state[5] = c;
  h.resid[0] = reln;                        // the only writer of this word in a deciding launch that goes on
  if (stn.done) {
    h.state[2] = stn.status; h.state[1] = 1;
    const unsigned long long rec = (unsigned long long)__builtin_bit_cast(unsigned, reln) |
                                   ((unsigned long long)(unsigned)((itn << 8) | (stn.status << 4) | 3) << 32);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(h.host_state + 8), rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __hip_atomic_store(h.host_state + 4, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);       // end-of-graph mark
}
