// Cross-workgroup hand-off of reduction partials: sc1 stores, a ticket, sc1 loads.
//
// Every workgroup writes its partials with st_sc1, then calls last_arrival on a ticket shared by the
// `count` workgroups that feed one result. It returns true in exactly one of them, the count-th
// arriver, which then reads everybody's partials with ld_sc1 / ld2_sc1 and finishes in a fixed order
// (deterministic whatever the arrival order). The last arriver re-arms the ticket (stores 0) right
// after its add: nobody else adds to it in this launch, and the next launch is ordered behind this
// one by the stream.
//
// Memory-model note (ISA-level, gfx950). The HIP/LLVM model gives relaxed atomics no happens-before,
// so correctness rests on the hardware, not the language:
//   (1) the partials are written with sc1 stores (agent-scope relaxed atomics: write-through to the
//       coherent level) and every storing wave waits vmcnt(0) before the workgroup barrier, so they
//       are globally visible before lane 0 issues the ticket add;
//   (2) the add's returned value names the last arriver; its other waves learn it through an LDS
//       word behind a second barrier;
//   (3) the last arriver reads the partials with sc1 loads, which miss the non-coherent caches. The
//       compiler cannot move those loads above the ticket: __syncthreads() after the flag write is a
//       workgroup-scope release/acquire fence pair, and the signal fence pins the order in the IR.
// tests/test_norm.py compares this hand-off bit for bit with the fence-based one on many-block shapes.
//
// Why not an agent-scope release fence: it writes back the XCD L2's dirty lines once per workgroup.
// Those lines are the kernel's own streaming output (the GEMM's output tiles, the backward's g
// tensor), so the fence is a per-workgroup cost at the tail of every launch: +110 us on a
// 401408 x 256 conv (profiles/r3_convbn.md). `fence = true` (PTDT_BN_FENCE=1, batchnorm.hip only,
// A/B measurements) selects that replaced form: plain stores and loads behind a release fence in
// every workgroup and an acquire fence in the last.
//
// Users, all following row 1 of the table "Hand-offs measured with sc1 loads" in MI355X_MICROARCH.md
// (one lane per workgroup adds to ONE unsharded counter; the last adder is told by the returned
// value; its other waves load after a barrier; 4-B sc1 stores, 4- or 8-B sc1 loads; memory from
// hipMalloc through the caching allocator):
//   * batchnorm.hip, bn_stats_kernel / bn_bwd_reduce_kernel: one ticket per channel tile, count =
//     row blocks (gridDim.x);
//   * gemm_big.hip, gemm_bn_stats_kernel: two levels, a ticket per (row-tile group, column tile) and
//     one per column tile;
//   * conv1x1_bn.hip, conv1x1_bn_stream_kernel: two levels, a ticket per (weight slab, workgroup
//     group) and one per slab.
// None of the three plainly meets that row's "one workgroup per CU" cell: the BatchNorm reductions
// launch ~1.5 512-thread workgroups per CU (a CU holds up to 4), the streaming conv is sized for 2
// per CU, and the tiled GEMM's residency follows its tile's LDS. The row was measured at one per CU;
// here the evidence is the bit-for-bit comparison with the fence arm above and the determinism tests
// of the conv+BN kernels, not the table.
#pragma once

#include "common.h"

namespace ptdt {

__device__ __forceinline__ void st_sc1(float* p, float v, bool fence = false) {
  if (fence) *p = v;
  else __hip_atomic_store(gptr_w(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p, bool fence = false) {
  if (fence) return *p;
  return __hip_atomic_load((float PTDT_GLOBAL*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// two consecutive floats (8-byte aligned) in one load
__device__ __forceinline__ void ld2_sc1(const float* p, float& x, float& y, bool fence = false) {
  uint64_t u;
  if (fence) u = *reinterpret_cast<const uint64_t*>(p);
  else u = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  x = __uint_as_float((uint32_t)u);
  y = __uint_as_float((uint32_t)(u >> 32));
}

// true in exactly one workgroup per ticket (the count-th arriver), after every workgroup's partial
// stores have landed; re-arms the ticket. sh_flag: one LDS word. Called by every thread.
__device__ __forceinline__ bool last_arrival(int* ticket, int count, int* sh_flag, bool fence = false) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's sc1 partial stores have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fence) {  // A/B: the replaced form (write-back of this XCD's L2 before the ticket)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const int prev = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == count - 1;
    if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (last && fence) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *sh_flag = last;
  }
  __syncthreads();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // no load of the partials is hoisted above this point
  return *sh_flag != 0;
}

}  // namespace ptdt
