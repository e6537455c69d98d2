// Operand tiles in LDS for the LDS-DMA GEMMs (gemm_big.hip, int8_mm.hip, conv1x1_bn.hip): bank swizzle,
// staging loop, fragment read, waits, fence-free barrier and the K loops over two buffers. The arithmetic
// is plain host / device code, checked on the host (tools/lds_tile_check.cpp, tests/test_lds_tile.py).
//
// A tile is rows of ROW_BYTES bytes, each row ROW_BYTES / 16 chunks of 16 B. global_load_lds_dwordx4
// (16 B per lane, no VGPR round trip) fills 1 KiB of LDS linearly per wave-instruction, so the swizzle
// is applied to the per-lane SOURCE address and undone by the ds_read_b128 (the same involution).
// Chunk c of row r lives in slot swz(r, c) of the row, chosen so that the 16 lanes of a fragment read
// (16 consecutive rows, one logical chunk) hit 16 distinct 16-B slots of the 256-B bank row:
//   * rows of 128 B (bf16 BK = 64, int8 BKB = 128): two rows share a bank row, so the row pair
//     (r >> 1) & 7 is XORed into the 8 chunks: slot16 = 8 (r & 1) + (c ^ ((r >> 1) & 7));
//   * rows of >= 256 B: every row starts a bank row, so r & 15 is XORed into the chunk's low four
//     bits. (The (r >> 1) & 7 form left two rows of a read on one bank here: PMC SQ_LDS_BANK_CONFLICT
//     3.6-7.2M cycles per launch, profiles/r3_pmc_convbn_stream.md.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PTDT_TILE_FN __host__ __device__ __forceinline__ constexpr
#else
#define PTDT_TILE_FN inline constexpr
#endif

namespace ptdt {

template <int ROW_BYTES>
PTDT_TILE_FN int swz(int row, int chunk) {
  static_assert(ROW_BYTES == 128 || ROW_BYTES == 256 || ROW_BYTES == 512, "no checked form for this row");
  return ROW_BYTES == 128 ? chunk ^ ((row >> 1) & 7) : chunk ^ (row & 15);
}
// byte offset of logical chunk `chunk` of row `row`
template <int ROW_BYTES>
PTDT_TILE_FN int tile_off(int row, int chunk) {
  return row * ROW_BYTES + swz<ROW_BYTES>(row, chunk) * 16;
}

// The staging loop's map. THREADS threads fill a ROWS-row tile in stage_rounds() rounds; thread t of
// round i writes the 16 B at linear chunk p = i * THREADS + t of the image, which holds logical chunk
// staged_chunk(p).c of tile row .r (the swizzle is an involution).
template <int ROWS, int ROW_BYTES, int THREADS>
PTDT_TILE_FN int stage_rounds() {
  static_assert(ROWS * ROW_BYTES % (THREADS * 16) == 0, "tile not a whole number of DMA rounds");
  return ROWS * ROW_BYTES / (THREADS * 16);
}
struct TileChunk { int r, c; };
template <int ROW_BYTES>
PTDT_TILE_FN TileChunk staged_chunk(int p) {
  constexpr int LOG = ROW_BYTES == 128 ? 3 : ROW_BYTES == 256 ? 4 : 5;  // chunks per row: a power of two
  static_assert(ROW_BYTES == 16 << LOG, "add the row size");
  return {p >> LOG, swz<ROW_BYTES>(p >> LOG, p & ((1 << LOG) - 1))};
}

// MFMA row i of tile j of a pair of 16-row tiles <-> channel: lane group q = i / 4 of pair p = j / 2
// holds channels 32p + 8q .. +7 over its two tiles (one 16-B store per lane and pair). conv1x1_bn.hip
// lays its weight rows out so, conv1x1_bwd.hip the rows of W^T.
PTDT_TILE_FN int pair_channel(int j, int i) { return 32 * (j >> 1) + 8 * (i >> 2) + 4 * (j & 1) + (i & 3); }

}  // namespace ptdt

#if defined(__HIPCC__)
namespace ptdt {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

// at most N of this wave's vector-memory operations (LDS-DMAs, loads, stores) still in flight
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// this wave's LDS reads and writes retired
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// workgroup barrier without __syncthreads' fence, which would drain every in-flight DMA and store;
// nothing is scheduled across it
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Issue the LDS-DMAs of one ROWS-row tile: elements k0 .. (ROW_BYTES of them) of the global rows
// row_of(r) (r = tile row; row_of clamps edge rows, which are computed and never stored) of a matrix
// of E with rows ld elements apart. wid must be wave-uniform (readfirstlane): the LDS base of a DMA
// is, the hardware adds lane * 16.
template <int ROWS, int ROW_BYTES, int THREADS, class E, class RowOf>
__device__ __forceinline__ void stage_rows(const E* __restrict__ src, int64_t ld, int k0, uint8_t* lds_tile, int wid,
                                           int lane, RowOf row_of) {
#pragma unroll
  for (int i = 0; i < stage_rounds<ROWS, ROW_BYTES, THREADS>(); ++i) {
    const TileChunk s = staged_chunk<ROW_BYTES>(i * THREADS + wid * 64 + lane);
    const E* g = src + (int64_t)row_of(s.r) * ld + k0 + s.c * (16 / (int)sizeof(E));
    __builtin_amdgcn_global_load_lds((gbl_void*)g, (lds_void*)(lds_tile + (i * THREADS + wid * 64) * 16), 16, 0, 0);
  }
}

template <class V, int ROW_BYTES>
__device__ __forceinline__ V read_frag(const uint8_t* lds_tile, int row, int chunk) {
  static_assert(sizeof(V) == 16, "one chunk");
  return *reinterpret_cast<const V*>(lds_tile + row * ROW_BYTES + swz<ROW_BYTES>(row, chunk) * 16);
}

// The K loops over two LDS buffers of buf_bytes. The kernel supplies stage(kt, buf): issue K-tile
// kt's DMAs into buf. K-tile kt+1 is in flight (its DMAs counted on vmcnt) while K-tile kt is
// multiplied; waits are counted and barriers raw (never __syncthreads: its fence drains the prefetch).
//
// Double-buffered: every wave runs mult(buf) -- read the fragments, multiply them -- on each K-tile, two
// barriers per tile. vmcnt(VM), VM = DMAs per thread and K-tile, and the first barrier retire exactly
// tile kt; the second, after the fragment reads, frees buffer kt & 1 for tile kt+2.
template <int VM, class Stage, class Mult>
__device__ __forceinline__ void kloop_double_buffered(int nk, uint8_t* smem, int buf_bytes, Stage stage, Mult mult) {
  stage(0, smem);
  for (int kt = 0; kt < nk; ++kt) {
    const uint8_t* cur = smem + (kt & 1) * buf_bytes;
    if (kt + 1 < nk) {
      stage(kt + 1, smem + ((kt + 1) & 1) * buf_bytes);
      vm_wait<VM>();  // tile kt landed, kt+1 still in flight
    } else {
      vm_wait<0>();
    }
    __builtin_amdgcn_s_barrier();  // every wave's DMA of tile kt is visible
    __builtin_amdgcn_sched_barrier(0);
    mult(cur);
    lds_wait();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // buffer kt & 1 free for tile kt+2
  }
}

// Ping-pong (8 waves): the two waves sharing a SIMD (w and w+4, leader / follower) run half a tile
// apart: while one multiplies K-tile t from registers, its partner reads K-tile t's fragments from
// LDS, so the SIMD's matrix pipe always has one wave feeding it. Slots are separated by workgroup
// barriers; followers start one slot late. Tile t+1's DMA is issued at the start of slot 2t and
// retired (vmcnt(0)) before the barrier closing slot 2t+1: its buffer's previous tile (t-1) was last
// read in slot 2t-1, and its first reader starts in slot 2t+2.
// read(buf) fills the kernel's fragment registers, mma() multiplies them. One loop per role (same
// barrier count): the register allocator then sees the fragments live only from read to MFMAs.
template <class Stage, class Read, class Mma>
__device__ __forceinline__ void kloop_pingpong(int nk, uint8_t* smem, int buf_bytes, bool is_leader, Stage stage,
                                               Read read, Mma mma) {
  stage(0, smem);
  vm_wait<0>();
  __builtin_amdgcn_s_barrier();  // tile 0 visible
  __builtin_amdgcn_sched_barrier(0);
  auto prefetch = [&](int kt) {
    if (kt + 1 < nk) stage(kt + 1, smem + ((kt + 1) & 1) * buf_bytes);
  };
  auto multiply = [&]() {
    __builtin_amdgcn_s_setprio(1);
    mma();
    __builtin_amdgcn_s_setprio(0);
  };
  if (is_leader) {  // slot 2kt reads tile kt, slot 2kt+1 multiplies it
    for (int kt = 0; kt < nk; ++kt) {
      const uint8_t* cur = smem + (kt & 1) * buf_bytes;
      prefetch(kt);
      read(cur);
      lds_wait();
      wg_barrier();
      multiply();
      vm_wait<0>();  // tile kt+1 landed (own DMAs)
      wg_barrier();
    }
  } else {  // follower: slot 2kt multiplies tile kt-1, slot 2kt+1 reads tile kt
    for (int kt = 0; kt < nk; ++kt) {
      const uint8_t* cur = smem + (kt & 1) * buf_bytes;
      prefetch(kt);
      if (kt > 0) multiply();
      wg_barrier();
      read(cur);
      lds_wait();
      vm_wait<0>();
      wg_barrier();
    }
    mma();
  }
}

}  // namespace ptdt
#endif
