// A thread's 16 elements of a kChunk-element chunk, loaded and stored with 16-byte accesses or one by
// one (layerwise.hip, averaging.hip). The blocks of those kernels have kChunkThreads threads, and a
// thread owns the same elements on both paths: groups of V consecutive elements, kChunkThreads groups
// apart.
#pragma once

#include "chunks.h"
#include "common.h"
#include "vec16.h"

namespace ptdt {

constexpr int kChunkThreads = 256;                  // threads of a block that walks a chunk this way
constexpr int kElems = kChunk / kChunkThreads;      // elements of a chunk per thread: 16

// Element e (< kElems) of this thread in a chunk whose threads own groups of V consecutive elements.
template <int V>
__device__ __forceinline__ int64_t elem_index(int64_t start, int e) {
  return start + (int64_t)((e / V) * kChunkThreads + (int)threadIdx.x) * V + (e % V);
}

// f[e] = x[elem_index<V>(start, e)]. FULL: the whole chunk exists and x is 16-byte aligned, 16-byte
// loads. Otherwise element loads, elements at or past `end` read as 0.
template <typename S, int V, bool FULL>
__device__ __forceinline__ void load_elems(const S* x, int64_t start, int64_t end, float* f) {
  constexpr int VS = Vec16<S>::N;
  static_assert(V % VS == 0 && kElems % V == 0, "groups are whole 16-byte vectors");
  if constexpr (FULL) {
    u32x4 w[kElems / VS];
#pragma unroll
    for (int q = 0; q < kElems / VS; ++q) w[q] = *(const u32x4 PTDT_GLOBAL*)(x + elem_index<V>(start, q * VS));
#pragma unroll
    for (int q = 0; q < kElems / VS; ++q) Vec16<S>::unpack(w[q], f + q * VS);
  } else {
#pragma unroll
    for (int e = 0; e < kElems; ++e) {
      const int64_t i = elem_index<V>(start, e);
      f[e] = i < end ? Cvt<S>::load(x, i) : 0.f;
    }
  }
}

template <typename S, int V, bool FULL>
__device__ __forceinline__ void store_elems(S* x, int64_t start, int64_t end, const float* f) {
  constexpr int VS = Vec16<S>::N;
  if constexpr (FULL) {
#pragma unroll
    for (int q = 0; q < kElems / VS; ++q)
      *(u32x4 PTDT_GLOBAL*)(x + elem_index<V>(start, q * VS)) = Vec16<S>::pack(f + q * VS);
  } else {
#pragma unroll
    for (int e = 0; e < kElems; ++e) {
      const int64_t i = elem_index<V>(start, e);
      if (i < end) Cvt<S>::store(x, i, f[e]);
    }
  }
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr,
                                          const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace ptdt
