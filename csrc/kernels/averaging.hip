// Weight averaging (gfx950): the EMA / SWA update of an fp32 average, a = a + w (p - a).
//
//   prepare : one single-wave launch reads the device int64 counter n (updates applied so far),
//             writes the weight w of this update as one float32 and stores n + 1
//   update  : one block per kChunk-element chunk; a = fmaf(w, p - a, a) on the fp32 average, the
//             source p fp32 or bf16; optionally two bf16 roundings of the new a in the same pass
//             (the autocast shadow, and the module's own parameter when the model is bf16)
//
// The update launches read w, never n, so no block can see the counter move under it and the
// increment needs no atomics. w is evaluated in double and rounded once. When w == 1.0f (the first
// update, and the plain copies of buffers against a constant-one slot) a block-uniform branch stores
// a = p exactly: fmaf(1, p - a, a) is not p. No atomics, no memsets, no host reads, no allocation:
// every launch is hipGraph-capturable. A thread owns the same 16 elements of a chunk whether it
// reaches them with 16-byte accesses (full chunk, every pointer 16-byte aligned; all loads issued
// before the first use) or one by one (tail chunk, unaligned view).
#include "chunk_elems.h"
#include "chunks.h"
#include "common.h"
#include "kernels.h"
#include "vec16.h"

namespace ptdt {
namespace {

constexpr int kBlock = kChunkThreads;
constexpr int kPrepareBlock = 64;  // one wave, lane 0 works

__global__ void __launch_bounds__(kPrepareBlock) avg_prepare_kernel(int64_t* __restrict__ n_dev,
                                                                    float* __restrict__ w_dev, int kind,
                                                                    double decay, int warmup) {
  if (threadIdx.x != 0) return;
  const int64_t n = *n_dev;
  double w = 1.0;  // n == 0: the first update is a copy
  if (n > 0) {
    if (kind == kAvgSwa) {
      w = 1.0 / (double)(n + 1);
    } else {
      double d = decay;
      if (warmup) d = fmin(d, (1.0 + (double)n) / (10.0 + (double)n));
      w = 1.0 - d;
    }
  }
  *w_dev = (float)w;
  *n_dev = n + 1;
}

// One chunk [start, end) of one pair. V: the group of consecutive elements a thread owns, the
// widest 16-byte vector among the operands (8 with a bf16 operand, else 4).
template <typename S, int V, bool FULL>
__device__ __forceinline__ void avg_chunk(float* a, const S* p, uint16_t* shadow, uint16_t* copy, int64_t start,
                                          int64_t end, float w) {
  float pf[kElems];
  if (w == 1.0f) {  // block-uniform: a = p, the old average is not read
    load_elems<S, V, FULL>(p, start, end, pf);
  } else {
    float af[kElems];
    load_elems<S, V, FULL>(p, start, end, pf);
    load_elems<float, V, FULL>(a, start, end, af);
#pragma unroll
    for (int e = 0; e < kElems; ++e) pf[e] = fmaf(w, pf[e] - af[e], af[e]);
  }
  store_elems<float, V, FULL>(a, start, end, pf);
  if constexpr (V == 8) {
    if (shadow != nullptr) store_elems<uint16_t, V, FULL>(shadow, start, end, pf);
    if (copy != nullptr) store_elems<uint16_t, V, FULL>(copy, start, end, pf);
  }
}

template <typename S>
__device__ __forceinline__ void avg_pair(float* a, const S* p, uint16_t* shadow, uint16_t* copy, int64_t start,
                                         int64_t numel, float w) {
  const int64_t end = min(start + (int64_t)kChunk, numel);
  const bool full = end - start == kChunk && aligned16(a, p, shadow, copy);
  constexpr bool kSrc16 = Vec16<S>::N == 8;
  if (kSrc16 || shadow != nullptr || copy != nullptr) {
    if (full)
      avg_chunk<S, 8, true>(a, p, shadow, copy, start, end, w);
    else
      avg_chunk<S, 8, false>(a, p, shadow, copy, start, end, w);
  } else if constexpr (!kSrc16) {
    if (full)
      avg_chunk<S, 4, true>(a, p, nullptr, nullptr, start, end, w);
    else
      avg_chunk<S, 4, false>(a, p, nullptr, nullptr, start, end, w);
  }
}

template <typename S>
__global__ void __launch_bounds__(kBlock) avg_update_multi_kernel(AvgList l, const float* __restrict__ w_dev) {
  int t;
  int64_t start;
  locate_chunk(l.numel, l.n, blockIdx.x, t, start);
  if (t >= l.n) return;  // block-uniform
  avg_pair<S>(l.a[t], static_cast<const S*>(l.p[t]), l.shadow[t], l.copy[t], start, l.numel[t], *w_dev);
}

template <typename S>
__global__ void __launch_bounds__(kBlock) avg_update_flat_kernel(float* a, const S* p, uint16_t* shadow,
                                                                 uint16_t* copy, int64_t numel,
                                                                 const float* __restrict__ w_dev) {
  const int64_t start = (int64_t)blockIdx.x * kChunk;
  if (start >= numel) return;
  avg_pair<S>(a, p, shadow, copy, start, numel, *w_dev);
}

}  // namespace

hipError_t avg_prepare(int64_t* n, float* w, int kind, double decay, int warmup, hipStream_t s) {
  if (n == nullptr || w == nullptr || (kind != kAvgSwa && kind != kAvgEma)) return hipErrorInvalidValue;
  if (kind == kAvgEma && !(decay > 0.0 && decay < 1.0)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(avg_prepare_kernel, dim3(1), dim3(kPrepareBlock), 0, s, n, w, kind, decay, warmup ? 1 : 0);
  return hipGetLastError();
}

hipError_t avg_update_multi(const AvgList& l, int src_dtype, const float* w, hipStream_t s) {
  if (l.n < 0 || l.n > kMaxTensorsPerLaunch || w == nullptr || (src_dtype != kF32 && src_dtype != kBF16))
    return hipErrorInvalidValue;
  for (int i = 0; i < l.n; ++i)
    if (l.numel[i] < 0 || (l.numel[i] > 0 && (l.a[i] == nullptr || l.p[i] == nullptr)) ||
        (src_dtype == kF32 && l.copy[i] != nullptr))
      return hipErrorInvalidValue;
  return src_dtype == kF32 ? launch_chunks(avg_update_multi_kernel<float>, kBlock, l, s, w)
                           : launch_chunks(avg_update_multi_kernel<uint16_t>, kBlock, l, s, w);
}

hipError_t avg_update_flat(float* a, const void* p, int src_dtype, uint16_t* shadow, uint16_t* copy, int64_t numel,
                           const float* w, hipStream_t s) {
  if (numel < 0 || w == nullptr || (src_dtype != kF32 && src_dtype != kBF16) ||
      (src_dtype == kF32 && copy != nullptr))
    return hipErrorInvalidValue;
  if (numel == 0) return hipSuccess;
  if (a == nullptr || p == nullptr) return hipErrorInvalidValue;
  const int64_t nb = (numel + kChunk - 1) / kChunk;
  if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
  if (src_dtype == kF32)
    hipLaunchKernelGGL(avg_update_flat_kernel<float>, dim3((unsigned)nb), dim3(kBlock), 0, s, a,
                       static_cast<const float*>(p), shadow, copy, numel, w);
  else
    hipLaunchKernelGGL(avg_update_flat_kernel<uint16_t>, dim3((unsigned)nb), dim3(kBlock), 0, s, a,
                       static_cast<const uint16_t*>(p), shadow, copy, numel, w);
  return hipGetLastError();
}

}  // namespace ptdt
