// Gradient clipping (gfx950): clip_grad_norm_ / clip_grad_value_ over lists of dense spans.
//
//   norm partials : one block per kChunk-element chunk -> one fp32 value in its own workspace slot
//   finalise      : one workgroup combines the slots in a fixed order -> {total_norm, clip_coef}
//   scale / clamp : the same span list, g *= clip_coef (skipped when it is exactly 1) / clamp
//
// No atomics, no memsets, no host reads: every kernel is hipGraph-capturable and gives the same
// bits for the same gradients at the same addresses. A chunk is 16 KiB of f32 (8 KiB of bf16):
// every thread issues all its 16-byte loads before it uses one, so the resident blocks of a CU
// keep well over the ~32 KiB in flight that a streaming read of HBM needs.
//
// The inf norm is taken on the bit patterns of |g|: for non-negative floats the unsigned order is
// the numeric order, and every NaN pattern lies above +inf, so a NaN wins the max and stays NaN.
#include "chunks.h"
#include "common.h"
#include "kernels.h"
#include "vec16.h"

namespace ptdt {
namespace {

constexpr int kBlock = 256;

// accumulator steps; an inf-norm accumulator is the bit pattern of a non-negative float
template <int NORM>
__device__ __forceinline__ float fold(float acc, float x) {
  if constexpr (NORM == kClipNorm2) {
    return fmaf(x, x, acc);
  } else {
    const uint32_t a = __float_as_uint(acc), b = __float_as_uint(x) & 0x7fffffffu;
    return __uint_as_float(a > b ? a : b);
  }
}
template <int NORM>
__device__ __forceinline__ float join(float a, float b) {
  if constexpr (NORM == kClipNorm2) {
    return a + b;
  } else {
    return __uint_as_float(max(__float_as_uint(a), __float_as_uint(b)));
  }
}

// bit-pattern max over the block (the DPP / permlane moves of common.h without their float max,
// which would drop a NaN); scratch: blockDim.x / 64 floats
__device__ __forceinline__ float block_bitmax(float v, float* scratch) {
  v = join<kClipNormInf>(v, dpp_f<kDppXor1>(v));
  v = join<kClipNormInf>(v, dpp_f<kDppXor2>(v));
  v = join<kClipNormInf>(v, dpp_f<kDppHalfMirror>(v));
  v = join<kClipNormInf>(v, dpp_f<kDppMirror>(v));
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
  v = join<kClipNormInf>(__int_as_float(p[0]), __int_as_float(p[1]));
  auto q = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
  v = join<kClipNormInf>(__int_as_float(q[0]), __int_as_float(q[1]));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < nw; ++i) r = join<kClipNormInf>(r, scratch[i]);
  return r;
}

template <typename T, int NORM>
__global__ void __launch_bounds__(kBlock) norm_partials_kernel(SpanList sl, float* __restrict__ ws,
                                                               int64_t first_slot) {
  __shared__ float scratch[kBlock / 64];
  int t;
  int64_t start;
  locate_chunk(sl.numel, sl.n, blockIdx.x, t, start);
  if (t >= sl.n) return;  // block-uniform
  const T* g = static_cast<const T*>(sl.p[t]);
  const int64_t end = min(start + (int64_t)kChunk, sl.numel[t]);
  constexpr int V = Vec16<T>::N;
  constexpr int kVecs = kChunk / V / kBlock;  // 16-byte loads per thread: 4 (f32), 2 (bf16)
  float a[4] = {0.f, 0.f, 0.f, 0.f};          // independent accumulators, joined in a fixed order
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    // chunk starts are multiples of kChunk elements, so the span pointer decides the alignment
    const int nvec = (int)((end - start) / V);
    const u32x4 PTDT_GLOBAL* gv = (const u32x4 PTDT_GLOBAL*)(g + start);
    u32x4 w[kVecs];
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int q = k * kBlock + threadIdx.x;
      w[k] = q < nvec ? gv[q] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      float f[V];
      Vec16<T>::unpack(w[k], f);
#pragma unroll
      for (int j = 0; j < V; ++j) a[j & 3] = fold<NORM>(a[j & 3], f[j]);
    }
    const int64_t i = start + (int64_t)nvec * V + threadIdx.x;  // tail: fewer than V elements
    if (i < end) a[0] = fold<NORM>(a[0], Cvt<T>::load(g, i));
  } else {
    int k = 0;
    for (int64_t i = start + threadIdx.x; i < end; i += kBlock, ++k)
      a[k & 3] = fold<NORM>(a[k & 3], Cvt<T>::load(g, i));
  }
  const float v = join<NORM>(join<NORM>(a[0], a[1]), join<NORM>(a[2], a[3]));
  const float r = NORM == kClipNorm2 ? block_sum(v, scratch) : block_bitmax(v, scratch);
  if (threadIdx.x == 0) ws[first_slot + blockIdx.x] = r;
}

__global__ void __launch_bounds__(kBlock) norm_finalize_kernel(const float* __restrict__ ws, int64_t n, int norm,
                                                               float max_norm, int partial,
                                                               float* __restrict__ rec) {
  __shared__ double ssum[kBlock];
  __shared__ uint32_t smax[kBlock];
  double s = 0.0;
  uint32_t m = 0u;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {  // loops when there are more slots than threads
    const float x = ws[i];
    s += (double)x;
    m = max(m, __float_as_uint(x));
  }
  ssum[threadIdx.x] = s;
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      ssum[threadIdx.x] += ssum[threadIdx.x + h];
      smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float total;
    if (norm == kClipNorm2)
      total = partial ? (float)ssum[0] : (float)sqrt(ssum[0]);
    else
      total = __uint_as_float(smax[0]);
    float coef = 1.f;
    if (!partial) {
      coef = max_norm / (total + 1e-6f);
      coef = coef > 1.f ? 1.f : coef;  // NaN stays NaN, as torch.clamp(max=1.0)
    }
    rec[0] = total;
    rec[1] = coef;
  }
}

enum { kOpScale = 0, kOpClamp = 1 };

// g = op(g) over the spans. kOpScale: g *= rec[1], nothing read or written when that is exactly 1.
// kOpClamp: g = min(max(g, -c), c) with NaN kept.
template <typename T, int OP>
__global__ void __launch_bounds__(kBlock) apply_spans_kernel(SpanList sl, const float* __restrict__ rec, float c) {
  float coef = 1.f;
  if constexpr (OP == kOpScale) {
    coef = rec[1];
    if (coef == 1.0f) return;  // a non-finite coefficient is applied
  }
  int t;
  int64_t start;
  locate_chunk(sl.numel, sl.n, blockIdx.x, t, start);
  if (t >= sl.n) return;
  T* g = static_cast<T*>(sl.p[t]);
  const int64_t end = min(start + (int64_t)kChunk, sl.numel[t]);
  auto op = [&](float x) {
    if constexpr (OP == kOpScale) {
      return x * coef;
    } else {
      x = x < -c ? -c : x;
      return x > c ? c : x;
    }
  };
  constexpr int V = Vec16<T>::N;
  constexpr int kVecs = kChunk / V / kBlock;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int nvec = (int)((end - start) / V);
    u32x4 PTDT_GLOBAL* gv = (u32x4 PTDT_GLOBAL*)(g + start);
    u32x4 w[kVecs];
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int q = k * kBlock + threadIdx.x;
      if (q < nvec) w[k] = gv[q];
    }
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int q = k * kBlock + threadIdx.x;
      if (q < nvec) {
        float f[V];
        Vec16<T>::unpack(w[k], f);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = op(f[j]);
        gv[q] = Vec16<T>::pack(f);
      }
    }
    const int64_t i = start + (int64_t)nvec * V + threadIdx.x;
    if (i < end) Cvt<T>::store(g, i, op(Cvt<T>::load(g, i)));
  } else {
    for (int64_t i = start + threadIdx.x; i < end; i += kBlock) Cvt<T>::store(g, i, op(Cvt<T>::load(g, i)));
  }
}

template <int OP>
hipError_t apply_spans(const SpanList& sl, int dtype, const float* rec, float c, hipStream_t s) {
  return dtype == kF32 ? launch_chunks(apply_spans_kernel<float, OP>, kBlock, sl, s, rec, c)
                       : launch_chunks(apply_spans_kernel<uint16_t, OP>, kBlock, sl, s, rec, c);
}

}  // namespace

hipError_t clip_norm_partials(const SpanList& sl, int dtype, int norm, float* ws, int64_t first_slot,
                              hipStream_t s) {
  if (chunk_blocks(sl) == 0) return hipSuccess;  // an empty list is accepted whatever the norm
  if (norm != kClipNorm2 && norm != kClipNormInf) return hipErrorInvalidValue;
  auto launch = [&](auto kernel) { return launch_chunks(kernel, kBlock, sl, s, ws, first_slot); };
  if (dtype == kF32)
    return norm == kClipNorm2 ? launch(norm_partials_kernel<float, kClipNorm2>)
                              : launch(norm_partials_kernel<float, kClipNormInf>);
  return norm == kClipNorm2 ? launch(norm_partials_kernel<uint16_t, kClipNorm2>)
                            : launch(norm_partials_kernel<uint16_t, kClipNormInf>);
}

hipError_t clip_norm_finalize(const float* ws, int64_t n, int norm, float max_norm, int partial, float* rec,
                              hipStream_t s) {
  if (n < 0 || (norm != kClipNorm2 && norm != kClipNormInf)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(kBlock), 0, s, ws, n, norm, max_norm, partial, rec);
  return hipGetLastError();
}

hipError_t clip_scale(const SpanList& sl, int dtype, const float* rec, hipStream_t s) {
  return apply_spans<kOpScale>(sl, dtype, rec, 0.f, s);
}

hipError_t clip_clamp(const SpanList& sl, int dtype, float c, hipStream_t s) {
  return apply_spans<kOpClamp>(sl, dtype, nullptr, c, s);
}

}  // namespace ptdt
