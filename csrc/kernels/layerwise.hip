// Layer-wise adaptive optimizers (gfx950): LARS on momentum SGD, LAMB on Adam.
//
//   partials : one block per kChunk-element chunk -> two fp32 sums in that chunk's own workspace slots
//              (LARS: sum p^2, sum g^2; LAMB: the moment update, then sum p^2, sum u^2)
//   finalise : one wave per tensor combines its slots in a fixed order (float64) -> ratio, w, n
//   update   : LARS: the multi-tensor SGD body with d = ratio[t] * (g' + wd p) (sgd_multi.h);
//              LAMB: u recomputed from the stored moments, p -= lr ratio[t] u
//
// No atomics, no memsets, no host reads: every kernel is hipGraph-capturable. A thread owns the same
// 16 elements of a chunk and adds them in the same order whether it reaches them with 16-byte loads
// (full chunk, all pointers 16-byte aligned) or one by one (tail chunk, unaligned view), so the sums
// and with them the ratios depend on the values alone, not on where a tensor lies. In the 16-byte
// form every thread issues all its loads (8 for LARS, 16 for LAMB on f32) before it uses one.
#include "chunk_elems.h"
#include "chunks.h"
#include "common.h"
#include "kernels.h"
#include "sgd_multi.h"
#include "vec16.h"

namespace ptdt {
namespace {

constexpr int kBlock = kSgdBlock;  // kElems (chunk_elems.h) elements of a chunk per thread: 16
static_assert(kBlock == kChunkThreads, "load_elems / store_elems walk a chunk with this block size");
constexpr int kFinalBlock = 64;          // the finalise: one wave per tensor

// the two sums of a thread's elements: four accumulators each, joined in a fixed order
struct Sum2 {
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  __device__ __forceinline__ void add(int e, float x, float y) {
    a[e & 3] = fmaf(x, x, a[e & 3]);
    b[e & 3] = fmaf(y, y, b[e & 3]);
  }
  __device__ __forceinline__ float2 total() const {
    return make_float2((a[0] + a[1]) + (a[2] + a[3]), (b[0] + b[1]) + (b[2] + b[3]));
  }
};

__device__ __forceinline__ void write_partials(float2 v, float* scratch, float* ws, int64_t first_slot) {
  const float2 r = block_sum2(v, scratch);
  if (threadIdx.x == 0) {
    ws[2 * (first_slot + blockIdx.x)] = r.x;
    ws[2 * (first_slot + blockIdx.x) + 1] = r.y;
  }
}

// ---------------------------------------------------------------- LARS partials
template <typename T, bool FULL>
__device__ __forceinline__ float2 lars_chunk(const T* p, const T* g, int64_t start, int64_t end) {
  constexpr int V = Vec16<T>::N;
  float pf[kElems], gf[kElems];
  load_elems<T, V, FULL>(p, start, end, pf);
  load_elems<T, V, FULL>(g, start, end, gf);
  Sum2 s;
#pragma unroll
  for (int e = 0; e < kElems; ++e) s.add(e, pf[e], gf[e]);  // elements past the end were read as 0
  return s.total();
}

// ws[2 (first_slot + b)] = sum p^2, ws[.. + 1] = sum g^2 of block b's chunk; g is the raw gradient,
// the finalise applies |gscale * gcoef|
template <typename T>
__global__ void __launch_bounds__(kBlock) lars_partials_kernel(TensorList tl, float* __restrict__ ws,
                                                               int64_t first_slot) {
  __shared__ float scratch[2 * kBlock / 64];
  int t;
  int64_t start;
  locate_chunk(tl.numel, tl.n, blockIdx.x, t, start);
  if (t >= tl.n) return;  // block-uniform
  const T* p = static_cast<const T*>(tl.p[t]);
  const T* g = static_cast<const T*>(tl.g[t]);
  const int64_t end = min(start + (int64_t)kChunk, tl.numel[t]);
  const bool full = end - start == kChunk && aligned16(p, g);
  const float2 v = full ? lars_chunk<T, true>(p, g, start, end) : lars_chunk<T, false>(p, g, start, end);
  write_partials(v, scratch, ws, first_slot);
}

// ---------------------------------------------------------------- LAMB
__device__ __forceinline__ void lamb_corrections(const LambHyper& h, const int32_t* step, float& bc1, float& bc2s) {
  bc1 = 1.f, bc2s = 1.f;
  if (h.bias_correction) {
    const float st = (float)(*step);
    bc1 = 1.f - powf(h.b1, st);
    bc2s = sqrtf(1.f - powf(h.b2, st));
  }
}

// The LAMB update direction from the moments as stored; adam_update's denominator (optim.hip). Both
// passes call this with the same bits in (m and v are stored as f32 and p is untouched in between),
// and every operation is spelled out so that no contraction can differ between the two call sites.
__device__ __forceinline__ float lamb_direction(float p, float m, float v, float bc1, float bc2s,
                                                const LambHyper& h) {
  const float denom = sqrtf(v) / bc2s + h.eps;
  return fmaf(h.wd, p, (m / bc1) / denom);
}

template <typename T, bool FULL>
__device__ __forceinline__ float2 lamb_moments_chunk(const T* p, const T* g, float* m, float* v, int64_t start,
                                                     int64_t end, float bc1, float bc2s, const LambHyper& h) {
  constexpr int V = Vec16<T>::N;
  float pf[kElems], gf[kElems], mf[kElems], vf[kElems];
  load_elems<T, V, FULL>(p, start, end, pf);
  load_elems<T, V, FULL>(g, start, end, gf);
  load_elems<float, V, FULL>(m, start, end, mf);
  load_elems<float, V, FULL>(v, start, end, vf);
  Sum2 s;
#pragma unroll
  for (int e = 0; e < kElems; ++e) {
    const float ge = gf[e] * h.gscale;
    mf[e] = h.b1 * mf[e] + (1.f - h.b1) * ge;
    vf[e] = h.b2 * vf[e] + (1.f - h.b2) * ge * ge;
    if (FULL || elem_index<V>(start, e) < end) s.add(e, pf[e], lamb_direction(pf[e], mf[e], vf[e], bc1, bc2s, h));
  }
  store_elems<float, V, FULL>(m, start, end, mf);
  store_elems<float, V, FULL>(v, start, end, vf);
  return s.total();
}

// m, v updated and stored; ws[2 (first_slot + b)] = sum p^2, ws[.. + 1] = sum u^2 of block b's chunk
template <typename T>
__global__ void __launch_bounds__(kBlock) lamb_moments_kernel(TensorList tl, const int32_t* step, LambHyper h,
                                                              const float* gcoef, float* __restrict__ ws,
                                                              int64_t first_slot) {
  __shared__ float scratch[2 * kBlock / 64];
  if (gcoef != nullptr) h.gscale *= *gcoef;
  int t;
  int64_t start;
  locate_chunk(tl.numel, tl.n, blockIdx.x, t, start);
  if (t >= tl.n) return;  // block-uniform
  float bc1, bc2s;
  lamb_corrections(h, step, bc1, bc2s);
  const T* p = static_cast<const T*>(tl.p[t]);
  const T* g = static_cast<const T*>(tl.g[t]);
  float* m = tl.s1[t];
  float* v = tl.s2[t];
  const int64_t end = min(start + (int64_t)kChunk, tl.numel[t]);
  const bool full = end - start == kChunk && aligned16(p, g, m, v);
  const float2 s = full ? lamb_moments_chunk<T, true>(p, g, m, v, start, end, bc1, bc2s, h)
                        : lamb_moments_chunk<T, false>(p, g, m, v, start, end, bc1, bc2s, h);
  write_partials(s, scratch, ws, first_slot);
}

template <typename T, bool FULL>
__device__ __forceinline__ void lamb_update_chunk(T* p, const float* m, const float* v, int64_t start, int64_t end,
                                                  float bc1, float bc2s, float scale, const LambHyper& h) {
  constexpr int V = Vec16<T>::N;
  float pf[kElems], mf[kElems], vf[kElems];
  load_elems<T, V, FULL>(p, start, end, pf);
  load_elems<float, V, FULL>(m, start, end, mf);
  load_elems<float, V, FULL>(v, start, end, vf);
#pragma unroll
  for (int e = 0; e < kElems; ++e) pf[e] = fmaf(-scale, lamb_direction(pf[e], mf[e], vf[e], bc1, bc2s, h), pf[e]);
  store_elems<T, V, FULL>(p, start, end, pf);
}

// p -= lr * ratio[t] * u
template <typename T>
__global__ void __launch_bounds__(kBlock) lamb_update_kernel(TensorList tl, const int32_t* step, LambHyper h,
                                                             const float* lr_dev, const float* __restrict__ ratio) {
  if (lr_dev != nullptr) h.lr = *lr_dev;
  int t;
  int64_t start;
  locate_chunk(tl.numel, tl.n, blockIdx.x, t, start);
  if (t >= tl.n) return;
  float bc1, bc2s;
  lamb_corrections(h, step, bc1, bc2s);
  T* p = static_cast<T*>(tl.p[t]);
  const float* m = tl.s1[t];
  const float* v = tl.s2[t];
  const float scale = h.lr * ratio[t];
  const int64_t end = min(start + (int64_t)kChunk, tl.numel[t]);
  if (end - start == kChunk && aligned16(p, m, v))
    lamb_update_chunk<T, true>(p, m, v, start, end, bc1, bc2s, scale, h);
  else
    lamb_update_chunk<T, false>(p, m, v, start, end, bc1, bc2s, scale, h);
}

// ---------------------------------------------------------------- finalise
// Block t: the slots of tensor t are the chunks before it in the launch (the prefix walk of
// locate_chunk) plus first_slot. Lane l adds slots l, l + 64, ... in float64, then a fixed tree.
__global__ void __launch_bounds__(kFinalBlock) trust_finalize_kernel(NumelList nl, const float* __restrict__ ws,
                                                                     int64_t first_slot, TrustRule r,
                                                                     const float* gcoef, float* __restrict__ rec,
                                                                     int64_t first_tensor, int64_t tensors) {
  __shared__ double sp[kFinalBlock], sq[kFinalBlock];
  const int t = blockIdx.x;
  if (t >= nl.n) return;
  int64_t slot = first_slot;
  for (int k = 0; k < t; ++k) slot += (nl.numel[k] + kChunk - 1) / kChunk;
  const int64_t chunks = (nl.numel[t] + kChunk - 1) / kChunk;
  const float2* pair = reinterpret_cast<const float2*>(ws) + slot;  // ws + 2 slot: 8-byte aligned with ws
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < chunks; i += kFinalBlock) {
    const float2 x = pair[i];
    a += (double)x.x;
    b += (double)x.y;
  }
  sp[threadIdx.x] = a;
  sq[threadIdx.x] = b;
  __syncthreads();
  for (int h = kFinalBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sp[threadIdx.x] += sp[threadIdx.x + h];
      sq[threadIdx.x] += sq[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double w = sqrt(sp[0]);
    double n = sqrt(sq[0]);
    double ratio = 1.0;
    if (r.kind == kTrustLars) {
      float gs = r.gscale;
      if (gcoef != nullptr) gs *= *gcoef;
      n *= fabs((double)gs);
      if (w > 0.0 && n > 0.0) ratio = (double)r.coef * w / (n + (double)r.wd * w + (double)r.eps);
    } else if (r.adapt && w > 0.0 && n > 0.0) {
      ratio = w / n;
    }
    rec[first_tensor + t] = (float)ratio;
    rec[tensors + first_tensor + t] = (float)w;
    rec[2 * tensors + first_tensor + t] = (float)n;
  }
}

// The LARS update: sgd_multi_kernel's body with the trust ratio of each tensor (ratio[t], t in the launch).
template <typename T>
__global__ void __launch_bounds__(kBlock) lars_update_kernel(TensorList tl, const int32_t* step, SgdHyper h,
                                                             const float* gcoef, const float* lr_dev,
                                                             const float* ratio) {
  sgd_multi_body<T, true>(tl, step, h, gcoef, lr_dev, ratio);
}

}  // namespace

hipError_t lars_partials(const TensorList& tl, int dtype, float* ws, int64_t first_slot, hipStream_t s) {
  return dtype == kF32 ? launch_chunks(lars_partials_kernel<float>, kBlock, tl, s, ws, first_slot)
                       : launch_chunks(lars_partials_kernel<uint16_t>, kBlock, tl, s, ws, first_slot);
}

hipError_t trust_finalize(const TensorList& tl, const float* ws, int64_t first_slot, const TrustRule& r,
                          const float* gcoef, float* rec, int64_t first_tensor, int64_t tensors, hipStream_t s) {
  if (tl.n <= 0) return hipSuccess;
  if (tl.n > kMaxTensorsPerLaunch || first_slot < 0 || first_tensor < 0 || first_tensor + tl.n > tensors ||
      (r.kind != kTrustLars && r.kind != kTrustLamb))
    return hipErrorInvalidValue;
  NumelList nl{};
  nl.n = tl.n;
  for (int i = 0; i < tl.n; ++i) nl.numel[i] = tl.numel[i];
  hipLaunchKernelGGL(trust_finalize_kernel, dim3(tl.n), dim3(kFinalBlock), 0, s, nl, ws, first_slot, r, gcoef, rec,
                     first_tensor, tensors);
  return hipGetLastError();
}

hipError_t lars_update(const TensorList& tl, int dtype, const int32_t* step, const SgdHyper& h, const float* gcoef,
                       const float* lr_dev, const float* ratio, hipStream_t s) {
  return dtype == kF32 ? launch_chunks(lars_update_kernel<float>, kBlock, tl, s, step, h, gcoef, lr_dev, ratio)
                       : launch_chunks(lars_update_kernel<uint16_t>, kBlock, tl, s, step, h, gcoef, lr_dev, ratio);
}

hipError_t lamb_moments(const TensorList& tl, int dtype, const int32_t* step, const LambHyper& h, const float* gcoef,
                        float* ws, int64_t first_slot, hipStream_t s) {
  return dtype == kF32 ? launch_chunks(lamb_moments_kernel<float>, kBlock, tl, s, step, h, gcoef, ws, first_slot)
                       : launch_chunks(lamb_moments_kernel<uint16_t>, kBlock, tl, s, step, h, gcoef, ws, first_slot);
}

hipError_t lamb_update(const TensorList& tl, int dtype, const int32_t* step, const LambHyper& h, const float* lr_dev,
                       const float* ratio, hipStream_t s) {
  return dtype == kF32 ? launch_chunks(lamb_update_kernel<float>, kBlock, tl, s, step, h, lr_dev, ratio)
                       : launch_chunks(lamb_update_kernel<uint16_t>, kBlock, tl, s, step, h, lr_dev, ratio);
}

}  // namespace ptdt
