// One 16-byte global access of T, unpacked to floats and back: the vector I/O of the NHWC kernels
// (batchnorm.hip, pool.hip) and of the flat elementwise / reduction kernels (gradclip.hip,
// layerwise.hip, averaging.hip, eval_metrics.hip).
#pragma once

#include "common.h"

namespace ptdt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte global access

// 16 bytes of T unpacked to N floats, and back; load / store take a 16-byte aligned pointer
template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void unpack(const u32x4& w, float* f) {
    f[0] = __uint_as_float(w.x), f[1] = __uint_as_float(w.y), f[2] = __uint_as_float(w.z), f[3] = __uint_as_float(w.w);
  }
  __device__ __forceinline__ static u32x4 pack(const float* f) {
    return u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
  }
  __device__ __forceinline__ static void load(const float* p, float* f) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    unpack(u32x4{u.x, u.y, u.z, u.w}, f);
  }
  __device__ __forceinline__ static void store(float* p, const float* f) {
    const u32x4 w = pack(f);
    *reinterpret_cast<uint4*>(p) = uint4{w.x, w.y, w.z, w.w};
  }
};
template <>
struct Vec16<uint16_t> {
  static constexpr int N = 8;
  __device__ __forceinline__ static void unpack(const u32x4& w, float* f) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = __uint_as_float(u[k] << 16);
      f[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
    }
  }
  __device__ __forceinline__ static u32x4 pack(const float* f) {
    return u32x4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                 pack_bf16x2(f[6], f[7])};
  }
  __device__ __forceinline__ static void load(const uint16_t* p, float* f) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    unpack(u32x4{u.x, u.y, u.z, u.w}, f);
  }
  __device__ __forceinline__ static void store(uint16_t* p, const float* f) {
    const u32x4 w = pack(f);
    *reinterpret_cast<uint4*>(p) = uint4{w.x, w.y, w.z, w.w};
  }
};

// T-rounded value (what a T tensor holds): identity for f32
template <typename T>
__device__ __forceinline__ float round_to(float v) {
  if constexpr (sizeof(T) == 4) return v;
  else return bf16_to_f32(f32_to_bf16(v));
}

}  // namespace ptdt
