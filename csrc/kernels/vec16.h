// One 16-byte global access of T, unpacked to floats and back (gradclip.hip, layerwise.hip).
#pragma once

#include "common.h"

namespace ptdt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte global access

template <typename T>
struct Vec16;  // 16 bytes of T unpacked to floats, and back
template <>
struct Vec16<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void unpack(const u32x4& w, float* f) {
    f[0] = __uint_as_float(w.x), f[1] = __uint_as_float(w.y), f[2] = __uint_as_float(w.z), f[3] = __uint_as_float(w.w);
  }
  __device__ __forceinline__ static u32x4 pack(const float* f) {
    return u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
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
};

}  // namespace ptdt
