// The operand path of the linked conv + BN backwards (conv1x1_bwd_tiled.hip, conv3x3_bwd.hip): the BN's
// coefficients applied to 16-B chunks of g and y on their way to LDS (dY = A g + B y + C, rounded to bf16,
// never stored), the LDS-DMA of a [64][128] image with clamped edge columns, and the transposing fragment
// read of a row-major image. Device code only; the swizzle and staging arithmetic is lds_tile.h's.
#pragma once

#include "common.h"
#include "lds_tile.h"

namespace ptdt {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;

struct Coef8 {
  f32x4_t a[2], b[2], c[2];
};
// coefficients of channels n .. n + 7 (n % 8 == 0) of coef[3][N]
__device__ __forceinline__ Coef8 load_coef(const float* __restrict__ coef, int N, int n) {
  Coef8 k;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    k.a[h] = *reinterpret_cast<const f32x4_t*>(coef + n + 4 * h);
    k.b[h] = *reinterpret_cast<const f32x4_t*>(coef + N + n + 4 * h);
    k.c[h] = *reinterpret_cast<const f32x4_t*>(coef + 2 * (int64_t)N + n + 4 * h);
  }
  return k;
}
// 8 channels of dY from 16-B chunks of g and y; !valid: zeros (not C)
__device__ __forceinline__ u32x4_t dy_chunk(u32x4_t gv, u32x4_t yv, const Coef8& k, bool valid) {
  float d[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float gg = bf16_to_f32((uint16_t)(gv[e >> 1] >> (16 * (e & 1))));
    const float yy = bf16_to_f32((uint16_t)(yv[e >> 1] >> (16 * (e & 1))));
    d[e] = valid ? fmaf(k.a[e >> 2][e & 3], gg, fmaf(k.b[e >> 2][e & 3], yy, k.c[e >> 2][e & 3])) : 0.f;
  }
  u32x4_t pk;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const f32x2_t f = {d[2 * h], d[2 * h + 1]};
    pk[h] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
  }
  return pk;
}

// LDS-DMA of a [64][128] bf16 image by THREADS threads: columns c0 .. c0 + 127 of the rows row_of(r) of a
// matrix with rows ld elements apart; 16-B chunks past the last one to read (cmax) re-read that one.
template <int THREADS, class RowOf>
__device__ __forceinline__ void stage_image(const uint16_t* __restrict__ src, int64_t ld, int c0, int cmax,
                                            uint8_t* img, int wid, int lane, RowOf row_of) {
  stage_rows<64, 256, THREADS>(src, ld, c0, img, wid, lane, row_of, [=](int e) { return c0 + e < cmax ? e : cmax - c0; });
}

// MFMA fragment of the transpose of a row-major image with rows of ROW_BYTES: lane fr of a 16-lane group
// receives, for reduction rows rb0 .. rb0 + 7 (rb0 = rb - tq), the column that lane group fr >> 2 addresses,
// element fr & 3. (chunk, half): the 8 bytes this lane addresses in row rb and row rb + 4.
template <int ROW_BYTES = 256>
__device__ __forceinline__ bf16x8_t read_tr(const uint8_t* img, int rb, int chunk, int half) {
  const s16x4_t lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + tile_off<ROW_BYTES>(rb, chunk) + 8 * half));
  const s16x4_t hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + tile_off<ROW_BYTES>(rb + 4, chunk) + 8 * half));
  return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace ptdt
