// Row image of the wave engine's layout F (linear_wave_impl.h) for one-output models with float targets,
// as plain host / device arithmetic: no device intrinsics, so the same code runs in the pack kernel
// (wave_row_image.hip), in the lean kernels, in the Python binding (tests/test_wave_row_image.py) and in
// a sanitizer-built host program (tools/wave_row_image_check.cpp).
//
// Layout F gives feature group q (q < 4) of a dataset row to DPP row q: KP consecutive features, zero
// past Din. The image stores a dataset row as 4 records, one per feature group, each of RS floats:
//
//   x[q KP .. q KP + KP - 1] (0 past Din) | 1.0f if KP is odd | the row's target y | zeros up to RS
//
// with RS = round_up(KP + (KP odd) + 1, 4): a lane gathers its whole record with 16-byte loads, finds
// its row's target in it (no gather of its own) and, for odd KP, the constant that pairs the last
// feature with the bias sum in one packed multiply-add. KP = 5: 8 floats per record, 128 B per row.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTDT_RI_HD __host__ __device__
#else
#define PTDT_RI_HD
#endif

namespace ptdt {

constexpr int kWaveImageGroups = 4;  // feature groups (DPP rows) of layout F

// what a float of a record holds
constexpr int kWaveImageOne = -1;   // 1.0f
constexpr int kWaveImageY = -2;     // the row's target
constexpr int kWaveImageZero = -3;  // 0.0f (a feature slot past Din, or the record's tail)

PTDT_RI_HD constexpr int wave_image_used(int kp) { return kp + (kp & 1) + 1; }          // floats a lane reads
PTDT_RI_HD constexpr int wave_image_rs(int kp) { return (wave_image_used(kp) + 3) & ~3; }  // floats per record
PTDT_RI_HD constexpr int wave_image_one_slot(int kp) { return (kp & 1) ? kp : -1; }      // -1: no 1.0f slot
PTDT_RI_HD constexpr int wave_image_y_slot(int kp) { return kp + (kp & 1); }
PTDT_RI_HD constexpr int wave_image_row_floats(int kp) { return kWaveImageGroups * wave_image_rs(kp); }
PTDT_RI_HD constexpr int64_t wave_image_row_bytes(int kp) { return (int64_t)wave_image_row_floats(kp) * 4; }
PTDT_RI_HD constexpr int64_t wave_image_bytes(int64_t n_rows, int kp) { return n_rows * wave_image_row_bytes(kp); }
// byte offset of record (row, q)
PTDT_RI_HD constexpr int64_t wave_image_offset(int64_t row, int q, int kp) {
  return row * wave_image_row_bytes(kp) + (int64_t)q * wave_image_rs(kp) * 4;
}
// Slot s (s < RS) of record q: the feature index k >= 0 it holds, or one of the codes above.
PTDT_RI_HD constexpr int wave_image_source(int din, int kp, int q, int s) {
  if (s < kp) {
    const int k = q * kp + s;
    return k < din ? k : kWaveImageZero;
  }
  if (s == wave_image_one_slot(kp)) return kWaveImageOne;
  if (s == wave_image_y_slot(kp)) return kWaveImageY;
  return kWaveImageZero;
}
// The layout's limits: the kernels gather through a buffer resource with 32-bit byte offsets computed
// as a 24-bit row index times the 24-bit row size (linear_wave_choose applies the same rule to X).
PTDT_RI_HD inline bool wave_image_fits(int64_t n_rows, int din, int kp) {
  return n_rows > 0 && din > 0 && kp > 0 && kWaveImageGroups * kp >= din && n_rows < (1 << 24) &&
         wave_image_row_bytes(kp) < (1 << 24) && wave_image_bytes(n_rows, kp) < ((int64_t)1 << 31);
}
// Element e of the image (e < n_rows * row_floats) from a dataset X [n_rows, ldx] and targets Y [n_rows].
PTDT_RI_HD inline float wave_image_value(const float* X, int64_t ldx, const float* Y, int din, int kp, int64_t e) {
  const int rf = wave_image_row_floats(kp), rs = wave_image_rs(kp);
  const int64_t row = e / rf;
  const int r = (int)(e - row * rf);
  const int src = wave_image_source(din, kp, r / rs, r % rs);
  if (src >= 0) return X[row * ldx + src];
  return src == kWaveImageOne ? 1.0f : src == kWaveImageY ? Y[row] : 0.0f;
}

}  // namespace ptdt
