// Stand-alone host check of the wave engine's row image (csrc/kernels/wave_row_image.h) against the
// layout written out below from its definition. Meant to be built with sanitizers and run on a CPU
// (tests/test_wave_row_image.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc \
//       tools/wave_row_image_check.cpp -o wave_row_image_check && ./wave_row_image_check
//
// Ranges: Din 1..24 (and 4 KP for the wide layouts), every KP of layout F's table that covers Din, N = 1, 3,
// 33 rows, X rows padded by 0 or 3 floats. X, Y and the image are heap arrays of exactly their sizes, so
// a read of X past Din, of a row past N or a write past the image is an overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "kernels/wave_row_image.h"

namespace {

const int kKP[] = {4, 5, 8, 10, 16};

int fail(const char* what, int din, int kp, long n, long at) {
  std::fprintf(stderr, "FAIL %s: Din=%d KP=%d N=%ld at %ld\n", what, din, kp, n, at);
  return 1;
}

int check(int din, int kp, long n, int pad) {
  using namespace ptdt;
  // the definition: KP features, 1.0f if KP is odd, y, zeros up to a multiple of 4 floats
  const int used = kp + (kp % 2) + 1, rs = (used + 3) / 4 * 4;
  if (wave_image_rs(kp) != rs || wave_image_row_floats(kp) != 4 * rs || wave_image_row_bytes(kp) != 16 * rs)
    return fail("record size", din, kp, n, rs);
  if (!wave_image_fits(n, din, kp)) return fail("fits", din, kp, n, 0);
  const long ldx = din + pad;
  float* X = (float*)std::malloc(sizeof(float) * ((n - 1) * ldx + din));  // the last row has no padding behind it
  float* Y = (float*)std::malloc(sizeof(float) * n);
  const long total = n * 4 * rs;
  float* img = (float*)std::malloc(sizeof(float) * total);
  for (long r = 0; r < n; ++r) {
    for (int k = 0; k < din; ++k) X[r * ldx + k] = 2.f + (float)(r * 31 + k);  // never 0 or 1
    Y[r] = -3.f - (float)r;
  }
  for (long e = 0; e < total; ++e) img[e] = wave_image_value(X, ldx, Y, din, kp, e);
  int rc = 0;
  for (long r = 0; !rc && r < n; ++r)
    for (int q = 0; !rc && q < 4; ++q) {
      const long off = wave_image_offset(r, q, kp);
      if (off != (r * 4 * rs + (long)q * rs) * 4 || off % 16 != 0 || off + rs * 4 > total * 4)
        rc = fail("offset", din, kp, n, off);
      const float* rec = img + off / 4;
      for (int s = 0; !rc && s < rs; ++s) {
        float want = 0.f;
        if (s < kp) want = q * kp + s < din ? X[r * ldx + q * kp + s] : 0.f;
        else if (kp % 2 == 1 && s == kp) want = 1.f;
        else if (s == kp + kp % 2) want = Y[r];
        if (std::memcmp(&rec[s], &want, 4) != 0) rc = fail("value", din, kp, n, r * 4 * rs + q * rs + s);
      }
    }
  std::free(X);
  std::free(Y);
  std::free(img);
  return rc;
}

}  // namespace

int main() {
  long cases = 0;
  for (int kp : kKP)
    for (int din = 1; din <= 4 * kp; ++din) {
      if (din > 24 && din != 4 * kp) continue;
      for (long n : {1L, 3L, 33L})
        for (int pad : {0, 3}) {
          if (check(din, kp, n, pad)) return 1;
          ++cases;
        }
    }
  // the limits: 2^24 rows, 2^31 bytes
  if (ptdt::wave_image_fits(1 << 24, 20, 5) || !ptdt::wave_image_fits((1 << 24) - 1, 20, 5) ||
      ptdt::wave_image_fits((1L << 31) / 320 + 1, 64, 16) || !ptdt::wave_image_fits((1L << 31) / 320, 64, 16) ||
      ptdt::wave_image_fits(8, 21, 5))
    return fail("limits", 0, 0, 0, 0);
  std::printf("wave row image: %ld cases ok\n", cases);
  return 0;
}
