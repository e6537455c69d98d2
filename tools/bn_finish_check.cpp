// Stand-alone host check of the BatchNorm per-channel finalise (csrc/kernels/bn_finish.h): the
// arithmetic every statistics kernel shares, evaluated on a grid of inputs and compared with long
// double. Meant to be built with sanitizers and run on a CPU (tests/test_bn_finish.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc \
//       tools/bn_finish_check.cpp -o bn_finish_check && ./bn_finish_check
//
// Grid: var = 0, var tiny against eps, |mean| = 1e4 with var = 1e-3, null-weight defaults (w = 1,
// b = 0), rows = 1 and 2 for the unbiased factor as each caller forms it (var * M / (M - 1) in the
// local kernels, m2 / (n - 1) in the cross-rank merge), momentum 0, 0.1 and 1.
// Bound: every output is the float rounding of a double expression, or at most three float
// operations on such roundings: 4 * 2^-24 relative to the sum of the magnitudes of its terms.
#include <cmath>
#include <cstdio>

#include "kernels/bn_finish.h"

namespace {

const long double kTol = 4.0L * 0x1p-24L;
long failures = 0, checks = 0;

void expect(const char* what, float got, long double ref, long double magnitude, double mean, double var, float w,
            float b, float eps) {
  ++checks;
  const long double err = fabsl((long double)got - ref);
  if (std::isfinite(got) && err <= kTol * magnitude) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: got %.9g ref %.12Lg err %.3Lg bound %.3Lg (mean %g var %g w %g b %g eps %g)\n", what,
               (double)got, ref, err, kTol * magnitude, mean, var, (double)w, (double)b, (double)eps);
}

void check_stats(double mean, double var, float w, float b, float eps) {
  const ptdt::BnChannelStats s = ptdt::bn_channel_stats(mean, var, w, b, eps);
  const long double invstd = 1.0L / sqrtl((long double)var + (long double)eps);
  const long double scaled = (long double)mean * w * invstd;
  expect("mean", s.mean, mean, fabsl((long double)mean), mean, var, w, b, eps);
  expect("invstd", s.invstd, invstd, invstd, mean, var, w, b, eps);
  expect("scale", s.scale, (long double)w * invstd, fabsl((long double)w * invstd), mean, var, w, b, eps);
  expect("shift", s.shift, (long double)b - scaled, fabsl((long double)b) + fabsl(scaled), mean, var, w, b, eps);
}

void check_running(float old, float momentum, double value) {
  const float got = ptdt::bn_running_update(old, momentum, value);
  const long double keep = (1.0L - (long double)momentum) * old, add = (long double)momentum * value;
  expect("running", got, keep + add, fabsl(keep) + fabsl(add), value, 0.0, old, momentum, 0.f);
}

}  // namespace

int main() {
  const double means[] = {0.0, 0.5, -3.0, 1e4, -1e4};
  const double vars[] = {0.0, 1e-12, 1e-3, 1.0, 1e4};  // 0, tiny against eps, ..., large
  const float affine[][2] = {{1.f, 0.f}, {0.5f, -2.f}, {-1.5f, 3.f}, {0.f, 0.25f}};  // first: null-weight defaults
  const float epss[] = {1e-5f, 1e-3f};
  const float momenta[] = {0.f, 0.1f, 1.f};
  const float olds[] = {0.f, 1.f, -2.5f, 1e4f};
  const long rows[] = {1, 2, 7, 4096};
  for (double mean : means)
    for (double var : vars) {
      for (const auto& a : affine)
        for (float eps : epss) check_stats(mean, var, a[0], a[1], eps);
      for (long M : rows) {
        // the unbiased variance as the local kernels and as the cross-rank merge form it
        const double Md = (double)M, m2 = var * Md;
        const double local = M > 1 ? var * Md / (Md - 1.0) : var;
        const double merged = Md > 1.0 ? m2 / (Md - 1.0) : var;
        const long double ref = M > 1 ? (long double)var * M / (M - 1) : (long double)var;
        if (fabsl(local - ref) > 4.0L * 0x1p-53L * ref || fabsl(merged - ref) > 4.0L * 0x1p-53L * ref) {
          ++failures;
          std::fprintf(stderr, "FAIL unbiased: var %g M %ld local %.17g merged %.17g\n", var, M, local, merged);
        }
        for (float momentum : momenta)
          for (float old : olds) {
            check_running(old, momentum, mean);
            check_running(old, momentum, local);
            check_running(old, momentum, merged);
          }
      }
    }
  if (failures) {
    std::fprintf(stderr, "bn finish: %ld of %ld checks failed\n", failures, checks);
    return 1;
  }
  std::printf("bn finish: %ld checks ok\n", checks);
  return 0;
}
