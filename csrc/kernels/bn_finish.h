// Per-channel finalise of the BatchNorm statistics and of the backward's coefficients: the one place
// where mean / invstd / scale / shift, the running buffers and dx = A g + B x + C are formed, for
// every producer of the [4, C] statistics (batchnorm.hip local and cross-rank, gemm_big.hip,
// conv1x1_bn.hip), so a layer's numbers do not depend on the engine ops/convbn.py picked.
//
// The forward arithmetic is plain host / device code (no device intrinsics): the kernels and a
// sanitizer-built host program (tools/bn_finish_check.cpp, tests/test_bn_finish.py) run the same
// functions. Callers form mean, var and the unbiased variance themselves, in double: their
// reductions differ (shifted sums, Chan merges), and so does the rounding of the unbiased factor.
#pragma once

#include <cmath>

#ifndef PTDT_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTDT_HD __host__ __device__
#else
#define PTDT_HD
#endif
#endif

namespace ptdt {

struct BnChannelStats {
  float mean, invstd, scale, shift;  // y = x * scale + shift
};
// w, b: the affine parameters (1, 0 without)
PTDT_HD inline BnChannelStats bn_channel_stats(double mean, double var, float w, float b, float eps) {
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  return {(float)mean, invstd, w * invstd, b - (float)mean * w * invstd};
}
// torch's running-buffer update; `value` is the batch mean or the unbiased batch variance
PTDT_HD inline float bn_running_update(float old, float momentum, double value) {
  return (float)((1.0 - momentum) * old + momentum * value);
}

}  // namespace ptdt

#if defined(__HIPCC__)
#include "kernels.h"

namespace ptdt {

__device__ __forceinline__ void bn_finish_channel(const BnParams& p, int c, double mean, double var,
                                                  double unbiased) {
  const BnChannelStats s =
      bn_channel_stats(mean, var, p.weight ? p.weight[c] : 1.f, p.bias ? p.bias[c] : 0.f, p.eps);
  p.mean[c] = s.mean;
  p.invstd[c] = s.invstd;
  p.scale[c] = s.scale;
  p.shift[c] = s.shift;
  if (p.running_mean) {
    p.running_mean[c] = bn_running_update(p.running_mean[c], p.momentum, mean);
    p.running_var[c] = bn_running_update(p.running_var[c], p.momentum, unbiased);
  }
}

// dx = A g + B x + C per channel from sdy = sum g, sdx = sum g (x - mean) over `rows` rows
__device__ __forceinline__ void bn_bwd_coef_channel(const BnBwdParams& p, int c, double sdy, double sdx,
                                                    double rows) {
  const double invstd = p.invstd[c], mean = p.mean[c];
  const double w = p.weight ? p.weight[c] : 1.0;
  const double k = w * invstd, s1 = sdy / rows, s2 = invstd * invstd * sdx / rows;
  p.coef_a[c] = (float)k;
  p.coef_b[c] = (float)(-k * s2);
  p.coef_c[c] = (float)(k * s2 * mean - k * s1);
}
// the parameter gradients and, with_coef, the coefficients
__device__ __forceinline__ void bn_bwd_finish_channel(const BnBwdParams& p, int c, double sdy, double sdx,
                                                      double rows, bool with_coef) {
  if (p.dweight) p.dweight[c] = (float)(sdx * (double)p.invstd[c]);
  if (p.dbias) p.dbias[c] = (float)sdy;
  if (with_coef) bn_bwd_coef_channel(p, c, sdy, sdx, rows);
}

}  // namespace ptdt
#endif
