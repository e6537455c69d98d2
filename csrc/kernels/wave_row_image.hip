// Pack kernel of the wave engine's row image (wave_row_image.h): one thread per output float.
#include "common.h"
#include "kernels.h"
#include "wave_row_image.h"

namespace ptdt {
namespace {

__global__ void __launch_bounds__(256) wave_pack_rows_kernel(const float* __restrict__ X, int64_t ldx,
                                                             const float* __restrict__ Y, int din, int kp,
                                                             int64_t total, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) out[e] = wave_image_value(X, ldx, Y, din, kp, e);
}

}  // namespace

hipError_t wave_pack_rows(const float* X, int64_t ldx, const float* Y, int64_t n_rows, int din, int kp, float* out,
                          hipStream_t s) {
  if (X == nullptr || Y == nullptr || out == nullptr || ldx < din || !wave_image_fits(n_rows, din, kp))
    return hipErrorInvalidValue;
  const int64_t total = n_rows * wave_image_row_floats(kp);  // < 2^29 floats (wave_image_fits)
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(wave_pack_rows_kernel, dim3(blocks), dim3(256), 0, s, X, ldx, Y, din, kp, total, out);
  return hipGetLastError();
}

}  // namespace ptdt
