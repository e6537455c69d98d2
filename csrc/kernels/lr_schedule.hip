// Learning-rate schedules on the device (gfx950): one single-wave launch per scheduler.step().
//
// The learning rate of a captured training step cannot come from the host, so it lives in a
// device buffer lr[G] (one float32 per parameter group) that the update kernels of optim.hip load,
// next to a device int32 step counter t. This kernel advances t (or leaves it, to write lr(t) for
// the current t) and evaluates the schedule at t for every group: lane g owns group g.
//
// The schedule is a by-value kernel argument (LrProgram), as TensorList is: no metadata in device
// memory, no host reads, no allocation, so the launch is hipGraph-capturable. The arithmetic is
// fp64 (cos, pow, division), rounded once to float32 at the store: the stored value is the closed
// form of the matching torch.optim.lr_scheduler class, correctly rounded up to libm error. One
// wave per step, so fp64 costs nothing here.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace ptdt {
namespace {

constexpr int kBlock = 64;  // one wave; lane g < kLrMaxGroups evaluates group g
static_assert(kLrMaxGroups <= kBlock, "one lane per parameter group");

// f(t') of one segment at the segment-local time tl >= 0; base: the group's base learning rate
__device__ double lr_factor(const LrSegment& s, int64_t tl, double base) {
  switch (s.kind) {
    case kLrConstant:
      return tl < s.n ? s.a : 1.0;
    case kLrLinear: {
      const int64_t c = tl < s.n ? tl : (int64_t)s.n;
      return s.a + (s.b - s.a) * (double)c / (double)s.n;
    }
    case kLrCosine: {
      const double r = base != 0.0 ? s.a / base : 0.0;  // eta_min / base_lr
      return r + (1.0 - r) * (1.0 + cos(M_PI * (double)tl / (double)s.n)) / 2.0;
    }
    case kLrStep:
      return pow(s.a, (double)(tl / s.n));
    case kLrMultiStep: {
      int hit = 0;
      for (int i = 0; i < s.n; ++i) hit += (int64_t)s.ms[i] <= tl;
      return pow(s.a, (double)hit);
    }
    case kLrExponential:
      return pow(s.a, (double)tl);
    case kLrPolynomial: {
      const int64_t c = tl < s.n ? tl : (int64_t)s.n;
      return pow(1.0 - (double)c / (double)s.n, s.b);
    }
    default:
      return 1.0;
  }
}

__global__ void __launch_bounds__(kBlock) lr_schedule_kernel(int32_t* __restrict__ t_dev,
                                                             float* __restrict__ lr, LrProgram prog,
                                                             int increment) {
  const int32_t t = *t_dev + (increment ? 1 : 0);
  __syncthreads();  // every lane has read the counter before lane 0 overwrites it
  if (increment && threadIdx.x == 0) *t_dev = t;
  const int g = threadIdx.x;
  if (g >= prog.groups) return;
  int k = 0;  // the active segment: bound[k-1] <= t < bound[k], the last one continues
  while (k + 1 < prog.segments && t >= prog.bound[k]) ++k;
  const int64_t tl = (int64_t)t - (k > 0 ? prog.bound[k - 1] : 0);
  const double base = prog.base[g];
  lr[g] = (float)(base * lr_factor(prog.seg[k], tl < 0 ? 0 : tl, base));
}

}  // namespace

hipError_t lr_schedule_step(int32_t* t, float* lr, const LrProgram& prog, int increment, hipStream_t s) {
  if (prog.groups < 1 || prog.groups > kLrMaxGroups || prog.segments < 1 || prog.segments > kLrMaxSegments)
    return hipErrorInvalidValue;
  for (int k = 0; k < prog.segments; ++k) {
    const LrSegment& sg = prog.seg[k];
    if (sg.kind < 0 || sg.kind >= kLrKinds) return hipErrorInvalidValue;
    if (sg.kind == kLrMultiStep && (sg.n < 0 || sg.n > kLrMaxMilestones)) return hipErrorInvalidValue;
    const bool divides = sg.kind == kLrLinear || sg.kind == kLrCosine || sg.kind == kLrStep || sg.kind == kLrPolynomial;
    if (divides && sg.n < 1) return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(kBlock), 0, s, t, lr, prog, increment);
  return hipGetLastError();
}

}  // namespace ptdt
