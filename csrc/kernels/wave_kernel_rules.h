// Per-instantiation rules of the wave engine's layout-F kernels (linear_wave_f_kernel in
// linear_wave_impl.h): plain constexpr arithmetic on the template parameters (R, KP, DOUT, VAR, AR),
// seen by the kernels and by the host dispatch (linear_wave.hip), which sizes the dynamic LDS from the
// same functions.
#pragma once
#include "kernels.h"

namespace ptdt {
namespace lw {

// Whether a lean kernel's step loop has two unrolled group bodies or one.
// Two unrolled group bodies hold the batch buffers in flight (R KP values each, a row record or features
// and targets) live across both, next to DOUT KP weights (and momenta). Built with two bodies
// everywhere (tools/wave_kernel_resources.py, profiles/wave_loop_runs.md): every R == 4 kernel ends
// within a few registers of the 256 or past them (copies through accumulation registers; <4,16,1>
// gains 88 to 644 bytes of scratch), <2,16,1> and most all-reduce kernels of two outputs or KP >= 8
// likewise, or they spill already and would carry the spill code twice. Those keep one body under
// the per-group flag. The rule holds for both lean variants and every loss: `var` does not enter it.
constexpr bool lean_two_bodies(int R, int KP, int DOUT, int var, bool ar) {
  (void)var;
  return ar ? (DOUT == 1 && R <= 2 && KP <= 5) : (R <= 2 && R * KP * DOUT <= 20);
}

// Batches of row gathers in flight (register buffers; steps per unrolled group; the loss ring has
// 2 S + depth slots) of one instantiation. The two-body lean kernels without the in-kernel all-reduce
// keep kWaveGatherDepth: their step has shrunk to ~0.13 us, so a batch requested three steps ahead has
// a lead of ~0.28 us, about the latency of a row gather from L2, and one more batch in flight measured
// 2.7 % off the benchmark's step; five and more measured slower than three
// (profiles/wave_gather_depth.md). At that depth none of them has scratch or copies through
// accumulation registers (tools/wave_kernel_resources.py). Everything else keeps kWavePrefetch: the
// generic kernels (the bitwise oracle), the all-reduce kernels (bound by the exchange) and the one-body
// kernels (R == 4 and the wide feature groups sit at the register limit: <4,16,1> has 348 at depth 3).
constexpr int kWaveGatherDepth = 4;
constexpr int wave_gather_depth(int R, int KP, int DOUT, int var, bool ar) {
  return var != kWaveGeneric && !ar && lean_two_bodies(R, KP, DOUT, var, ar) ? kWaveGatherDepth : kWavePrefetch;
}

}  // namespace lw
}  // namespace ptdt
