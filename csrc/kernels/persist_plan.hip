// Host side of the persistent step engines: which engine runs a configuration
// (persistent_select, the only place that knows the variant rules), the launch
// plan built from that choice, and the relaunch. No device code.
#include "common.h"
#include "kernels.h"

namespace ptdt {

// Two callers. The plan (fused_mlp_persistent_prepare) passes the real dataset: X's row stride
// in a.ldx, its zero-padding flag and its row count in p.N. The engine query of the bindings
// (persistent_engine / persistent_choice) has no tensor yet and passes a.ldx = kWaveLdxAny,
// a.x_padded = 1 and p.N = max(num_samples, 1); nothing else differs between the two. Past layout
// F's limits (2^24 rows, 2^31 bytes) the query, which sees num_samples rows and not the dataset's,
// can therefore name a wave layout that the plan of the full dataset rejects.
PersistChoice persistent_select(const FusedMlpArgs& a, const PersistArgs& p) {
  const int v = p.variant;
  PersistChoice c;
  // the wave engine: every variant that does not name another engine
  if (v != kPersistWorkgroup && v != kPersistMfma && v != kPersistTp && v != kPersistTpBf16 &&
      linear_wave_choose(a, p, &c))
    return c;
  if ((v == kPersistAuto || v == kPersistTp || v == kPersistTpBf16) && a.H > 0 && mlp_tp_supported(a, p)) {
    c.engine = v == kPersistTpBf16 ? kEngTpBf16 : kEngTp;
    c.waves = a.H / 16;
    return c;
  }
  if (v >= kPersistWave && v != kPersistMfma) return c;  // a forced wave / tp variant its engine refused
  const bool mfma = (v == kPersistAuto || v == kPersistMfma) && mlp_mfma_supported(a);
  if (v == kPersistMfma && !mfma) return c;
  const PersistEngine wg = mfma ? kEngWorkgroupMfma : kEngWorkgroup;
  const bool fits = fused_mlp_persistent_lds_bytes(a.B, a.Din, a.H, a.Dout, p.num_samples, a.ar.world) <= 160 * 1024;
  if (fits) c.engine = wg;
  else c.refused = wg;
  return c;
}

hipError_t persist_set_kernel(PersistLaunch* L, const void* fn, int threads, size_t lds) {
  if (lds > 64 * 1024) PTDT_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  L->fn = fn;
  L->threads = threads;
  L->lds = lds;
  return hipSuccess;
}

hipError_t fused_mlp_persistent_prepare(PersistLaunch* L) {
  const FusedMlpArgs& a = L->a;
  const PersistArgs& p = L->p;
  L->choice = persistent_select(a, p);
  PTDT_HIP_CHECK(fused_mlp_check_dims(a));
  if (a.update_mode != 2 || a.accumulate || p.cursor == nullptr || p.losses == nullptr || p.num_samples <= 0 ||
      p.N <= 0 || p.W <= 0 || p.rank < 0 || p.rank >= p.W)
    return hipErrorInvalidValue;
  if (a.ar.world > 1 && (fused_mlp_num_params(a) > a.ar.max_elems || a.ar.world != p.W || a.ar.rank != p.rank))
    return hipErrorInvalidValue;
  switch (L->choice.engine) {
    case kEngWave: return linear_wave_prepare(L);
    case kEngTp:
    case kEngTpBf16: return mlp_tp_prepare(L);
    case kEngWorkgroupMfma:
    case kEngWorkgroup: return fused_mlp_workgroup_prepare(L);
    default: return hipErrorInvalidValue;
  }
}

hipError_t persistent_launch(PersistLaunch& L, int n_steps, int64_t cursor_host_pos, hipStream_t s, int start_e,
                             int start_j) {
  if (n_steps <= 0) return hipSuccess;
  if (L.fn == nullptr || !persist_span_ok(L, cursor_host_pos, n_steps)) return hipErrorInvalidValue;
  persist_set_position(L, n_steps, cursor_host_pos, start_e, start_j);
  void* args[] = {&L.a, &L.p};
  L.host_ns[0] = mono_ns();
  const hipError_t e = hipLaunchKernel(L.fn, dim3(1), dim3(L.threads), args, L.lds, s);
  L.host_ns[1] = mono_ns();
  return e;
}

}  // namespace ptdt
