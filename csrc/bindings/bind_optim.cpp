// Bindings of the optimizer steps, gradient clipping, learning-rate schedules and the
// multi-tensor copies / casts the optimizers and the DDP buckets use.
#include <limits>

#include "common.h"

namespace ptdt {
namespace {

// ------------------------------------------------------------- optimizers
// An optional one-element f32 operand of the optimizer steps, on the parameters' device (a
// one-element tensor is contiguous whatever its strides, so that term never decides).
const float* dev_scalar(const c10::optional<Tensor>& t, const Tensor& p, const char* msg) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->device() == p.device() && t->scalar_type() == at::kFloat && t->numel() == 1 &&
                  t->is_contiguous(),
              msg);
  return t->data_ptr<float>();
}

// the optional clip coefficient of the optimizer steps: one f32 value on the parameters' device
const float* gcoef_ptr(const c10::optional<Tensor>& gcoef, const Tensor& p) {
  return dev_scalar(gcoef, p, "gcoef must be one float32 value on the parameters' device");
}

// the optional device learning rate of the optimizer steps: the group's slot of a schedule's lr buffer
const float* lr_dev_ptr(const c10::optional<Tensor>& lr_dev, const Tensor& p) {
  return dev_scalar(lr_dev, p, "lr_dev must be one contiguous float32 value on the parameters' device");
}

void sgd_flat_(Tensor p, Tensor g, c10::optional<Tensor> mom, c10::optional<Tensor> step, double lr,
               double momentum, double dampening, double wd, bool nesterov, double grad_scale,
               c10::optional<Tensor> gcoef, c10::optional<Tensor> lr_dev) {
  check_gpu(p, "param");
  check_gpu(g, "grad");
  TORCH_CHECK(p.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat && p.numel() == g.numel());
  c10::hip::HIPGuard guard(p.device().index());
  const SgdHyper h{(float)lr, (float)momentum, (float)dampening, (float)wd, (float)grad_scale, nesterov};
  hip_check(sgd_flat(p.data_ptr<float>(), g.data_ptr<float>(), ptr_or_null<float>(mom), ptr_or_null<int32_t>(step),
                     p.numel(), h, gcoef_ptr(gcoef, p), lr_dev_ptr(lr_dev, p), cur_stream(p)),
            "sgd_flat");
}

void adam_flat_(Tensor p, Tensor g, Tensor m, Tensor v, Tensor step, double lr, double b1, double b2,
                double eps, double wd, bool decoupled, double grad_scale, c10::optional<Tensor> gcoef,
                c10::optional<Tensor> lr_dev) {
  check_gpu(p, "param");
  TORCH_CHECK(p.scalar_type() == at::kFloat && g.numel() == p.numel() && m.numel() == p.numel() &&
              v.numel() == p.numel() && step.scalar_type() == at::kInt);
  c10::hip::HIPGuard guard(p.device().index());
  const AdamHyper h{(float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)grad_scale, decoupled};
  hip_check(adam_flat(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                      step.data_ptr<int32_t>(), p.numel(), h, gcoef_ptr(gcoef, p), lr_dev_ptr(lr_dev, p),
                      cur_stream(p)),
            "adam_flat");
}

// The TensorList of the pairs (ps[i], gs[i]), a <= i < b: the p / g / numel slots, filled after
// slots(l, k, i) ran the caller's checks on pair i and filled what else slot k carries (the checks stay
// with the callers: the optimizers check the layout first, the cast the dtypes, and that order shows).
template <typename Slots>
TensorList tensor_list(const std::vector<Tensor>& ps, const std::vector<Tensor>& gs, size_t a, size_t b,
                       Slots&& slots) {
  TensorList l{};
  l.n = (int)(b - a);
  for (size_t i = a; i < b; ++i) {
    slots(l, i - a, i);
    l.numel[i - a] = ps[i].numel();
    l.p[i - a] = ps[i].data_ptr();
    l.g[i - a] = gs[i].data_ptr();
  }
  return l;
}

// The slot filler of an SGD-shaped TensorList (sgd_multi_, lars_multi_): layout and dtype checks of
// pair i, s1 = momentum buffer or null, s2 = bf16 shadow or null.
auto sgd_slots(const std::vector<Tensor>& ps, const std::vector<Tensor>& gs, const std::vector<Tensor>& moms,
               const std::vector<Tensor>& shadows, int dt, const char* who) {
  return [&ps, &gs, &moms, &shadows, dt, who](TensorList& l, size_t k, size_t i) {
    check_dense_like(ps[i], ps[i], "param");
    check_dense_like(ps[i], gs[i], "grad");
    if (!moms.empty()) check_dense_like(ps[i], moms[i], "momentum buffer");
    TORCH_CHECK(dt_of(ps[i]) == dt && gs[i].scalar_type() == ps[i].scalar_type() && gs[i].numel() == ps[i].numel());
    l.s1[k] = moms.empty() ? nullptr : moms[i].data_ptr<float>();
    l.s2[k] = nullptr;
    if (!shadows.empty()) {
      TORCH_CHECK(shadows[i].scalar_type() == at::kBFloat16 && shadows[i].numel() == ps[i].numel(), who,
                  ": shadow must be a bf16 tensor of the param's size");
      check_dense_like(ps[i], shadows[i], "bf16 shadow");
      l.s2[k] = reinterpret_cast<float*>(shadows[i].data_ptr());
    }
  };
}

// The slot filler of an Adam-shaped TensorList (adam_multi_, lamb_multi_): s1 = exp_avg, s2 = exp_avg_sq.
auto adam_slots(const std::vector<Tensor>& ps, const std::vector<Tensor>& gs, const std::vector<Tensor>& ms,
                const std::vector<Tensor>& vs, int dt) {
  return [&ps, &gs, &ms, &vs, dt](TensorList& l, size_t k, size_t i) {
    check_dense_like(ps[i], ps[i], "param");
    check_dense_like(ps[i], gs[i], "grad");
    check_dense_like(ps[i], ms[i], "exp_avg");
    check_dense_like(ps[i], vs[i], "exp_avg_sq");
    TORCH_CHECK(dt_of(ps[i]) == dt && gs[i].numel() == ps[i].numel());
    TORCH_CHECK(ms[i].scalar_type() == at::kFloat && vs[i].scalar_type() == at::kFloat);
    l.s1[k] = ms[i].data_ptr<float>();
    l.s2[k] = vs[i].data_ptr<float>();
  };
}

// The list sizes of an SGD-shaped call. lars_multi_ needs the momentum buffers its momentum asks for
// (sgd_multi_ takes the step without momentum when it has none).
void check_sgd_lists(const std::vector<Tensor>& ps, const std::vector<Tensor>& gs, const std::vector<Tensor>& moms,
                     const std::vector<Tensor>& shadows, bool need_moms, const char* who) {
  TORCH_CHECK(ps.size() == gs.size() && (moms.empty() || moms.size() == ps.size()));
  TORCH_CHECK(!need_moms || !moms.empty(), who, ": momentum needs momentum buffers");
  TORCH_CHECK(shadows.empty() || (shadows.size() == ps.size() && ps[0].scalar_type() == at::kFloat), who,
              ": bf16 shadows need one per (f32) param");
}

// ... and of an Adam-shaped one
void check_adam_lists(const std::vector<Tensor>& ps, const std::vector<Tensor>& gs, const std::vector<Tensor>& ms,
                      const std::vector<Tensor>& vs) {
  TORCH_CHECK(ps.size() == gs.size() && ms.size() == ps.size() && vs.size() == ps.size());
}

void sgd_multi_(std::vector<Tensor> ps, std::vector<Tensor> gs, std::vector<Tensor> moms,
                c10::optional<Tensor> step, double lr, double momentum, double dampening, double wd,
                bool nesterov, double grad_scale, std::vector<Tensor> shadows, c10::optional<Tensor> gcoef,
                c10::optional<Tensor> lr_dev) {
  if (ps.empty()) return;
  check_sgd_lists(ps, gs, moms, shadows, false, "sgd_multi_");
  const int dt = dt_of(ps[0]);
  const SgdHyper h{(float)lr, (float)momentum, (float)dampening, (float)wd, (float)grad_scale, nesterov};
  const float *gc = gcoef_ptr(gcoef, ps[0]), *lrd = lr_dev_ptr(lr_dev, ps[0]);
  c10::hip::HIPGuard guard(ps[0].device().index());
  hipStream_t s = cur_stream(ps[0]);
  for_tensor_chunks(ps.size(), [&](size_t a, size_t b) {
    const TensorList tl = tensor_list(ps, gs, a, b, sgd_slots(ps, gs, moms, shadows, dt, "sgd_multi_"));
    hip_check(sgd_multi(tl, dt, ptr_or_null<int32_t>(step), h, gc, lrd, s), "sgd_multi");
  });
}

void adam_multi_(std::vector<Tensor> ps, std::vector<Tensor> gs, std::vector<Tensor> ms,
                 std::vector<Tensor> vs, Tensor step, double lr, double b1, double b2, double eps,
                 double wd, bool decoupled, double grad_scale, c10::optional<Tensor> gcoef,
                 c10::optional<Tensor> lr_dev) {
  if (ps.empty()) return;
  check_adam_lists(ps, gs, ms, vs);
  const int dt = dt_of(ps[0]);
  const AdamHyper h{(float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)grad_scale, decoupled};
  const float *gc = gcoef_ptr(gcoef, ps[0]), *lrd = lr_dev_ptr(lr_dev, ps[0]);
  c10::hip::HIPGuard guard(ps[0].device().index());
  hipStream_t s = cur_stream(ps[0]);
  for_tensor_chunks(ps.size(), [&](size_t a, size_t b) {
    const TensorList tl = tensor_list(ps, gs, a, b, adam_slots(ps, gs, ms, vs, dt));
    hip_check(adam_multi(tl, dt, step.data_ptr<int32_t>(), h, gc, lrd, s), "adam_multi");
  });
}

// ------------------------------------------------------------- layer-wise adaptive rates
// The workspace, the ratio record and the step counter of a layer-wise step, checked against the
// parameter list: ws float32 with two slots per chunk of every tensor, rec float32[3][tensors]
// (ratio, w, n), step int32[1]; all on the parameters' device.
void check_layerwise(const std::vector<Tensor>& ps, const Tensor& step, const Tensor& ws, const Tensor& rec,
                     const char* who) {
  const Tensor& p = ps[0];
  int64_t chunks = 0;
  for (const Tensor& t : ps) {
    TORCH_CHECK(t.is_cuda() && t.device() == p.device(), who, ": one device per call");
    chunks += (t.numel() + kChunk - 1) / kChunk;
  }
  TORCH_CHECK(step.is_cuda() && step.device() == p.device() && step.scalar_type() == at::kInt && step.numel() == 1,
              who, ": step must be int32[1] on the parameters' device");
  TORCH_CHECK(ws.is_cuda() && ws.device() == p.device() && ws.scalar_type() == at::kFloat && ws.is_contiguous() &&
                  ws.numel() >= 2 * chunks && reinterpret_cast<uintptr_t>(ws.data_ptr()) % 8 == 0,
              who, ": ws must be contiguous float32 on the parameters' device, two slots per chunk (", 2 * chunks, ")");
  TORCH_CHECK(rec.is_cuda() && rec.device() == p.device() && rec.scalar_type() == at::kFloat && rec.is_contiguous() &&
                  rec.numel() == 3 * (int64_t)ps.size(),
              who, ": rec must be contiguous float32[3][", ps.size(), "] on the parameters' device");
}

// LARS over an SGD-shaped list: per <= 32 tensors, partials -> finalise -> update. The caller
// advances the step counter afterwards, as after sgd_multi_.
void lars_multi_(std::vector<Tensor> ps, std::vector<Tensor> gs, std::vector<Tensor> moms, Tensor step, double lr,
                 double momentum, double dampening, double wd, bool nesterov, double grad_scale,
                 double trust_coefficient, double eps, std::vector<Tensor> shadows, Tensor ws, Tensor rec,
                 c10::optional<Tensor> gcoef, c10::optional<Tensor> lr_dev) {
  if (ps.empty()) return;
  check_sgd_lists(ps, gs, moms, shadows, momentum != 0.0, "lars_multi_");
  check_layerwise(ps, step, ws, rec, "lars_multi_");
  const int dt = dt_of(ps[0]);
  const int64_t T = (int64_t)ps.size();
  const SgdHyper h{(float)lr, (float)momentum, (float)dampening, (float)wd, (float)grad_scale, nesterov};
  const TrustRule rule{kTrustLars, 1, (float)trust_coefficient, h.wd, (float)eps, h.gscale};
  const float *gc = gcoef_ptr(gcoef, ps[0]), *lrd = lr_dev_ptr(lr_dev, ps[0]);
  c10::hip::HIPGuard guard(ps[0].device().index());
  hipStream_t s = cur_stream(ps[0]);
  int64_t slot = 0;
  for_tensor_chunks(ps.size(), [&](size_t a, size_t b) {
    const TensorList tl = tensor_list(ps, gs, a, b, sgd_slots(ps, gs, moms, shadows, dt, "lars_multi_"));
    hip_check(lars_partials(tl, dt, ws.data_ptr<float>(), slot, s), "lars_partials");
    hip_check(trust_finalize(tl, ws.data_ptr<float>(), slot, rule, gc, rec.data_ptr<float>(), (int64_t)a, T, s),
              "trust_finalize");
    hip_check(lars_update(tl, dt, step.data_ptr<int32_t>(), h, gc, lrd, rec.data_ptr<float>() + a, s), "lars_update");
    slot += chunk_blocks(tl);
  });
}

// LAMB over an Adam-shaped list: per <= 32 tensors, moments + partials -> finalise -> update.
// step already counts this update, as for adam_multi_.
void lamb_multi_(std::vector<Tensor> ps, std::vector<Tensor> gs, std::vector<Tensor> ms, std::vector<Tensor> vs,
                 Tensor step, double lr, double b1, double b2, double eps, double wd, bool bias_correction, bool adapt,
                 double grad_scale, Tensor ws, Tensor rec, c10::optional<Tensor> gcoef, c10::optional<Tensor> lr_dev) {
  if (ps.empty()) return;
  check_adam_lists(ps, gs, ms, vs);
  check_layerwise(ps, step, ws, rec, "lamb_multi_");
  const int dt = dt_of(ps[0]);
  const int64_t T = (int64_t)ps.size();
  const LambHyper h{(float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)grad_scale, bias_correction};
  const TrustRule rule{kTrustLamb, adapt ? 1 : 0, 0.f, 0.f, 0.f, 1.f};
  const float *gc = gcoef_ptr(gcoef, ps[0]), *lrd = lr_dev_ptr(lr_dev, ps[0]);
  c10::hip::HIPGuard guard(ps[0].device().index());
  hipStream_t s = cur_stream(ps[0]);
  const int32_t* st = step.data_ptr<int32_t>();
  int64_t slot = 0;
  for_tensor_chunks(ps.size(), [&](size_t a, size_t b) {
    const TensorList tl = tensor_list(ps, gs, a, b, adam_slots(ps, gs, ms, vs, dt));
    for (size_t i = a; i < b; ++i)
      TORCH_CHECK(gs[i].scalar_type() == ps[i].scalar_type(), "lamb_multi_: a gradient of its parameter's dtype");
    hip_check(lamb_moments(tl, dt, st, h, gc, ws.data_ptr<float>(), slot, s), "lamb_moments");
    hip_check(trust_finalize(tl, ws.data_ptr<float>(), slot, rule, nullptr, rec.data_ptr<float>(), (int64_t)a, T, s),
              "trust_finalize");
    hip_check(lamb_update(tl, dt, st, h, lrd, rec.data_ptr<float>() + a, s), "lamb_update");
    slot += chunk_blocks(tl);
  });
}

// ------------------------------------------------------------- gradient clipping
// spans: <= kMaxTensorsPerLaunch dense 1-D views of one dtype on one device (ops/clip.py plans them)
SpanList span_list(const std::vector<Tensor>& spans, const char* what) {
  TORCH_CHECK(!spans.empty() && spans.size() <= (size_t)kMaxTensorsPerLaunch, what, ": 1..", kMaxTensorsPerLaunch,
              " spans per launch");
  SpanList sl{};
  sl.n = (int)spans.size();
  for (size_t i = 0; i < spans.size(); ++i) {
    const Tensor& t = spans[i];
    TORCH_CHECK(t.is_cuda() && t.is_non_overlapping_and_dense(), what, ": spans must be dense GPU tensors");
    TORCH_CHECK(t.device() == spans[0].device() && t.scalar_type() == spans[0].scalar_type(), what,
                ": one device and one dtype per launch");
    sl.numel[i] = t.numel();
    sl.p[i] = t.data_ptr();
  }
  return sl;
}

void check_clip_rec(const Tensor& rec, const Tensor& like, const char* what) {
  TORCH_CHECK(rec.is_cuda() && rec.device() == like.device() && rec.scalar_type() == at::kFloat &&
                  rec.is_contiguous() && rec.numel() >= 2,
              what, ": rec must be float32[2] on the gradients' device");
}

// ws[first_slot + b] = partial of chunk b of the spans; returns the number of slots written
int64_t clip_norm_partials_(std::vector<Tensor> spans, Tensor ws, int64_t first_slot, int64_t norm) {
  const SpanList sl = span_list(spans, "clip_norm_partials_");
  const int64_t nb = chunk_blocks(sl);
  TORCH_CHECK(ws.is_cuda() && ws.device() == spans[0].device() && ws.scalar_type() == at::kFloat &&
                  ws.is_contiguous() && first_slot >= 0 && first_slot + nb <= ws.numel(),
              "clip_norm_partials_: ws must be float32 on the gradients' device with first_slot + chunks slots");
  c10::hip::HIPGuard guard(ws.device().index());
  hip_check(clip_norm_partials(sl, dt_of(spans[0]), (int)norm, ws.data_ptr<float>(), first_slot, cur_stream(ws)),
            "clip_norm_partials");
  return nb;
}

void clip_norm_finalize_(Tensor ws, int64_t n, int64_t norm, double max_norm, bool partial, Tensor rec) {
  check_clip_rec(rec, ws, "clip_norm_finalize_");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kFloat && ws.is_contiguous() && n >= 0 && n <= ws.numel(),
              "clip_norm_finalize_: ws must hold n float32 slots");
  c10::hip::HIPGuard guard(ws.device().index());
  hip_check(clip_norm_finalize(ws.data_ptr<float>(), n, (int)norm, (float)max_norm, partial ? 1 : 0,
                               rec.data_ptr<float>(), cur_stream(ws)),
            "clip_norm_finalize");
}

void clip_scale_(std::vector<Tensor> spans, Tensor rec) {
  const SpanList sl = span_list(spans, "clip_scale_");
  check_clip_rec(rec, spans[0], "clip_scale_");
  c10::hip::HIPGuard guard(rec.device().index());
  hip_check(clip_scale(sl, dt_of(spans[0]), rec.data_ptr<float>(), cur_stream(rec)), "clip_scale");
}

void clip_clamp_(std::vector<Tensor> spans, double c) {
  const SpanList sl = span_list(spans, "clip_clamp_");
  c10::hip::HIPGuard guard(spans[0].device().index());
  hip_check(clip_clamp(sl, dt_of(spans[0]), (float)c, cur_stream(spans[0])), "clip_clamp");
}

// ------------------------------------------------------------- learning-rate schedules
// One launch: t += increment, lr[g] = base_lrs[g] * f(t). The program arrives as parallel lists, one
// entry per segment (ops/lr_scheduler.py builds and validates them; the caps are checked again here).
void lr_schedule_step_(Tensor t, Tensor lr, std::vector<double> base_lrs, std::vector<int64_t> bounds,
                       std::vector<int64_t> kinds, std::vector<int64_t> ns, std::vector<double> as,
                       std::vector<double> bs, std::vector<std::vector<int64_t>> milestones, bool increment) {
  const size_t S = kinds.size();
  TORCH_CHECK(S >= 1 && S <= (size_t)kLrMaxSegments, "lr_schedule_step_: 1..", kLrMaxSegments, " segments, got ", S);
  TORCH_CHECK(ns.size() == S && as.size() == S && bs.size() == S && milestones.size() == S && bounds.size() == S - 1,
              "lr_schedule_step_: one n, a, b and milestone list per segment, segments - 1 bounds");
  TORCH_CHECK(!base_lrs.empty() && base_lrs.size() <= (size_t)kLrMaxGroups, "lr_schedule_step_: 1..", kLrMaxGroups,
              " parameter groups per launch, got ", base_lrs.size());
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.numel() == 1, "lr_schedule_step_: t must be int32[1]");
  TORCH_CHECK(lr.is_cuda() && lr.device() == t.device() && lr.scalar_type() == at::kFloat && lr.is_contiguous() &&
                  lr.numel() == (int64_t)base_lrs.size(),
              "lr_schedule_step_: lr must be float32[groups] on t's device");
  constexpr int64_t kMaxT = std::numeric_limits<int32_t>::max();
  LrProgram prog{};
  prog.groups = (int)base_lrs.size();
  prog.segments = (int)S;
  for (size_t g = 0; g < base_lrs.size(); ++g) prog.base[g] = base_lrs[g];
  for (size_t k = 0; k + 1 < S; ++k) {
    TORCH_CHECK(bounds[k] > (k ? bounds[k - 1] : 0) && bounds[k] <= kMaxT,
                "lr_schedule_step_: bounds must be ascending positive int32 values");
    prog.bound[k] = (int32_t)bounds[k];
  }
  for (size_t k = 0; k < S; ++k) {
    LrSegment& sg = prog.seg[k];
    TORCH_CHECK(kinds[k] >= 0 && kinds[k] < kLrKinds, "lr_schedule_step_: unknown segment kind ", kinds[k]);
    TORCH_CHECK(ns[k] >= 0 && ns[k] <= kMaxT, "lr_schedule_step_: segment n out of range");
    TORCH_CHECK(milestones[k].size() <= (size_t)kLrMaxMilestones, "lr_schedule_step_: at most ", kLrMaxMilestones,
                " milestones per segment, got ", milestones[k].size());
    sg.kind = (int)kinds[k];
    sg.n = sg.kind == kLrMultiStep ? (int)milestones[k].size() : (int)ns[k];
    sg.a = as[k];
    sg.b = bs[k];
    for (size_t i = 0; i < milestones[k].size(); ++i) {
      TORCH_CHECK(milestones[k][i] >= 0 && milestones[k][i] <= kMaxT, "lr_schedule_step_: milestone out of range");
      sg.ms[i] = (int32_t)milestones[k][i];
    }
  }
  c10::hip::HIPGuard guard(t.device().index());
  hip_check(lr_schedule_step(t.data_ptr<int32_t>(), lr.data_ptr<float>(), prog, increment ? 1 : 0, cur_stream(t)),
            "lr_schedule_step");
}

void bucket_copy(std::vector<Tensor> ts, Tensor flat, double scale, bool unpack) {
  if (ts.empty()) return;
  check_gpu(flat, "flat");
  const int dt = dt_of(flat);
  c10::hip::HIPGuard guard(flat.device().index());
  int64_t off = 0;
  for_tensor_chunks(ts.size(), [&](size_t a, size_t b) {
    CopyList cl{};
    cl.n = (int)(b - a);
    for (size_t i = a; i < b; ++i) {
      check_gpu(ts[i], "tensor");
      TORCH_CHECK(ts[i].scalar_type() == flat.scalar_type());
      cl.numel[i - a] = ts[i].numel();
      cl.offset[i - a] = off;
      cl.t[i - a] = ts[i].data_ptr();
      off += ts[i].numel();
    }
    TORCH_CHECK(off <= flat.numel(), "bucket_copy: flat buffer too small");
    hip_check(unpack ? bucket_unpack(cl, flat.data_ptr(), dt, (float)scale, cur_stream(flat))
                     : bucket_pack(cl, flat.data_ptr(), dt, (float)scale, cur_stream(flat)),
              "bucket_copy");
  });
}

// dsts[i] (f32) = srcs[i] (bf16), one multi-tensor launch per <= 32 pairs; pairs must share shape and strides
void cast_multi_(std::vector<Tensor> dsts, std::vector<Tensor> srcs) {
  TORCH_CHECK(dsts.size() == srcs.size(), "cast_multi_: one source per destination");
  if (dsts.empty()) return;
  c10::hip::HIPGuard guard(dsts[0].device().index());
  for_tensor_chunks(dsts.size(), [&](size_t a, size_t b) {
    const TensorList tl = tensor_list(dsts, srcs, a, b, [&](TensorList&, size_t, size_t i) {
      TORCH_CHECK(dsts[i].scalar_type() == at::kFloat && srcs[i].scalar_type() == at::kBFloat16,
                  "cast_multi_: f32 destinations, bf16 sources");
      TORCH_CHECK(dsts[i].device() == dsts[0].device() && srcs[i].device() == dsts[0].device(),
                  "cast_multi_: one device");
      check_dense_like(dsts[i], dsts[i], "destination");
      check_dense_like(dsts[i], srcs[i], "source");
    });
    hip_check(cast_bf16_f32_multi(tl, cur_stream(dsts[0])), "cast_bf16_f32_multi");
  });
}

void scale_(Tensor x, double s) {
  check_gpu(x, "x");
  c10::hip::HIPGuard guard(x.device().index());
  hip_check(scale_inplace(x.data_ptr(), x.numel(), dt_of(x), (float)s, cur_stream(x)), "scale_inplace");
}

}  // namespace

void bind_optim(py::module_& m) {
  // gcoef (optional, last): a device float multiplied into the gradient scale, the clip coefficient
  m.def("sgd_flat_", &sgd_flat_, py::arg("p"), py::arg("g"), py::arg("mom"), py::arg("step"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("nesterov"), py::arg("grad_scale"),
        py::arg("gcoef") = py::none(), py::arg("lr_dev") = py::none());
  m.def("adam_flat_", &adam_flat_, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("step"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("decoupled"),
        py::arg("grad_scale"), py::arg("gcoef") = py::none(), py::arg("lr_dev") = py::none());
  m.def("sgd_multi_", &sgd_multi_, py::arg("ps"), py::arg("gs"), py::arg("moms"), py::arg("step"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("nesterov"), py::arg("grad_scale"),
        py::arg("shadows") = std::vector<Tensor>{}, py::arg("gcoef") = py::none(), py::arg("lr_dev") = py::none());
  m.def("adam_multi_", &adam_multi_, py::arg("ps"), py::arg("gs"), py::arg("ms"), py::arg("vs"), py::arg("step"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("decoupled"),
        py::arg("grad_scale"), py::arg("gcoef") = py::none(), py::arg("lr_dev") = py::none());
  m.def("lars_multi_", &lars_multi_, py::arg("ps"), py::arg("gs"), py::arg("moms"), py::arg("step"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("nesterov"), py::arg("grad_scale"),
        py::arg("trust_coefficient"), py::arg("eps"), py::arg("shadows"), py::arg("ws"), py::arg("rec"),
        py::arg("gcoef") = py::none(), py::arg("lr_dev") = py::none(),
        "LARS: rec = {ratio, |p|, |g'|} per tensor, then the SGD step on ratio * (g' + wd p)");
  m.def("lamb_multi_", &lamb_multi_, py::arg("ps"), py::arg("gs"), py::arg("ms"), py::arg("vs"), py::arg("step"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("bias_correction"),
        py::arg("adapt"), py::arg("grad_scale"), py::arg("ws"), py::arg("rec"), py::arg("gcoef") = py::none(),
        py::arg("lr_dev") = py::none(), "LAMB: moments, rec = {ratio, |p|, |u|} per tensor, p -= lr ratio u");
  m.def("clip_norm_partials_", &clip_norm_partials_, py::arg("spans"), py::arg("ws"), py::arg("first_slot"),
        py::arg("norm"), "per-chunk norm partials (norm 0: sum of squares, 1: max |g|); returns the slot count");
  m.def("clip_norm_finalize_", &clip_norm_finalize_, py::arg("ws"), py::arg("n"), py::arg("norm"), py::arg("max_norm"),
        py::arg("partial"), py::arg("rec"), "rec = {total_norm, clip_coef} from n partial slots");
  m.def("clip_scale_", &clip_scale_, py::arg("spans"), py::arg("rec"), "spans *= rec[1] (skipped when exactly 1)");
  m.def("clip_clamp_", &clip_clamp_, py::arg("spans"), py::arg("c"), "spans = clamp(spans, -c, c), NaN kept");
  m.def("lr_schedule_step_", &lr_schedule_step_, py::arg("t"), py::arg("lr"), py::arg("base_lrs"), py::arg("bounds"),
        py::arg("kinds"), py::arg("ns"), py::arg("as_"), py::arg("bs"), py::arg("milestones"), py::arg("increment"),
        "t += increment; lr[g] = base_lrs[g] * schedule(t): one single-wave launch, capturable");
  m.attr("LR_MAX_SEGMENTS") = kLrMaxSegments;
  m.attr("LR_MAX_MILESTONES") = kLrMaxMilestones;
  m.attr("LR_MAX_GROUPS") = kLrMaxGroups;
  m.def("bucket_copy", &bucket_copy);
  m.def("scale_", &scale_);
  m.def("cast_multi_", &cast_multi_, py::arg("dsts"), py::arg("srcs"));
}

}  // namespace ptdt
