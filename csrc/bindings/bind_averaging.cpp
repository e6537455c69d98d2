// Bindings of weight averaging (csrc/kernels/averaging.hip): the weight of an update from the device
// counter, and the EMA / SWA update over a tensor list or over one pair of flat spans.
#include "common.h"

namespace ptdt {
namespace {

// [data_ptr, data_ptr + bytes) of two dense tensors intersect
bool overlaps(const Tensor& x, const Tensor& y) {
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(x.data_ptr()), x1 = x0 + x.numel() * x.element_size();
  const uintptr_t y0 = reinterpret_cast<uintptr_t>(y.data_ptr()), y1 = y0 + y.numel() * y.element_size();
  return x0 < y1 && y0 < x1;
}

// n: int64[1], w: float32[1], both on `dev`
void check_counter(const Tensor& n, const char* who) {
  TORCH_CHECK(n.is_cuda() && n.scalar_type() == at::kLong && n.numel() == 1, who,
              ": n must be one int64 value on the GPU");
}

const float* weight_ptr(const Tensor& w, const at::Device& dev, const char* who) {
  TORCH_CHECK(w.is_cuda() && w.device() == dev && w.scalar_type() == at::kFloat && w.numel() == 1, who,
              ": w must be one float32 value on the tensors' device");
  return w.data_ptr<float>();
}

// One (average, source) pair and its optional bf16 copies: dtypes, device, density, equal layout, no alias.
void check_pair(const Tensor& a, const Tensor& p, const Tensor* shadow, const Tensor* copy, const at::Device& dev,
                at::ScalarType src, const char* who) {
  TORCH_CHECK(a.is_cuda() && p.is_cuda() && a.device() == dev && p.device() == dev, who, ": one device per call");
  TORCH_CHECK(a.scalar_type() == at::kFloat, who, ": averages must be float32, got ", a.scalar_type());
  TORCH_CHECK(p.scalar_type() == src && (src == at::kFloat || src == at::kBFloat16), who,
              ": sources must be all float32 or all bfloat16");
  TORCH_CHECK(a.numel() == p.numel(), who, ": an average and its source differ in numel (", a.numel(), " vs ",
              p.numel(), ")");
  TORCH_CHECK(a.is_non_overlapping_and_dense() && p.is_non_overlapping_and_dense(), who,
              ": averages and sources must be dense (non-overlapping)");
  TORCH_CHECK(a.sizes() == p.sizes() && (a.strides() == p.strides() || same_memory_order(a, p)), who,
              ": an average must have its source's shape and strides");
  TORCH_CHECK(!overlaps(a, p), who, ": an average aliases its source");
  for (const Tensor* c : {shadow, copy}) {
    if (c == nullptr) continue;
    TORCH_CHECK(c->is_cuda() && c->device() == dev && c->scalar_type() == at::kBFloat16 &&
                    c->is_non_overlapping_and_dense() && c->sizes() == a.sizes() &&
                    (c->strides() == a.strides() || same_memory_order(*c, a)),
                who, ": a bf16 copy must be a dense bfloat16 tensor with the average's shape and strides");
    TORCH_CHECK(!overlaps(*c, a) && !overlaps(*c, p), who, ": a bf16 copy aliases its average or source");
  }
  if (shadow != nullptr && copy != nullptr) TORCH_CHECK(!overlaps(*shadow, *copy), who, ": the bf16 copies alias");
  TORCH_CHECK(copy == nullptr || src == at::kBFloat16, who, ": module copies go with bfloat16 sources");
}

uint16_t* bf16_ptr(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

void avg_prepare_(Tensor n, Tensor w, c10::optional<double> decay, bool warmup) {
  check_counter(n, "avg_prepare_");
  weight_ptr(w, n.device(), "avg_prepare_");
  TORCH_CHECK(!decay.has_value() || (*decay > 0.0 && *decay < 1.0), "avg_prepare_: decay must lie in (0, 1), got ",
              decay.value_or(0.0));
  TORCH_CHECK(decay.has_value() || !warmup, "avg_prepare_: warmup goes with a decay");
  c10::hip::HIPGuard guard(n.device().index());
  hip_check(avg_prepare(n.data_ptr<int64_t>(), w.data_ptr<float>(), decay.has_value() ? kAvgEma : kAvgSwa,
                        decay.value_or(0.0), warmup ? 1 : 0, cur_stream(n)),
            "avg_prepare");
}

void avg_update_multi_(std::vector<Tensor> avgs, std::vector<Tensor> srcs, Tensor w, std::vector<Tensor> shadows,
                       std::vector<Tensor> copies) {
  TORCH_CHECK(avgs.size() == srcs.size(), "avg_update_multi_: one source per average");
  TORCH_CHECK(shadows.empty() || shadows.size() == avgs.size(), "avg_update_multi_: one shadow per average, or none");
  TORCH_CHECK(copies.empty() || copies.size() == avgs.size(), "avg_update_multi_: one copy per average, or none");
  if (avgs.empty()) return;
  const at::Device dev = avgs[0].device();
  const at::ScalarType src = srcs[0].scalar_type();
  const float* wp = weight_ptr(w, dev, "avg_update_multi_");
  // every pair is checked before the first launch
  for (size_t i = 0; i < avgs.size(); ++i)
    check_pair(avgs[i], srcs[i], shadows.empty() ? nullptr : &shadows[i], copies.empty() ? nullptr : &copies[i], dev,
               src, "avg_update_multi_");
  const int dt = dt_of(srcs[0]);
  c10::hip::HIPGuard guard(dev.index());
  for_tensor_chunks(avgs.size(), [&](size_t a, size_t b) {
    AvgList l{};
    l.n = (int)(b - a);
    for (size_t i = a; i < b; ++i) {
      l.numel[i - a] = avgs[i].numel();
      l.a[i - a] = avgs[i].data_ptr<float>();
      l.p[i - a] = srcs[i].data_ptr();
      l.shadow[i - a] = shadows.empty() ? nullptr : bf16_ptr(shadows[i]);
      l.copy[i - a] = copies.empty() ? nullptr : bf16_ptr(copies[i]);
    }
    hip_check(avg_update_multi(l, dt, wp, cur_stream(avgs[0])), "avg_update_multi");
  });
}

void avg_update_flat_(Tensor avg, Tensor src, Tensor w, c10::optional<Tensor> shadow, c10::optional<Tensor> copy) {
  const float* wp = weight_ptr(w, avg.device(), "avg_update_flat_");
  TORCH_CHECK(avg.dim() == 1 && src.dim() == 1, "avg_update_flat_: 1-D spans");
  check_pair(avg, src, has(shadow) ? &*shadow : nullptr, has(copy) ? &*copy : nullptr, avg.device(),
             src.scalar_type(), "avg_update_flat_");
  c10::hip::HIPGuard guard(avg.device().index());
  hip_check(avg_update_flat(avg.data_ptr<float>(), src.data_ptr(), dt_of(src), has(shadow) ? bf16_ptr(*shadow) : nullptr,
                            has(copy) ? bf16_ptr(*copy) : nullptr, avg.numel(), wp, cur_stream(avg)),
            "avg_update_flat");
}

}  // namespace

void bind_averaging(py::module_& m) {
  m.def("avg_prepare_", &avg_prepare_, py::arg("n"), py::arg("w"), py::arg("decay") = py::none(),
        py::arg("warmup") = false,
        "w = weight of update number n (1 at n == 0; SWA 1 / (n + 1); EMA 1 - decay, with warmup "
        "1 - min(decay, (1 + n) / (10 + n))), then n += 1: one single-wave launch, capturable");
  m.def("avg_update_multi_", &avg_update_multi_, py::arg("avgs"), py::arg("srcs"), py::arg("w"),
        py::arg("shadows") = std::vector<Tensor>{}, py::arg("copies") = std::vector<Tensor>{},
        "avgs[i] = fmaf(w, srcs[i] - avgs[i], avgs[i]) (a copy when w == 1), bf16 roundings into shadows / copies");
  m.def("avg_update_flat_", &avg_update_flat_, py::arg("avg"), py::arg("src"), py::arg("w"),
        py::arg("shadow") = py::none(), py::arg("copy") = py::none(), "avg_update_multi_ over one pair of 1-D spans");
}

}  // namespace ptdt
