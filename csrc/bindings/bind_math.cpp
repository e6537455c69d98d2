// Bindings of the losses, the GEMMs, the small reductions and the data kernels (RNG, sampler
// orders, gathers, the RGB packer).
#include "common.h"

namespace ptdt {
namespace {

// ------------------------------------------------------------- torch-identical sampler orders
void torch_perm_py(Tensor seeds, int64_t n, int64_t W, int64_t rank, int64_t num_samples, Tensor out,
                   c10::optional<Tensor> ws) {
  check_gpu(seeds, "seeds");
  check_gpu(out, "out");
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.dim() == 1, "torch_perm: seeds int64[E]");
  TORCH_CHECK(out.scalar_type() == at::kInt && out.dim() == 2 && out.size(0) == seeds.size(0) &&
                  out.size(1) >= num_samples && out.device() == seeds.device(),
              "torch_perm: out int32[E, >= num_samples] on the seeds' device");
  TORCH_CHECK(n >= 2 && n < (1ll << 31) && W > 0 && rank >= 0 && rank < W && num_samples > 0,
              "torch_perm: bad sampler geometry");
  int32_t* wsp = nullptr;
  if (torch_perm_lds_bytes((int)n) + 624 * 4 > 160 * 1024) {
    TORCH_CHECK(has(ws) && ws->is_cuda() && ws->scalar_type() == at::kInt && ws->is_contiguous() &&
                    ws->numel() >= seeds.size(0) * 4 * n,
                "torch_perm: n too large for LDS, pass ws = int32[E * 4n]");
    wsp = ws->data_ptr<int32_t>();
  }
  c10::hip::HIPGuard guard(out.device().index());
  hip_check(torch_perm(seeds.data_ptr<int64_t>(), (int)seeds.size(0), (int)n, (int)W, (int)rank, (int)num_samples,
                       out.data_ptr<int32_t>(), (int)out.size(1), wsp, cur_stream(out)),
            "torch_perm");
}

// [N, 3, H, W] channels_last f32/bf16 -> [N, 4, H, W] channels_last bf16 with a zero 4th channel
Tensor rgb4_pack_(Tensor x) {
  TORCH_CHECK(x.is_cuda(), "rgb4_pack: x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "rgb4_pack: x must be a channels_last [N, 3, H, W] tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "rgb4_pack: f32 or bf16");
  c10::hip::HIPGuard guard(x.device().index());
  Tensor y = at::empty({x.size(0), 4, x.size(2), x.size(3)},
                       x.options().dtype(at::kBFloat16).memory_format(at::MemoryFormat::ChannelsLast));
  hip_check(rgb4_pack(x.data_ptr(), dt_of(x), static_cast<uint16_t*>(y.data_ptr()), x.numel() / 3, cur_stream(x)),
            "rgb4_pack");
  return y;
}

// ------------------------------------------------------------- losses
// returns (loss[1], lse_ws[3B], valid[1])
std::vector<Tensor> ce_fwd(Tensor logits, c10::optional<Tensor> soft, c10::optional<Tensor> index,
                           int64_t ignore_index, double label_smoothing) {
  check_gpu(logits, "logits");
  TORCH_CHECK(logits.dim() == 2, "cross_entropy: logits must be [B, C]");
  const int64_t B = logits.size(0), C = logits.size(1);
  if (has(soft)) {
    check_gpu(*soft, "soft target");
    TORCH_CHECK(soft->scalar_type() == at::kFloat && soft->numel() == B * C, "soft targets: float [B, C]");
  } else {
    TORCH_CHECK(has(index), "cross_entropy: need soft or index targets");
    check_gpu(*index, "index target");
    TORCH_CHECK(index->scalar_type() == at::kLong && index->numel() == B, "index targets: int64 [B]");
  }
  c10::hip::HIPGuard guard(logits.device().index());
  auto fopt = logits.options().dtype(at::kFloat);
  Tensor loss = at::empty({}, fopt), lse = at::empty({3 * B}, fopt), valid = at::empty({1}, fopt);
  hip_check(ce_forward(logits.data_ptr(), dt_of(logits), ptr_or_null<const float>(soft),
                       ptr_or_null<const int64_t>(index), (int)B, (int)C, (int)ignore_index,
                       (float)label_smoothing, loss.data_ptr<float>(), lse.data_ptr<float>(),
                       valid.data_ptr<float>(), cur_stream(logits)),
            "ce_forward");
  return {loss, lse, valid};
}

Tensor ce_bwd(Tensor logits, c10::optional<Tensor> soft, c10::optional<Tensor> index, Tensor lse,
              Tensor valid, c10::optional<Tensor> grad_out, int64_t ignore_index, double label_smoothing) {
  check_gpu(logits, "logits");
  const int64_t B = logits.size(0), C = logits.size(1);
  c10::hip::HIPGuard guard(logits.device().index());
  Tensor d = at::empty_like(logits);
  hip_check(ce_backward(logits.data_ptr(), dt_of(logits), ptr_or_null<const float>(soft),
                        ptr_or_null<const int64_t>(index), lse.data_ptr<float>(), valid.data_ptr<float>(),
                        ptr_or_null<const float>(grad_out), (int)B, (int)C, (int)ignore_index,
                        (float)label_smoothing, d.data_ptr(), cur_stream(logits)),
            "ce_backward");
  return d;
}

Tensor mse_fwd(Tensor x, Tensor y) {
  check_gpu(x, "input");
  check_gpu(y, "target");
  TORCH_CHECK(x.numel() == y.numel() && x.scalar_type() == y.scalar_type(), "mse: shape/dtype mismatch");
  c10::hip::HIPGuard guard(x.device().index());
  Tensor ws = at::empty({1 + 1024}, x.options().dtype(at::kFloat));
  hip_check(mse_forward(x.data_ptr(), y.data_ptr(), dt_of(x), x.numel(), ws.data_ptr<float>(), cur_stream(x)),
            "mse_forward");
  return ws.narrow(0, 0, 1).reshape({}).clone();
}

std::vector<Tensor> mse_bwd(Tensor x, Tensor y, c10::optional<Tensor> grad_out, bool need_dx, bool need_dy) {
  check_gpu(x, "input");
  check_gpu(y, "target");
  c10::hip::HIPGuard guard(x.device().index());
  Tensor dx = need_dx ? at::empty_like(x) : Tensor();
  Tensor dy = need_dy ? at::empty_like(y) : Tensor();
  hip_check(mse_backward(x.data_ptr(), y.data_ptr(), dt_of(x), x.numel(), ptr_or_null<const float>(grad_out),
                         need_dx ? dx.data_ptr() : nullptr, need_dy ? dy.data_ptr() : nullptr, cur_stream(x)),
            "mse_backward");
  return {dx, dy};
}

// ------------------------------------------------------------- GEMM / Linear
// C = alpha*A.B (+beta C) (+bias) (relu); A/B/C/mask are 2-D (possibly transposed views).
void gemm_(Tensor A, Tensor B, Tensor C, c10::optional<Tensor> bias, c10::optional<Tensor> amask, bool relu,
           double alpha, double beta, c10::optional<Tensor> colsum, int64_t split_k) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && C.is_cuda(), "gemm: GPU tensors");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && C.dim() == 2, "gemm: 2-D operands");
  TORCH_CHECK(A.size(1) == B.size(0) && C.size(0) == A.size(0) && C.size(1) == B.size(1), "gemm: shape mismatch ",
              A.sizes(), " x ", B.sizes(), " -> ", C.sizes());
  TORCH_CHECK(A.scalar_type() == B.scalar_type(), "gemm: A/B dtype mismatch");
  GemmArgs g{};
  g.M = (int)A.size(0);
  g.N = (int)B.size(1);
  g.K = (int)A.size(1);
  g.A = A.data_ptr(); g.sam = A.stride(0); g.sak = A.stride(1);
  g.B = B.data_ptr(); g.sbk = B.stride(0); g.sbn = B.stride(1);
  g.C = C.data_ptr(); g.scm = C.stride(0); g.scn = C.stride(1);
  g.in_dtype = dt_of(A);
  g.out_dtype = dt_of(C);
  if (has(bias)) {
    check_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == g.N, "gemm: bias must have N entries");
    g.bias = bias->data_ptr();
    g.bias_dtype = dt_of(*bias);
  }
  if (has(amask)) {
    TORCH_CHECK(amask->sizes() == A.sizes() && amask->scalar_type() == A.scalar_type(), "gemm: mask like A");
    g.amask = amask->data_ptr(); g.smm = amask->stride(0); g.smk = amask->stride(1);
  }
  if (has(colsum)) {
    check_gpu(*colsum, "colsum");
    TORCH_CHECK(colsum->scalar_type() == at::kFloat && colsum->numel() == g.M, "gemm: colsum f32 [M]");
    g.colsum_out = colsum->data_ptr<float>();
  }
  g.relu = relu ? 1 : 0;
  g.alpha = (float)alpha;
  g.beta = (float)beta;
  g.split_k = (int)split_k;
  c10::hip::HIPGuard guard(A.device().index());
  hip_check(gemm(g, cur_stream(A)), "gemm");
}

// C = alpha*A.Bt^T (+beta C) (+bias) (relu) on the LDS-DMA kernel (gemm_big.hip): 256x256 or 128x128
// block tile, optional split-K (f32 C pre-zeroed by the caller).
// A [M,K], Bt [N,K]: bf16 with unit K stride; C [M,N] f32/bf16 with unit column stride.
bool gemm_big_ok(Tensor A, Tensor Bt) {
  return A.is_cuda() && Bt.is_cuda() && A.dim() == 2 && Bt.dim() == 2 && A.scalar_type() == at::kBFloat16 &&
         Bt.scalar_type() == at::kBFloat16 && A.stride(1) == 1 && Bt.stride(1) == 1 && A.size(1) == Bt.size(1) &&
         gemm_bf16_big_supported((int)A.size(0), (int)Bt.size(0), (int)A.size(1), A.stride(0), Bt.stride(0),
                                 A.data_ptr(), Bt.data_ptr());
}

void gemm_big_(Tensor A, Tensor Bt, Tensor C, c10::optional<Tensor> bias, bool relu, double alpha, double beta,
               int64_t sched, int64_t tile, int64_t split_k) {
  TORCH_CHECK(gemm_big_ok(A, Bt), "gemm_big: needs bf16 A[M,K], Bt[N,K] with unit K stride, K % 64 == 0, "
              "16-B aligned rows; got ", A.sizes(), A.strides(), " / ", Bt.sizes(), Bt.strides());
  TORCH_CHECK(C.is_cuda() && C.dim() == 2 && C.size(0) == A.size(0) && C.size(1) == Bt.size(0) && C.stride(1) == 1,
              "gemm_big: C must be [M,N] with unit column stride");
  TORCH_CHECK(C.scalar_type() == at::kFloat || C.scalar_type() == at::kBFloat16, "gemm_big: C f32 or bf16");
  BigGemmArgs g{};
  g.M = (int)A.size(0);
  g.N = (int)Bt.size(0);
  g.K = (int)A.size(1);
  g.A = A.data_ptr(); g.lda = A.stride(0);
  g.Bt = Bt.data_ptr(); g.ldb = Bt.stride(0);
  g.C = C.data_ptr(); g.ldc = C.stride(0);
  g.out_dtype = dt_of(C);
  if (has(bias)) {
    check_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == g.N, "gemm_big: bias must have N entries");
    g.bias = bias->data_ptr();
    g.bias_dtype = dt_of(*bias);
  }
  g.relu = relu ? 1 : 0;
  g.alpha = (float)alpha;
  g.beta = (float)beta;
  g.tile = tile == 128 ? 128 : 256;
  g.sched = sched < 0 ? (g.tile == 256 ? 4 : 0) : (int)sched;  // 256 tile: 8-phase schedule, grouped tile order
  g.split_k = split_k > 1 ? (int)split_k : 1;
  TORCH_CHECK(g.split_k == 1 || (C.scalar_type() == at::kFloat && !relu && beta == 0.0),
              "gemm_big: split-K accumulates fp32 atomics: C must be f32 (pre-zeroed), no relu/beta");
  c10::hip::HIPGuard guard(A.device().index());
  hip_check(gemm_bf16_big(g, cur_stream(A)), "gemm_big");
}

Tensor relu_bwd(Tensor dy, Tensor y) {
  check_gpu(dy, "dy");
  check_gpu(y, "y");
  TORCH_CHECK(y.scalar_type() == dy.scalar_type() && y.numel() == dy.numel() && y.device() == dy.device(),
              "relu_bwd: dy and y must share dtype, size and device");
  c10::hip::HIPGuard guard(dy.device().index());
  Tensor dx = at::empty_like(dy);
  hip_check(relu_backward(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dt_of(dy), dy.numel(), cur_stream(dy)),
            "relu_backward");
  return dx;
}

Tensor sum_all_(Tensor x) {
  check_gpu(x, "x");
  auto out = torch::empty({}, x.options().dtype(at::kFloat));
  c10::hip::HIPGuard guard(x.device().index());
  hip_check(sum_all(x.data_ptr(), dt_of(x), x.numel(), out.data_ptr<float>(), cur_stream(x)), "sum_all");
  return out;
}

void col_sum_(Tensor x, Tensor out, bool accumulate) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && out.scalar_type() == at::kFloat && out.numel() == x.size(1));
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.device() == x.device(), "col_sum_: out must be on x's device");
  c10::hip::HIPGuard guard(x.device().index());
  const int nsplit = col_sum_splits(x.size(0), x.size(1));
  Tensor ws = nsplit > 1 ? at::empty({nsplit, x.size(1)}, out.options()) : Tensor();
  hip_check(col_sum(x.data_ptr(), dt_of(x), x.size(0), x.size(1), out.data_ptr<float>(), accumulate,
                    nsplit > 1 ? ws.data_ptr<float>() : nullptr, nsplit, cur_stream(x)),
            "col_sum");
}

// ------------------------------------------------------------- data
void philox_(Tensor out, int64_t seed, int64_t offset, int64_t dist) {
  check_gpu(out, "out");
  TORCH_CHECK(out.scalar_type() == at::kFloat);
  c10::hip::HIPGuard guard(out.device().index());
  hip_check(philox_fill(out.data_ptr<float>(), out.numel(), (uint64_t)seed, (uint64_t)offset, (int)dist,
                        cur_stream(out)),
            "philox_fill");
}

Tensor one_hot_(Tensor idx, int64_t C) {
  check_gpu(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 1);
  c10::hip::HIPGuard guard(idx.device().index());
  Tensor out = at::empty({idx.size(0), C}, idx.options().dtype(at::kFloat));
  hip_check(one_hot(idx.data_ptr<int64_t>(), out.data_ptr<float>(), (int)idx.size(0), (int)C, cur_stream(idx)),
            "one_hot");
  return out;
}

void gather_rows_(Tensor src, Tensor idx, Tensor out) {
  check_gpu(src, "src");
  check_gpu(idx, "idx");
  check_gpu(out, "out");
  TORCH_CHECK(idx.scalar_type() == at::kInt && out.scalar_type() == src.scalar_type());
  TORCH_CHECK(src.dim() >= 1 && out.size(0) == idx.numel(), "gather_rows: out rows == idx count");
  const int64_t cols = src.numel() / std::max<int64_t>(src.size(0), 1);
  TORCH_CHECK(out.numel() == idx.numel() * cols);
  c10::hip::HIPGuard guard(src.device().index());
  hip_check(gather_rows(src.data_ptr(), idx.data_ptr<int32_t>(), out.data_ptr(), idx.numel(), cols,
                        (int)src.element_size(), cur_stream(src)),
            "gather_rows");
}

void device_sampler_(Tensor out, int64_t N, int64_t W, int64_t rank, int64_t num_samples, int64_t seed,
                     Tensor epoch, bool shuffle) {
  check_gpu(out, "out");
  TORCH_CHECK(out.scalar_type() == at::kInt && out.numel() >= num_samples, "sampler out: int32 [num_samples]");
  TORCH_CHECK(epoch.is_cuda() && epoch.scalar_type() == at::kInt && epoch.numel() == 1, "epoch: int32 [1] on GPU");
  TORCH_CHECK(N > 0 && W > 0 && rank >= 0 && rank < W, "device_sampler: bad N/W/rank");
  c10::hip::HIPGuard guard(out.device().index());
  hip_check(device_sampler(out.data_ptr<int32_t>(), N, (int)W, (int)rank, num_samples, (uint64_t)seed,
                           epoch.data_ptr<int32_t>(), shuffle ? 1 : 0, cur_stream(out)),
            "device_sampler");
}

}  // namespace

void bind_math(py::module_& m) {
  m.def("rgb4_pack", &rgb4_pack_);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("mse_fwd", &mse_fwd);
  m.def("mse_bwd", &mse_bwd);
  m.def("gemm_", &gemm_, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias") = py::none(),
        py::arg("amask") = py::none(), py::arg("relu") = false, py::arg("alpha") = 1.0, py::arg("beta") = 0.0,
        py::arg("colsum") = py::none(), py::arg("split_k") = 1);
  m.def("gemm_big_ok", &gemm_big_ok);
  m.def("gemm_big_", &gemm_big_, py::arg("A"), py::arg("Bt"), py::arg("C"), py::arg("bias") = py::none(),
        py::arg("relu") = false, py::arg("alpha") = 1.0, py::arg("beta") = 0.0, py::arg("sched") = -1,
        py::arg("tile") = 256, py::arg("split_k") = 1);
  m.def("relu_bwd", &relu_bwd);
  m.def("col_sum_", &col_sum_);
  m.def("sum_all", &sum_all_);
  m.def("philox_", &philox_);
  m.def("one_hot", &one_hot_);
  m.def("gather_rows_", &gather_rows_);
  m.def("device_sampler_", &device_sampler_);
  m.def("torch_perm_", &torch_perm_py, py::arg("seeds"), py::arg("n"), py::arg("W"), py::arg("rank"),
        py::arg("num_samples"), py::arg("out"), py::arg("ws") = py::none());
  m.def("torch_perm_needs_ws", [](int64_t n) { return torch_perm_lds_bytes((int)n) + 624 * 4 > 160 * 1024; });
}

}  // namespace ptdt
