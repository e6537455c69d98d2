// Bindings of the int8 kernels: weight-only int8 linear and the LLM.int8 pieces (outlier columns,
// row quantisation, the int8 GEMM and the decode GEMV).
#include "common.h"

namespace ptdt {
namespace {

// ------------------------------------------------------------- int8
std::vector<Tensor> quantize_int8(Tensor w) {
  check_gpu(w, "weight");
  TORCH_CHECK(w.dim() == 2);
  c10::hip::HIPGuard guard(w.device().index());
  Tensor q = at::empty(w.sizes(), w.options().dtype(at::kChar));
  Tensor s = at::empty({w.size(0)}, w.options().dtype(at::kFloat));
  hip_check(quantize_rowwise_int8(w.data_ptr(), dt_of(w), w.size(0), w.size(1), q.data_ptr<int8_t>(),
                                  s.data_ptr<float>(), cur_stream(w)),
            "quantize_int8");
  return {q, s};
}

Tensor int8_linear(Tensor x, Tensor q, Tensor scale, c10::optional<Tensor> bias) {
  check_gpu(x, "x");
  check_gpu(q, "q");
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && x.size(1) == q.size(1) && q.scalar_type() == at::kChar);
  TORCH_CHECK(scale.numel() == q.size(0));
  if (has(bias)) TORCH_CHECK(bias->numel() == q.size(0) && bias->scalar_type() == x.scalar_type());
  c10::hip::HIPGuard guard(x.device().index());
  Tensor y = at::empty({x.size(0), q.size(0)}, x.options());
  hip_check(int8_weight_gemm(x.data_ptr(), dt_of(x), q.data_ptr<int8_t>(), scale.data_ptr<float>(),
                             has(bias) ? bias->data_ptr() : nullptr, (int)x.size(0),
                             (int)q.size(0), (int)x.size(1), y.data_ptr(), dt_of(y), cur_stream(x)),
            "int8_weight_gemm");
  return y;
}

// LLM.int8 pieces
Tensor int8_col_outliers_(Tensor x, double threshold) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "int8_col_outliers: contiguous [M, K]");
  c10::hip::HIPGuard guard(x.device().index());
  Tensor mask = at::empty({x.size(1)}, x.options().dtype(at::kByte));
  Tensor ws = at::empty({x.size(1)}, x.options().dtype(at::kInt));
  hip_check(int8_col_outliers(x.data_ptr(), dt_of16(x), (int)x.size(0), (int)x.size(1), (float)threshold,
                              mask.data_ptr<uint8_t>(), reinterpret_cast<unsigned*>(ws.data_ptr<int32_t>()),
                              cur_stream(x)),
            "int8_col_outliers");
  return mask;
}

std::vector<Tensor> int8_quant_rows_(Tensor x, c10::optional<Tensor> mask) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "int8_quant_rows: contiguous [M, K]");
  const uint8_t* mp = nullptr;
  if (has(mask)) {
    TORCH_CHECK(mask->scalar_type() == at::kByte && mask->numel() == x.size(1) && mask->is_cuda());
    mp = mask->data_ptr<uint8_t>();
  }
  c10::hip::HIPGuard guard(x.device().index());
  Tensor q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  Tensor s = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
  hip_check(int8_quant_rows(x.data_ptr(), dt_of16(x), (int)x.size(0), (int)x.size(1), mp, q.data_ptr<int8_t>(),
                            s.data_ptr<float>(), cur_stream(x)),
            "int8_quant_rows");
  return {q, s};
}

Tensor int8_mm_(Tensor A, Tensor sa, Tensor B, Tensor sb, c10::optional<Tensor> addend, c10::optional<Tensor> bias,
                const std::string& out_dtype) {
  check_gpu(A, "A");
  check_gpu(B, "B");
  TORCH_CHECK(A.scalar_type() == at::kChar && B.scalar_type() == at::kChar && A.dim() == 2 && B.dim() == 2 &&
                  A.is_contiguous() && B.is_contiguous() && A.size(1) == B.size(1),
              "int8_mm: contiguous int8 A[M,K], B[N,K]");
  const int64_t M = A.size(0), N = B.size(0), K = A.size(1);
  TORCH_CHECK(K % 16 == 0, "int8_mm: K must be a multiple of 16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "int8_mm: 16-byte aligned operands");
  TORCH_CHECK(sa.scalar_type() == at::kFloat && sa.numel() == M && sb.scalar_type() == at::kFloat && sb.numel() == N);
  const float* ad = nullptr;
  if (has(addend)) {
    TORCH_CHECK(addend->scalar_type() == at::kFloat && addend->is_contiguous() && addend->numel() == M * N);
    ad = addend->data_ptr<float>();
  }
  const void* bp = nullptr;
  int bias_dt = kF32;
  if (has(bias)) {
    TORCH_CHECK(bias->numel() == N && bias->is_contiguous(), "int8_mm: bias [N]");
    bp = bias->data_ptr();
    bias_dt = dt_of16(*bias);
  }
  c10::hip::HIPGuard guard(A.device().index());
  Tensor y = at::empty({M, N}, A.options().dtype(scalar_of(out_dtype)));
  hip_check(int8_mm(A.data_ptr<int8_t>(), sa.data_ptr<float>(), B.data_ptr<int8_t>(), sb.data_ptr<float>(), ad, bp,
                    bias_dt, (int)M, (int)N, (int)K, y.data_ptr(), dt_of16(y), cur_stream(A)),
            "int8_mm");
  return y;
}

// LLM.int8 decode (M <= 32): y = int8 product with outlier columns, two launches, no host sync
// pre-shuffled weights for the decode GEMV (int8_decode.hip): [ceil(N / 16) * 16 * K] int8
Tensor int8_decode_pack_(Tensor q) {
  check_gpu(q, "weight_q");
  TORCH_CHECK(q.dim() == 2 && q.scalar_type() == at::kChar && q.is_contiguous() && q.size(1) % 64 == 0,
              "int8_decode_pack: contiguous int8 [N, K], K % 64 == 0");
  c10::hip::HIPGuard guard(q.device().index());
  const int N = (int)q.size(0), K = (int)q.size(1);
  Tensor p = at::empty({(int64_t)int8_decode_packed_bytes(N, K)}, q.options());
  hip_check(int8_decode_pack(q.data_ptr<int8_t>(), N, K, p.data_ptr<int8_t>(), cur_stream(q)), "int8_decode_pack");
  return p;
}

Tensor int8_decode_(Tensor x, Tensor q, Tensor sw, c10::optional<Tensor> bias, double threshold,
                    const std::string& out_dtype, c10::optional<Tensor> packed) {
  check_gpu(x, "x");
  check_gpu(q, "weight_q");
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && q.scalar_type() == at::kChar && x.size(1) == q.size(1),
              "int8_decode: x [M, K], weight_q int8 [N, K]");
  const int64_t M = x.size(0), N = q.size(0), K = x.size(1);
  TORCH_CHECK(int8_decode_supported((int)M, (int)N, (int)K), "int8_decode: M <= 32, K % 64 == 0, K <= ",
              kInt8DecodeMaxK, " (got M=", M, ", K=", K, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0, "int8_decode: 16-B aligned weight");
  TORCH_CHECK(sw.scalar_type() == at::kFloat && sw.numel() == N && sw.is_contiguous(), "int8_decode: scale [N]");
  const void* bp = nullptr;
  int bias_dt = kF32;
  if (has(bias)) {
    TORCH_CHECK(bias->numel() == N && bias->is_contiguous() && bias->is_cuda(), "int8_decode: bias [N]");
    bp = bias->data_ptr();
    bias_dt = dt_of16(*bias);
  }
  c10::hip::HIPGuard guard(x.device().index());
  if (!x.is_contiguous() || reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0)
    x = x.contiguous().clone();  // the prep kernel reads 16-B chunks
  Tensor ws = at::empty({(int64_t)int8_decode_ws_bytes((int)M, (int)K)}, x.options().dtype(at::kByte));
  Tensor y = at::empty({M, N}, x.options().dtype(scalar_of(out_dtype)));
  const int8_t* wp = nullptr;
  if (has(packed)) {
    TORCH_CHECK(packed->scalar_type() == at::kChar && packed->is_contiguous() && packed->is_cuda() &&
                    packed->numel() == (int64_t)int8_decode_packed_bytes((int)N, (int)K),
                "int8_decode: packed weights from int8_decode_pack");
    wp = packed->data_ptr<int8_t>();
  }
  hip_check(int8_decode(x.data_ptr(), dt_of16(x), (int)M, (int)K, (float)threshold, q.data_ptr<int8_t>(), wp,
                        sw.data_ptr<float>(), bp, bias_dt, (int)N, y.data_ptr(), dt_of16(y), ws.data_ptr(),
                        cur_stream(x)),
            "int8_decode");
  return y;
}

}  // namespace

void bind_int8(py::module_& m) {
  m.def("int8_decode", &int8_decode_, "LLM.int8 decode path (M <= 32): outliers + quantise + int8 GEMV, no host sync",
        py::arg("x"), py::arg("q"), py::arg("sw"), py::arg("bias"), py::arg("threshold"), py::arg("out_dtype"),
        py::arg("packed") = py::none());
  m.def("int8_decode_pack", &int8_decode_pack_, "pre-shuffled int8 weights for the decode GEMV");
  m.def("int8_decode_supported", &int8_decode_supported);
  m.def("quantize_int8", &quantize_int8);
  m.def("int8_linear", &int8_linear);
  m.def("int8_col_outliers", &int8_col_outliers_, py::arg("x"), py::arg("threshold"));
  m.def("int8_quant_rows", &int8_quant_rows_, py::arg("x"), py::arg("mask") = py::none());
  m.def("int8_mm", &int8_mm_, py::arg("A"), py::arg("sa"), py::arg("B"), py::arg("sb"), py::arg("addend") = py::none(),
        py::arg("bias") = py::none(), py::arg("out_dtype") = "float32");
}

}  // namespace ptdt
