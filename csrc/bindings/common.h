// Shared by the Python binding files (csrc/bindings/*.cpp), one translation unit per domain:
// gfx950 kernels (csrc/kernels), the RCCL communicator (csrc/comm) and the DDP reducer
// (csrc/reducer).
//
// Every kernel wrapper validates device/dtype/contiguity/shape on the host
// before launching (a bad launch on MI355X can reset the whole node) and
// launches on the caller's current HIP stream, so all of them are capturable
// into hipGraphs via torch.cuda.graph.
#pragma once

#include <utility>
#include <vector>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>

#include "kernels/chunks.h"
#include "kernels/kernels.h"

namespace py = pybind11;

namespace ptdt {

using at::Tensor;

// One binder per file; module.cpp calls them. The order matters to the signature strings pybind11
// writes at def time (a class-typed argument is spelled by its Python name only once registered).
void bind_engine(py::module_& m);
void bind_optim(py::module_& m);
void bind_averaging(py::module_& m);
void bind_eval(py::module_& m);
void bind_math(py::module_& m);
void bind_norm(py::module_& m);
void bind_int8(py::module_& m);
void bind_comm(py::module_& m);

inline hipStream_t cur_stream(const Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

inline void hip_check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " failed: ", hipGetErrorString(e));
}

inline int dt_of(const Tensor& t) {
  if (t.scalar_type() == at::kFloat) return kF32;
  if (t.scalar_type() == at::kBFloat16) return kBF16;
  TORCH_CHECK(false, "ptdt kernels support float32 and bfloat16, got ", t.scalar_type());
  return -1;
}

// the LLM.int8 pieces also take IEEE half (the reference's load_in_8bit Llama runs in fp16)
inline int dt_of16(const Tensor& t) {
  if (t.scalar_type() == at::kHalf) return kF16;
  return dt_of(t);
}

inline at::ScalarType scalar_of(const std::string& name) {
  if (name == "float32") return at::kFloat;
  if (name == "bfloat16") return at::kBFloat16;
  if (name == "float16") return at::kHalf;
  TORCH_CHECK(false, "int8_mm: out dtype must be float32, bfloat16 or float16, got ", name);
  return at::kFloat;
}

inline void check_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Elementwise optimizer operands: any dense memory order (channels_last conv
// weights), as long as every operand of one parameter shares it.
// same element order in memory: equal strides on every dimension of size > 1 (size-1 dimensions
// carry arbitrary strides, e.g. a [C, K, 1, 1] tensor contiguous vs channels_last)
inline bool same_memory_order(const Tensor& a, const Tensor& b) {
  if (a.sizes() != b.sizes()) return false;
  for (int64_t d = 0; d < a.dim(); ++d)
    if (a.size(d) > 1 && a.stride(d) != b.stride(d)) return false;
  return true;
}

inline void check_dense_like(const Tensor& p, const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_non_overlapping_and_dense(), name, " must be dense (non-overlapping)");
  TORCH_CHECK(t.numel() == p.numel() &&
                  (t.strides() == p.strides() || (t.is_contiguous() && p.is_contiguous()) || same_memory_order(t, p)),
              name, " must have the parameter's memory layout");
}

// an optional tensor argument that was given (not None, not an undefined tensor)
inline bool has(const c10::optional<Tensor>& t) { return t.has_value() && t->defined(); }

template <typename T>
T* ptr_or_null(const c10::optional<Tensor>& t) {
  return has(t) ? static_cast<T*>(t->data_ptr()) : nullptr;
}

template <typename F>
void for_tensor_chunks(size_t n, F&& f) {
  for (size_t s = 0; s < n; s += kMaxTensorsPerLaunch) f(s, std::min(n, s + (size_t)kMaxTensorsPerLaunch));
}

}  // namespace ptdt
