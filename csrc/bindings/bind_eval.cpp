// Bindings of the evaluation metrics (csrc/kernels/eval_metrics.hip): the row pass on its own, and
// one meter update (row pass + accumulate) on caller-owned workspaces.
#include <climits>

#include "common.h"

namespace ptdt {
namespace {

// [B, C] f32 / bf16 logits with unit column stride and rows that do not overlap, int64[B] targets on
// the same device. Returns (B, C, row stride in elements).
struct RowsShape {
  int B, C;
  int64_t ld;
};

RowsShape check_rows(const Tensor& logits, const Tensor& target, const char* who) {
  TORCH_CHECK(logits.is_cuda() && target.is_cuda() && logits.device() == target.device(), who,
              ": logits and target must be on one GPU");
  dt_of(logits);
  TORCH_CHECK(target.scalar_type() == at::kLong, who, ": target must be int64, got ", target.scalar_type());
  TORCH_CHECK(logits.dim() == 2, who, ": logits must be [B, C], got ", logits.dim(), " dimensions");
  const int64_t B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(B >= 1 && C >= 1, who, ": logits must have at least one row and one class, got [", B, ", ", C, "]");
  TORCH_CHECK(B <= INT_MAX && C <= INT_MAX - 64, who, ": logits [", B, ", ", C, "] exceed the 32-bit launch geometry");
  TORCH_CHECK(C == 1 || logits.stride(1) == 1, who, ": logits rows must be contiguous (column stride 1, got ",
              logits.stride(1), "); pass logits.contiguous()");
  TORCH_CHECK(B == 1 || logits.stride(0) >= C, who, ": logits rows overlap (row stride ", logits.stride(0),
              " < C = ", C, ")");
  TORCH_CHECK(target.dim() == 1 && target.numel() == B && target.is_contiguous(), who,
              ": target must be a contiguous int64[B] with B = ", B, ", got ", target.sizes());
  return {(int)B, (int)C, B == 1 ? C : logits.stride(0)};
}

void launch_rows(const Tensor& logits, const Tensor& target, const RowsShape& sh, int64_t ignore_index,
                 const Tensor& row_loss, const Tensor& rank) {
  hip_check(eval_rows(logits.data_ptr(), dt_of(logits), sh.ld, target.data_ptr<int64_t>(), sh.B, sh.C, ignore_index,
                      row_loss.data_ptr<float>(), rank.data_ptr<int32_t>(), cur_stream(logits)),
            "eval_rows");
}

std::pair<Tensor, Tensor> eval_rows_(Tensor logits, Tensor target, int64_t ignore_index) {
  const RowsShape sh = check_rows(logits, target, "eval_rows");
  c10::hip::HIPGuard guard(logits.device().index());
  Tensor row_loss = at::empty({sh.B}, logits.options().dtype(at::kFloat));
  Tensor rank = at::empty({sh.B}, logits.options().dtype(at::kInt));
  launch_rows(logits, target, sh, ignore_index, row_loss, rank);
  return {row_loss, rank};
}

void eval_update_(Tensor logits, Tensor target, int64_t ignore_index, std::vector<int64_t> topk, Tensor counters,
                  Tensor loss_sum, Tensor row_loss, Tensor rank) {
  const char* who = "eval_update_";
  const RowsShape sh = check_rows(logits, target, who);
  const at::Device dev = logits.device();
  TORCH_CHECK(!topk.empty() && topk.size() <= (size_t)kEvalMaxK, who, ": 1 to ", kEvalMaxK, " values of k, got ",
              topk.size());
  EvalTopK ks{};
  ks.n = (int)topk.size();
  for (size_t i = 0; i < topk.size(); ++i) {
    TORCH_CHECK(topk[i] >= 1 && topk[i] <= sh.C, who, ": k = ", topk[i], " is outside [1, C = ", sh.C, "]");
    TORCH_CHECK(i == 0 || topk[i] > topk[i - 1], who, ": the ks must be strictly increasing");
    ks.k[i] = (int)topk[i];
  }
  TORCH_CHECK(counters.is_cuda() && counters.device() == dev && counters.scalar_type() == at::kLong &&
                  counters.dim() == 1 && counters.numel() == kEvalCounters + ks.n && counters.is_contiguous(),
              who, ": counters must be a contiguous int64[", kEvalCounters + ks.n, "] on the logits' device");
  TORCH_CHECK(loss_sum.is_cuda() && loss_sum.device() == dev && loss_sum.scalar_type() == at::kDouble &&
                  loss_sum.numel() == 1,
              who, ": loss_sum must be one float64 value on the logits' device");
  TORCH_CHECK(row_loss.is_cuda() && row_loss.device() == dev && row_loss.scalar_type() == at::kFloat &&
                  row_loss.dim() == 1 && row_loss.numel() == sh.B && row_loss.is_contiguous(),
              who, ": the row_loss workspace must be a contiguous float32[B] on the logits' device");
  TORCH_CHECK(rank.is_cuda() && rank.device() == dev && rank.scalar_type() == at::kInt && rank.dim() == 1 &&
                  rank.numel() == sh.B && rank.is_contiguous(),
              who, ": the rank workspace must be a contiguous int32[B] on the logits' device");
  c10::hip::HIPGuard guard(dev.index());
  launch_rows(logits, target, sh, ignore_index, row_loss, rank);
  hip_check(eval_accumulate(row_loss.data_ptr<float>(), rank.data_ptr<int32_t>(), sh.B, ks,
                            counters.data_ptr<int64_t>(), loss_sum.data_ptr<double>(), cur_stream(logits)),
            "eval_accumulate");
}

}  // namespace

void bind_eval(py::module_& m) {
  m.attr("EVAL_MAX_K") = kEvalMaxK;
  m.attr("EVAL_ROWS_PER_BLOCK") = kEvalRowsPerBlock;
  m.attr("EVAL_WAVE_ROW_MAX_C") = kEvalWaveRowMaxC;
  m.def("eval_rows", &eval_rows_, py::arg("logits"), py::arg("target"), py::arg("ignore_index") = -100,
        "(row_loss float32[B], rank int32[B]) of [B, C] logits: lse - z_y, and the target's position in a stable "
        "descending sort; ignore_index rows (0, -1), other out-of-range targets (0, -2)");
  m.def("eval_update_", &eval_update_, py::arg("logits"), py::arg("target"), py::arg("ignore_index"), py::arg("topk"),
        py::arg("counters"), py::arg("loss_sum"), py::arg("row_loss"), py::arg("rank"),
        "eval_rows into the row_loss / rank workspaces, then counters += [rows, valid, ignored, bad_target, nonfinite, "
        "correct@k...] and loss_sum += the finite losses: two launches, fixed order, capturable");
}

}  // namespace ptdt
