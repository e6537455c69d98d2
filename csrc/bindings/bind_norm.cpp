// Bindings of the NHWC layer kernels: BatchNorm (local and cross-rank statistics), the fused
// 1x1 convolution + BatchNorm passes and max pooling.
#include <map>
#include <mutex>

#include "common.h"

namespace ptdt {
namespace {

Tensor bn_relu(Tensor x, Tensor scale, Tensor shift, bool relu) {
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() >= 2);
  const int64_t N = x.size(0), C = x.size(1);
  const int64_t HW = x.numel() / std::max<int64_t>(N * C, 1);
  TORCH_CHECK(scale.numel() == C && shift.numel() == C && scale.scalar_type() == at::kFloat);
  c10::hip::HIPGuard guard(x.device().index());
  Tensor y = at::empty_like(x);
  hip_check(bn_relu_apply(x.data_ptr(), dt_of(x), scale.data_ptr<float>(), shift.data_ptr<float>(), N, C, HW,
                          relu, y.data_ptr(), cur_stream(x)),
            "bn_relu_apply");
  return y;
}

// ------------------------------------------------------------- batchnorm
// Activations as [M, C] rows: NHWC (channels_last-contiguous 4D) or contiguous 2D.
void bn_rows(const Tensor& x, int64_t* M, int* C) {
  TORCH_CHECK(x.is_cuda(), "batchnorm: GPU tensor expected");
  if (x.dim() == 2) {
    TORCH_CHECK(x.is_contiguous(), "batchnorm: 2D input must be contiguous");
  } else {
    TORCH_CHECK(x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
                "batchnorm: 4D input must be channels_last-contiguous (NHWC)");
  }
  *C = (int)x.size(1);
  *M = x.numel() / std::max<int64_t>(*C, 1);
  const int V = x.scalar_type() == at::kFloat ? 4 : 8;
  TORCH_CHECK(*C % V == 0, "batchnorm: channels must be a multiple of ", V);
  TORCH_CHECK(*C <= bn_max_channels(), "batchnorm: at most ", bn_max_channels(),
              " channels (the per-channel tables of the elementwise passes live in LDS)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "batchnorm: 16-byte aligned data expected");
}

void same_rows(const Tensor& a, const Tensor& x, const char* name) {
  TORCH_CHECK(a.defined() && a.sizes() == x.sizes() && a.strides() == x.strides() &&
                  a.scalar_type() == x.scalar_type() && a.device() == x.device(),
              "batchnorm: ", name, " must match x (shape, strides, dtype, device)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0, "batchnorm: ", name, " not 16-byte aligned");
}

// an optional operand laid out as x (a residual, a second gradient addend): its data, or null
const void* opt_rows(const c10::optional<Tensor>& t, const Tensor& x, const char* name) {
  if (!has(t)) return nullptr;
  same_rows(*t, x, name);
  return t->data_ptr();
}

// elements of the ReLU bit mask of x as [M, C] rows: one byte per 16-B vector of x
int64_t bn_mask_numel(const Tensor& x, int64_t M, int C) { return M * C / (x.scalar_type() == at::kFloat ? 4 : 8); }

// Ticket array for the last-block hand-off: the caller's (a zeroed int32 tensor
// owned by the BN module, so two modules never share one), else one per device
// created outside graph capture. The kernels re-arm what they use.
int* bn_tickets(const Tensor& x, const c10::optional<Tensor>& given, int need) {
  if (has(given)) {
    TORCH_CHECK(given->is_cuda() && given->device() == x.device() && given->scalar_type() == at::kInt &&
                    given->is_contiguous() && given->numel() >= need,
                "batchnorm: tickets must be a zeroed int32 tensor of >= ", need, " elements on x's device");
    return given->data_ptr<int>();
  }
  static std::mutex mu;
  static std::map<int, int*> per_device;
  constexpr int kMax = 1024;
  TORCH_CHECK(need <= kMax, "batchnorm: too many channel tiles");
  std::lock_guard<std::mutex> g(mu);
  const int dev = (int)x.device().index();
  auto it = per_device.find(dev);
  if (it != per_device.end()) return it->second;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  hip_check(hipStreamIsCapturing(cur_stream(x), &st), "hipStreamIsCapturing");
  TORCH_CHECK(st == hipStreamCaptureStatusNone,
              "batchnorm: pass a tickets tensor (ops.norm.BatchNorm2d does) or run once before graph capture");
  int* t = nullptr;
  hip_check(hipMalloc(&t, kMax * sizeof(int)), "hipMalloc(bn tickets)");
  hip_check(hipMemset(t, 0, kMax * sizeof(int)), "hipMemset(bn tickets)");
  per_device[dev] = t;
  return t;
}

const float* opt_f32(const c10::optional<Tensor>& t, int64_t C, const char* name) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == C,
              "batchnorm: ", name, " must be a contiguous f32 GPU tensor of C elements");
  return t->data_ptr<float>();
}

// The affine parameters, the running statistics with their counter, momentum and eps of a training
// forward over C channels (the batch statistics' destinations: split_stats).
void fill_bn_params(BnParams& p, int C, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& bias,
                    const c10::optional<Tensor>& running_mean, const c10::optional<Tensor>& running_var,
                    const c10::optional<Tensor>& num_batches_tracked, double momentum, double eps) {
  p.weight = opt_f32(weight, C, "weight");
  p.bias = opt_f32(bias, C, "bias");
  p.running_mean = const_cast<float*>(opt_f32(running_mean, C, "running_mean"));
  p.running_var = const_cast<float*>(opt_f32(running_var, C, "running_var"));
  TORCH_CHECK((p.running_mean == nullptr) == (p.running_var == nullptr), "batchnorm: running_mean/var together");
  if (has(num_batches_tracked)) {
    TORCH_CHECK(num_batches_tracked->is_cuda() && num_batches_tracked->scalar_type() == at::kLong &&
                num_batches_tracked->numel() == 1, "batchnorm: num_batches_tracked must be a 1-element int64 tensor");
    p.num_batches_tracked = num_batches_tracked->data_ptr<int64_t>();
  }
  p.momentum = (float)momentum;
  p.eps = (float)eps;
}

// stats [4, C] = mean, invstd, scale, shift: a forward's statistics handed back by the caller ...
float* checked_stats(const Tensor& stats, int64_t C) {
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kFloat && stats.is_contiguous() && stats.numel() == 4 * C,
              "batchnorm: stats must be the [4, C] forward statistics");
  return stats.data_ptr<float>();
}

// ... and its four rows as the kernels' parameter blocks (BnParams, BnBwdParams) take them
template <typename P>
void split_stats(P& p, float* st, int64_t C) {
  p.mean = st;
  p.invstd = st + C;
  p.scale = st + 2 * C;
  p.shift = st + 3 * C;
}

// Training forward: returns (y, stats[4, C] = mean, invstd, scale, shift).
std::vector<Tensor> bn_fwd_train(Tensor x, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                                 c10::optional<Tensor> running_mean, c10::optional<Tensor> running_var,
                                 c10::optional<Tensor> num_batches_tracked, c10::optional<Tensor> residual, bool relu,
                                 double momentum, double eps, c10::optional<Tensor> tickets, bool want_mask,
                                 bool stats_only) {
  int64_t M;
  int C;
  bn_rows(x, &M, &C);
  c10::hip::HIPGuard guard(x.device().index());
  BnFwdArgs a{};
  a.x = x.data_ptr();
  a.residual = opt_rows(residual, x, "residual");
  Tensor y = stats_only ? Tensor() : at::empty_like(x);
  Tensor stats = at::empty({4, C}, x.options().dtype(at::kFloat));
  Tensor ws = at::empty({bn_workspace_floats(M, C, dt_of(x))}, x.options().dtype(at::kFloat));
  a.y = stats_only ? nullptr : y.data_ptr();
  a.dtype = dt_of(x);
  a.M = M;
  a.C = C;
  a.relu = relu ? 1 : 0;
  a.workspace = ws.data_ptr<float>();
  a.tickets = bn_tickets(x, tickets, bn_num_tickets(C, a.dtype));
  fill_bn_params(a.p, C, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps);
  split_stats(a.p, stats.data_ptr<float>(), C);
  Tensor mask;
  if (want_mask && relu && a.residual != nullptr && !stats_only) {
    mask = at::empty({bn_mask_numel(x, M, C)}, x.options().dtype(at::kByte));
    a.mask_out = mask.data_ptr<uint8_t>();
  }
  hip_check(bn_forward_train(a, cur_stream(x)), "bn_forward_train");
  return {y, stats, mask};
}

// Training forward from precomputed statistics (conv1x1_bn_stats wrote stats = mean, invstd, scale,
// shift and the running statistics): the apply pass only. Returns (y, mask).
std::vector<Tensor> bn_fwd_apply(Tensor x, Tensor stats, c10::optional<Tensor> residual, bool relu, bool want_mask) {
  int64_t M;
  int C;
  bn_rows(x, &M, &C);
  c10::hip::HIPGuard guard(x.device().index());
  BnFwdArgs a{};
  split_stats(a.p, checked_stats(stats, C), C);
  a.x = x.data_ptr();
  a.residual = opt_rows(residual, x, "residual");
  Tensor y = at::empty_like(x);
  a.y = y.data_ptr();
  a.dtype = dt_of(x);
  a.M = M;
  a.C = C;
  a.relu = relu ? 1 : 0;
  a.stats_ready = 1;
  Tensor mask;
  if (want_mask && relu && a.residual != nullptr) {
    mask = at::empty({bn_mask_numel(x, M, C)}, x.options().dtype(at::kByte));
    a.mask_out = mask.data_ptr<uint8_t>();
  }
  hip_check(bn_forward_train(a, cur_stream(x)), "bn_forward_apply");
  return {y, mask};
}

// tile 0: the streaming kernel (conv1x1_bn.hip), else the tiled GEMM's block tile
int64_t conv1x1_bn_num_tickets(int64_t M, int64_t N, int64_t tile, int64_t K) {
  if (tile == 0) return conv1x1_bn_stream_num_tickets((int)M, (int)K, (int)N);
  return gemm_bn_num_tickets((int)M, (int)N, (int)tile);
}

// 1x1 convolution (stride 1) + the training BatchNorm's batch statistics of its output:
// y[M, N] = x[M, K] . w[N, K]^T in bf16 (x: the NHWC activation as rows, w: the [Cout, Cin] weight)
// and stats [4, N] = mean, invstd, scale, shift; running statistics and num_batches_tracked updated.
std::vector<Tensor> conv1x1_bn_stats(Tensor x, Tensor w, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                                     c10::optional<Tensor> running_mean, c10::optional<Tensor> running_var,
                                     c10::optional<Tensor> num_batches_tracked, double momentum, double eps,
                                     Tensor tickets, int64_t tile) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.device() == w.device(), "conv1x1_bn_stats: GPU operands");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1), "conv1x1_bn_stats: x [M, K], w [N, K]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "conv1x1_bn_stats: bf16");
  TORCH_CHECK(x.stride(1) == 1 && w.stride(1) == 1, "conv1x1_bn_stats: K-contiguous operands");
  TORCH_CHECK(tile == 0 || tile == 128 || tile == 256, "conv1x1_bn_stats: tile 0 (streaming kernel), 128 or 256");
  const int M = (int)x.size(0), N = (int)w.size(0), K = (int)x.size(1);
  TORCH_CHECK(tile != 0 || (conv1x1_bn_stream_supported(K, N) && x.stride(0) == K && w.stride(0) == K),
              "conv1x1_bn_stats: the streaming kernel has no (K, N) = (", K, ", ", N, ") instance");
  TORCH_CHECK(x.size(0) < (1LL << 31) && N % 8 == 0, "conv1x1_bn_stats: N % 8 == 0");
  TORCH_CHECK(gemm_bf16_big_supported(M, N, K, x.stride(0), w.stride(0), x.data_ptr(), w.data_ptr()),
              "conv1x1_bn_stats: K % 64 == 0, 16-B aligned rows");
  c10::hip::HIPGuard guard(x.device().index());
  TORCH_CHECK(tickets.is_cuda() && tickets.device() == x.device() && tickets.scalar_type() == at::kInt &&
                  tickets.is_contiguous() && tickets.numel() >= conv1x1_bn_num_tickets(M, N, tile, K),
              "conv1x1_bn_stats: tickets must be a zeroed int32 tensor of >= ", conv1x1_bn_num_tickets(M, N, tile, K),
              " elements");
  Tensor y = at::empty({M, N}, x.options());
  Tensor stats = at::empty({4, N}, x.options().dtype(at::kFloat));
  Tensor ws = at::empty({tile == 0 ? conv1x1_bn_stream_ws_floats(M, K, N) : gemm_bn_ws_floats(M, N, (int)tile)},
                        x.options().dtype(at::kFloat));
  BigGemmArgs g{};
  g.M = M, g.N = N, g.K = K;
  g.A = x.data_ptr(), g.lda = x.stride(0);
  g.Bt = w.data_ptr(), g.ldb = w.stride(0);
  g.C = y.data_ptr(), g.ldc = N;
  g.out_dtype = kBF16;
  g.alpha = 1.f;
  g.sched = 1;
  g.tile = (int)tile;
  g.split_k = 1;
  GemmBnEpi e{};
  e.ws = ws.data_ptr<float>();
  e.tickets = tickets.data_ptr<int>();
  fill_bn_params(e.p, N, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps);
  split_stats(e.p, stats.data_ptr<float>(), N);
  if (tile == 0)
    hip_check(conv1x1_bn_stream(x.data_ptr(), w.data_ptr(), y.data_ptr(), M, K, N, e, cur_stream(x)),
              "conv1x1_bn_stream");
  else
    hip_check(gemm_bn_stats(g, e, cur_stream(x)), "conv1x1_bn_stats");
  return {y, stats};
}

// The checks, kernel arguments and output tensors of a backward launch; the caller launches, with
// `guard` still on x's device. reduce_only: g goes out through dres (want_dres is true), dx stays null.
// with_coef: dwb is [5, C] = dweight, dbias, A, B, C with coef_a/b/c on its last three rows; else
// [2, C] and they stay null (the cross-rank pass computes them after the all-reduce).
struct BnBwdCall {
  c10::hip::OptionalHIPGuard guard;
  BnBwdArgs a{};
  Tensor dx, dres, dwb, ws;
  Tensor dw, db;  // the parameter gradients to return: undefined without want_dweight

  BnBwdCall(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& y, const c10::optional<Tensor>& weight,
            const Tensor& stats, bool relu, bool want_dres, bool want_dweight, const c10::optional<Tensor>& tickets,
            const c10::optional<Tensor>& dweight_out, const c10::optional<Tensor>& dbias_out,
            const c10::optional<Tensor>& dy2, const c10::optional<Tensor>& mask, bool reduce_only, bool with_coef) {
    int64_t M;
    int C;
    bn_rows(x, &M, &C);
    same_rows(dy, x, "dy");
    guard.set_index(x.device().index());
    split_stats(a.p, checked_stats(stats, C), C);
    a.dy = dy.data_ptr();
    a.dy2 = opt_rows(dy2, x, "dy2");  // second addend (residual link), same layout as x
    a.x = x.data_ptr();
    if (relu && has(mask)) {  // the forward's bit mask (needs want_dres)
      TORCH_CHECK(want_dres && mask->is_cuda() && mask->scalar_type() == at::kByte &&
                      mask->numel() == bn_mask_numel(x, M, C),
                  "batchnorm: mask must be the forward's [M*C/V] byte mask", reduce_only ? "" : ", with want_dres");
      a.mask = mask->data_ptr<uint8_t>();
    } else if (relu && has(y)) {  // else: the mask is recomputed from x (no residual)
      same_rows(*y, x, "y");
      a.y = y->data_ptr();
    }
    if (!reduce_only) dx = at::empty_like(x);
    if (want_dres) dres = at::empty_like(x);
    dwb = at::empty({with_coef ? 5 : 2, C}, x.options().dtype(at::kFloat));
    ws = at::empty({bn_workspace_floats(M, C, dt_of(x))}, x.options().dtype(at::kFloat));
    a.dx = reduce_only ? nullptr : dx.data_ptr();
    a.dres = want_dres ? dres.data_ptr() : nullptr;
    a.reduce_only = reduce_only ? 1 : 0;
    a.dtype = dt_of(x);
    a.M = M;
    a.C = C;
    a.relu = relu ? 1 : 0;
    a.workspace = ws.data_ptr<float>();
    a.tickets = bn_tickets(x, tickets, bn_num_tickets(C, a.dtype));
    a.p.weight = opt_f32(weight, C, "weight");
    float* d = dwb.data_ptr<float>();
    if (want_dweight) {
      // parameter-gradient destinations given by the caller (DDP bucket slots): written in place
      a.p.dweight = has(dweight_out) ? const_cast<float*>(opt_f32(dweight_out, C, "dweight_out")) : d;
      a.p.dbias = has(dbias_out) ? const_cast<float*>(opt_f32(dbias_out, C, "dbias_out")) : d + C;
      dw = has(dweight_out) ? *dweight_out : dwb[0];
      db = has(dbias_out) ? *dbias_out : dwb[1];
    }
    if (with_coef) {
      a.p.coef_a = d + 2 * C;
      a.p.coef_b = d + 3 * C;
      a.p.coef_c = d + 4 * C;
    }
  }
};

// Backward: returns (dx, dweight, dbias, dres); dres undefined unless want_dres.
std::vector<Tensor> bn_bwd(Tensor dy, Tensor x, c10::optional<Tensor> y, c10::optional<Tensor> weight, Tensor stats,
                           bool relu, bool want_dres, bool want_dweight, c10::optional<Tensor> tickets,
                           c10::optional<Tensor> dweight_out, c10::optional<Tensor> dbias_out,
                           c10::optional<Tensor> dy2, c10::optional<Tensor> mask) {
  // a residual gradient means the forward added a residual, and then x alone does not give the
  // ReLU mask: only the forward's y or its mask bytes do
  TORCH_CHECK(!(relu && want_dres) || has(y) || has(mask),
              "batchnorm: bn_bwd with relu and want_dres needs the forward's y or mask");
  BnBwdCall c(dy, x, y, weight, stats, relu, want_dres, want_dweight, tickets, dweight_out, dbias_out, dy2, mask,
              /*reduce_only=*/false, /*with_coef=*/true);
  hip_check(bn_backward(c.a, cur_stream(x)), "bn_backward");
  return {c.dx, c.dw, c.db, c.dres};
}

// BN backward reduce pass only (for conv1x1_bwd_): returns (g, dweight, dbias, coef[3, C]) where g is the
// masked incoming gradient (ReLU mask, + dy2) and dx = coef[0] g + coef[1] x + coef[2] per channel.
std::vector<Tensor> bn_bwd_reduce(Tensor dy, Tensor x, c10::optional<Tensor> weight, Tensor stats, bool relu,
                                  bool want_dweight, c10::optional<Tensor> tickets, c10::optional<Tensor> dweight_out,
                                  c10::optional<Tensor> dbias_out, c10::optional<Tensor> dy2,
                                  c10::optional<Tensor> mask) {
  BnBwdCall c(dy, x, c10::nullopt, weight, stats, relu, /*want_dres=*/true, want_dweight, tickets, dweight_out,
              dbias_out, dy2, mask, /*reduce_only=*/true, /*with_coef=*/true);
  hip_check(bn_backward(c.a, cur_stream(x)), "bn_backward(reduce)");
  return {c.dres, c.dw, c.db, c.dwb.narrow(0, 2, 3)};
}

// ---- cross-rank statistics (ops.norm.SyncBatchNorm)
double* f64_of(const Tensor& t, const Tensor& x, int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device() && t.scalar_type() == at::kDouble && t.is_contiguous() &&
                  t.numel() == numel,
              "batchnorm: ", name, " must be a contiguous float64 tensor of ", numel, " elements on x's device");
  return t.data_ptr<double>();
}

// This rank's record (local mean[C], M2[C], row count) into rec[2 C + 1] (float64, written in place).
void bn_sync_stats_(Tensor x, Tensor rec, c10::optional<Tensor> tickets) {
  int64_t M;
  int C;
  bn_rows(x, &M, &C);
  c10::hip::HIPGuard guard(x.device().index());
  double* r = f64_of(rec, x, 2 * (int64_t)C + 1, "rec");
  Tensor ws = at::empty({bn_workspace_floats(M, C, dt_of(x))}, x.options().dtype(at::kFloat));
  hip_check(bn_sync_stats(x.data_ptr(), dt_of(x), M, C, ws.data_ptr<float>(),
                          bn_tickets(x, tickets, bn_num_tickets(C, dt_of(x))), r, cur_stream(x)),
            "bn_sync_stats");
}

// Merge of the gathered records [W, 2 C + 1]: returns (stats[4, C], count[1] float64 = global rows);
// running statistics and num_batches_tracked updated.
std::vector<Tensor> bn_sync_merge_(Tensor rec, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                                   c10::optional<Tensor> running_mean, c10::optional<Tensor> running_var,
                                   c10::optional<Tensor> num_batches_tracked, double momentum, double eps) {
  TORCH_CHECK(rec.is_cuda() && rec.scalar_type() == at::kDouble && rec.is_contiguous() && rec.dim() == 2 &&
                  rec.size(0) >= 1 && rec.size(1) >= 3 && rec.size(1) % 2 == 1,
              "batchnorm: rec must be the gathered [W, 2 C + 1] float64 records");
  const int W = (int)rec.size(0), C = (int)((rec.size(1) - 1) / 2);
  c10::hip::HIPGuard guard(rec.device().index());
  Tensor stats = at::empty({4, C}, rec.options().dtype(at::kFloat));
  Tensor count = at::empty({1}, rec.options());
  BnParams p{};
  fill_bn_params(p, C, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps);
  split_stats(p, stats.data_ptr<float>(), C);
  hip_check(bn_sync_merge(rec.data_ptr<double>(), W, C, p, count.data_ptr<double>(), cur_stream(rec)),
            "bn_sync_merge");
  return {stats, count};
}

// Backward reduce pass with the global statistics: returns (g, dweight, dbias, sums[2, C] float64) --
// the LOCAL sums (to be all-reduced) and the LOCAL parameter gradients.
std::vector<Tensor> bn_sync_bwd_reduce(Tensor dy, Tensor x, c10::optional<Tensor> weight, Tensor stats, bool relu,
                                       bool want_dweight, c10::optional<Tensor> tickets,
                                       c10::optional<Tensor> dweight_out, c10::optional<Tensor> dbias_out,
                                       c10::optional<Tensor> dy2, c10::optional<Tensor> mask) {
  BnBwdCall c(dy, x, c10::nullopt, weight, stats, relu, /*want_dres=*/true, want_dweight, tickets, dweight_out,
              dbias_out, dy2, mask, /*reduce_only=*/true, /*with_coef=*/false);
  Tensor sums = at::empty({2, c.a.C}, x.options().dtype(at::kDouble));
  hip_check(bn_sync_backward_reduce(c.a, sums.data_ptr<double>(), cur_stream(x)), "bn_sync_backward_reduce");
  return {c.dres, c.dw, c.db, sums};
}

// coef[3, C] of dx = A g + B x + C from the all-reduced sums[2, C] and the global row count[1].
Tensor bn_sync_coef_(Tensor sums, Tensor count, c10::optional<Tensor> weight, Tensor stats) {
  // C comes from stats itself here, so its shape is checked in place of checked_stats' element count
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kFloat && stats.is_contiguous() && stats.dim() == 2 &&
                  stats.size(0) == 4,
              "batchnorm: stats must be the [4, C] forward statistics");
  const int C = (int)stats.size(1);
  c10::hip::HIPGuard guard(stats.device().index());
  const double* sm = f64_of(sums, stats, 2 * (int64_t)C, "sums");
  const double* cnt = f64_of(count, stats, 1, "count");
  Tensor coef = at::empty({3, C}, stats.options());
  BnBwdParams p{};
  p.weight = opt_f32(weight, C, "weight");
  split_stats(p, stats.data_ptr<float>(), C);  // the kernel reads mean and invstd only
  float* d = coef.data_ptr<float>();
  p.coef_a = d;
  p.coef_b = d + C;
  p.coef_c = d + 2 * C;
  hip_check(bn_sync_coef(sm, cnt, C, p, cur_stream(stats)), "bn_sync_coef");
  return coef;
}

// dx = coef[0] g + coef[1] x + coef[2] per channel (the backward's apply pass over a materialised g).
Tensor bn_bwd_apply_g(Tensor g, Tensor x, Tensor coef) {
  int64_t M;
  int C;
  bn_rows(x, &M, &C);
  same_rows(g, x, "g");
  c10::hip::HIPGuard guard(x.device().index());
  TORCH_CHECK(coef.is_cuda() && coef.device() == x.device() && coef.scalar_type() == at::kFloat &&
                  coef.is_contiguous() && coef.numel() == 3 * (int64_t)C,
              "batchnorm: coef must be [3, C] float");
  Tensor dx = at::empty_like(x);
  hip_check(bn_backward_apply_g(g.data_ptr(), x.data_ptr(), dx.data_ptr(), dt_of(x), coef.data_ptr<float>(), M, C,
                                cur_stream(x)),
            "bn_backward_apply_g");
  return dx;
}

bool conv1x1_bwd_supported_(int64_t K, int64_t N) { return conv1x1_bwd_supported((int)K, (int)N); }

// Backward of BN(conv1x1(x)) from bn_bwd_reduce's (g, coef): returns (dx [M, K], dw [N, K]) in bf16.
std::vector<Tensor> conv1x1_bwd_(Tensor g, Tensor y, Tensor x, Tensor w, Tensor coef) {
  TORCH_CHECK(g.is_cuda() && y.is_cuda() && x.is_cuda() && w.is_cuda() && coef.is_cuda(), "conv1x1_bwd: GPU operands");
  TORCH_CHECK(g.dim() == 2 && y.sizes() == g.sizes() && x.dim() == 2 && w.dim() == 2 && x.size(0) == g.size(0) &&
                  w.size(0) == g.size(1) && w.size(1) == x.size(1),
              "conv1x1_bwd: g, y [M, N], x [M, K], w [N, K]");
  for (const Tensor* t : {&g, &y, &x, &w})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->is_contiguous(), "conv1x1_bwd: contiguous bf16 operands");
  const int64_t M = g.size(0), N = g.size(1), K = x.size(1);
  TORCH_CHECK(conv1x1_bwd_supported((int)K, (int)N), "conv1x1_bwd: no (K, N) = (", K, ", ", N, ") instance");
  TORCH_CHECK(coef.scalar_type() == at::kFloat && coef.is_contiguous() && coef.numel() == 3 * N,
              "conv1x1_bwd: coef [3, N] float");
  TORCH_CHECK(M < (1LL << 31), "conv1x1_bwd: M < 2^31");
  c10::hip::HIPGuard guard(g.device().index());
  Tensor dx = at::empty({M, K}, x.options());
  Tensor dw = at::empty({N, K}, w.options());
  Tensor ws = at::empty({conv1x1_bwd_ws_floats((int)M, (int)K, (int)N)}, g.options().dtype(at::kFloat));
  hip_check(conv1x1_bwd(g.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), coef.data_ptr<float>(), dx.data_ptr(),
                        dw.data_ptr(), ws.data_ptr<float>(), (int)M, (int)K, (int)N,
                        cur_stream(g)),
            "conv1x1_bwd");
  return {dx, dw};
}

// y = ReLU?(x*scale + shift (+ residual)), per channel (eval-mode BN).
Tensor bn_apply_(Tensor x, c10::optional<Tensor> residual, Tensor scale, Tensor shift, bool relu) {
  int64_t M;
  int C;
  bn_rows(x, &M, &C);
  c10::hip::HIPGuard guard(x.device().index());
  const void* r = opt_rows(residual, x, "residual");
  const float* sc = opt_f32(scale, C, "scale");
  const float* sf = opt_f32(shift, C, "shift");
  Tensor y = at::empty_like(x);
  hip_check(bn_apply(x.data_ptr(), r, y.data_ptr(), dt_of(x), sc, sf, M, C, relu ? 1 : 0, cur_stream(x)), "bn_apply");
  return y;
}

// ------------------------------------------------------------- max pooling (NHWC)
PoolArgs pool_args(const Tensor& x, int64_t Ho, int64_t Wo, std::vector<int64_t> k, std::vector<int64_t> st,
                   std::vector<int64_t> pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "maxpool: x must be a channels_last-contiguous 4D GPU tensor");
  TORCH_CHECK(k.size() == 2 && st.size() == 2 && pad.size() == 2, "maxpool: 2D kernel/stride/padding");
  PoolArgs a{};
  a.N = (int)x.size(0); a.C = (int)x.size(1); a.H = (int)x.size(2); a.W = (int)x.size(3);
  a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.kh = (int)k[0]; a.kw = (int)k[1]; a.sh = (int)st[0]; a.sw = (int)st[1]; a.ph = (int)pad[0]; a.pw = (int)pad[1];
  TORCH_CHECK(a.kh >= 1 && a.kw >= 1 && a.kh * a.kw <= 256 && a.sh >= 1 && a.sw >= 1 && a.ph >= 0 && a.pw >= 0 &&
                  2 * a.ph <= a.kh && 2 * a.pw <= a.kw,
              "maxpool: unsupported window");
  TORCH_CHECK((int64_t)(a.H + 2 * a.ph - a.kh) / a.sh + 1 == Ho && (int64_t)(a.W + 2 * a.pw - a.kw) / a.sw + 1 == Wo,
              "maxpool: output size mismatch");
  const int V = x.scalar_type() == at::kFloat ? 4 : 8;
  TORCH_CHECK(a.C % V == 0, "maxpool: channels must be a multiple of ", V);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "maxpool: 16-byte aligned data expected");
  return a;
}

// scale/shift (f32 [C], optional): y = maxpool(ReLU?(x * scale + shift)) -- a training BatchNorm's
// apply pass folded into the pool (ops/norm.bn_relu_maxpool)
std::vector<Tensor> maxpool2d_fwd(Tensor x, std::vector<int64_t> k, std::vector<int64_t> st, std::vector<int64_t> pad,
                                  c10::optional<Tensor> scale, c10::optional<Tensor> shift, bool relu) {
  const int64_t Ho = (x.size(2) + 2 * pad[0] - k[0]) / st[0] + 1, Wo = (x.size(3) + 2 * pad[1] - k[1]) / st[1] + 1;
  PoolArgs a = pool_args(x, Ho, Wo, k, st, pad);
  if (has(scale)) {
    TORCH_CHECK(has(shift), "maxpool: scale and shift together");
    a.scale = opt_f32(scale, x.size(1), "scale");
    a.shift = opt_f32(shift, x.size(1), "shift");
    a.relu = relu ? 1 : 0;
  }
  c10::hip::HIPGuard guard(x.device().index());
  auto opts = x.options().memory_format(at::MemoryFormat::ChannelsLast);
  Tensor y = at::empty({x.size(0), x.size(1), Ho, Wo}, opts);
  Tensor arg = at::empty({x.size(0), x.size(1), Ho, Wo}, opts.dtype(at::kByte));
  hip_check(maxpool2d_nhwc_forward(x.data_ptr(), y.data_ptr(), arg.data_ptr<uint8_t>(), dt_of(x), a, cur_stream(x)),
            "maxpool2d_nhwc_forward");
  return {y, arg};
}

Tensor maxpool2d_bwd(Tensor gy, Tensor arg, std::vector<int64_t> in_size, std::vector<int64_t> k,
                     std::vector<int64_t> st, std::vector<int64_t> pad) {
  TORCH_CHECK(in_size.size() == 4, "maxpool: input size [N, C, H, W]");
  TORCH_CHECK(gy.is_cuda() && gy.dim() == 4 && gy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  arg.sizes() == gy.sizes() && arg.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  arg.device() == gy.device() && arg.scalar_type() == at::kByte,
              "maxpool backward: gy / argmax must be matching channels_last tensors");
  Tensor gx = at::empty(in_size, gy.options().memory_format(at::MemoryFormat::ChannelsLast));
  PoolArgs a = pool_args(gx, gy.size(2), gy.size(3), k, st, pad);
  c10::hip::HIPGuard guard(gy.device().index());
  hip_check(maxpool2d_nhwc_backward(gy.data_ptr(), arg.data_ptr<uint8_t>(), gx.data_ptr(), dt_of(gy), a,
                                    cur_stream(gy)),
            "maxpool2d_nhwc_backward");
  return gx;
}

}  // namespace

void bind_norm(py::module_& m) {
  m.def("bn_bwd_reduce", &bn_bwd_reduce, "BN backward reduce pass only: (g, dweight, dbias, coef[3, C])");
  m.def("conv1x1_bwd", &conv1x1_bwd_, "fused BN-apply + 1x1 conv data and weight gradients (bf16)");
  m.def("conv1x1_bwd_supported", &conv1x1_bwd_supported_);
  m.def("bn_relu", &bn_relu);
  m.def("bn_max_channels", &bn_max_channels, "widest channel count the NHWC BatchNorm kernels take");
  m.def("bn_geometry", [](int64_t M, int64_t C, bool f32) {
    int g[4];
    bn_geometry(M, (int)C, f32 ? kF32 : kBF16, g);
    return py::make_tuple(g[0], g[1], g[2], g[3], bn_workspace_floats(M, (int)C, f32 ? kF32 : kBF16),
                          bn_num_tickets((int)C, f32 ? kF32 : kBF16));
  }, "reduction launch geometry of an [M, C] tensor: (TC, RPI, gx, gy, workspace floats, tickets)", py::arg("M"),
        py::arg("C"), py::arg("f32"));
  m.def("bn_fwd_train", &bn_fwd_train, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("num_batches_tracked"), py::arg("residual"), py::arg("relu"),
        py::arg("momentum"), py::arg("eps"), py::arg("tickets") = py::none(), py::arg("want_mask") = false,
        py::arg("stats_only") = false);
  m.def("bn_bwd", &bn_bwd, py::arg("dy"), py::arg("x"), py::arg("y"), py::arg("weight"), py::arg("stats"),
        py::arg("relu"), py::arg("want_dres"), py::arg("want_dweight"), py::arg("tickets") = py::none(),
        py::arg("dweight_out") = py::none(), py::arg("dbias_out") = py::none(), py::arg("dy2") = py::none(),
        py::arg("mask") = py::none());
  m.def("maxpool2d_fwd", &maxpool2d_fwd, py::arg("x"), py::arg("k"), py::arg("s"), py::arg("p"),
        py::arg("scale") = py::none(), py::arg("shift") = py::none(), py::arg("relu") = false);
  m.def("maxpool2d_bwd", &maxpool2d_bwd);
  m.def("bn_fwd_apply", &bn_fwd_apply, py::arg("x"), py::arg("stats"), py::arg("residual"), py::arg("relu"),
        py::arg("want_mask"));
  m.def("bn_sync_stats", &bn_sync_stats_, "this rank's BN record (mean[C], M2[C], rows) into rec[2C+1] float64",
        py::arg("x"), py::arg("rec"), py::arg("tickets") = py::none());
  m.def("bn_sync_merge", &bn_sync_merge_, "gathered records [W, 2C+1] -> (stats[4, C], global row count[1])",
        py::arg("rec"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"), py::arg("running_var"),
        py::arg("num_batches_tracked"), py::arg("momentum"), py::arg("eps"));
  m.def("bn_sync_bwd_reduce", &bn_sync_bwd_reduce, "BN backward reduce, raw: (g, dweight, dbias, sums[2, C] float64)",
        py::arg("dy"), py::arg("x"), py::arg("weight"), py::arg("stats"), py::arg("relu"), py::arg("want_dweight"),
        py::arg("tickets") = py::none(), py::arg("dweight_out") = py::none(), py::arg("dbias_out") = py::none(),
        py::arg("dy2") = py::none(), py::arg("mask") = py::none());
  m.def("bn_sync_coef", &bn_sync_coef_, "coef[3, C] from the all-reduced sums and the global row count",
        py::arg("sums"), py::arg("count"), py::arg("weight"), py::arg("stats"));
  m.def("bn_bwd_apply_g", &bn_bwd_apply_g, "dx = coef[0] g + coef[1] x + coef[2]", py::arg("g"), py::arg("x"),
        py::arg("coef"));
  m.def("conv1x1_bn_stats", &conv1x1_bn_stats, py::arg("x"), py::arg("w"), py::arg("weight"), py::arg("bias"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("num_batches_tracked"), py::arg("momentum"),
        py::arg("eps"), py::arg("tickets"), py::arg("tile") = 256);
  m.def("conv1x1_bn_num_tickets", &conv1x1_bn_num_tickets, py::arg("M"), py::arg("N"), py::arg("tile") = 256,
        py::arg("K") = 0);
  m.def("conv1x1_bn_stream_supported", &conv1x1_bn_stream_supported, py::arg("K"), py::arg("N"));
  m.def("bn_apply", &bn_apply_, py::arg("x"), py::arg("residual"), py::arg("scale"), py::arg("shift"),
        py::arg("relu"));
}

}  // namespace ptdt
