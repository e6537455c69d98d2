// Bindings of the fused small-MLP step and the persistent engines (plan, launch, engine queries),
// with the runtime helpers around them: timeline probes, device / stream set-up, hipGraph inspection.
#include "common.h"

#include "comm/xgmi_comm.h"
#include "kernels/wave_loop_schedule.h"
#include "kernels/wave_row_image.h"

namespace ptdt {
namespace {

// ------------------------------------------------------------- fused step
void fused_mlp_step_py(Tensor X, c10::optional<Tensor> Yf, c10::optional<Tensor> Yi,
                    c10::optional<Tensor> idx, Tensor P, Tensor G, c10::optional<Tensor> mom,
                    c10::optional<Tensor> opt_step, Tensor loss_out, int64_t B, int64_t Din, int64_t H,
                    int64_t Dout, int64_t loss_kind, int64_t ignore_index, bool has_bias,
                    double grad_scale, bool accumulate, int64_t update_mode, double lr, double momentum,
                    double dampening, double weight_decay, bool nesterov, std::shared_ptr<XgmiComm> ar) {
  check_gpu(X, "X");
  check_gpu(P, "P");
  check_gpu(G, "G");
  TORCH_CHECK(X.scalar_type() == at::kFloat && P.scalar_type() == at::kFloat && G.scalar_type() == at::kFloat,
              "fused_mlp_step: fp32 dataset/params/grads");
  TORCH_CHECK(X.dim() == 2 && X.size(1) == Din, "fused_mlp_step: X must be [N, Din]");
  FusedMlpArgs a{};
  a.B = (int)B; a.Din = (int)Din; a.H = (int)H; a.Dout = (int)Dout;
  a.has_bias = has_bias ? 1 : 0;
  const int64_t np = fused_mlp_num_params(a);
  TORCH_CHECK(P.numel() == np && G.numel() == np, "fused_mlp_step: flat param/grad size mismatch (want ",
              np, ")");
  TORCH_CHECK(loss_out.is_cuda() && loss_out.scalar_type() == at::kFloat && loss_out.numel() >= 1);
  const int64_t N = X.size(0);
  if (has(idx)) {
    check_gpu(*idx, "idx");
    TORCH_CHECK(idx->scalar_type() == at::kInt && idx->numel() >= B, "idx must be int32 with >= B entries");
  } else {
    TORCH_CHECK(B <= N, "fused_mlp_step: B > N without indices");
  }
  if (loss_kind == kLossCEIndex) {
    TORCH_CHECK(has(Yi) && Yi->scalar_type() == at::kLong && Yi->numel() == N, "CE-index needs int64 labels [N]");
    check_gpu(*Yi, "Yi");
  } else {
    TORCH_CHECK(has(Yf) && Yf->scalar_type() == at::kFloat && Yf->numel() == N * Dout,
                "soft-CE/MSE need float targets [N, Dout]");
    check_gpu(*Yf, "Yf");
  }
  if (has(mom)) TORCH_CHECK(mom->numel() == np && mom->is_cuda());
  TORCH_CHECK(fused_mlp_lds_bytes((int)B, (int)Din, (int)H, (int)Dout) <= 160 * 1024,
              "fused_mlp_step: model/batch too large for one workgroup's LDS; use the layered path");
  c10::hip::HIPGuard guard(X.device().index());
  a.X = X.data_ptr<float>();
  a.Yf = ptr_or_null<const float>(Yf);
  a.Yi = ptr_or_null<const int64_t>(Yi);
  a.idx = ptr_or_null<const int32_t>(idx);
  a.P = P.data_ptr<float>();
  a.G = G.data_ptr<float>();
  a.mom = ptr_or_null<float>(mom);
  a.opt_step = ptr_or_null<int32_t>(opt_step);
  a.loss_out = loss_out.data_ptr<float>();
  a.loss_kind = (int)loss_kind;
  a.ignore_index = (int)ignore_index;
  a.grad_scale = (float)grad_scale;
  a.accumulate = accumulate ? 1 : 0;
  a.update_mode = (int)update_mode;
  a.lr = (float)lr;
  a.momentum = (float)momentum;
  a.dampening = (float)dampening;
  a.weight_decay = (float)weight_decay;
  a.nesterov = nesterov ? 1 : 0;
  if (ar) {
    TORCH_CHECK(ar->ready(), "fused_mlp_step: xGMI communicator not opened");
    TORCH_CHECK(np <= ar->max_elems(), "fused_mlp_step: bucket larger than the xGMI buffer");
    TORCH_CHECK(update_mode != 1 && !accumulate, "fused_mlp_step: in-kernel all-reduce needs update_mode 0/2");
    a.ar = ar->args();
  }
  hip_check(ptdt::fused_mlp_step(a, cur_stream(X)), "fused_mlp_step");
}

// Query-format name of a selected engine: "wave:L<lanes per row>R<rows per lane group>K<features
// per lane>", "tp:<n>waves", "tp_bf16:<n>waves", "workgroup:mfma" or "workgroup".
std::string engine_name(const PersistChoice& c) {
  switch (c.engine) {
    case kEngWave: return "wave:L" + std::to_string(c.L) + "R" + std::to_string(c.R) + "K" + std::to_string(c.kp);
    case kEngTp: return "tp:" + std::to_string(c.waves) + "waves";
    case kEngTpBf16: return "tp_bf16:" + std::to_string(c.waves) + "waves";
    case kEngWorkgroupMfma: return "workgroup:mfma";
    case kEngWorkgroup: return "workgroup";
    // the query has always named a workgroup engine for configurations the plan refuses
    default: return c.refused == kEngWorkgroupMfma ? "workgroup:mfma" : "workgroup";
  }
}

// A persistent engine launch planned once: arguments validated, engine and
// kernel chosen, LDS attribute set, tensors kept alive. launch(n) is a bare
// hipLaunchKernel on the caller's current stream -- the short-run fixed cost
// (bench --steps 20, one launch per Trainer.train) is the kernel, not the host.
class PersistentPlan {
 public:
  // Throws on any shape/dtype/sharding mismatch: a bad launch of a resident kernel can reset the node.
  PersistentPlan(Tensor X, c10::optional<Tensor> Yf, c10::optional<Tensor> Yi, Tensor P, Tensor G,
                 c10::optional<Tensor> mom, c10::optional<Tensor> opt_step, int64_t B, int64_t Din, int64_t H,
                 int64_t Dout, int64_t loss_kind, int64_t ignore_index, bool has_bias, double lr, double momentum,
                 double dampening, double weight_decay, bool nesterov, std::shared_ptr<XgmiComm> ar, int64_t W,
                 int64_t rank, int64_t num_samples, bool shuffle, int64_t seed, Tensor cursor, Tensor losses,
                 c10::optional<Tensor> stamps, int64_t variant, bool x_zero_padded, c10::optional<Tensor> idx,
                 c10::optional<Tensor> lcache, int64_t idx_e0, c10::optional<Tensor> row_image, int64_t row_image_kp)
      : keep_{X, P, G, cursor, losses}, ar_(ar), capacity_(losses.numel()), dev_(X.device().index()) {
    for (const auto* t : {&Yf, &Yi, &mom, &opt_step, &stamps, &idx, &lcache, &row_image})
      if (has(*t)) keep_.push_back(**t);
    steps_per_epoch_ = (num_samples + B - 1) / B;
    TORCH_CHECK(X.is_cuda(), "X must be a GPU tensor");  // rows may be padded: checked below
    check_gpu(P, "P");
    check_gpu(G, "G");
    TORCH_CHECK(X.scalar_type() == at::kFloat && P.scalar_type() == at::kFloat && G.scalar_type() == at::kFloat);
    TORCH_CHECK(X.dim() == 2 && X.size(1) == Din && X.stride(1) == 1 && X.stride(0) >= Din,
                "persistent: X must be [N, Din] with unit column stride (rows may be padded)");
    const int64_t N = X.size(0);
    FusedMlpArgs& a = L_.a;
    a.B = (int)B; a.Din = (int)Din; a.H = (int)H; a.Dout = (int)Dout;
    a.has_bias = has_bias ? 1 : 0;
    const int64_t np = fused_mlp_num_params(a);
    TORCH_CHECK(P.numel() == np && G.numel() == np, "persistent: flat param/grad size mismatch");
    TORCH_CHECK(cursor.is_cuda() && cursor.scalar_type() == at::kInt && cursor.numel() == 2, "cursor: int32[2] GPU");
    TORCH_CHECK(losses.is_cuda() && losses.scalar_type() == at::kFloat && losses.numel() >= 1, "losses: f32[n]");
    TORCH_CHECK(num_samples > 0 && num_samples * W >= N && W > 0 && rank >= 0 && rank < W, "persistent: bad sampler");
    if (loss_kind == kLossCEIndex) {
      TORCH_CHECK(has(Yi) && Yi->scalar_type() == at::kLong && Yi->numel() == N);
    } else {
      TORCH_CHECK(has(Yf) && Yf->scalar_type() == at::kFloat && Yf->numel() == N * Dout);
    }
    if (has(mom)) TORCH_CHECK(mom->numel() == np && mom->is_cuda());
    TORCH_CHECK((ar ? ar->world() : 1) == W, "persistent: all-reduce world != sampler world");
    a.X = X.data_ptr<float>();
    a.Yf = ptr_or_null<const float>(Yf);
    a.Yi = ptr_or_null<const int64_t>(Yi);
    a.P = P.data_ptr<float>();
    a.G = G.data_ptr<float>();
    a.mom = ptr_or_null<float>(mom);
    a.opt_step = ptr_or_null<int32_t>(opt_step);
    a.ldx = (int)X.stride(0);
    a.x_padded = x_zero_padded ? 1 : 0;
    a.loss_kind = (int)loss_kind;
    a.ignore_index = (int)ignore_index;
    a.grad_scale = 1.f;
    a.update_mode = 2;
    a.lr = (float)lr; a.momentum = (float)momentum; a.dampening = (float)dampening;
    a.weight_decay = (float)weight_decay; a.nesterov = nesterov ? 1 : 0;
    if (ar && ar->world() > 1) {
      TORCH_CHECK(ar->ready(), "persistent: xGMI communicator not opened");
      TORCH_CHECK(np <= ar->max_elems(), "persistent: bucket larger than the xGMI buffer");
      TORCH_CHECK(ar->rank() == rank, "persistent: rank mismatch");
      a.ar = ar->args();
    } else {
      a.ar.world = 1;
    }
    PersistArgs& pa = L_.p;
    pa.n_steps = 1;
    pa.N = (int)N;
    pa.W = (int)W;
    pa.rank = (int)rank;
    pa.num_samples = (int)num_samples;
    pa.shuffle = shuffle ? 1 : 0;
    pa.seed = (uint64_t)seed;
    pa.cursor = cursor.data_ptr<int32_t>();
    pa.losses = losses.data_ptr<float>();
    if (has(stamps)) {
      TORCH_CHECK(stamps->is_cuda() && stamps->scalar_type() == at::kLong && stamps->numel() >= 9, "stamps: int64[9]");
      pa.stamps = stamps->data_ptr<int64_t>();
      pa.stamps_n = (int)stamps->numel();
    }
    pa.variant = (int)variant;
    pa.cursor_host_pos = -1;
    if (has(idx)) {
      // [num_samples] (one epoch: positions are steps in it) or [E, num_samples]
      // (epochs idx_e0..idx_e0+E-1: positions are absolute, epoch * S + step)
      TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kInt && idx->is_contiguous() &&
                      idx->size(-1) == num_samples && idx->dim() <= 2 && idx->device() == X.device(),
                  "persistent: idx must be a contiguous int32 GPU tensor [E,] num_samples on X's device");
      pa.idx = idx->data_ptr<int32_t>();
      pa.idx_epochs = idx->dim() == 2 ? (int)idx->size(0) : 1;
      pa.idx_e0 = idx->dim() == 2 ? (int)idx_e0 : 0;
      pa.cursor_host_pos = (int64_t)pa.idx_e0 * steps_per_epoch_;
      TORCH_CHECK(persist_span_ok(L_, pa.cursor_host_pos, 1),
                  "persistent: with explicit index lists a launch must stay inside the provided epochs");
    }
    if (has(lcache)) {  // [2][al4(num_samples)] lists + [2] epoch tags
      const int64_t stride = (num_samples + 3) & ~int64_t(3);
      TORCH_CHECK(lcache->is_cuda() && lcache->scalar_type() == at::kInt && lcache->is_contiguous() &&
                      lcache->numel() == 2 * stride + 2 && lcache->device() == X.device(),
                  "persistent: list cache must be int32[2 * al4(num_samples) + 2] on X's device");
      pa.lcache = lcache->data_ptr<int32_t>();
      pa.ltag = pa.lcache + 2 * stride;
    }
    if (has(row_image)) {  // the dataset packed for the wave engine's lean kernels (wave_row_image.h)
      TORCH_CHECK(row_image->is_cuda() && row_image->scalar_type() == at::kFloat && row_image->is_contiguous() &&
                      row_image->device() == X.device() && row_image_kp > 0 && row_image_kp <= 64 &&
                      row_image->numel() == N * wave_image_row_floats((int)row_image_kp),
                  "persistent: row_image must be a contiguous f32 GPU tensor of N x 4 RS(row_image_kp) floats on X's device");
      L_.image = row_image->data_ptr<float>();
      L_.image_kp = (int)row_image_kp;
      L_.image_rows = N;
    }
    c10::hip::HIPGuard guard(dev_);
    const hipError_t e = fused_mlp_persistent_prepare(&L_);
    const PersistChoice& c = L_.choice;
    TORCH_CHECK(c.engine != kEngNone || c.refused != kEngNone,
                "persistent: the requested engine variant does not support this configuration");
    TORCH_CHECK(c.engine != kEngNone, "persistent: model + epoch index list do not fit one workgroup's LDS");
    hip_check(e, "persistent plan");
    engine_ = engine_name(c);
  }
  // n steps from the device cursor; with explicit index lists, cursor_pos is
  // the host's view of the cursor (epoch * steps_per_epoch + step; one-epoch
  // list: the step in it) and the launch must stay inside the provided epochs
  void launch(int64_t n, int64_t cursor_pos) { launch_impl(n, cursor_pos, -1, 0); }
  void launch_impl(int64_t n, int64_t cursor_pos, int start_e, int start_j) {
    TORCH_CHECK(n >= 0 && n <= capacity_, "persistent plan: n_steps exceeds the losses buffer");
    TORCH_CHECK(persist_span_ok(L_, cursor_pos, (int)n),
                "persistent plan: with explicit index lists a launch must stay inside the provided epochs");
    c10::hip::HIPGuard guard(dev_);
    hip_check(persistent_launch(L_, (int)n, L_.p.idx ? cursor_pos : -1, c10::hip::getCurrentHIPStream(dev_).stream(),
                                start_e, start_j),
              "persistent launch");
  }
  // n steps from absolute position pos = epoch * steps_per_epoch + step, which the
  // caller asserts the device cursor holds (its own step count, e.g. the bench's
  // warm-up): the engines skip the dependent cursor load at kernel entry
  void launch_at(int64_t n, int64_t pos) {
    TORCH_CHECK(pos >= 0, "persistent plan: launch_at needs a position >= 0");
    const int64_t S = steps_per_epoch_;
    TORCH_CHECK(pos / S < (int64_t)1 << 30, "persistent plan: position out of range");
    launch_impl(n, pos, (int)(pos / S), (int)(pos % S));
  }
  int64_t capacity() const { return capacity_; }
  // query-format name (persistent_engine) of the engine this plan prepared
  const std::string& engine() const { return engine_; }
  // which instantiation of the engine's kernel the plan launches (wave engine, layout F: "generic",
  // "lean-plain", "lean-mom"; see linear_wave_variant); "" for the other engines
  std::string kernel_variant() const {
    return L_.choice.engine == kEngWave ? wave_variant_name(L_.kernel_variant) : "";
  }
  // bytes of the row image the plan's kernel gathers from; 0 when it reads X and Y (no image offered,
  // or a kernel that does not take one)
  int64_t image_bytes() const { return L_.uses_image ? wave_image_bytes(L_.image_rows, L_.image_kp) : 0; }
  ~PersistentPlan() {
    if (ev_) hipEventDestroy(ev_);
  }
  // launch timeline probe (tools/driver_timeline.py): the engine stamps its realtime counter
  // into tl[0..3] (a device or host-mapped int64 address; 0 turns it off)
  void set_timeline(int64_t addr) { L_.p.tl = reinterpret_cast<int64_t*>(addr); }
  // CLOCK_MONOTONIC ns right before / after the last hipLaunchKernel of this plan
  std::vector<int64_t> last_launch_ns() const { return {L_.host_ns[0], L_.host_ns[1]}; }
  // Timeline probe: launch n steps at pos and wait for them with one of the runtime's completion
  // paths, all in C++ (mode 0 hipDeviceSynchronize, 1 hipStreamSynchronize, 2 hipEventRecord +
  // hipEventSynchronize, 3 hipExtLaunchKernel with a stop event + hipEventSynchronize, 4 spin on
  // hipStreamQuery, 5 hipExtLaunchKernel with a stop event + spin on hipEventQuery). Returns
  // CLOCK_MONOTONIC ns [before the launch call, after it, when the wait returned].
  std::vector<int64_t> launch_wait_at(int64_t n, int64_t pos, int64_t mode) {
    TORCH_CHECK(n > 0 && n <= capacity_ && pos >= 0, "launch_wait_at: bad n / pos");
    TORCH_CHECK(mode >= 0 && mode <= 5, "launch_wait_at: mode 0..5");
    const int64_t S = steps_per_epoch_;
    c10::hip::HIPGuard guard(dev_);
    hipStream_t st = c10::hip::getCurrentHIPStream(dev_).stream();
    if (ev_ == nullptr) hip_check(hipEventCreate(&ev_), "hipEventCreate");
    const int64_t t0 = mono_ns();
    if (mode == 3 || mode == 5) {
      persist_set_position(L_, (int)n, -1, (int)(pos / S), (int)(pos % S));
      void* args[] = {&L_.a, &L_.p};
      hip_check(hipExtLaunchKernel(L_.fn, dim3(1), dim3(L_.threads), args, L_.lds, st, nullptr, ev_, 0),
                "hipExtLaunchKernel");
    } else {
      launch_impl(n, pos, (int)(pos / S), (int)(pos % S));
      if (mode == 2) hip_check(hipEventRecord(ev_, st), "hipEventRecord");
    }
    const int64_t t1 = mono_ns();
    switch (mode) {
      case 0: hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize"); break;
      case 1: hip_check(hipStreamSynchronize(st), "hipStreamSynchronize"); break;
      case 2:
      case 3: hip_check(hipEventSynchronize(ev_), "hipEventSynchronize"); break;
      case 4: {
        hipError_t e;
        while ((e = hipStreamQuery(st)) == hipErrorNotReady) {
        }
        hip_check(e, "hipStreamQuery");
        break;
      }
      default: {
        hipError_t e;
        while ((e = hipEventQuery(ev_)) == hipErrorNotReady) {
        }
        hip_check(e, "hipEventQuery");
      }
    }
    return {t0, t1, mono_ns()};
  }

 private:
  std::vector<Tensor> keep_;
  std::shared_ptr<XgmiComm> ar_;
  int64_t capacity_;
  int dev_;
  int64_t steps_per_epoch_ = 0;
  PersistLaunch L_;
  std::string engine_;
  hipEvent_t ev_ = nullptr;  // timeline probe (launch_wait_at)
};

// Host-mapped, coherent int64 words a kernel can store into and the host can poll
// (launch timelines: tools/driver_timeline.py).
class HostMapped {
 public:
  explicit HostMapped(int64_t n) : n_(n) {
    TORCH_CHECK(n > 0 && n <= (1 << 20), "HostMapped: 1..2^20 words");
    hip_check(hipHostMalloc((void**)&h_, n * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent),
              "hipHostMalloc(HostMapped)");
    hip_check(hipHostGetDevicePointer((void**)&d_, h_, 0), "hipHostGetDevicePointer(HostMapped)");
    zero();
  }
  ~HostMapped() {
    if (h_) hipHostFree(h_);
  }
  HostMapped(const HostMapped&) = delete;
  HostMapped& operator=(const HostMapped&) = delete;
  void zero() {
    volatile int64_t* v = h_;
    for (int64_t k = 0; k < n_; ++k) v[k] = 0;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
  }
  std::vector<int64_t> read() const {
    volatile int64_t* v = h_;
    std::vector<int64_t> out(n_);
    for (int64_t k = 0; k < n_; ++k) out[k] = v[k];
    return out;
  }
  // spin until word k is non-zero; CLOCK_MONOTONIC ns when it was seen, -1 after timeout_ns
  int64_t spin(int64_t k, int64_t timeout_ns) const {
    TORCH_CHECK(k >= 0 && k < n_);
    volatile int64_t* v = h_ + k;
    const int64_t t0 = mono_ns();
    for (;;) {
      if (*v != 0) return mono_ns();
      const int64_t t = mono_ns();
      if (t - t0 > timeout_ns) return -1;
    }
  }
  int64_t device_ptr() const { return reinterpret_cast<int64_t>(d_); }

 private:
  int64_t n_;
  int64_t* h_ = nullptr;
  int64_t* d_ = nullptr;
};

std::vector<std::vector<int64_t>> clock_calibrate_py(int64_t n) {
  std::vector<int64_t> a(n), b(n), c(n);
  hip_check(clock_calibrate((int)n, a.data(), b.data(), c.data()), "clock_calibrate");
  return {a, b, c};
}

// Fills a / pa (zero-initialised by the caller) for an engine query and returns the engine selected.
// A query comes before there is a dataset tensor: any row stride (the caller zero-pads X rows to the
// layout's x_width when needed) and num_samples rows.
PersistChoice persist_query(FusedMlpArgs& a, PersistArgs& pa, int64_t B, int64_t Din, int64_t H, int64_t Dout,
                            int64_t loss_kind, int64_t num_samples, int64_t world, int64_t variant, bool has_bias,
                            double momentum = 0.0, double weight_decay = 0.0) {
  a.B = (int)B; a.Din = (int)Din; a.H = (int)H; a.Dout = (int)Dout; a.loss_kind = (int)loss_kind;
  a.has_bias = has_bias ? 1 : 0;
  a.ar.world = (int)world;
  a.ldx = kWaveLdxAny;
  a.x_padded = 1;
  a.momentum = (float)momentum;
  a.weight_decay = (float)weight_decay;
  pa.num_samples = (int)num_samples;
  pa.variant = (int)variant;
  pa.N = (int)std::max<int64_t>(num_samples, 1);
  return persistent_select(a, pa);
}

// Which persistent engine a plan would run for this configuration.
PersistChoice persistent_choice(int64_t B, int64_t Din, int64_t H, int64_t Dout, int64_t loss_kind, int64_t num_samples,
                                int64_t world, int64_t variant, bool has_bias) {
  FusedMlpArgs a{};
  PersistArgs pa{};
  return persist_query(a, pa, B, Din, H, Dout, loss_kind, num_samples, world, variant, has_bias);
}

// The kernel variant (PersistentPlan.kernel_variant) a plan of this configuration would launch, under the
// same assumptions as persistent_choice; momentum != 0 stands for "a momentum buffer exists".
std::string persistent_kernel_variant(int64_t B, int64_t Din, int64_t H, int64_t Dout, int64_t loss_kind,
                                      int64_t num_samples, int64_t world, int64_t variant, bool has_bias,
                                      double momentum, double weight_decay, bool stamps) {
  FusedMlpArgs a{};
  PersistArgs pa{};
  const PersistChoice c = persist_query(a, pa, B, Din, H, Dout, loss_kind, num_samples, world, variant, has_bias,
                                        momentum, weight_decay);
  if (c.engine != kEngWave) return "";
  return wave_variant_name(linear_wave_variant(a, pa, c, momentum != 0.0, stamps));
}

// ------------------------------------------------------------- hipGraph inspection (graph_memset.hip)
std::vector<int64_t> graph_node_census_(int64_t graph) {
  std::vector<int> c(16, 0);
  const int n = graph_node_census(reinterpret_cast<void*>(graph), c.data(), (int)c.size());
  TORCH_CHECK(n >= 0, "graph_node_census: hipGraph query failed");
  std::vector<int64_t> out(c.begin(), c.end());
  out.insert(out.begin(), n);
  return out;  // [total, count of hipGraphNodeType 0, 1, ...]
}

// hipMemsetAsync of a whole tensor (byte value) on the current stream: a capturable memset for the
// graph-editing tests (tests/test_graphs_gpu.py); the framework's own paths issue none
void memset_async_(Tensor t, int64_t value) {
  check_gpu(t, "t");
  TORCH_CHECK(t.is_contiguous(), "memset_async_: contiguous tensor");
  c10::hip::HIPGuard guard(t.device().index());
  hip_check(hipMemsetAsync(t.data_ptr(), (int)value, t.numel() * t.element_size(), cur_stream(t)), "memset_async_");
}

std::vector<std::vector<int64_t>> graph_memset_params_(int64_t graph) {
  std::vector<std::vector<int64_t>> out;
  TORCH_CHECK(graph_memset_params(reinterpret_cast<void*>(graph), &out) >= 0, "graph_memset_params: query failed");
  return out;
}

// a standalone graph with one memset node over t's storage (the runtime's memset-node path alone)
void graph_memset_run_(Tensor t, int64_t value, int64_t esize, int64_t width, int64_t height, int64_t pitch,
                       int64_t reps) {
  check_gpu(t, "t");
  const int64_t rows = height > 0 ? height : 1;
  const int64_t span = (rows - 1) * (pitch > 0 ? pitch : width * esize) + width * esize;
  TORCH_CHECK(esize == 1 || esize == 2 || esize == 4, "graph_memset_run: element size 1, 2 or 4");
  TORCH_CHECK(span <= t.numel() * t.element_size(), "graph_memset_run: the memset exceeds the tensor");
  c10::hip::HIPGuard guard(t.device().index());
  hip_check(graph_memset_run(t.data_ptr(), (uint32_t)value, (int)esize, (size_t)width, (size_t)height,
                             (size_t)pitch, (int)reps, cur_stream(t)),
            "graph_memset_run");
}

int64_t graph_replace_memsets_(int64_t graph) {
  const int r = graph_replace_memsets(reinterpret_cast<void*>(graph));
  TORCH_CHECK(r >= 0, "graph_replace_memsets: hipGraph edit failed");
  return r;
}

}  // namespace

void bind_engine(py::module_& m) {
  m.def("fused_mlp_step", &fused_mlp_step_py, py::arg("X"), py::arg("Yf"), py::arg("Yi"), py::arg("idx"),
        py::arg("P"), py::arg("G"), py::arg("mom"), py::arg("opt_step"), py::arg("loss_out"), py::arg("B"),
        py::arg("Din"), py::arg("H"), py::arg("Dout"), py::arg("loss_kind"), py::arg("ignore_index"),
        py::arg("has_bias"), py::arg("grad_scale"), py::arg("accumulate"), py::arg("update_mode"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"), py::arg("nesterov"),
        py::arg("ar") = nullptr);
  py::class_<PersistentPlan, std::shared_ptr<PersistentPlan>>(m, "PersistentPlan")
      .def(py::init<Tensor, c10::optional<Tensor>, c10::optional<Tensor>, Tensor, Tensor, c10::optional<Tensor>,
                    c10::optional<Tensor>, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, bool, double, double,
                    double, double, bool, std::shared_ptr<XgmiComm>, int64_t, int64_t, int64_t, bool, int64_t, Tensor,
                    Tensor, c10::optional<Tensor>, int64_t, bool, c10::optional<Tensor>, c10::optional<Tensor>,
                    int64_t, c10::optional<Tensor>, int64_t>(),
           py::arg("X"), py::arg("Yf"), py::arg("Yi"), py::arg("P"), py::arg("G"), py::arg("mom"),
           py::arg("opt_step"), py::arg("B"), py::arg("Din"), py::arg("H"), py::arg("Dout"), py::arg("loss_kind"),
           py::arg("ignore_index"), py::arg("has_bias"), py::arg("lr"), py::arg("momentum"), py::arg("dampening"),
           py::arg("weight_decay"), py::arg("nesterov"), py::arg("ar"), py::arg("W"), py::arg("rank"),
           py::arg("num_samples"), py::arg("shuffle"), py::arg("seed"), py::arg("cursor"), py::arg("losses"),
           py::arg("stamps") = py::none(), py::arg("variant") = 0, py::arg("x_zero_padded") = false,
           py::arg("idx") = py::none(), py::arg("lcache") = py::none(), py::arg("idx_e0") = 0,
           py::arg("row_image") = py::none(), py::arg("row_image_kp") = 0)
      .def("launch", &PersistentPlan::launch, py::arg("n_steps"), py::arg("cursor_pos") = -1)
      .def("launch_at", &PersistentPlan::launch_at, py::arg("n_steps"), py::arg("pos"))
      .def_property_readonly("capacity", &PersistentPlan::capacity)
      .def_property_readonly("engine", &PersistentPlan::engine)
      .def_property_readonly("kernel_variant", &PersistentPlan::kernel_variant)
      .def_property_readonly("image_bytes", &PersistentPlan::image_bytes)
      .def("set_timeline", &PersistentPlan::set_timeline, py::arg("addr"))
      .def("last_launch_ns", &PersistentPlan::last_launch_ns)
      .def("launch_wait_at", &PersistentPlan::launch_wait_at, py::arg("n_steps"), py::arg("pos"), py::arg("mode"),
           py::call_guard<py::gil_scoped_release>());
  py::class_<HostMapped, std::shared_ptr<HostMapped>>(m, "HostMapped")
      .def(py::init<int64_t>(), py::arg("n"))
      .def("zero", &HostMapped::zero)
      .def("read", &HostMapped::read)
      .def("spin", &HostMapped::spin, py::arg("k"), py::arg("timeout_ns"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("device_ptr", &HostMapped::device_ptr);
  m.def("clock_calibrate", &clock_calibrate_py, py::arg("n"), py::call_guard<py::gil_scoped_release>());
  m.def("mono_ns", &mono_ns);
  // raw synchronisation primitives with a CLOCK_MONOTONIC return stamp (timeline probes)
  m.def("hip_device_sync_ns", []() {
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return mono_ns();
  });
  m.def("hip_stream_sync_ns", [](int64_t dev) {
    hip_check(hipStreamSynchronize(c10::hip::getCurrentHIPStream((int)dev).stream()), "hipStreamSynchronize");
    return mono_ns();
  });
  py::class_<PersistChoice>(m, "PersistChoice")
      .def_property_readonly("name", &engine_name)
      .def_readonly("x_width", &PersistChoice::x_width)
      .def_readonly("kp", &PersistChoice::kp)
      // the KP a row image must be packed for when the lean kernels of this choice gather from one, else 0
      .def("image_kp", [](const PersistChoice& c, int64_t Dout, int64_t loss_kind) {
        return linear_wave_reads_image(c, (int)Dout, (int)loss_kind) ? c.kp : 0;
      }, py::arg("Dout"), py::arg("loss_kind"));
  m.def("persistent_choice", &persistent_choice, py::arg("B"), py::arg("Din"), py::arg("H"), py::arg("Dout"),
        py::arg("loss_kind"), py::arg("num_samples"), py::arg("world"), py::arg("variant") = 0,
        py::arg("has_bias") = true);
  m.def(
      "persistent_engine",
      [](int64_t B, int64_t Din, int64_t H, int64_t Dout, int64_t loss_kind, int64_t num_samples, int64_t world,
         int64_t variant, bool has_bias) {
        return engine_name(persistent_choice(B, Din, H, Dout, loss_kind, num_samples, world, variant, has_bias));
      },
      py::arg("B"), py::arg("Din"), py::arg("H"), py::arg("Dout"), py::arg("loss_kind"), py::arg("num_samples"),
      py::arg("world"), py::arg("variant") = 0, py::arg("has_bias") = true);
  m.def("persistent_kernel_variant", &persistent_kernel_variant, py::arg("B"), py::arg("Din"), py::arg("H"),
        py::arg("Dout"), py::arg("loss_kind"), py::arg("num_samples"), py::arg("world"), py::arg("variant") = 0,
        py::arg("has_bias") = true, py::arg("momentum") = 0.0, py::arg("weight_decay") = 0.0,
        py::arg("stamps") = false);
  m.def("fused_mlp_lds_bytes", [](int B, int Din, int H, int Dout) { return fused_mlp_lds_bytes(B, Din, H, Dout); });
  // The lean wave loop's control (wave_loop_schedule.h) for a launch of n steps from (e0, j0) over epochs
  // of S batches of B entries: (read offsets, barrier-in-front flags, loss ring slots, barriers taken,
  // list stride). The kernel runs the same functions.
  m.def(
      "wave_loop_schedule",
      [](int S, int B, int e0, int j0, int n, int depth) {
        TORCH_CHECK(S > 0 && B > 0 && j0 >= 0 && j0 < S && n >= 0 && depth > 0, "wave_loop_schedule: bad arguments");
        const int estride = wave_list_stride(S * B, B), ring = 2 * S + depth;
        std::vector<int> ofs(n + depth + 2), slots(n + 1);
        std::vector<unsigned char> bar(ofs.size());
        int barriers = 0;
        const int nr = wave_loop_enumerate(S, B, estride, e0, j0, n, depth, ring, ofs.data(), bar.data(), (int)ofs.size(),
                                           slots.data(), (int)slots.size(), &barriers);
        TORCH_CHECK(nr >= 0, "wave_loop_schedule: more reads or steps than a launch of n steps has");
        ofs.resize(nr);
        slots.resize(n);
        std::vector<int> flags(bar.begin(), bar.begin() + nr);
        return py::make_tuple(ofs, flags, slots, barriers, estride);
      },
      py::arg("S"), py::arg("B"), py::arg("e0"), py::arg("j0"), py::arg("n"), py::arg("depth") = kWavePrefetch);
  // Run length of the lean wave loop from one state (ij reads made in the list, ring slot rslot,
  // groups_left whole groups left in the launch), and the state after advance(run):
  // (run, ij, lofs, rslot), with lofs counted from ij * B.
  m.def(
      "wave_loop_run_length",
      [](int S, int B, int depth, int ring, int ij, int rslot, int groups_left) {
        TORCH_CHECK(S > 0 && B > 0 && depth > 0 && ring > depth && ij >= 0 && ij <= S && rslot >= 0 && rslot < ring &&
                        groups_left >= 0,
                    "wave_loop_run_length: bad arguments");
        WaveLoopSchedule s;
        s.init(S, B, wave_list_stride(S * B, B), 0, 0, 0, depth, ring);
        s.ij = ij;
        s.lofs = ij * B;
        s.rslot = rslot;
        const int r = s.run(groups_left);
        s.advance(r);
        return py::make_tuple(r, s.ij, s.lofs, s.rslot);
      },
      py::arg("S"), py::arg("B"), py::arg("depth"), py::arg("ring"), py::arg("ij"), py::arg("rslot"),
      py::arg("groups_left"));
  // wave_loop_check_runs over every start j0 of an epoch of S batches and every launch length
  // 0..n_max, ring = 2 S + depth: (launches, group boundaries checked, first launch that differs as
  // (j0, n) or None).
  m.def(
      "wave_loop_check_runs",
      [](int S, int B, int depth, int n_max) {
        TORCH_CHECK(S > 0 && B > 0 && depth > 0 && n_max >= 0, "wave_loop_check_runs: bad arguments");
        const int estride = wave_list_stride(S * B, B), ring = 2 * S + depth;
        int64_t launches = 0, boundaries = 0;
        for (int j0 = 0; j0 < S; ++j0)
          for (int n = 0; n <= n_max; ++n) {
            const long c = wave_loop_check_runs(S, B, estride, j0 & 1, j0, n, depth, ring);
            if (c < 0) return py::make_tuple(launches, boundaries, py::cast(std::make_pair(j0, n)));
            ++launches;
            boundaries += c;
          }
        return py::make_tuple(launches, boundaries, py::object(py::none()));
      },
      py::arg("S"), py::arg("B"), py::arg("depth"), py::arg("n_max"));

  // Row image of the wave engine (wave_row_image.h). wave_row_image_layout(Din, KP): (floats per
  // record RS, bytes per row, slot of 1.0f or -1, slot of y, source[q][s] of every record slot: a
  // feature index, or -1 for 1.0f, -2 for y, -3 for zero). wave_pack_rows packs X [N, Din] (rows may be
  // padded) and Y [N] or [N, 1] into out [N, 4 RS] on the current stream.
  m.def(
      "wave_row_image_layout",
      [](int Din, int KP) {
        TORCH_CHECK(Din > 0 && KP > 0 && kWaveImageGroups * KP >= Din, "wave_row_image_layout: 4 KP must cover Din");
        std::vector<std::vector<int>> src(kWaveImageGroups, std::vector<int>(wave_image_rs(KP)));
        for (int q = 0; q < kWaveImageGroups; ++q)
          for (int s = 0; s < wave_image_rs(KP); ++s) src[q][s] = wave_image_source(Din, KP, q, s);
        return py::make_tuple(wave_image_rs(KP), wave_image_row_bytes(KP), wave_image_one_slot(KP), wave_image_y_slot(KP),
                              src);
      },
      py::arg("Din"), py::arg("KP"));
  m.def("wave_row_image_offset", [](int64_t row, int q, int KP) { return wave_image_offset(row, q, KP); }, py::arg("row"),
        py::arg("q"), py::arg("KP"));
  m.def("wave_row_image_fits", [](int64_t N, int Din, int KP) { return wave_image_fits(N, Din, KP); }, py::arg("N"),
        py::arg("Din"), py::arg("KP"));
  m.def(
      "wave_pack_rows",
      [](Tensor X, Tensor Y, int64_t Din, int64_t KP, Tensor out) {
        TORCH_CHECK(X.is_cuda(), "X must be a GPU tensor");  // rows may be padded: checked below
        check_gpu(Y, "Y");
        check_gpu(out, "out");
        const int64_t N = X.size(0);
        TORCH_CHECK(X.scalar_type() == at::kFloat && Y.scalar_type() == at::kFloat && out.scalar_type() == at::kFloat,
                    "wave_pack_rows: f32 tensors");
        TORCH_CHECK(X.dim() == 2 && X.size(1) == Din && X.stride(1) == 1 && X.stride(0) >= Din,
                    "wave_pack_rows: X must be [N, Din] with unit column stride");
        TORCH_CHECK(Y.numel() == N && Y.is_contiguous(), "wave_pack_rows: Y must hold one target per row");
        TORCH_CHECK(wave_image_fits(N, (int)Din, (int)KP), "wave_pack_rows: the image exceeds the layout's limits");
        TORCH_CHECK(out.is_contiguous() && out.numel() == N * wave_image_row_floats((int)KP) &&
                        out.device() == X.device() && Y.device() == X.device(),
                    "wave_pack_rows: out must be contiguous [N, 4 RS] on X's device");
        c10::hip::HIPGuard guard(X.device().index());
        hip_check(wave_pack_rows(X.data_ptr<float>(), X.stride(0), Y.data_ptr<float>(), N, (int)Din, (int)KP,
                                 out.data_ptr<float>(), cur_stream(X)),
                  "wave_pack_rows");
      },
      py::arg("X"), py::arg("Y"), py::arg("Din"), py::arg("KP"), py::arg("out"));

  // A HIP stream restricted to a set of CUs (hipExtStreamCreateWithCUMask), for
  // single-workgroup persistent engines: every launch lands on the same CU, so its
  // code, dataset rows and parameters stay in that XCD's L2 (and the CU's
  // instruction cache) between launches. Returns the raw handle (wrap with
  // torch.cuda.ExternalStream); the stream lives as long as the process.
  // hipSetDeviceFlags before the device's context exists (0 auto, 1 spin, 2 yield,
  // 4 blocking sync): how host waits (hipDeviceSynchronize/events) poll the GPU.
  m.def("set_device_flags", [](int device, unsigned flags) {
    TORCH_CHECK(hipSetDevice(device) == hipSuccess, "hipSetDevice");
    const hipError_t e = hipSetDeviceFlags(flags);
    TORCH_CHECK(e == hipSuccess, "hipSetDeviceFlags: ", hipGetErrorString(e));
  });
  m.def("cu_masked_stream", [](int device, std::vector<int> cus) {
    c10::hip::HIPGuard guard(device);
    int n_cu = 0;
    hip_check(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device), "CU count");
    std::vector<uint32_t> mask((n_cu + 31) / 32, 0u);
    for (int c : cus) {
      TORCH_CHECK(c >= 0 && c < n_cu, "cu_masked_stream: CU ", c, " out of range [0, ", n_cu, ")");
      mask[c / 32] |= 1u << (c % 32);
    }
    hipStream_t st = nullptr;
    hip_check(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()), "hipExtStreamCreateWithCUMask");
    return (uintptr_t)st;
  }, py::arg("device"), py::arg("cus"));
  m.def("graph_node_census", &graph_node_census_, "node count and per-hipGraphNodeType counts of a raw hipGraph_t");
  m.def("memset_async_", &memset_async_, "hipMemsetAsync of a whole tensor (tests of the graph memset rewrite)");
  m.def("graph_memset_params", &graph_memset_params_,
        "memset nodes of a raw hipGraph_t: [dst, value, elementSize, width, height, pitch] each");
  m.def("graph_memset_run", &graph_memset_run_, py::arg("t"), py::arg("value"), py::arg("esize"), py::arg("width"),
        py::arg("height"), py::arg("pitch"), py::arg("reps") = 1);
  m.def("graph_replace_memsets", &graph_replace_memsets_, "replace a raw hipGraph_t's memset nodes by fill-kernel nodes");
}

}  // namespace ptdt
