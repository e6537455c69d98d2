// Bindings of the communicators (RCCL, single-process RCCL clique, xGMI) and the DDP reducer.
#include "common.h"

#include "comm/rccl_comm.h"
#include "comm/xgmi_comm.h"
#include "reducer/reducer.h"

namespace ptdt {
namespace {

// ------------------------------------------------------------- comm
ncclDataType_t nccl_dt(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return ncclFloat32;
    case at::kBFloat16: return ncclBfloat16;
    case at::kHalf: return ncclFloat16;
    case at::kDouble: return ncclFloat64;
    case at::kInt: return ncclInt32;
    case at::kLong: return ncclInt64;
    case at::kChar: return ncclInt8;
    case at::kByte: return ncclUint8;
    default: TORCH_CHECK(false, "RcclComm: unsupported dtype ", t.scalar_type());
  }
  return ncclFloat32;
}

hipStream_t stream_arg(const Tensor& t, int64_t s) {
  return s != 0 ? reinterpret_cast<hipStream_t>(s) : cur_stream(t);
}

// a clique collective's operands: one buffer per device, each on its tensor's current stream
struct CliqueBufs {
  std::vector<void*> b;
  std::vector<hipStream_t> s;
};
CliqueBufs clique_bufs(std::vector<Tensor>& ts) {
  CliqueBufs r;
  for (auto& t : ts) {
    r.b.push_back(t.data_ptr());
    r.s.push_back(cur_stream(t));
  }
  return r;
}

}  // namespace

void bind_comm(py::module_& m) {
  m.def("plan_buckets", &plan_buckets);

  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def_static("new_unique_id",
                  []() {
                    auto v = RcclComm::new_unique_id();
                    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
                  })
      .def(py::init([](int rank, int world, py::bytes uid, int device, double timeout_s, bool fingerprint) {
             std::string s = uid;
             std::vector<uint8_t> v(s.begin(), s.end());
             py::gil_scoped_release nogil;
             return std::make_shared<RcclComm>(rank, world, v, device, timeout_s, fingerprint);
           }),
           py::arg("rank"), py::arg("world"), py::arg("uid"), py::arg("device"), py::arg("timeout_s") = 600.0,
           py::arg("fingerprint") = false)
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("world", &RcclComm::world)
      .def_property_readonly("device", &RcclComm::device)
      .def_property_readonly("seq", &RcclComm::seq)
      .def("all_reduce",
           [](RcclComm& c, Tensor t, int op, int64_t stream) {
             TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "all_reduce: contiguous GPU tensor");
             c.all_reduce(t.data_ptr(), t.data_ptr(), t.numel(), nccl_dt(t), (ncclRedOp_t)op, stream_arg(t, stream));
           },
           py::arg("t"), py::arg("op") = 0, py::arg("stream") = 0)
      .def("broadcast",
           [](RcclComm& c, Tensor t, int root, int64_t stream) {
             TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "broadcast: contiguous GPU tensor");
             c.broadcast(t.data_ptr(), t.data_ptr(), t.numel(), nccl_dt(t), root, stream_arg(t, stream));
           },
           py::arg("t"), py::arg("root") = 0, py::arg("stream") = 0)
      .def("reduce",
           [](RcclComm& c, Tensor t, int root, int op, int64_t stream) {
             TORCH_CHECK(t.is_cuda() && t.is_contiguous());
             c.reduce(t.data_ptr(), t.data_ptr(), t.numel(), nccl_dt(t), (ncclRedOp_t)op, root, stream_arg(t, stream));
           },
           py::arg("t"), py::arg("root") = 0, py::arg("op") = 0, py::arg("stream") = 0)
      .def("all_gather",
           [](RcclComm& c, Tensor out, Tensor in, int64_t stream) {
             TORCH_CHECK(out.is_cuda() && in.is_cuda() && out.is_contiguous() && in.is_contiguous());
             TORCH_CHECK(out.numel() == in.numel() * c.world(), "all_gather: out must be world x in");
             c.all_gather(in.data_ptr(), out.data_ptr(), in.numel(), nccl_dt(in), stream_arg(in, stream));
           },
           py::arg("out"), py::arg("inp"), py::arg("stream") = 0)
      .def("reduce_scatter",
           [](RcclComm& c, Tensor out, Tensor in, int op, int64_t stream) {
             TORCH_CHECK(out.is_cuda() && in.is_cuda() && out.is_contiguous() && in.is_contiguous());
             TORCH_CHECK(in.numel() == out.numel() * c.world(), "reduce_scatter: in must be world x out");
             c.reduce_scatter(in.data_ptr(), out.data_ptr(), out.numel(), nccl_dt(in), (ncclRedOp_t)op,
                              stream_arg(in, stream));
           },
           py::arg("out"), py::arg("inp"), py::arg("op") = 0, py::arg("stream") = 0)
      .def("all_to_all",
           [](RcclComm& c, Tensor out, Tensor in, int64_t stream) {
             TORCH_CHECK(out.is_cuda() && in.is_cuda() && out.numel() == in.numel() && in.numel() % c.world() == 0);
             c.all_to_all(in.data_ptr(), out.data_ptr(), in.numel() / c.world(), nccl_dt(in), stream_arg(in, stream));
           },
           py::arg("out"), py::arg("inp"), py::arg("stream") = 0)
      .def("send",
           [](RcclComm& c, Tensor t, int peer, int64_t stream) {
             TORCH_CHECK(t.is_cuda() && t.is_contiguous());
             c.send(t.data_ptr(), t.numel(), nccl_dt(t), peer, stream_arg(t, stream));
           },
           py::arg("t"), py::arg("peer"), py::arg("stream") = 0)
      .def("recv",
           [](RcclComm& c, Tensor t, int peer, int64_t stream) {
             TORCH_CHECK(t.is_cuda() && t.is_contiguous());
             c.recv(t.data_ptr(), t.numel(), nccl_dt(t), peer, stream_arg(t, stream));
           },
           py::arg("t"), py::arg("peer"), py::arg("stream") = 0)
      .def("group_start", &RcclComm::group_start)
      .def("group_end", &RcclComm::group_end)
      .def("error", &RcclComm::error)
      .def("abort", &RcclComm::abort)
      .def_property_readonly("aborted", &RcclComm::aborted)
      .def("fingerprints", &RcclComm::fingerprints)
      .def_property_readonly("captured", &RcclComm::captured)
      .def("expect_captured", &RcclComm::expect_captured, py::arg("k"))
      .def_property_readonly("completed_captured", &RcclComm::completed_captured)
      .def_property_readonly("event_pool_size", &RcclComm::event_pool_size)
      .def_property_readonly("events_created", &RcclComm::events_created);

  py::class_<XgmiComm, std::shared_ptr<XgmiComm>>(m, "XgmiComm")
      .def(py::init<int, int, int, int>(), py::arg("rank"), py::arg("world"), py::arg("max_elems"), py::arg("device"))
      .def("handle", [](XgmiComm& c) { return py::bytes(c.handle()); })
      .def("open", [](XgmiComm& c, std::vector<py::bytes> hs, std::vector<int> devices) {
        std::vector<std::string> v;
        for (auto& h : hs) v.push_back(std::string(h));
        c.open(v, devices);
      }, py::arg("handles"), py::arg("devices") = std::vector<int>{})
      .def_property_readonly("ready", &XgmiComm::ready)
      .def_property_readonly("rank", &XgmiComm::rank)
      .def_property_readonly("world", &XgmiComm::world)
      .def_property_readonly("max_elems", &XgmiComm::max_elems)
      .def_property("max_polls", &XgmiComm::max_polls, &XgmiComm::set_max_polls)
      .def("error", &XgmiComm::error)
      .def("reset_error", &XgmiComm::reset_error)
      .def("all_reduce_avg", [](XgmiComm& c, Tensor t) {
        check_gpu(t, "xgmi all_reduce tensor");
        TORCH_CHECK(t.scalar_type() == at::kFloat, "xgmi all_reduce: fp32");
        TORCH_CHECK(c.ready(), "xgmi all_reduce: communicator not opened");
        TORCH_CHECK(t.numel() <= c.max_elems(), "xgmi all_reduce: tensor larger than the xGMI buffer");
        c10::hip::HIPGuard guard(t.device().index());
        hip_check(xgmi_allreduce_avg(c.args(), t.data_ptr<float>(), (int)t.numel(), cur_stream(t)),
                  "xgmi_allreduce_avg");
      });

  py::class_<RcclClique, std::shared_ptr<RcclClique>>(m, "RcclClique")
      .def(py::init<const std::vector<int>&>())
      .def_property_readonly("size", &RcclClique::size)
      .def("broadcast",
           [](RcclClique& c, std::vector<Tensor> ts, int root) {
             const CliqueBufs o = clique_bufs(ts);
             c.broadcast(o.b, ts.at(0).numel(), nccl_dt(ts.at(0)), root, o.s);
           })
      .def("reduce",
           [](RcclClique& c, std::vector<Tensor> ts, int root) {
             const CliqueBufs o = clique_bufs(ts);
             c.reduce(o.b, ts.at(0).numel(), nccl_dt(ts.at(0)), root, o.s);
           })
      .def("all_reduce", [](RcclClique& c, std::vector<Tensor> ts) {
        const CliqueBufs o = clique_bufs(ts);
        c.all_reduce(o.b, ts.at(0).numel(), nccl_dt(ts.at(0)), o.s);
      });

  py::class_<Reducer, std::shared_ptr<Reducer>>(m, "Reducer")
      .def(py::init([](std::vector<Tensor> params, std::vector<std::vector<int64_t>> buckets,
                       std::shared_ptr<RcclComm> comm, py::object py_allreduce, bool find_unused) {
             Reducer::PyAllReduce fn;
             if (!py_allreduce.is_none()) {
               fn = [py_allreduce](Tensor t) {
                 py::gil_scoped_acquire g;
                 py_allreduce(t);
               };
             }
             return std::make_shared<Reducer>(std::move(params), std::move(buckets), std::move(comm), fn,
                                              find_unused);
           }),
           py::arg("params"), py::arg("buckets"), py::arg("comm"), py::arg("py_allreduce"),
           py::arg("find_unused") = false)
      .def("prepare_for_backward", &Reducer::prepare_for_backward)
      .def("mark_ready", &Reducer::mark_ready)
      .def("finalize", &Reducer::finalize)
      .def("rebuild", &Reducer::rebuild)
      .def("ready_order", &Reducer::ready_order)
      .def("buckets", &Reducer::buckets)
      .def("bucket_tensors", &Reducer::bucket_tensors)
      .def("zero_grads", &Reducer::zero_grads)
      .def("zero_grads_except", &Reducer::zero_grads_except)
      .def("grad_view", &Reducer::grad_view)
      .def_property_readonly("iteration", &Reducer::iteration)
      .def_property_readonly("in_backward", &Reducer::in_backward);
}

}  // namespace ptdt
