// The _C extension module: its attributes, and one binder per domain file next to this one.
#include "common.h"

PYBIND11_MODULE(_C, m) {
  using namespace ptdt;
  m.doc() = "MI355X-native kernels, RCCL communicator and DDP reducer";
  m.attr("ARCH") = "gfx950";
  // engine before comm: PersistentPlan.__init__ and fused_mlp_step take an XgmiComm and have always
  // been defined before that class is registered (their signatures spell it by its C++ name)
  bind_engine(m);
  bind_optim(m);
  bind_averaging(m);
  bind_eval(m);
  bind_math(m);
  bind_norm(m);
  bind_int8(m);
  bind_comm(m);
}
