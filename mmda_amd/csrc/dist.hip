// The data-parallel piece of the C ABI that talks to RCCL (the reference is single-device, its only trace of multi-GPU is the
// commented nn.DataParallel at solver.py:88-91): mmda_allreduce, the in-place sum all-reduce of a float buffer on an RCCL communicator,
// for hosts that own one (a native trainer; the Python host goes through torch.distributed, whose communicator is not exposed).  The
// deterministic sum of all-gathered (id, row) pairs, mmda_embed_segment_sum, lives with the rest of the rows code in embed_rows.hip.
#include "common.h"
#include "internal.h"
#include <dlfcn.h>

// ---------------------------------------------------------------------------------------------- RCCL all-reduce
// The entry points are looked up at run time: first among the symbols already loaded in the process (the library that created the
// caller's communicator -- a communicator is only valid inside the library instance it came from), then in librccl.so.  The shared
// library therefore carries no link-time dependency on RCCL and loads on machines without it.
namespace {
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
nccl_allreduce_fn find_allreduce() {
  static nccl_allreduce_fn fn = nullptr;
  static bool looked = false;
  if (looked) return fn;
  looked = true;
  void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
  if (!sym) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (h) sym = dlsym(h, "ncclAllReduce");
  }
  fn = (nccl_allreduce_fn)sym;
  return fn;
}
}  // namespace

extern "C" int mmda_allreduce(void* buf, size_t n_floats, void* nccl_comm, void* stream) {
  if (!buf || !nccl_comm) return MMDA_EINVAL;
  if (n_floats == 0) return MMDA_OK;
  nccl_allreduce_fn ar = find_allreduce();
  if (!ar) { mmda_set_error("mmda_allreduce: ncclAllReduce not found (librccl.so)", hipErrorNotFound); return MMDA_ELAUNCH; }
  // ncclFloat32 = 7, ncclSum = 0 (rccl.h); in place
  const int rc = ar(buf, buf, n_floats, 7, 0, nccl_comm, (hipStream_t)stream);
  if (rc != 0) { mmda_set_error("mmda_allreduce: ncclAllReduce failed", hipErrorUnknown); return MMDA_ELAUNCH; }
  return MMDA_OK;
}
