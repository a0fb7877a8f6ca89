// host_stage.cpp -- the thread-local objects of the host layer: every module's error slot and
// the staging buffer shared by the synchronous wrappers.
#include "host_stage.h"

namespace slamgpu {

thread_local ErrorSlot t_opt_err;
thread_local ErrorSlot t_bow_err;
thread_local ErrorSlot t_kfdb_err;
thread_local ErrorSlot t_kf_err;
thread_local ErrorSlot t_s3_err;
thread_local ErrorSlot t_pnp_err;
thread_local ErrorSlot t_init_err;
thread_local ErrorSlot t_io_err;
thread_local ErrorSlot t_create_err;

ThreadStage& thread_stage() {
  thread_local ThreadStage* s = new ThreadStage();
  return *s;
}

int StageLease::reserve(size_t need) {
  if (!held_)
    return err_.fail(SLAMGPU_EINVAL,
                     "a synchronous call is already using this thread's staging buffer");
  ThreadStage& S = s_;
  int dev = 0;
  HIPCHECK(err_, hipGetDevice(&dev));
  if (S.device != dev) {
    if (S.buf) (void)hipFree(S.buf);
    if (S.stream) (void)hipStreamDestroy(S.stream);
    S.buf = nullptr;
    S.stream = nullptr;
    S.bytes = 0;
    HIPCHECK(err_, hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    S.device = dev;
  }
  if (need > S.bytes) {
    if (S.buf) HIPCHECK(err_, hipFree(S.buf));
    S.buf = nullptr;
    S.bytes = 0;
    const size_t cap = need < (1u << 20) ? (1u << 20) : need;
    HIPCHECK(err_, hipMalloc(&S.buf, cap));
    S.bytes = cap;
  }
  return 0;
}

}  // namespace slamgpu
