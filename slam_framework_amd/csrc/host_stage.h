// host_stage.h -- the per-thread staging buffer and stream of the synchronous C-ABI wrappers
// (optimizer, BoW, kfmatch, loopmatch, sim3solver, pnpsolver). A wrapper takes a StageLease, lays
// its arrays out with a StageLayout (stage_layout.h), reserves layout.size() bytes, uploads,
// launches its *_device form on the stage's stream, downloads and synchronises before it returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "host_common.h"

namespace slamgpu {

struct ThreadStage {
  int device = -1;  // the device buf and stream belong to
  hipStream_t stream = nullptr;  // non-blocking
  char* buf = nullptr;
  size_t bytes = 0;
  bool leased = false;
};

// One per calling thread, never destroyed: its device buffer and stream live until the process
// ends (the runtime reclaims them); freeing them from a thread-exit destructor at process exit
// would run after the HIP runtime's own teardown has begun.
ThreadStage& thread_stage();

// The calling thread's stage for the length of one synchronous call. The stage holds one call's
// data at a time: a second lease on the same thread (a wrapper called from inside another) is
// refused by reserve() with SLAMGPU_EINVAL instead of overwriting live data.
class StageLease {
 public:
  explicit StageLease(ErrorSlot& err) : s_(thread_stage()), err_(err), held_(!s_.leased) {
    if (held_) s_.leased = true;
  }
  ~StageLease() {
    if (held_) s_.leased = false;
  }
  StageLease(const StageLease&) = delete;
  StageLease& operator=(const StageLease&) = delete;

  // Makes the buffer at least `need` bytes on the current device: a change of device drops the
  // buffer and recreates the stream; growth frees and allocates max(need, 1 MiB). Pointers from
  // at() are valid after this and until the lease ends.
  int reserve(size_t need);

  template <typename T>
  T* at(size_t offset) const { return reinterpret_cast<T*>(s_.buf + offset); }
  // Queues the copy of a host array to its slot (nothing for an empty or absent array).
  hipError_t upload(size_t offset, const void* src, size_t bytes) const {
    if (!src || !bytes) return hipSuccess;
    return hipMemcpyAsync(s_.buf + offset, src, bytes, hipMemcpyHostToDevice, s_.stream);
  }
  // Queues the copy back of a slot; the data is there after the stream is synchronised.
  hipError_t download(void* dst, size_t offset, size_t bytes) const {
    if (!dst || !bytes) return hipSuccess;
    return hipMemcpyAsync(dst, s_.buf + offset, bytes, hipMemcpyDeviceToHost, s_.stream);
  }
  hipStream_t stream() const { return s_.stream; }
  int device() const { return s_.device; }

 private:
  ThreadStage& s_;
  ErrorSlot& err_;
  bool held_;
};

}  // namespace slamgpu
