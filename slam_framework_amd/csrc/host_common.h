// host_common.h -- error reporting of the host code behind the C ABI (HIP-free itself: the
// HIPCHECK macro names HIP only where it is expanded).
//
// Every module reports through an ErrorSlot: one per calling thread and module (defined in
// host_stage.cpp, so that slamgpu_*_last_error() of one module never shows another's failure;
// kfmatch and loopmatch share t_kf_err), or one per front-end context (runtime.cpp).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/slamgpu.h"

namespace slamgpu {

// The one message formatter: at most 511 characters.
inline std::string format_message(const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof(buf), fmt, ap);
  return buf;
}

struct ErrorSlot {
  std::string msg;
  // Records the message and returns `code`, so that call sites read `return err.fail(...)`.
  int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    msg = format_message(fmt, ap);
    va_end(ap);
    return code;
  }
  const char* c_str() const { return msg.c_str(); }
};

extern thread_local ErrorSlot t_opt_err;     // slamgpu_optimizer_last_error
extern thread_local ErrorSlot t_bow_err;     // slamgpu_bow_last_error
extern thread_local ErrorSlot t_kfdb_err;    // slamgpu_kfdb_last_error
extern thread_local ErrorSlot t_kf_err;     // slamgpu_kfmatch_last_error == slamgpu_loopmatch_last_error
extern thread_local ErrorSlot t_s3_err;      // slamgpu_sim3solver_last_error
extern thread_local ErrorSlot t_pnp_err;     // slamgpu_pnpsolver_last_error
extern thread_local ErrorSlot t_init_err;    // slamgpu_initializer_last_error
extern thread_local ErrorSlot t_io_err;      // slamgpu_io_last_error
extern thread_local ErrorSlot t_create_err;  // slamgpu_last_error(NULL): why slamgpu_create failed

}  // namespace slamgpu

// Returns SLAMGPU_EHIP from the enclosing function, through `slot`, when the HIP call fails.
#define HIPCHECK(slot, x)                                                           \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess)                                                           \
      return (slot).fail(SLAMGPU_EHIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)
