// device_math_check_sim3.hip -- the helpers of sim3_kernels.hip for tests/device_math_check
// (its anonymous-namespace names collide with pose_kernels.hip's, hence a unit of its own).
#include "../slam_framework_amd/csrc/sim3_kernels.hip"

#include "device_math_check.h"

namespace slamgpu {
namespace {

struct OpLdlt7 {  // H (28, packed upper), lambda, b (7) -> ok, x (7)
  static constexpr int kIn = 36, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double H[kNH7], b[7], x[7];
    for (int i = 0; i < kNH7; i++) H[i] = in[i];
    for (int i = 0; i < 7; i++) {
      b[i] = in[29 + i];
      x[i] = dmc::kSentinel;
    }
    out[0] = ldlt_solve7(H, in[28], b, x) ? 1.0 : 0.0;
    for (int i = 0; i < 7; i++) out[1 + i] = x[i];
  }
};
struct OpHuberSim3 {  // (e, delta) -> rho, rho'
  static constexpr int kIn = 2, kOut = 2;
  __device__ static void run(const double* in, double* out) { huber(in[0], in[1], out[0], out[1]); }
};

}  // namespace
}  // namespace slamgpu

namespace dmc {
hipError_t run_ldlt7(const double* d_in, double* d_out, int n) {
  return run_cases<slamgpu::OpLdlt7>(d_in, d_out, n);
}
hipError_t run_huber_sim3(const double* d_in, double* d_out, int n) {
  return run_cases<slamgpu::OpHuberSim3>(d_in, d_out, n);
}
}  // namespace dmc
