// device_math_check_eg.hip -- the helpers of eg_kernels.hip for tests/device_math_check (its
// anonymous-namespace names collide with the other solvers', hence a unit of its own).
#include "../slam_framework_amd/csrc/eg_kernels.hip"

#include "device_math_check.h"

namespace slamgpu {
namespace {

struct OpEgEdgeError {  // M = Sji (8), Si (8), Sj (8) -> e (7), chi2
  static constexpr int kIn = 24, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double m[8], a[8], b[8], e[7];
    for (int i = 0; i < 8; i++) {
      m[i] = in[i];
      a[i] = in[8 + i];
      b[i] = in[16 + i];
    }
    out[7] = edge_error(sim3::sim3_load(m), sim3::sim3_load(a), sim3::sim3_load(b), e);
    for (int i = 0; i < 7; i++) out[i] = e[i];
  }
};
struct OpEgOplusAxis {  // S (8), axis d, step h, fix_scale -> exp(h e_d) * S
  static constexpr int kIn = 11, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double s[8], v[8];
    for (int i = 0; i < 8; i++) s[i] = in[i];
    sim3::sim3_store(oplus_axis(sim3::sim3_load(s), (int)in[8], in[9], (int)in[10]), v);
    for (int i = 0; i < 8; i++) out[i] = v[i];
  }
};

}  // namespace
}  // namespace slamgpu

namespace dmc {
hipError_t run_eg_edge_error(const double* d_in, double* d_out, int n) {
  return run_cases<slamgpu::OpEgEdgeError>(d_in, d_out, n);
}
hipError_t run_eg_oplus_axis(const double* d_in, double* d_out, int n) {
  return run_cases<slamgpu::OpEgOplusAxis>(d_in, d_out, n);
}
}  // namespace dmc
