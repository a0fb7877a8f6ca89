// device_math_check.h -- what the translation units of tests/device_math_check share: the
// operation ids of the case file and the per-case kernel. One translation unit per library .hip
// (their anonymous-namespace names collide); each runs its operations through run_cases<Op>.
//
// Case file (all fields 8 bytes, little endian): magic, record count, then per record
//   op id, case count n, doubles per case in, doubles per case out, n * in doubles.
// The output file has the same layout with n * out doubles per record.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dmc {

constexpr uint64_t kMagic = 0x31304b4843444d44ull;  // "DMDCHK01"
constexpr uint64_t kMaxRecords = 64, kMaxCases = 1u << 16;

enum Op : uint64_t {
  kRcp = 1,
  kRsq = 2,
  kHuber = 3,
  kLdlt6 = 4,
  kLeftUpdate = 5,
  kQuatFromR = 6,
  kNormalizeRot = 7,
  kQuatRotate = 8,
  kQuatToR = 9,
  kSim3Exp = 10,
  kSim3Log = 11,
  kSim3Mul = 12,
  kSim3Inv = 13,
  kSim3Affine = 14,
  kLu3 = 15,
  kTriRc = 16,
  kDiagLdlt = 17,
  kPanelRow = 18,
  kBlockBack6 = 19,
  kFactorDiagBlock = 20,
  kBlockSolve = 21,
  kEvalEdge = 22,
  kLdlt7 = 30,
  kHuberSim3 = 31,
  kEgEdgeError = 40,
  kEgOplusAxis = 41,
};

// What ldlt_solve6 / ldlt_solve7 find in x before the call; a failed solve must leave it.
constexpr double kSentinel = -12345.0;

// One thread per case: Op::run(in + i * Op::kIn, out + i * Op::kOut).
template <class OpT>
__global__ __launch_bounds__(64) void case_kernel(const double* in, double* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) OpT::run(in + (size_t)i * OpT::kIn, out + (size_t)i * OpT::kOut);
}

template <class OpT>
hipError_t run_cases(const double* d_in, double* d_out, int n) {
  if (n <= 0) return hipSuccess;
  case_kernel<OpT><<<(n + 63) / 64, 64>>>(d_in, d_out, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipDeviceSynchronize();
}

// The operations of sim3_kernels.hip and eg_kernels.hip (their own translation units).
hipError_t run_ldlt7(const double* d_in, double* d_out, int n);
hipError_t run_huber_sim3(const double* d_in, double* d_out, int n);
hipError_t run_eg_edge_error(const double* d_in, double* d_out, int n);
hipError_t run_eg_oplus_axis(const double* d_in, double* d_out, int n);

}  // namespace dmc
