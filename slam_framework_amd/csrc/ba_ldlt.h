// ba_ldlt.h -- the register-level pieces of the 6x6-blocked LDLT that ba_coop.hip's three
// factorisations of the reduced camera system share (factor_solve: dense, in LDS;
// factor_solve_profile: block-profile storage, work-group 0; factor_profile_grid: the same over
// the whole grid), and the small synchronisation and timing helpers around them. The solvers
// keep their own loops over rows, loads and stores; every arithmetic statement of a diagonal
// block, a panel row and a backward block step is here, once. Each piece sets its own FMA
// contraction: the library is built with -ffp-contract=off and this is the tolerance-compared
// FP64 path, so a helper without the pragma would stop fusing and change the results.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_device.h"

#ifndef FS_PROF
#define FS_PROF 0
#endif

namespace slamgpu {
namespace ba {

// ---- synchronisation -------------------------------------------------------------------------
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Work-group barrier ordering LDS only (no vmcnt drain of pending global loads or stores).
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// One wave: what its lanes wrote (LDS or global) before is visible to all of them after.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- phase timer -----------------------------------------------------------------------------
__device__ __forceinline__ uint64_t phase_clock() {  // the 100 MHz realtime counter
  return __builtin_amdgcn_s_memrealtime();
}

// The diagnostic build's (-DFS_PROF=1) split of a factorisation: tick(k) adds the microseconds
// since the previous tick to acc[k] (a null acc: this thread does not time). Empty otherwise.
#if FS_PROF
struct PhaseTimer {
  double* acc;
  uint64_t t0;
  __device__ __forceinline__ explicit PhaseTimer(double* a) : acc(a), t0(phase_clock()) {}
  __device__ __forceinline__ void tick(int k) {
    if (acc) {
      const uint64_t t = phase_clock();
      acc[k] += 0.01 * (double)(t - t0);
      t0 = t;
    }
  }
};
#else
struct PhaseTimer {
  __device__ __forceinline__ explicit PhaseTimer(double*) {}
  __device__ __forceinline__ void tick(int) {}
};
#endif

// ---- row addressing --------------------------------------------------------------------------
// Where row i of the factor starts: packed lower (dense), or the block-profile's row table.
struct DenseRows {
  __device__ __forceinline__ int off(int i) const { return tri(i); }
};
struct ProfileRows {
  const int64_t* prow;
  __device__ __forceinline__ int64_t off(int i) const { return prow[i]; }
};

// Packed lower-triangle index e = r (r + 1) / 2 + c -> (r, c), c <= r.
__device__ __forceinline__ void tri_rc(int e, int& r, int& c) {
  r = 0;
  while ((r + 1) * (r + 2) / 2 <= e) r++;
  c = e - r * (r + 1) / 2;
}

// ---- the diagonal block ----------------------------------------------------------------------
// The 6x6 LDLT of a diagonal block (lower triangle A, 21 doubles row-major packed) with the
// forward solve of its rhs slice y: strict lower L, D (on A's diagonal) and the solved y in
// place, D^-1 (one reciprocal per pivot) in rdg. False on an exact zero pivot.
__device__ __forceinline__ bool diag_ldlt(double (&A)[21], double (&y)[6], double (&rdg)[6]) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  bool good = true;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double d = A[c * (c + 3) / 2];
    good = good && d != 0.0;
    const double rd = d != 0.0 ? 1.0 / d : 0.0;
    rdg[c] = rd;
    double l[6];
#pragma unroll
    for (int r = c + 1; r < 6; r++) {
      l[r] = A[r * (r + 1) / 2 + c] * rd;
      y[r] -= l[r] * y[c];
      A[r * (r + 1) / 2 + c] = l[r];
    }
#pragma unroll
    for (int r = c + 1; r < 6; r++) {
      const double ld = l[r] * d;
#pragma unroll
      for (int k = c + 1; k <= r; k++) A[r * (r + 1) / 2 + k] -= ld * l[k];
    }
  }
  return good;
}

// Block J = j0 / 6 factored in place in the factor storage, by one lane: the block and its rhs
// slice to registers, diag_ldlt, then strict lower L, D, D^-1 and the solved rhs back.
template <typename PtrT, typename Rows>
__device__ __forceinline__ bool factor_diag_block(PtrT Lp, Rows rows, PtrT rhs, PtrT dg, PtrT idg,
                                                  int j0) {
  double A[21], y[6], rdg[6];
#pragma unroll
  for (int r = 0; r < 6; r++) {
    y[r] = rhs[j0 + r];
#pragma unroll
    for (int k = 0; k <= r; k++) A[r * (r + 1) / 2 + k] = Lp[rows.off(j0 + r) + j0 + k];
  }
  const bool good = diag_ldlt(A, y, rdg);
#pragma unroll
  for (int r = 0; r < 6; r++) {
#pragma unroll
    for (int k = 0; k < r; k++) Lp[rows.off(j0 + r) + j0 + k] = A[r * (r + 1) / 2 + k];
    dg[j0 + r] = A[r * (r + 3) / 2];
    idg[j0 + r] = rdg[r];
    rhs[j0 + r] = y[r];
  }
  return good;
}

// The 15 strict-lower entries of block J = j0 / 6, by column c then k < c (index
// c (c - 1) / 2 + k): the order the panel's forward substitution and block_back6 read them.
template <typename PtrT, typename Rows>
__device__ __forceinline__ void load_strict_lower(PtrT Lp, Rows rows, int j0, double (&L)[15]) {
#pragma unroll
  for (int c = 1; c < 6; c++)
#pragma unroll
    for (int k = 0; k < c; k++) L[c * (c - 1) / 2 + k] = Lp[rows.off(j0 + c) + j0 + k];
}

// ---- a panel row -----------------------------------------------------------------------------
// Row i below block J, from its six entries a = A_iJ: v = A_iJ L_JJ^-T (forward substitution
// against Ljj), l = L_iJ = v D_J^-1, and the fused forward solve r = rhs_i - L_iJ y_J.
__device__ __forceinline__ void panel_row(const double (&a)[6], const double (&Ljj)[15],
                                          const double (&rdg)[6], const double (&yj)[6],
                                          double (&v)[6], double (&l)[6], double& r) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  int q = 0;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double s = a[c];
#pragma unroll
    for (int k = 0; k < c; k++) s -= v[k] * Ljj[q++];
    v[c] = s;
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    l[c] = v[c] * rdg[c];
    r -= l[c] * yj[c];
  }
}

// ---- the backward solve ----------------------------------------------------------------------
// L_JJ^T x = z within one block, in registers: x_c is final when c is reached, descending.
__device__ __forceinline__ void block_back6(const double (&Lb)[15], double (&x)[6]) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
#pragma unroll
  for (int c = 5; c >= 0; c--)
#pragma unroll
    for (int r = 0; r < c; r++) x[r] -= Lb[c * (c - 1) / 2 + r] * x[c];
}

}  // namespace ba
}  // namespace slamgpu
