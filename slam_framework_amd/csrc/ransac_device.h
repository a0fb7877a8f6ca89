// ransac_device.h -- what sim3_ransac.hip, pnp_ransac.hip and init_ransac.hip share around their
// models (DESIGN.md "What the RANSAC solvers share"): the draw checks, the swap-and-pop from draws
// to sample indices, the mask word, the best of a wave, the compaction. The first part is plain
// integer C++ that g++ compiles alone (tests/ransac_common_check.cpp), the rest needs hipcc.
#pragma once
#include <stdint.h>

#include "host_common.h"
#ifdef __HIPCC__
#include "device_math.h"
#define SLAMGPU_HOST_DEVICE __host__ __device__
#else
#define SLAMGPU_HOST_DEVICE
#endif

namespace slamgpu {

// The sample of one iteration: idx = avail[randi], avail[randi] = avail.back(), pop_back -- S
// times. avail is the identity but for the (position, value) pairs written so far; later writes
// win. Every draw must be in its range; idx takes the S indices.
template <int S>
SLAMGPU_HOST_DEVICE inline void resolve_sample(const int32_t* draws, int n, int* idx) {
  int pos[S], val[S], size = n;
#pragma unroll
  for (int i = 0; i < S; i++) {
    const int r = draws[i];
    int at_r = r, at_back = size - 1;
#pragma unroll
    for (int j = 0; j < i; j++) {
      if (pos[j] == r) at_r = val[j];
      if (pos[j] == size - 1) at_back = val[j];
    }
    idx[i] = at_r;
    pos[i] = r;
    val[i] = at_back;
    size--;
  }
}

// Draw i of a schedule (i % S = its place in the sample), of value r, lies in [0, n - 1 - i % S].
template <int S>
SLAMGPU_HOST_DEVICE inline bool draw_in_range(int r, int i, int n) {
  return r >= 0 && r <= n - 1 - i % S;
}

// The synchronous wrappers' check of a whole schedule.
template <int S>
inline int check_draws(ErrorSlot& err, const int32_t* draws, int n_its, int n) {
  for (int i = 0; i < S * n_its; i++)
    if (!draw_in_range<S>(draws[i], i, n))
      return err.fail(SLAMGPU_EINVAL, "iteration %d: draw %d = %d outside [0, %d]", i / S, i % S,
                      draws[i], n - 1 - i % S);
  return 0;
}

#ifdef __HIPCC__

// One wave checks a whole schedule. Only called for a job whose ranges are inside the arrays.
template <int S>
__device__ __forceinline__ bool draws_ok(const int32_t* draws, int n_its, int n, int lane) {
  int bad = 0;
  for (int i = lane; i < S * n_its; i += 64) bad |= !draw_in_range<S>(draws[i], i, n);
  return __ballot(bad) == 0;
}

// The mask word of 64 correspondences: lane 0 stores the ballot, every lane gets its popcount.
__device__ __forceinline__ int store_mask_word(bool in, uint64_t* word, int lane) {
  const uint64_t mask = __ballot(in);
  if (lane == 0) *word = mask;
  return __popcll(mask);
}

// Compaction: this lane's output slot if `mask` keeps it; count moves past the mask's lanes.
__device__ __forceinline__ int compact_slot(uint64_t mask, int& count) {
  const int slot = count + lanes_below(mask);
  count += __popcll(mask);
  return slot;
}

// Every lane gets the wave's largest value and, of the lanes that hold it, the lowest index >= 0:
// a NaN never wins, and index -1 (no candidate) never displaces a real one.
template <typename T>
__device__ __forceinline__ void wave_first_best(T& value, int& index) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(value, off, 64);
    const int oi = __shfl_xor(index, off, 64);
    if (o > value || (o == value && oi >= 0 && (index < 0 || oi < index))) {
      value = o;
      index = oi;
    }
  }
}

#endif  // __HIPCC__

}  // namespace slamgpu
