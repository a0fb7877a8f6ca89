// orb_device.h -- device helpers that more than one extractor stage uses (orb_*.hip only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slamgpu {

// v_dot2_u32_u16: a.lo * b.lo + a.hi * b.hi + c (pyramid: horizontal pass; orient_desc: blur taps)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t dot2u(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), c,
                                false);
}

}  // namespace slamgpu
