// kfmatch_common.h -- what kfmatch.hip (LocalMapper matchers) and loopmatch.hip (LoopCloser
// matchers) share: the descriptor distance, OpenCV's small gemm row, the KeyFrame grid-window
// arithmetic of GetFeaturesInArea, and the host side of the synchronous calls (per-thread error
// string, staging buffer + stream, keyframe validation and upload).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/slamgpu_kfmatch.h"
#include "device_math.h"

namespace slamgpu {

constexpr int kThLow = 50, kThHigh = 100, kHisto = 30, kGridCols = 64, kGridRows = 48;
constexpr int kMaxFeat = SLAMGPU_KF_MAX_FEATURES;

static_assert(sizeof(slamgpu_kf) == 128, "slamgpu_kf layout");
static_assert(sizeof(slamgpu_fuse_point) == 80, "slamgpu_fuse_point layout");

__device__ __forceinline__ int hamming32(const uint8_t* a, const uint8_t* b) {
  const uint4* p = reinterpret_cast<const uint4*>(a);
  const uint4* q = reinterpret_cast<const uint4*>(b);
  const uint4 a0 = p[0], a1 = p[1], b0 = q[0], b1 = q[1];
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// OpenCV's small float gemm row (Rcw * X + tcw): float dot, then (double) add.
__device__ __forceinline__ float gemm_row(const float* R, const float* x, float c) {
  const float dot = R[0] * x[0] + R[1] * x[1] + R[2] * x[2];
  return (float)((double)dot + (double)c);
}

// KeyFrame::GetFeaturesInArea (keyframe.cpp:442-476) cell window of a search square of half
// side r around (u, v); false when the window misses the grid.
__device__ __forceinline__ bool grid_window(float u, float v, float r, const slamgpu_kf_grid& g,
                                            int* cx0, int* cx1, int* cy0, int* cy1) {
  *cx0 = max(0, (int)floorf((u - g.min_x - r) / g.cell_w));
  *cx1 = min(kGridCols - 1, (int)ceilf((u - g.min_x + r) / g.cell_w));
  *cy0 = max(0, (int)floorf((v - g.min_y - r) / g.cell_h));
  *cy1 = min(kGridRows - 1, (int)ceilf((v - g.min_y + r) / g.cell_h));
  return !(*cx1 < 0 || *cx0 >= kGridCols || *cy1 < 0 || *cy0 >= kGridRows);
}

// Frame::PosInGrid (frame.cpp:339-346): the cell AssignFeaturesToGrid put a keypoint in (a cell
// outside the 64 x 48 grid means the keypoint is in no cell).
__device__ __forceinline__ void kp_cell(float x, float y, const slamgpu_kf_grid& g, int* px,
                                        int* py) {
  *px = (int)roundf((x - g.min_x) / g.cell_w);
  *py = (int)roundf((y - g.min_y) / g.cell_h);
}

inline thread_local std::string t_err;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  t_err = buf;
  return code;
}

#define KF_HIPCHECK(x)                                                                  \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) return fail(SLAMGPU_EHIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// Per-thread staging buffer + stream of the synchronous calls.
struct Stage {
  int device = -1;
  hipStream_t stream = nullptr;
  char* buf = nullptr;
  size_t bytes = 0;
  ~Stage() {
    if (buf) (void)hipFree(buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
inline thread_local Stage t_stage;

inline int stage_reserve(size_t need) {
  Stage& S = t_stage;
  int dev = 0;
  KF_HIPCHECK(hipGetDevice(&dev));
  if (S.device != dev) {
    if (S.buf) (void)hipFree(S.buf);
    if (S.stream) (void)hipStreamDestroy(S.stream);
    S.buf = nullptr;
    S.stream = nullptr;
    S.bytes = 0;
    KF_HIPCHECK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    S.device = dev;
  }
  if (need > S.bytes) {
    if (S.buf) KF_HIPCHECK(hipFree(S.buf));
    S.buf = nullptr;
    S.bytes = 0;
    const size_t cap = need < (1u << 20) ? (1u << 20) : need;
    KF_HIPCHECK(hipMalloc(&S.buf, cap));
    S.bytes = cap;
  }
  return 0;
}

inline int check_levels(const slamgpu_levels* lv) {
  if (!lv || lv->nlevels < 1 || lv->nlevels > 32)
    return fail(SLAMGPU_EINVAL, "levels: nlevels outside [1, 32]");
  return 0;
}

inline int check_kf(const slamgpu_kf* k, bool fv, const char* name) {
  if (!k) return fail(SLAMGPU_EINVAL, "%s is NULL", name);
  if (k->n < 0 || k->n > kMaxFeat)
    return fail(SLAMGPU_EINVAL, "%s: n %d outside [0, %d]", name, k->n, kMaxFeat);
  if (k->n > 0 && (!k->kps || !k->desc || !k->u_right || (fv && !k->has_mp)))
    return fail(SLAMGPU_EINVAL, "%s: NULL keypoint arrays", name);
  if (fv) {
    if (k->n_nodes < 0 || k->n_nodes > k->n)
      return fail(SLAMGPU_EINVAL, "%s: n_nodes %d outside [0, n]", name, k->n_nodes);
    if (k->n_nodes > 0) {
      if (!k->nodes || !k->node_start || !k->node_feats)
        return fail(SLAMGPU_EINVAL, "%s: NULL FeatureVector", name);
      if (k->node_start[0] != 0) return fail(SLAMGPU_EINVAL, "%s: node_start[0] != 0", name);
      for (int i = 0; i < k->n_nodes; i++) {
        if (k->node_start[i + 1] < k->node_start[i] || k->node_start[i + 1] > k->n)
          return fail(SLAMGPU_EINVAL, "%s: node_start not ascending within [0, n]", name);
        if (i > 0 && k->nodes[i] <= k->nodes[i - 1])
          return fail(SLAMGPU_EINVAL, "%s: nodes not strictly ascending", name);
      }
      for (int j = 0; j < k->node_start[k->n_nodes]; j++)
        if (k->node_feats[j] >= (uint32_t)k->n)
          return fail(SLAMGPU_EINVAL, "%s: feature index >= n", name);
    }
  }
  for (int j = 0; j < k->n; j++)
    if (k->kps[j].octave < 0 || k->kps[j].octave >= 32)
      return fail(SLAMGPU_EINVAL, "%s: keypoint %d octave %d outside [0, 32)", name, j,
                  k->kps[j].octave);
  return 0;
}

// Copies a host keyframe's arrays into the staging buffer at *off; returns its device twin.
inline slamgpu_kf stage_kf(const slamgpu_kf& k, bool fv, size_t* off) {
  char* base = t_stage.buf;
  slamgpu_kf d = k;
  auto put = [&](const void* src, size_t bytes) -> void* {
    void* dst = base + *off;
    *off += al256(bytes ? bytes : 1);
    if (bytes) (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, t_stage.stream);
    return dst;
  };
  d.kps = (const slamgpu_keypoint*)put(k.kps, (size_t)k.n * sizeof(slamgpu_keypoint));
  d.desc = (const uint8_t*)put(k.desc, (size_t)k.n * 32);
  d.u_right = (const float*)put(k.u_right, (size_t)k.n * 4);
  d.has_mp = fv ? (const uint8_t*)put(k.has_mp, (size_t)k.n) : nullptr;
  if (fv && k.n_nodes > 0) {
    d.nodes = (const uint32_t*)put(k.nodes, (size_t)k.n_nodes * 4);
    d.node_start = (const int32_t*)put(k.node_start, (size_t)(k.n_nodes + 1) * 4);
    d.node_feats = (const uint32_t*)put(k.node_feats, (size_t)k.node_start[k.n_nodes] * 4);
  } else {
    d.nodes = nullptr;
    d.node_start = nullptr;
    d.node_feats = nullptr;
    d.n_nodes = 0;
  }
  return d;
}

inline size_t kf_bytes(const slamgpu_kf& k, bool fv) {
  size_t b = al256((size_t)k.n * sizeof(slamgpu_keypoint) + 1) + al256((size_t)k.n * 32 + 1) +
             al256((size_t)k.n * 4 + 1) + al256((size_t)k.n + 1);
  if (fv && k.n_nodes > 0)
    b += al256((size_t)k.n_nodes * 4) + al256((size_t)(k.n_nodes + 1) * 4) +
         al256((size_t)k.node_start[k.n_nodes] * 4 + 1);
  return b;
}

}  // namespace slamgpu
