// kfmatch_common.h -- the host side of a keyframe that kfmatch.hip (LocalMapper matchers) and
// loopmatch.hip (LoopCloser matchers) share: its validation and its place in and upload to the
// staging buffer (host_stage.h; errors go to t_kf_err). The matchers' device rules are in
// orbmatch_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slamgpu_kfmatch.h"
#include "host_stage.h"
#include "orbmatch_device.h"
#include "stage_layout.h"

namespace slamgpu {

constexpr int kMaxFeat = SLAMGPU_KF_MAX_FEATURES;

static_assert(sizeof(slamgpu_kf) == 128, "slamgpu_kf layout");
static_assert(sizeof(slamgpu_fuse_point) == 80, "slamgpu_fuse_point layout");

inline int check_levels(const slamgpu_levels* lv) {
  if (!lv || lv->nlevels < 1 || lv->nlevels > 32)
    return t_kf_err.fail(SLAMGPU_EINVAL, "levels: nlevels outside [1, 32]");
  return 0;
}

inline int check_grid(const slamgpu_kf_grid* grid) {
  if (!(grid->cell_w > 0) || !(grid->cell_h > 0))
    return t_kf_err.fail(SLAMGPU_EINVAL, "grid cell size");
  return 0;
}

inline int check_kf(const slamgpu_kf* k, bool fv, const char* name) {
  if (!k) return t_kf_err.fail(SLAMGPU_EINVAL, "%s is NULL", name);
  if (k->n < 0 || k->n > kMaxFeat)
    return t_kf_err.fail(SLAMGPU_EINVAL, "%s: n %d outside [0, %d]", name, k->n, kMaxFeat);
  if (k->n > 0 && (!k->kps || !k->desc || !k->u_right || (fv && !k->has_mp)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "%s: NULL keypoint arrays", name);
  if (fv) {
    if (k->n_nodes < 0 || k->n_nodes > k->n)
      return t_kf_err.fail(SLAMGPU_EINVAL, "%s: n_nodes %d outside [0, n]", name, k->n_nodes);
    if (k->n_nodes > 0)
      if (int r = check_feature_vector(t_kf_err, name, k->n, k->n_nodes, k->nodes, k->node_start,
                                       k->node_feats, "%s: feature index >= n"))
        return r;
  }
  for (int j = 0; j < k->n; j++)
    if (k->kps[j].octave < 0 || k->kps[j].octave >= 32)
      return t_kf_err.fail(SLAMGPU_EINVAL, "%s: keypoint %d octave %d outside [0, 32)", name, j,
                           k->kps[j].octave);
  return 0;
}

// Copies a host keyframe's arrays to their places; returns its device twin (arrays without a
// place are NULL there).
inline slamgpu_kf upload_kf(const StageLease& S, const slamgpu_kf& k, const KfPlace& p) {
  slamgpu_kf d = k;
  auto put = [&](size_t at, const void* src, size_t bytes) -> const void* {
    if (at == kNoSlot) return nullptr;
    void* dst = S.at<char>(at);
    if (bytes) (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S.stream());
    return dst;
  };
  d.kps = (const slamgpu_keypoint*)put(p.kps, k.kps, (size_t)k.n * sizeof(slamgpu_keypoint));
  d.desc = (const uint8_t*)put(p.desc, k.desc, (size_t)k.n * 32);
  d.u_right = (const float*)put(p.u_right, k.u_right, (size_t)k.n * 4);
  d.has_mp = (const uint8_t*)put(p.has_mp, k.has_mp, (size_t)k.n);
  const bool fv = p.nodes != kNoSlot;
  if (!fv) d.n_nodes = 0;
  d.nodes = (const uint32_t*)put(p.nodes, k.nodes, (size_t)d.n_nodes * 4);
  d.node_start = (const int32_t*)put(p.node_start, k.node_start, (size_t)(d.n_nodes + 1) * 4);
  d.node_feats = (const uint32_t*)put(p.node_feats, k.node_feats,
                                      fv ? (size_t)k.node_start[k.n_nodes] * 4 : 0);
  return d;
}

}  // namespace slamgpu
