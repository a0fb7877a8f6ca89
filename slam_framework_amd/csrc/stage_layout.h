// stage_layout.h -- where every synchronous wrapper puts its arrays in the per-thread staging
// buffer (host_stage.h). HIP-free: tests/host_stage_check.cpp walks these layouts on the CPU.
//
// A wrapper takes all its offsets from one StageLayout, reserves size() bytes, and only then turns
// offsets into pointers: there is no second size expression to keep in step. The layout functions
// return their structs as braced lists, whose clauses run left to right: a struct's fields are in
// take order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/slamgpu.h"
#include "../../include/slamgpu_bow.h"
#include "../../include/slamgpu_initializer.h"
#include "../../include/slamgpu_loopmatch.h"
#include "../../include/slamgpu_optimizer.h"
#include "../../include/slamgpu_pnpsolver.h"
#include "../../include/slamgpu_sim3solver.h"
#include "host_common.h"

namespace slamgpu {

// Bump allocator over offsets. Every slot starts on a 256-byte boundary and is followed by at
// least one spare byte, so a zero-byte request still gets a slot of its own.
struct StageLayout {
  size_t take(size_t bytes) {
    const size_t at = off_;
    off_ += (bytes + 256) / 256 * 256;
    if (log) log->emplace_back(at, bytes);
    return at;
  }
  template <typename T>
  size_t take(size_t count) { return take(count * sizeof(T)); }
  size_t size() const { return off_; }
  std::vector<std::pair<size_t, size_t>>* log = nullptr;  // (offset, bytes) of every take: tests

 private:
  size_t off_ = 0;
};

constexpr size_t kNoSlot = ~(size_t)0;  // an array the call does not stage

// PoseOptimization / OptimizeSim3 of one problem: its n items (edges / matches), the state that
// is refined in place (Tcw / S12) and the per-item flags.
struct SolveLayout { size_t start, items, state, flags, result; };
inline SolveLayout layout_solve(StageLayout& L, size_t n, size_t item_bytes, size_t state_bytes) {
  return {L.take<int32_t>(2), L.take(n * item_bytes), L.take(state_bytes), L.take(n),
          L.take<int32_t>(1)};
}

// Local / global BA on the cooperative solver. [0, er) goes up and [0, io) comes back in one copy
// each through a pinned twin, so the order of the fields is part of the contract; the solver's
// workspace follows at ws == io.
struct CoopLayout { size_t T, mode, pts, ps, obs, free_of, kf_of, pfirst, prow, er, ctl, io, ws; };
inline CoopLayout layout_coop(StageLayout& L, size_t n_kf, size_t K, size_t n_points, size_t n_obs,
                              size_t ws_bytes) {
  return {L.take(64 * n_kf), L.take(n_kf + 1), L.take(12 * n_points + 4),
          L.take(4 * (n_points + 1)), L.take(sizeof(slamgpu_ba_obs) * n_obs + 4),
          L.take(4 * n_kf + 4), L.take(4 * K + 4), L.take(4 * K + 4), L.take(8 * 6 * K + 8),
          L.take(n_obs + 4), L.take<int32_t>(8), L.size(), L.take(ws_bytes)};
}

struct BowTransformLayout {
  size_t desc, cnt, words, values, n_words, nodes, node_start, node_feats, n_nodes, feat_leaf,
      feat_node;
};
inline BowTransformLayout layout_bow_transform(StageLayout& L, size_t cap) {
  return {L.take(cap * 32), L.take<int32_t>(1), L.take<uint32_t>(cap), L.take<double>(cap),
          L.take<int32_t>(1), L.take<uint32_t>(cap), L.take<int32_t>(cap + 1),
          L.take<uint32_t>(cap), L.take<int32_t>(1), L.take<uint32_t>(cap), L.take<uint32_t>(cap)};
}

struct BowSetPlace { size_t desc, kps, valid, cnt, nodes, node_start, node_feats; };
inline BowSetPlace place_bow_set(StageLayout& L, size_t n, size_t n_nodes) {
  return {L.take(n * 32), L.take<slamgpu_keypoint>(n), L.take(n), L.take<int32_t>(2),
          L.take<uint32_t>(n_nodes), L.take<int32_t>(n_nodes + 1), L.take<uint32_t>(n)};
}
struct BowSearchLayout { BowSetPlace a, b; size_t views, match, nmatches; };
inline BowSearchLayout layout_search_by_bow(StageLayout& L, size_t na, size_t na_nodes, size_t nb,
                                            size_t nb_nodes) {
  return {place_bow_set(L, na, na_nodes), place_bow_set(L, nb, nb_nodes),
          L.take<slamgpu_bow_view>(2), L.take<int32_t>(na + 1), L.take<int32_t>(1)};
}

struct DistinctiveLayout { size_t desc, start, best, out; };
inline DistinctiveLayout layout_distinctive(StageLayout& L, size_t n_points, size_t total) {
  return {L.take(total * 32 + 4), L.take<int32_t>(n_points + 1), L.take<int32_t>(n_points),
          L.take(n_points * 32)};
}

struct GrayLayout { size_t src, dst; };
inline GrayLayout layout_gray(StageLayout& L, size_t src_bytes, size_t dst_bytes) {
  return {L.take(src_bytes), L.take(dst_bytes)};
}

// Which of a slamgpu_kf's arrays a matcher reads: the Sim3 matchers keypoints and descriptors,
// Fuse u_right too, SearchForTriangulation has_mp and the FeatureVector as well.
enum KfParts { kKfLoop = 0, kKfStereo = 1, kKfFeatureVector = 2 };
struct KfPlace { size_t kps, desc, u_right, has_mp, nodes, node_start, node_feats; };
// n_feats = node_start[n_nodes], of a keyframe that passed check_kf.
inline KfPlace place_kf(StageLayout& L, KfParts parts, size_t n, size_t n_nodes, size_t n_feats) {
  const bool fv = parts >= kKfFeatureVector, nodes = fv && n_nodes > 0;
  return {L.take<slamgpu_keypoint>(n), L.take(n * 32),
          parts >= kKfStereo ? L.take<float>(n) : kNoSlot, fv ? L.take(n) : kNoSlot,
          nodes ? L.take<uint32_t>(n_nodes) : kNoSlot,
          nodes ? L.take<int32_t>(n_nodes + 1) : kNoSlot,
          nodes ? L.take<uint32_t>(n_feats) : kNoSlot};
}

struct TriLayout { KfPlace kf[2]; size_t kfs, pair, match, nmatches; };
inline TriLayout layout_search_tri(StageLayout& L, const int n[2], const int n_nodes[2],
                                   const int n_feats[2]) {
  return {{place_kf(L, kKfFeatureVector, n[0], n_nodes[0], n_feats[0]),
           place_kf(L, kKfFeatureVector, n[1], n_nodes[1], n_feats[1])},
          L.take<slamgpu_kf>(2), L.take<slamgpu_tri_pair>(1), L.take<int32_t>((size_t)n[0] + 1),
          L.take<int32_t>(1)};
}

// Fuse (parts = kKfStereo) and the loop closer's Sim3 Fuse (kKfLoop).
struct FuseLayout { KfPlace kf; size_t kfs, pts, best_idx, best_dist; };
inline FuseLayout layout_fuse(StageLayout& L, KfParts parts, size_t n, size_t n_pts) {
  return {place_kf(L, parts, n, 0, 0), L.take<slamgpu_kf>(1), L.take<slamgpu_fuse_point>(n_pts),
          L.take<int32_t>(n_pts), L.take<int32_t>(n_pts)};
}

struct SbpSim3Layout {
  KfPlace kf;
  size_t kfs, pts, job, matched_in, kp_point, point_kp, nmatches, scratch;
};
inline SbpSim3Layout layout_sbp_sim3(StageLayout& L, size_t n, size_t n_pts, size_t scratch_bytes) {
  return {place_kf(L, kKfLoop, n, 0, 0), L.take<slamgpu_kf>(1), L.take<slamgpu_fuse_point>(n_pts),
          L.take<slamgpu_sbp_job>(1), L.take(n), L.take<int32_t>(n), L.take<int32_t>(n_pts),
          L.take<int32_t>(1), L.take(scratch_bytes)};
}

// SearchBySim3: the per-keypoint arrays of both keyframes share the stride max(n1, n2).
struct SearchSim3Layout {
  KfPlace kf[2];
  size_t kfs, mp, pair, already1, already2, match12, vn_match1, vn_match2, nfound;
};
inline SearchSim3Layout layout_search_sim3(StageLayout& L, size_t n1, size_t n2) {
  const size_t stride = n1 > n2 ? n1 : n2;
  return {{place_kf(L, kKfLoop, n1, 0, 0), place_kf(L, kKfLoop, n2, 0, 0)},
          L.take<slamgpu_kf>(2), L.take<slamgpu_fuse_point>(n1 + n2),
          L.take<slamgpu_sim3_pair>(1), L.take(stride), L.take(stride), L.take<int32_t>(stride),
          L.take<int32_t>(stride), L.take<int32_t>(stride), L.take<int32_t>(1)};
}

// The RANSAC Sim3 solver of one candidate: n correspondences, n_its iterations of 3 draws; the
// mask rows are SLAMGPU_SIM3_MASK_WORDS(n) words each.
struct Sim3RansacLayout { size_t matches, draws, job, hyp, bits, events, n_events; };
inline Sim3RansacLayout layout_sim3_ransac(StageLayout& L, size_t n, size_t n_its) {
  return {L.take<slamgpu_sim3_match>(n), L.take<int32_t>(3 * n_its),
          L.take<slamgpu_sim3_ransac_job>(1), L.take<slamgpu_sim3_hyp>(n_its),
          L.take<uint64_t>(n_its * SLAMGPU_SIM3_MASK_WORDS(n)), L.take<int32_t>(n_its),
          L.take<int32_t>(1)};
}

// The RANSAC EPnP solver of one candidate: n correspondences, n_its iterations of 4 draws; the
// mask rows (hypotheses and refined) are SLAMGPU_PNP_MASK_WORDS(n) words each.
struct PnpRansacLayout {
  size_t matches, draws, job, hyp, bits, refined, refined_bits, events, n_events;
};
inline PnpRansacLayout layout_pnp_ransac(StageLayout& L, size_t n, size_t n_its) {
  return {L.take<slamgpu_pnp_match>(n), L.take<int32_t>(4 * n_its),
          L.take<slamgpu_pnp_ransac_job>(1), L.take<slamgpu_pnp_hyp>(n_its),
          L.take<uint64_t>(n_its * SLAMGPU_PNP_MASK_WORDS(n)), L.take<slamgpu_pnp_hyp>(n_its),
          L.take<uint64_t>(n_its * SLAMGPU_PNP_MASK_WORDS(n)), L.take<int32_t>(n_its),
          L.take<int32_t>(1)};
}

// The monocular Initializer of one pair of frames: n1 and n2 keys, n_its iterations of 8 draws;
// every row is sized by n1 and n_its, the mask rows are SLAMGPU_INIT_MASK_WORDS(n1) words each.
struct InitRansacLayout {
  size_t keys1, matches12, keys2, draws, job, hyp, bits, result, pairs, motion, good_bits, p3d;
};
inline InitRansacLayout layout_init_ransac(StageLayout& L, size_t n1, size_t n2, size_t n_its) {
  const size_t words = SLAMGPU_INIT_MASK_WORDS(n1);
  return {L.take<float>(2 * n1), L.take<int32_t>(n1), L.take<float>(2 * n2),
          L.take<int32_t>(8 * n_its), L.take<slamgpu_init_job>(1),
          L.take<slamgpu_init_hyp>(2 * n_its), L.take<uint64_t>(2 * n_its * words),
          L.take<slamgpu_init_result>(1), L.take<int32_t>(2 * n1),
          L.take<slamgpu_init_motion>(SLAMGPU_INIT_MAX_MOTIONS),
          L.take<uint64_t>(SLAMGPU_INIT_MAX_MOTIONS * words),
          L.take<float>(SLAMGPU_INIT_MAX_MOTIONS * 3 * n1)};
}

// The synchronous SearchByProjection calls of one frame (frame-to-frame, local map,
// relocalisation): nq queries of query_bytes each, then the pose record (extra_bytes; the
// local-map search has none).
struct FrameSearchLayout { size_t queries, extra; };
inline FrameSearchLayout layout_frame_search(StageLayout& L, size_t nq, size_t query_bytes,
                                             size_t extra_bytes) {
  return {L.take(nq * query_bytes), L.take(extra_bytes)};
}

// The synchronous SearchForInitialization of one frame: n1 queries, the parameters, and the
// arrays parallel to the queries (vbPrevMatched in and out, vnMatches12 out).
struct InitSearchLayout { size_t queries, params, prev_matched, matches12; };
inline InitSearchLayout layout_init_search(StageLayout& L, size_t n1) {
  return {L.take<slamgpu_init_query>(n1), L.take<slamgpu_init_search>(1), L.take<float>(2 * n1),
          L.take<int32_t>(n1)};
}

// A host FeatureVector (n_nodes > 0) must be well formed before its indices reach the device:
// slamgpu_bow_score of n_pairs pairs: both sides' words and values packed back to back
// (total_words entries each), their counts and the views that point at them.
struct BowScoreLayout { size_t words, values, counts, views, scores; };
inline BowScoreLayout layout_bow_score(StageLayout& L, size_t n_pairs, size_t total_words) {
  return {L.take<uint32_t>(total_words), L.take<double>(total_words),
          L.take<int32_t>(2 * n_pairs), L.take<slamgpu_bow_vec_view>(2 * n_pairs),
          L.take<double>(n_pairs)};
}

// One BowVector on its way into the database, or a relocalisation query's.
struct KfdbVecLayout { size_t words, values, n; };
inline KfdbVecLayout layout_kfdb_vec(StageLayout& L, size_t n) {
  return {L.take<uint32_t>(n), L.take<double>(n), L.take<int32_t>(1)};
}
// A detect call: the id lists of the loop query, the outputs ([0, out_end) from min_score on come
// back), the scratch.
struct KfdbDetectLayout {
  size_t connected, covisible, min_score, n_candidates, candidates, common_words, scores, scratch;
};
inline KfdbDetectLayout layout_kfdb_detect(StageLayout& L, size_t max_kf, size_t n_connected,
                                           size_t n_covisible, size_t scratch_bytes) {
  return {L.take<int32_t>(n_connected), L.take<int32_t>(n_covisible), L.take<float>(1),
          L.take<int32_t>(1), L.take<int32_t>(max_kf), L.take<int32_t>(max_kf),
          L.take<float>(max_kf), L.take(scratch_bytes)};
}

// node_start[0] == 0 and ascending within [0, n], nodes strictly ascending, feature indices < n.
// feat_fmt is the caller's wording of the last failure; it is given (name, index).
inline int check_feature_vector(ErrorSlot& err, const char* name, int n, int n_nodes,
                                const uint32_t* nodes, const int32_t* node_start,
                                const uint32_t* node_feats, const char* feat_fmt) {
  if (!nodes || !node_start || !node_feats)
    return err.fail(SLAMGPU_EINVAL, "%s: NULL FeatureVector", name);
  if (node_start[0] != 0) return err.fail(SLAMGPU_EINVAL, "%s: node_start[0] != 0", name);
  for (int i = 0; i < n_nodes; i++) {
    if (node_start[i + 1] < node_start[i] || node_start[i + 1] > n)
      return err.fail(SLAMGPU_EINVAL, "%s: node_start not ascending within [0, n]", name);
    if (i > 0 && nodes[i] <= nodes[i - 1])
      return err.fail(SLAMGPU_EINVAL, "%s: nodes not strictly ascending", name);
  }
  for (int j = 0; j < node_start[n_nodes]; j++)
    if (node_feats[j] >= (uint32_t)n) return err.fail(SLAMGPU_EINVAL, feat_fmt, name, node_feats[j]);
  return 0;
}

}  // namespace slamgpu
