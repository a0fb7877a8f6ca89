// slamgpu_adapters.hpp -- the graph gathering and write-back of the reference's Optimizer and
// OrbMatcher entry points, as OpenCV- and g2o-free C++17 over plain views of the map (header only).
//
// The reference builds its g2o graphs and matcher inputs from Frame / KeyFrame / MapPoint objects
// (src/optimizer/optimizer.cpp, src/orb_features/orb_matcher.cpp). The C ABI (slamgpu.h,
// slamgpu_optimizer.h) takes arrays instead. These helpers turn plain views of those objects into
// the ABI records in exactly the order optimizer.cpp creates its vertices and edges, and apply the
// results back as the reference does, so a reference-side adapter is a loop that fills the views
// (Frame::GetMapPoint, KeyFrame::GetMapPointMatches, MapPoint::GetObservations, ...) and calls
// one function. tests/adapter_check.cpp drives them against an independent restatement of the
// reference's gathering (tests/test_adapters.py), and tests/capi_check.cpp feeds their output to
// the device.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "slamgpu.h"
#include "slamgpu_bow.h"
#include "slamgpu_initializer.h"
#include "slamgpu_kfdb.h"
#include "slamgpu_kfmatch.h"
#include "slamgpu_loopmatch.h"
#include "slamgpu_optimizer.h"
#include "slamgpu_pnpsolver.h"
#include "slamgpu_sim3solver.h"

namespace slamgpu_adapter {

// ---- views of the reference's objects (indices into caller-owned arrays, -1 = none) ---------

// One observation of a map point: MapPoint::GetObservations()'s (KeyFrame*, keypoint index),
// the keyframe given as its index in the keyframe array.
struct ObsRef {
  int32_t keyframe;
  int32_t keypoint;
};

struct MapPointView {
  int64_t id;                // MapPoint::GetId()
  bool bad;                  // isBad()
  float xyz[3];              // GetWorldPos()
  const uint8_t* desc;       // GetDescriptor() (32 B)
  const ObsRef* obs;         // GetObservations(), in the std::map's iteration order
  int n_obs;                 // NumObservations() counts these
};

struct KeyFrameView {
  int64_t id;                          // KeyFrame::Id()
  bool bad;                            // isBad()
  const float* Tcw;                    // GetPose(): 4x4 row-major f32
  const slamgpu_keypoint* undist_kps;  // undistorted_keypoints
  const float* right_coords;           // right_coords (< 0: monocular)
  const int32_t* map_points;           // GetMapPointMatches(): map point index per keypoint
  int n_kps;
  const int32_t* covisible;            // GetVectorCovisibleKeyFrames(): keyframe indices
  int n_covisible;
};

struct FrameView {
  const float* Tcw;                    // GetPose(): 4x4 row-major f32
  const slamgpu_keypoint* kps;         // GetKeys()
  const slamgpu_keypoint* undist_kps;  // GetUndistortedKeys()
  const float* right_coords;           // StereoCoordRight()
  const int32_t* map_points;           // GetMapPoint(i): map point index or -1
  const uint8_t* outlier;              // IsOutlier(i)
  int n_kps;
};

// ---- ORBextractor (orb_extractor.h:25-93) without OpenCV ----------------------------------------

// The ctor's tables (orb_extractor.cpp:351-387), host-side: what GetScaleFactors /
// GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares return.
struct OrbTables {
  int rc = SLAMGPU_EINVAL;
  std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
  std::vector<int> features_per_level;
};

inline OrbTables orb_scale_tables(const slamgpu_orb_params& p) {
  OrbTables t;
  const int n = p.nlevels > 0 && p.nlevels <= 12 ? p.nlevels : 0;
  t.scale.resize(n);
  t.inv_scale.resize(n);
  t.sigma2.resize(n);
  t.inv_sigma2.resize(n);
  t.features_per_level.resize(n);
  t.rc = slamgpu_orb_scale_tables(&p, t.scale.data(), t.inv_scale.data(), t.sigma2.data(),
                                  t.inv_sigma2.data(), t.features_per_level.data());
  return t;
}

// The ORBextractor surface over plain buffers: the device context is created on the first
// Compute (and again when the image size changes); the tables never need one. The OpenCV class
// (slamgpu_orb_adapter.hpp) is a thin shell over this one.
class OrbExtractorCore {
 public:
  OrbExtractorCore(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                   int device = 0)
      : params_{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST}, device_(device),
        tables_(orb_scale_tables(params_)) {
    if (tables_.rc != SLAMGPU_OK) throw std::invalid_argument("slamgpu: invalid ORB parameters");
  }
  ~OrbExtractorCore() { slamgpu_destroy(ctx_); }
  OrbExtractorCore(const OrbExtractorCore&) = delete;
  OrbExtractorCore& operator=(const OrbExtractorCore&) = delete;

  // orb_extractor.cpp:985-1049 on an 8-bit image: kps / desc (N x 32) replaced; returns N. An
  // empty image (rows or cols 0) leaves the outputs untouched and returns -1 (:990-991).
  int Compute(const uint8_t* image, int rows, int cols, size_t step,
              std::vector<slamgpu_keypoint>& kps, std::vector<uint8_t>& desc) {
    if (!image || rows <= 0 || cols <= 0) return -1;
    ensure(cols, rows);
    const int cap = slamgpu_kp_capacity(ctx_);
    kps.resize(cap);
    desc.resize((size_t)cap * 32);
    int n = 0;
    check(slamgpu_extract(ctx_, image, step, kps.data(), desc.data(), cap, &n));
    kps.resize(n);
    desc.resize((size_t)n * 32);
    pyramid_valid_ = false;
    return n;
  }

  int GetLevels() const { return params_.nlevels; }
  float GetScaleFactor() const { return params_.scale_factor; }
  const std::vector<float>& GetScaleFactors() const { return tables_.scale; }
  const std::vector<float>& GetInverseScaleFactors() const { return tables_.inv_scale; }
  const std::vector<float>& GetScaleSigmaSquares() const { return tables_.sigma2; }
  const std::vector<float>& GetInverseScaleSigmaSquares() const { return tables_.inv_sigma2; }

  // GetImagePyramid (orb_extractor.h:62) of the last Compute, downloaded on first use: level l is
  // pyramid_size(l) = (cols, rows), rows of `cols` bytes.
  const std::vector<std::vector<uint8_t>>& GetImagePyramid() {
    if (!pyramid_valid_) {
      if (!ctx_) throw std::logic_error("slamgpu: GetImagePyramid before Compute");
      pyramid_.assign(params_.nlevels, {});
      sizes_.assign(params_.nlevels, {0, 0});
      for (int l = 0; l < params_.nlevels; l++) {
        int w = 0, h = 0;
        check(slamgpu_get_pyramid_level(ctx_, 0, l, nullptr, 0, &w, &h));
        pyramid_[l].resize((size_t)w * h);
        check(slamgpu_get_pyramid_level(ctx_, 0, l, pyramid_[l].data(), (size_t)w, &w, &h));
        sizes_[l] = {w, h};
      }
      pyramid_valid_ = true;
    }
    return pyramid_;
  }
  std::pair<int, int> pyramid_size(int level) const { return sizes_.at(level); }

  slamgpu_ctx* context() { return ctx_; }

 private:
  void ensure(int cols, int rows) {
    if (ctx_ && cols == cols_ && rows == rows_) return;
    slamgpu_destroy(ctx_);
    ctx_ = nullptr;
    check(slamgpu_create(device_, &params_, cols, rows, 1, &ctx_));
    cols_ = cols;
    rows_ = rows;
  }
  void check(int rc) const {
    if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") +
                                                   slamgpu_last_error(ctx_));
  }

  slamgpu_orb_params params_;
  int device_;
  OrbTables tables_;
  slamgpu_ctx* ctx_ = nullptr;
  int cols_ = 0, rows_ = 0;
  bool pyramid_valid_ = false;
  std::vector<std::vector<uint8_t>> pyramid_;
  std::vector<std::pair<int, int>> sizes_;
};

// ---- Optimizer::PoseOptimization (optimizer.cpp:209-411) ---------------------------------------

struct PoseGraph {
  std::vector<slamgpu_pose_edge> edges;  // one per keypoint with a map point, keypoint order
  std::vector<int32_t> keypoint;         // the keypoint of each edge (vnIndexEdgeMono/Stereo)
};

// optimizer.cpp:247-327: an edge for every keypoint that has a map point (no isBad test there),
// monocular when StereoCoordRight()[i] < 0, with the undistorted keypoint as the measurement.
inline PoseGraph gather_pose_optimization(const FrameView& f, const MapPointView* mps) {
  PoseGraph g;
  for (int i = 0; i < f.n_kps; ++i) {
    const int m = f.map_points[i];
    if (m < 0) continue;
    const slamgpu_keypoint& k = f.undist_kps[i];
    slamgpu_pose_edge e;
    std::memcpy(e.xw, mps[m].xyz, sizeof e.xw);
    e.u = k.x;
    e.v = k.y;
    e.ur = f.right_coords[i];
    e.octave = k.octave;
    g.edges.push_back(e);
    g.keypoint.push_back(i);
  }
  return g;
}

// optimizer.cpp:262,289 + :349-397: the frame's outlier flags after the call (every keypoint with
// an edge is (re)classified; the others keep theirs).
inline void apply_pose_optimization(const PoseGraph& g, const uint8_t* edge_outlier,
                                    uint8_t* frame_outlier) {
  for (size_t k = 0; k < g.keypoint.size(); ++k) frame_outlier[g.keypoint[k]] = edge_outlier[k];
}

// ---- Optimizer::LocalBundleAdjustment (optimizer.cpp:413-716) ----------------------------------

struct LocalBaGraph {
  std::vector<int32_t> keyframe;      // keyframe index of each vertex: local keyframes, then fixed
  std::vector<float> kf_Tcw;          // [n][16]
  std::vector<uint8_t> kf_mode;       // SLAMGPU_KF_*
  std::vector<int32_t> map_point;     // map point index of each point vertex
  std::vector<float> points;          // [n][3]
  std::vector<int32_t> point_obs_start;
  std::vector<slamgpu_ba_obs> obs;    // edges, per point in observation order
  std::vector<ObsRef> obs_ref;        // (keyframe index, keypoint index) of each edge
  int n_local = 0;
};

// The graph gathering of optimizer.cpp:416-605. Local keyframes: the current one and its
// covisible keyframes that are not bad (every covisible one is marked local, bad or not,
// :422-427); local map points: the local keyframes' map point matches in order, not bad, each
// once (:431-442); fixed cameras: keyframes observing a local point that are neither marked
// local nor already fixed, in observation order, kept if not bad (:445-461). Vertices: local
// keyframes (fixed when Id() == 0), fixed cameras, then the points; edges per point in
// GetObservations() order, skipping bad keyframes (:537-605).
inline LocalBaGraph gather_local_bundle_adjustment(const KeyFrameView* kfs, int n_kf,
                                                   const MapPointView* mps, int n_mp,
                                                   int current) {
  LocalBaGraph g;
  std::vector<uint8_t> kf_local(n_kf, 0), kf_fixed(n_kf, 0), mp_local(n_mp, 0);
  std::vector<int32_t> local_kfs, fixed_kfs, vertex_of(n_kf, -1);
  kf_local[current] = 1;
  local_kfs.push_back(current);
  const KeyFrameView& cur = kfs[current];
  for (int c = 0; c < cur.n_covisible; ++c) {
    const int k = cur.covisible[c];
    kf_local[k] = 1;
    if (!kfs[k].bad) local_kfs.push_back(k);
  }
  for (int k : local_kfs) {
    const KeyFrameView& kf = kfs[k];
    for (int i = 0; i < kf.n_kps; ++i) {
      const int m = kf.map_points[i];
      if (m >= 0 && !mps[m].bad && !mp_local[m]) {
        mp_local[m] = 1;
        g.map_point.push_back(m);
      }
    }
  }
  for (int m : g.map_point) {
    for (int o = 0; o < mps[m].n_obs; ++o) {
      const int k = mps[m].obs[o].keyframe;
      if (!kf_local[k] && !kf_fixed[k]) {
        kf_fixed[k] = 1;
        if (!kfs[k].bad) fixed_kfs.push_back(k);
      }
    }
  }
  auto add_kf = [&](int k, uint8_t mode) {
    vertex_of[k] = (int32_t)g.keyframe.size();
    g.keyframe.push_back(k);
    g.kf_Tcw.insert(g.kf_Tcw.end(), kfs[k].Tcw, kfs[k].Tcw + 16);
    g.kf_mode.push_back(mode);
  };
  for (int k : local_kfs) add_kf(k, kfs[k].id == 0 ? SLAMGPU_KF_LOCAL_FIXED : SLAMGPU_KF_LOCAL);
  g.n_local = (int)local_kfs.size();
  for (int k : fixed_kfs) add_kf(k, SLAMGPU_KF_FIXED);
  g.point_obs_start.push_back(0);
  for (int m : g.map_point) {
    g.points.insert(g.points.end(), mps[m].xyz, mps[m].xyz + 3);
    for (int o = 0; o < mps[m].n_obs; ++o) {
      const ObsRef r = mps[m].obs[o];
      if (kfs[r.keyframe].bad) continue;
      const slamgpu_keypoint& kp = kfs[r.keyframe].undist_kps[r.keypoint];
      slamgpu_ba_obs e;
      e.keyframe = vertex_of[r.keyframe];
      e.u = kp.x;
      e.v = kp.y;
      e.ur = kfs[r.keyframe].right_coords[r.keypoint];
      e.octave = kp.octave;
      g.obs.push_back(e);
      g.obs_ref.push_back(r);
    }
    g.point_obs_start.push_back((int32_t)g.obs.size());
  }
  return g;
}

// The write-back of optimizer.cpp:667-716 as a list of changes for the caller to apply under
// map->map_update_mutex: the (keyframe, keypoint) / (map point, keyframe) pairs to erase
// (EraseMapPointMatch + EraseObservation for every erase[e]), the local keyframes' poses
// (SetPose), every point's position (SetWorldPos + UpdateNormalAndDepth).
struct LocalBaResult {
  std::vector<ObsRef> erase_match;      // KeyFrame::EraseMapPointMatch(keypoint)
  std::vector<int32_t> erase_obs_point; // MapPoint::EraseObservation(keyframe) of these points
  std::vector<int32_t> pose_keyframe;   // SetPose(pose[16 k]) of these keyframes
  std::vector<float> pose;
};

inline LocalBaResult local_bundle_adjustment_result(const LocalBaGraph& g, const uint8_t* erase) {
  LocalBaResult r;
  for (size_t p = 0; p + 1 < g.point_obs_start.size(); ++p)
    for (int e = g.point_obs_start[p]; e < g.point_obs_start[p + 1]; ++e)
      if (erase[e]) {
        r.erase_match.push_back(g.obs_ref[e]);
        r.erase_obs_point.push_back(g.map_point[p]);
      }
  for (int v = 0; v < g.n_local; ++v) {
    r.pose_keyframe.push_back(g.keyframe[v]);
    r.pose.insert(r.pose.end(), g.kf_Tcw.begin() + 16 * v, g.kf_Tcw.begin() + 16 * v + 16);
  }
  return r;
}

// ---- OrbMatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (orb_matcher.cpp:1312) ----

struct F2FInput {
  std::vector<slamgpu_f2f_query> queries;  // one per last-frame map point that is not an outlier
  std::vector<int32_t> query_map_point;    // map point index of each query (mp_id = position)
  slamgpu_f2f_pose pose;
};

// tlc = Rlw * (-Rcw^T tcw) + tlw in f32, as the cv::Mat expressions of :1326-1333.
inline float f2f_tlc_z(const float* Tcw_cur, const float* Tcw_last) {
  float twc[3];
  for (int k = 0; k < 3; ++k)
    twc[k] = -(Tcw_cur[0 * 4 + k] * Tcw_cur[3] + Tcw_cur[1 * 4 + k] * Tcw_cur[7] +
               Tcw_cur[2 * 4 + k] * Tcw_cur[11]);
  return Tcw_last[8] * twc[0] + Tcw_last[9] * twc[1] + Tcw_last[10] * twc[2] + Tcw_last[11];
}

// The queries of :1337-1341 (a last-frame keypoint with a map point, not an outlier) in
// last-frame keypoint order, and the pose record. A query's `blocks` is NumObservations() > 0
// (the claim it makes on a current-frame keypoint blocks later queries, :1389-1393).
inline F2FInput gather_search_by_projection_frame(const FrameView& current, const FrameView& last,
                                                  const MapPointView* mps, float baseline,
                                                  float th, bool mono, bool check_ori) {
  F2FInput in;
  for (int i = 0; i < last.n_kps; ++i) {
    const int m = last.map_points[i];
    if (m < 0 || last.outlier[i]) continue;
    slamgpu_f2f_query q{};
    std::memcpy(q.xyz, mps[m].xyz, sizeof q.xyz);
    q.last_angle = last.undist_kps[i].angle;
    q.last_octave = last.kps[i].octave;
    q.mp_id = (int32_t)in.queries.size();
    q.blocks = mps[m].n_obs > 0;
    std::memcpy(q.desc, mps[m].desc, 32);
    in.queries.push_back(q);
    in.query_map_point.push_back(m);
  }
  slamgpu_f2f_pose& p = in.pose;
  std::memset(&p, 0, sizeof p);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.Rcw[3 * r + c] = current.Tcw[4 * r + c];
    p.tcw[r] = current.Tcw[4 * r + 3];
  }
  p.tlc_z = f2f_tlc_z(current.Tcw, last.Tcw);
  p.baseline = baseline;
  p.th = th;
  p.mono = mono ? 1 : 0;
  p.check_ori = check_ori ? 1 : 0;
  return in;
}

// The current frame's claim state before either SearchByProjection: slot[i] = -1 (no query has
// claimed keypoint i yet); blocked[i] = its map point has observations -- both overloads skip
// such keypoints (:1389-1393, :59-63), including the ones claimed earlier in the same call.
inline void current_claim_state(const FrameView& current, const MapPointView* mps,
                                int32_t* slot, uint8_t* blocked) {
  for (int i = 0; i < current.n_kps; ++i) {
    const int m = current.map_points[i];
    slot[i] = -1;
    blocked[i] = m >= 0 && mps[m].n_obs > 0;
  }
}
inline void f2f_current_state(const FrameView& current, const MapPointView* mps,
                              int32_t* slot, uint8_t* blocked) {
  current_claim_state(current, mps, slot, blocked);
}

// After a call: the current frame's map point per keypoint -- the queried map point a slot was
// given (F.SetMapPoint(bestIdx, pMP): :1414-1415, :99-100), the previous one elsewhere.
// Returns the number of slots the search assigned.
inline int apply_claims(const std::vector<int32_t>& query_map_point, const int32_t* slot,
                        int32_t* current_map_points, int n) {
  int assigned = 0;
  for (int i = 0; i < n; ++i)
    if (slot[i] >= 0) {
      current_map_points[i] = query_map_point[slot[i]];
      ++assigned;
    }
  return assigned;
}
inline int apply_search_by_projection_frame(const F2FInput& in, const int32_t* slot,
                                            int32_t* current_map_points, int n) {
  return apply_claims(in.query_map_point, slot, current_map_points, n);
}

// The whole call on frame `frame` of the context's last frame / frontend call: gather, claim
// state, slamgpu_search_by_projection_frame, write-back into current_map_points (the frame's
// map point indices, in/out). Returns the reference's nmatches; throws on a device error.
inline int search_by_projection_frame(slamgpu_ctx* ctx, int frame, const FrameView& current,
                                      const FrameView& last, const MapPointView* mps,
                                      float baseline, float th, bool mono, bool check_ori,
                                      int32_t* current_map_points) {
  const F2FInput in = gather_search_by_projection_frame(current, last, mps, baseline, th, mono,
                                                        check_ori);
  std::vector<int32_t> slot(current.n_kps);
  std::vector<uint8_t> blocked(current.n_kps);
  current_claim_state(current, mps, slot.data(), blocked.data());
  int nm = 0;
  const int rc = slamgpu_search_by_projection_frame(ctx, frame, in.queries.data(),
                                                    (int)in.queries.size(), &in.pose, slot.data(),
                                                    blocked.data(), current.n_kps, &nm);
  if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") + slamgpu_last_error(ctx));
  apply_search_by_projection_frame(in, slot.data(), current_map_points, current.n_kps);
  return nm;
}

// ---- OrbMatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (orb_matcher.cpp:13) --

// A map point's tracking fields, MapPoint::track_* as Frame::IsInFrustum (frame.cpp:277-337)
// left them when Tracker::SearchLocalPoints (tracker.cpp:1176-1227) ran it on the current frame.
struct TrackView {
  bool in_view;             // track_is_in_view
  float proj_x, proj_y;     // track_projected_x / _y
  float proj_xr;            // track_projected_x_right
  float view_cos;           // track_view_cos
  int32_t level;            // track_scale_level
};

struct MpsInput {
  std::vector<slamgpu_mps_query> queries;  // one per in-view, not-bad point of vpMapPoints
  std::vector<int32_t> query_map_point;    // map point index of each query (mp_id = position)
};

// The queries of :18-26 in vpMapPoints order (a point that is not in view or is bad does nothing
// in the reference's loop, so it is left out), with the fields the loop reads: the track_*
// values, NumObservations() > 0 (the claim it makes blocks later points, :59-63) and
// GetDescriptor(). `track` is indexed like `mps` (the fields live on the MapPoint).
inline MpsInput gather_search_by_projection_mps(const int32_t* map_points, int n,
                                                const MapPointView* mps, const TrackView* track) {
  MpsInput in;
  for (int i = 0; i < n; ++i) {
    const int m = map_points[i];
    const TrackView& t = track[m];
    if (!t.in_view || mps[m].bad) continue;
    slamgpu_mps_query q{};
    q.proj_x = t.proj_x;
    q.proj_y = t.proj_y;
    q.proj_xr = t.proj_xr;
    q.view_cos = t.view_cos;
    q.level = t.level;
    q.in_view = 1;
    q.is_bad = 0;
    q.mp_id = (int32_t)in.queries.size();
    q.blocks = mps[m].n_obs > 0;
    std::memcpy(q.desc, mps[m].desc, 32);
    in.queries.push_back(q);
    in.query_map_point.push_back(m);
  }
  return in;
}

inline int apply_search_by_projection_mps(const MpsInput& in, const int32_t* slot,
                                          int32_t* current_map_points, int n) {
  return apply_claims(in.query_map_point, slot, current_map_points, n);
}

// The whole call (SearchLocalPoints' matcher.SearchByProjection(current_frame_,
// local_map_points_, th) with OrbMatcher(nnratio)): gather, claim state,
// slamgpu_search_by_projection_mps, write-back. Returns nmatches; throws on a device error.
inline int search_by_projection_mps(slamgpu_ctx* ctx, int frame, const FrameView& current,
                                    const MapPointView* mps, const int32_t* map_points, int n,
                                    const TrackView* track, float nnratio, int th,
                                    int32_t* current_map_points) {
  const MpsInput in = gather_search_by_projection_mps(map_points, n, mps, track);
  std::vector<int32_t> slot(current.n_kps);
  std::vector<uint8_t> blocked(current.n_kps);
  current_claim_state(current, mps, slot.data(), blocked.data());
  int nm = 0;
  const int rc = slamgpu_search_by_projection_mps(ctx, frame, in.queries.data(),
                                                  (int)in.queries.size(), nnratio, th,
                                                  slot.data(), blocked.data(), current.n_kps, &nm);
  if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") + slamgpu_last_error(ctx));
  apply_search_by_projection_mps(in, slot.data(), current_map_points, current.n_kps);
  return nm;
}

// ---- the stereo Frame ctor (frame.cpp:61-111) ----------------------------------------------------

// What the stereo ctor leaves in the Frame: both views' keypoints and descriptors (ExtractORB
// :86-89), the undistorted left keypoints (:96), StereoCoordRight / StereoDepth
// (ComputeStereoMatches :97), map points all null and no outliers (:99-100).
struct StereoFrame {
  int N = 0;                                     // num_keypoints_ (left view)
  std::vector<slamgpu_keypoint> keys, keys_right, undist_keys;
  std::vector<uint8_t> desc, desc_right;         // N x 32, N_right x 32
  std::vector<float> right_coords, depth;        // N each, -1 = no stereo match
  std::vector<int32_t> map_points;               // N x -1
  std::vector<uint8_t> outlier;                  // N x 0
};

// One device context per tracker holding the current frame (frame 0): Make() runs
// slamgpu_frame_stereo (extraction of both views + ComputeStereoMatches + undistortion + the
// grid) and downloads what the Frame keeps; the matchers above then run on the same context
// (frame 0) against the frame's device-resident grid. The context is created on the first call
// and again when the image size changes; the distortion is set once per context.
class StereoFrameCore {
 public:
  StereoFrameCore(const slamgpu_orb_params& params, const slamgpu_camera& cam,
                  const float* dist_coef = nullptr, int n_dist = 0, int device = 0)
      : params_(params), cam_(cam), dist_(dist_coef, dist_coef + (dist_coef ? n_dist : 0)),
        device_(device) {}
  ~StereoFrameCore() { slamgpu_destroy(ctx_); }
  StereoFrameCore(const StereoFrameCore&) = delete;
  StereoFrameCore& operator=(const StereoFrameCore&) = delete;

  // frame.cpp:61-111 on two 8-bit images of the same size and row step. An empty left view
  // leaves N = 0 and the rest empty (:91-94).
  void Make(const uint8_t* left, const uint8_t* right, int rows, int cols, size_t step,
            StereoFrame& f) {
    f = StereoFrame();
    if (!left || !right || rows <= 0 || cols <= 0) return;
    ensure(cols, rows);
    check(slamgpu_frame_stereo(ctx_, left, right, step, &cam_));
    const int cap = slamgpu_kp_capacity(ctx_);
    int n = 0, nr = 0, ns = 0, nu = 0;
    f.keys.resize(cap);
    f.desc.resize((size_t)cap * 32);
    check(slamgpu_download_keypoints(ctx_, 0, f.keys.data(), f.desc.data(), cap, &n));
    f.keys_right.resize(cap);
    f.desc_right.resize((size_t)cap * 32);
    check(slamgpu_download_keypoints(ctx_, 1, f.keys_right.data(), f.desc_right.data(), cap, &nr));
    f.keys.resize(n);
    f.desc.resize((size_t)n * 32);
    f.keys_right.resize(nr);
    f.desc_right.resize((size_t)nr * 32);
    f.N = n;
    if (n == 0) return;
    f.right_coords.resize(n);
    f.depth.resize(n);
    check(slamgpu_download_stereo(ctx_, 0, f.right_coords.data(), f.depth.data(), n, &ns));
    f.undist_keys.resize(n);
    check(slamgpu_download_undistorted_keypoints(ctx_, 0, f.undist_keys.data(), n, &nu));
    if (ns != n || nu != n) throw std::logic_error("slamgpu: inconsistent frame downloads");
    f.map_points.assign(n, -1);
    f.outlier.assign(n, 0);
  }

  // A FrameView of `f` (pose Tcw: 4x4 row-major, caller-owned) for the matchers and
  // PoseOptimization above.
  static FrameView view(const StereoFrame& f, const float* Tcw) {
    FrameView v;
    v.Tcw = Tcw;
    v.kps = f.keys.data();
    v.undist_kps = f.undist_keys.data();
    v.right_coords = f.right_coords.data();
    v.map_points = f.map_points.data();
    v.outlier = f.outlier.data();
    v.n_kps = f.N;
    return v;
  }

  slamgpu_ctx* context() { return ctx_; }

 private:
  void ensure(int cols, int rows) {
    if (ctx_ && cols == cols_ && rows == rows_) return;
    slamgpu_destroy(ctx_);
    ctx_ = nullptr;
    check(slamgpu_create(device_, &params_, cols, rows, 1, &ctx_));
    if (!dist_.empty()) check(slamgpu_set_distortion(ctx_, dist_.data(), (int)dist_.size()));
    cols_ = cols;
    rows_ = rows;
  }
  void check(int rc) const {
    if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") +
                                                   slamgpu_last_error(ctx_));
  }

  slamgpu_orb_params params_;
  slamgpu_camera cam_;
  std::vector<float> dist_;
  int device_;
  slamgpu_ctx* ctx_ = nullptr;
  int cols_ = 0, rows_ = 0;
};


// =================================================================================================
// The keyframe-rate surfaces: SearchByBoW, SearchForTriangulation, Fuse,
// OptimizeSim3 and the global BundleAdjustment, gathered from the same views, called, written back.

// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) as arrays: node ids ascending,
// each node's feature indices in insertion order.
struct FeatureVecView {
  const uint32_t* nodes = nullptr;
  const int32_t* node_start = nullptr;  // [n_nodes + 1]
  const uint32_t* node_feats = nullptr;
  int n_nodes = 0;
};

// What the keyframe-rate matchers read of a KeyFrame beyond KeyFrameView: its descriptors
// (KeyFrame::descriptors), feature_vec, and GetCameraCenter() (the stored Ow).
struct KeyFrameFeatures {
  const uint8_t* desc = nullptr;
  FeatureVecView fv;
  const float* Ow = nullptr;
};

inline void throw_if(int rc, const char* (*msg)(void)) {
  if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") + msg());
}

inline slamgpu_bow_set bow_set(const uint8_t* desc, const slamgpu_keypoint* kps, const uint8_t* valid,
                               int n, const FeatureVecView& fv) {
  slamgpu_bow_set b;
  b.desc = desc;
  b.kps = kps;
  b.valid = valid;
  b.nodes = fv.nodes;
  b.node_start = fv.node_start;
  b.node_feats = fv.node_feats;
  b.n = n;
  b.n_nodes = fv.n_nodes;
  return b;
}

// A keyframe's features whose map point exists and is not bad (the `if(!pMP) continue; if
// (pMP->isBad()) continue;` of both SearchByBoW overloads).
inline std::vector<uint8_t> good_map_point_mask(const KeyFrameView& kf, const MapPointView* mps) {
  std::vector<uint8_t> v(kf.n_kps);
  for (int i = 0; i < kf.n_kps; ++i) v[i] = kf.map_points[i] >= 0 && !mps[kf.map_points[i]].bad;
  return v;
}

// ---- OrbMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&) (orb_matcher.cpp:
// 133-262): Tracker::TrackReferenceKeyFrame (tracker.cpp:666, OrbMatcher(0.7, true)) and the
// relocalisation (:860, 0.75). map_point_matches[j] = the keyframe map point matched to frame
// keypoint j, or -1 (the vpMapPointMatches the caller then gives to Frame::SetMapPoints).
inline int search_by_bow(const KeyFrameView& kf, const KeyFrameFeatures& kff,
                         const MapPointView* mps, const slamgpu_keypoint* f_keys,
                         const uint8_t* f_desc, int f_n, const FeatureVecView& f_fv,
                         float nnratio, bool check_ori, std::vector<int32_t>& map_point_matches) {
  const std::vector<uint8_t> valid = good_map_point_mask(kf, mps);
  const slamgpu_bow_set a = bow_set(kff.desc, kf.undist_kps, valid.data(), kf.n_kps, kff.fv);
  const slamgpu_bow_set b = bow_set(f_desc, f_keys, nullptr, f_n, f_fv);
  std::vector<int32_t> match(kf.n_kps > 0 ? kf.n_kps : 1);
  int nm = 0;
  throw_if(slamgpu_search_by_bow(&a, &b, 0, nnratio, check_ori ? 1 : 0, match.data(), &nm),
           slamgpu_bow_last_error);
  map_point_matches.assign(f_n, -1);
  for (int i = 0; i < kf.n_kps; ++i)
    if (match[i] >= 0) map_point_matches[match[i]] = kf.map_points[i];
  return nm;
}

// ---- OrbMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
// (orb_matcher.cpp:499-632): LoopCloser::ComputeSim3 (loop_closer.cpp:327, OrbMatcher(0.75,
// true)). matches12[i] = pKF2's map point matched to pKF1 feature i, or -1.
inline int search_by_bow(const KeyFrameView& kf1, const KeyFrameFeatures& f1,
                         const KeyFrameView& kf2, const KeyFrameFeatures& f2,
                         const MapPointView* mps, float nnratio, bool check_ori,
                         std::vector<int32_t>& matches12) {
  const std::vector<uint8_t> v1 = good_map_point_mask(kf1, mps), v2 = good_map_point_mask(kf2, mps);
  const slamgpu_bow_set a = bow_set(f1.desc, kf1.undist_kps, v1.data(), kf1.n_kps, f1.fv);
  const slamgpu_bow_set b = bow_set(f2.desc, kf2.undist_kps, v2.data(), kf2.n_kps, f2.fv);
  std::vector<int32_t> match(kf1.n_kps > 0 ? kf1.n_kps : 1);
  int nm = 0;
  throw_if(slamgpu_search_by_bow(&a, &b, 1, nnratio, check_ori ? 1 : 0, match.data(), &nm),
           slamgpu_bow_last_error);
  matches12.assign(kf1.n_kps, -1);
  for (int i = 0; i < kf1.n_kps; ++i)
    if (match[i] >= 0) matches12[i] = kf2.map_points[match[i]];
  return nm;
}

// The matchers' record of one keyframe (pose split as KeyFrame::GetRotation / GetTranslation
// return it; has_mp[i] = GetMapPoint(i) != NULL, bad or not, as SearchForTriangulation tests it).
struct KfRecord {
  slamgpu_kf kf;
  std::vector<uint8_t> has_mp;
};
inline KfRecord kf_record(const KeyFrameView& v, const KeyFrameFeatures& f) {
  KfRecord r;
  r.has_mp.resize(v.n_kps > 0 ? v.n_kps : 1);
  for (int i = 0; i < v.n_kps; ++i) r.has_mp[i] = v.map_points[i] >= 0;
  slamgpu_kf& k = r.kf;
  std::memset(&k, 0, sizeof(k));
  k.kps = v.undist_kps;
  k.desc = f.desc;
  k.u_right = v.right_coords;
  k.has_mp = r.has_mp.data();
  k.nodes = f.fv.nodes;
  k.node_start = f.fv.node_start;
  k.node_feats = f.fv.node_feats;
  k.n = v.n_kps;
  k.n_nodes = f.fv.n_nodes;
  for (int r0 = 0; r0 < 3; ++r0) {
    for (int c = 0; c < 3; ++c) k.Rcw[3 * r0 + c] = v.Tcw[4 * r0 + c];
    k.tcw[r0] = v.Tcw[4 * r0 + 3];
    k.Ow[r0] = f.Ow[r0];
  }
  return r;
}

// ---- OrbMatcher::SearchForTriangulation (orb_matcher.cpp:634-802) as LocalMapper::
// CreateNewMapPoints calls it (local_mapper.cpp:312, OrbMatcher(0.6, false), only_stereo =
// false): F12 from LocalMapper::ComputeFundamentalMatrix; cam / lv = pKF2's calibration and
// level tables. Returns vMatchedPairs: (pKF1 index, pKF2 index), ascending pKF1 index.
inline std::vector<std::pair<int, int>> search_for_triangulation(
    const KeyFrameView& kf1, const KeyFrameFeatures& f1, const KeyFrameView& kf2,
    const KeyFrameFeatures& f2, const float F12[9], const slamgpu_camera& cam,
    const slamgpu_levels& lv, bool only_stereo, bool check_ori) {
  const KfRecord r1 = kf_record(kf1, f1), r2 = kf_record(kf2, f2);
  std::vector<int32_t> match(kf1.n_kps > 0 ? kf1.n_kps : 1);
  int nm = 0;
  throw_if(slamgpu_search_for_triangulation(&r1.kf, &r2.kf, F12, &cam, &lv, only_stereo ? 1 : 0,
                                            check_ori ? 1 : 0, match.data(), &nm),
           slamgpu_kfmatch_last_error);
  std::vector<std::pair<int, int>> pairs;
  for (int i = 0; i < kf1.n_kps; ++i)
    if (match[i] >= 0) pairs.emplace_back(i, match[i]);
  return pairs;
}

// ---- LocalMapper::ComputeFundamentalMatrix (local_mapper.cpp:615-630) under the cv::Mat rules
// of DESIGN.md "CreateNewMapPoints": a product is a double sum over ascending k rounded to float
// once, a chain runs left to right as written (R12 = R1w * R2w.t(); t12 = ((-R1w) * R2w.t()) *
// t2w + t1w; F12 = ((K1.t().inv() * t12x) * R12) * K2.inv()), inv() of a 3 x 3 is the closed
// (cofactor) form in double rounded once. K = fx, fy, cx, cy of slamgpu_camera.
inline void cv_mat3_mul(const float* a, const float* b, float* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc += (double)a[3 * i + k] * (double)b[3 * k + j];
      c[3 * i + j] = (float)acc;
    }
}
inline void cv_mat3_inv(const float* a, float* o) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6],
               a7 = a[7], a8 = a[8];
  const double det = a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6) + a2 * (a3 * a7 - a4 * a6);
  o[0] = (float)((a4 * a8 - a5 * a7) / det);
  o[1] = (float)((a2 * a7 - a1 * a8) / det);
  o[2] = (float)((a1 * a5 - a2 * a4) / det);
  o[3] = (float)((a5 * a6 - a3 * a8) / det);
  o[4] = (float)((a0 * a8 - a2 * a6) / det);
  o[5] = (float)((a2 * a3 - a0 * a5) / det);
  o[6] = (float)((a3 * a7 - a4 * a6) / det);
  o[7] = (float)((a1 * a6 - a0 * a7) / det);
  o[8] = (float)((a0 * a4 - a1 * a3) / det);
}
inline void compute_fundamental_matrix(const KeyFrameView& kf1, const KeyFrameView& kf2,
                                       const slamgpu_camera& K1, const slamgpu_camera& K2,
                                       float F12[9]) {
  float R1[9], R2t[9], nR1[9], t1[3], t2[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      R1[3 * r + c] = kf1.Tcw[4 * r + c];
      nR1[3 * r + c] = -kf1.Tcw[4 * r + c];
      R2t[3 * c + r] = kf2.Tcw[4 * r + c];
    }
    t1[r] = kf1.Tcw[4 * r + 3];
    t2[r] = kf2.Tcw[4 * r + 3];
  }
  float R12[9], m[9], t12[3];
  cv_mat3_mul(R1, R2t, R12);
  cv_mat3_mul(nR1, R2t, m);
  for (int i = 0; i < 3; ++i) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) acc += (double)m[3 * i + k] * (double)t2[k];
    t12[i] = (float)acc + t1[i];
  }
  const float t12x[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
  const float K1t[9] = {K1.fx, 0.0f, 0.0f, 0.0f, K1.fy, 0.0f, K1.cx, K1.cy, 1.0f};
  const float K2m[9] = {K2.fx, 0.0f, K2.cx, 0.0f, K2.fy, K2.cy, 0.0f, 0.0f, 1.0f};
  float K1ti[9], K2i[9], a[9], b[9];
  cv_mat3_inv(K1t, K1ti);
  cv_mat3_inv(K2m, K2i);
  cv_mat3_mul(K1ti, t12x, a);
  cv_mat3_mul(a, R12, b);
  cv_mat3_mul(b, K2i, F12);
}

// ---- LocalMapper::CreateNewMapPoints (local_mapper.cpp:258-492) ----------------------------------
// What it reads of a KeyFrame beyond KeyFrameView and KeyFrameFeatures: depths, the raw keypoints
// (UnprojectStereo, keyframe.cpp:478-492), fx fy cx cy mbf and mb.
struct KeyFrameStereo {
  const float* depths = nullptr;
  const slamgpu_keypoint* kps = nullptr;  // KeyFrame::keypoints; nullptr = undistorted_keypoints
  slamgpu_camera cam = {0, 0, 0, 0, 0};
  float mb = 0;
};

// One `new MapPoint(x3D, current_keyframe_, map_)` with what :478-488 then does to it, for the
// caller to replay: AddObservation(kfs[kf1], idx1), AddObservation(kfs[kf2], idx2), AddMapPoint on
// both keyframes, descriptor (ComputeDistinctiveDescriptors), normal and min / max distance
// (UpdateNormalAndDepth), Map::AddMapPoint, recently_added_map_points_.push_back.
struct NewPoint {
  float xyz[3];
  int32_t kf1, idx1, kf2, idx2;
  uint8_t desc[32];
  float normal[3];
  float min_dist, max_dist;
  int32_t source;  // SLAMGPU_NP_DLT / _STEREO1 / _STEREO2
};
struct NewPointsResult {
  std::vector<NewPoint> points;     // in the reference's order: neighbour, then vMatchedIndices
  std::vector<uint8_t> skipped;     // [n_neighbours] the baseline test (:290-304) dropped it
  std::vector<int8_t> status;       // [n_neighbours][n_kps of the current keyframe] SLAMGPU_NP_*
  int n_kps = 0;
};

// neighbours: GetBestCovisibilityKeyFrames(is_monocular ? 20 : 10) as keyframe indices.
// median_depth[k]: neighbour k's ComputeSceneMedianDepth(2), read only when is_monocular.
// first_obs[k]: 0 when the current keyframe precedes neighbour k in a std::map<KeyFrame*, size_t>
// (its address is the lower one), 1 otherwise: with two observations ComputeDistinctiveDescriptors
// keeps the first entry's descriptor (map_point.cpp:287-298, both medians 0, strict <).
// The baseline tests run here, everything else in one slamgpu_create_new_map_points call with
// OrbMatcher(0.6f, false)'s check_ori = false. The reference's `if (i > 0 &&
// CheckNewKeyFrames()) return;` (:285) maps to "use the rows of the first k neighbours": a
// neighbour's points and status row do not depend on later neighbours, so a caller that sees a
// new keyframe arrive applies points[.kf2 among the first k neighbours] and drops the rest, or
// passes only the neighbours it wants. The search reads one calibration for all neighbours (the
// first neighbour's; keyframes of one sensor share it).
inline NewPointsResult create_new_map_points(int cur, const KeyFrameView* kfs,
                                             const KeyFrameFeatures* features,
                                             const KeyFrameStereo* stereo, const int32_t* neighbours,
                                             int n_neighbours, bool is_monocular,
                                             const float* median_depth, const int32_t* first_obs,
                                             const slamgpu_levels& lv, bool check_ori = false) {
  NewPointsResult out;
  const KeyFrameView& K1 = kfs[cur];
  out.n_kps = K1.n_kps;
  out.skipped.assign(n_neighbours > 0 ? n_neighbours : 0, 0);
  out.status.assign((size_t)(n_neighbours > 0 ? n_neighbours : 0) * K1.n_kps, 0);
  if (n_neighbours <= 0) return out;
  std::vector<KfRecord> rec;
  rec.reserve(1 + n_neighbours);
  std::vector<slamgpu_kf> hk(1 + n_neighbours);
  std::vector<slamgpu_kf_stereo> hs(1 + n_neighbours);
  std::vector<slamgpu_newpoints_nbor> nb(n_neighbours);
  for (int k = -1; k < n_neighbours; ++k) {
    const int idx = k < 0 ? cur : neighbours[k];
    rec.push_back(kf_record(kfs[idx], features[idx]));
    hk[k + 1] = rec.back().kf;
    hs[k + 1].depth = stereo[idx].depths;
    hs[k + 1].raw_kps = stereo[idx].kps;
    hs[k + 1].cam = stereo[idx].cam;
    hs[k + 1].mb = stereo[idx].mb;
  }
  const float* O1 = features[cur].Ow;
  for (int k = 0; k < n_neighbours; ++k) {
    const int idx = neighbours[k];
    const float* O2 = features[idx].Ow;
    double s = 0.0;  // cv::norm(nbor_pos - current_pos) (:292)
    for (int c = 0; c < 3; ++c) {
      const float d = O2[c] - O1[c];
      s += (double)d * (double)d;
    }
    const float baseline = (float)std::sqrt(s);
    bool skip;
    if (is_monocular) skip = baseline / median_depth[k] < 0.01f;  // :294-299
    else skip = baseline < stereo[idx].mb;                        // :300-304
    out.skipped[k] = skip;
    std::memset(&nb[k], 0, sizeof(nb[k]));
    nb[k].kf2 = 1 + k;
    nb[k].skip = skip ? 1 : 0;
    nb[k].first_obs = first_obs[k];
    if (!skip) compute_fundamental_matrix(K1, kfs[idx], stereo[cur].cam, stereo[idx].cam, nb[k].F12);
  }
  const int n1 = K1.n_kps;
  std::vector<uint8_t> has_mp1(rec[0].has_mp);
  std::vector<slamgpu_fuse_point> pts(n1 > 0 ? n1 : 1);
  std::vector<slamgpu_new_point> news(n1 > 0 ? n1 : 1);
  int n_new = 0;
  throw_if(slamgpu_create_new_map_points(hk.data(), hs.data(), nb.data(), n_neighbours,
                                         &stereo[neighbours[0]].cam, &lv, check_ori ? 1 : 0,
                                         has_mp1.data(), pts.data(), news.data(),
                                         out.status.empty() ? nullptr : out.status.data(), &n_new),
           slamgpu_kfmatch_last_error);
  if (n_new < 0)
    throw std::runtime_error("slamgpu: create_new_map_points: a keyframe the search cannot take");
  out.points.resize(n_new);
  for (int i = 0; i < n_new; ++i) {
    NewPoint& p = out.points[i];
    for (int c = 0; c < 3; ++c) {
      p.xyz[c] = pts[i].xyz[c];
      p.normal[c] = pts[i].normal[c];
    }
    p.kf1 = cur;
    p.idx1 = news[i].idx1;
    p.kf2 = neighbours[news[i].neighbour];
    p.idx2 = news[i].idx2;
    std::memcpy(p.desc, pts[i].desc, 32);
    p.min_dist = pts[i].min_dist;
    p.max_dist = pts[i].max_dist;
    p.source = news[i].source;
  }
  return out;
}

// ---- OrbMatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)
// (orb_matcher.cpp:804-954), LocalMapper::SearchInNeighbors (local_mapper.cpp:521, 540).
// What Fuse reads of a map point beyond MapPointView: GetNormal(), min_dist_ / max_dist_ and
// NumObservations() (the stereo-weighted count AddObservation keeps, map_point.cpp:114-125).
struct MapPointGeometry {
  float normal[3];
  float min_dist, max_dist;
  int32_t num_observations;
};

// The object-graph changes of one Fuse call, in the reference's order, for the caller to apply
// to its MapPoints / KeyFrame:
//   kReplaceByKf:  point->Replace(other)   (other = the keyframe's map point, more observations)
//   kReplaceKf:    other->Replace(point)
//   kAdd:          point->AddObservation(pKF, keypoint); pKF->AddMapPoint(point, keypoint)
//   kNone:         the keyframe's map point at keypoint is bad: nothing (still counted as fused)
struct FuseAction {
  enum Kind : int32_t { kNone = 0, kReplaceByKf = 1, kReplaceKf = 2, kAdd = 3 };
  int32_t kind, point, other, keypoint;
};
struct FuseResult {
  int nfused = 0;
  std::vector<FuseAction> actions;
};

// The reference checks isBad() and IsInKeyFrame(pKF) of each offered point when the loop reaches
// it, after the Replace / AddObservation calls of earlier points (:821-828). The device search
// of a point does not depend on those calls (it reads the keyframe's keypoints, not its map
// points), so the candidates are searched once with the skip state at the start, and the walk
// below replays the loop on a model of the state those calls change: bad flags, the keyframe's
// slots, each touched point's keyframes and observation count (Replace, map_point.cpp:190-226:
// the survivor takes the other's observations in keyframes it is not in and the other's slot
// there; where both were, the keyframe drops the replaced point's slot).
inline FuseResult fuse(int kf_index, const KeyFrameView* kfs, const KeyFrameFeatures& kff,
                       const MapPointView* mps, const MapPointGeometry* geom, int n_mp,
                       const int32_t* points, int n_points, float th, const slamgpu_camera& cam,
                       const slamgpu_levels& lv, const slamgpu_kf_grid& grid) {
  const KeyFrameView& kf = kfs[kf_index];
  auto in_kf0 = [&](int m) {
    for (int o = 0; o < mps[m].n_obs; ++o)
      if (mps[m].obs[o].keyframe == kf_index) return true;
    return false;
  };
  std::vector<slamgpu_fuse_point> pts(n_points > 0 ? n_points : 1);
  for (int i = 0; i < n_points; ++i) {
    slamgpu_fuse_point& q = pts[i];
    std::memset(&q, 0, sizeof(q));
    const int m = points[i];
    q.skip = m < 0 || mps[m].bad || in_kf0(m);
    if (m < 0) continue;
    std::memcpy(q.xyz, mps[m].xyz, sizeof(q.xyz));
    std::memcpy(q.normal, geom[m].normal, sizeof(q.normal));
    q.min_dist = geom[m].min_dist;
    q.max_dist = geom[m].max_dist;
    std::memcpy(q.desc, mps[m].desc, 32);
  }
  const KfRecord rec = kf_record(kf, kff);
  std::vector<int32_t> best(n_points > 0 ? n_points : 1), dist(n_points > 0 ? n_points : 1);
  int nf = 0;
  throw_if(slamgpu_fuse(&rec.kf, pts.data(), n_points, th, &cam, &lv, &grid, best.data(),
                        dist.data(), &nf),
           slamgpu_kfmatch_last_error);
  // the model: touched points' keyframe -> keypoint maps, counts and bad flags
  std::vector<uint8_t> bad(n_mp);
  std::vector<int32_t> nobs(n_mp);
  std::vector<std::vector<ObsRef>> obs(n_mp);
  std::vector<uint8_t> loaded(n_mp, 0);
  for (int m = 0; m < n_mp; ++m) {
    bad[m] = mps[m].bad;
    nobs[m] = geom[m].num_observations;
  }
  auto load = [&](int m) -> std::vector<ObsRef>& {
    if (!loaded[m]) {
      obs[m].assign(mps[m].obs, mps[m].obs + mps[m].n_obs);
      loaded[m] = 1;
    }
    return obs[m];
  };
  std::vector<int32_t> slot(kf.map_points, kf.map_points + kf.n_kps);  // pKF->GetMapPoint(i)
  auto find = [](const std::vector<ObsRef>& o, int k) {
    for (size_t j = 0; j < o.size(); ++j)
      if (o[j].keyframe == k) return (int)j;
    return -1;
  };
  auto weight = [&](int k, int idx) { return kfs[k].right_coords[idx] >= 0 ? 2 : 1; };
  // this->Replace(point): map_point.cpp:190-226, on the model
  auto replace = [&](int victim, int survivor) {
    if (victim == survivor) return;
    bad[victim] = 1;
    std::vector<ObsRef>& vo = load(victim);
    std::vector<ObsRef>& so = load(survivor);
    for (const ObsRef& r : vo) {
      if (find(so, r.keyframe) < 0) {  // ReplaceMapPointMatch + AddObservation
        if (r.keyframe == kf_index) slot[r.keypoint] = survivor;
        so.push_back(r);
        nobs[survivor] += weight(r.keyframe, r.keypoint);
      } else if (r.keyframe == kf_index) {  // EraseMapPointMatch
        slot[r.keypoint] = -1;
      }
    }
    vo.clear();
  };
  FuseResult res;
  for (int i = 0; i < n_points; ++i) {
    const int m = points[i];
    if (m < 0 || bad[m] || find(load(m), kf_index) >= 0) continue;  // :821-828
    if (best[i] < 0) continue;                                       // bestDist > TH_LOW
    const int j = best[i], cur = slot[j];
    FuseAction a{FuseAction::kNone, m, cur, j};
    if (cur >= 0) {
      if (!bad[cur]) {
        if (nobs[cur] > nobs[m]) {
          a.kind = FuseAction::kReplaceByKf;
          replace(m, cur);
        } else {
          a.kind = FuseAction::kReplaceKf;
          replace(cur, m);
        }
      }
    } else {
      a.kind = FuseAction::kAdd;
      load(m).push_back(ObsRef{kf_index, j});
      nobs[m] += weight(kf_index, j);
      slot[j] = m;
    }
    res.actions.push_back(a);
    res.nfused++;
  }
  return res;
}

// ---- Optimizer::OptimizeSim3 (optimizer.cpp:962-1152), LoopCloser::ComputeSim3
// (loop_closer.cpp:393): the correspondences of :1020-1096 -- match i kept when both map points
// exist, are not bad and pKF2 observes the second (GetIndexInKeyFrame(pKF2) >= 0) -- with the
// points in their keyframes' camera frames as the f32 cv::Mat expression R*X + t forms them
// (one gemm: float dot, then (float)((double)dot + (double)t)).
struct Sim3Problem {
  std::vector<slamgpu_sim3_match> matches;
  std::vector<int32_t> match_index;  // i of each correspondence
};
inline float cv_gemm_row(const float* T, int r, const float* x) {
  const float dot = T[4 * r] * x[0] + T[4 * r + 1] * x[1] + T[4 * r + 2] * x[2];
  return (float)((double)dot + (double)T[4 * r + 3]);
}
inline Sim3Problem gather_optimize_sim3(int kf1_index, int kf2_index, const KeyFrameView* kfs,
                                        const MapPointView* mps, const int32_t* matches1, int n) {
  const KeyFrameView& kf1 = kfs[kf1_index];
  const KeyFrameView& kf2 = kfs[kf2_index];
  Sim3Problem p;
  for (int i = 0; i < n; ++i) {
    const int m2 = matches1[i];
    if (m2 < 0) continue;
    const int m1 = kf1.map_points[i];
    if (m1 < 0) continue;
    int i2 = -1;
    for (int o = 0; o < mps[m2].n_obs; ++o)
      if (mps[m2].obs[o].keyframe == kf2_index) i2 = mps[m2].obs[o].keypoint;
    if (mps[m1].bad || mps[m2].bad || i2 < 0) continue;
    slamgpu_sim3_match c;
    for (int r = 0; r < 3; ++r) {
      c.x1c[r] = cv_gemm_row(kf1.Tcw, r, mps[m1].xyz);
      c.x2c[r] = cv_gemm_row(kf2.Tcw, r, mps[m2].xyz);
    }
    c.u1 = kf1.undist_kps[i].x;
    c.v1 = kf1.undist_kps[i].y;
    c.u2 = kf2.undist_kps[i2].x;
    c.v2 = kf2.undist_kps[i2].y;
    c.octave1 = kf1.undist_kps[i].octave;
    c.octave2 = kf2.undist_kps[i2].octave;
    p.matches.push_back(c);
    p.match_index.push_back(i);
  }
  return p;
}
// The whole call: matches1 (vpMatches1: pKF2's map point per pKF1 feature, -1 none) is updated
// as the reference nulls its outliers (:1103-1106, :1135-1140; also on the early return); S12
// (qx, qy, qz, qw, tx, ty, tz, s) is updated unless the reference returns early. Returns nIn.
inline int optimize_sim3(int kf1_index, int kf2_index, const KeyFrameView* kfs,
                         const MapPointView* mps, int32_t* matches1, int n, const float K1[4],
                         const float K2[4], const float* inv_sigma2_1, const float* inv_sigma2_2,
                         int nlevels, double S12[8], float th2, bool fix_scale) {
  const Sim3Problem p = gather_optimize_sim3(kf1_index, kf2_index, kfs, mps, matches1, n);
  std::vector<uint8_t> inl(p.matches.size() + 1, 1);
  int n_in = 0;
  throw_if(slamgpu_optimize_sim3(K1, K2, inv_sigma2_1, inv_sigma2_2, nlevels, p.matches.data(),
                                 (int)p.matches.size(), th2, fix_scale ? 1 : 0, S12, inl.data(),
                                 &n_in),
           slamgpu_optimizer_last_error);
  for (size_t c = 0; c < p.matches.size(); ++c)
    if (!inl[c]) matches1[p.match_index[c]] = -1;
  return n_in;
}

// ---- Sim3Solver (src/solvers/sim3solver.h, sim3solver.cpp), LoopCloser::ComputeSim3
// (loop_closer.cpp:336-376) ---------------------------------------------------------------------
// The effective mRansacMaxIts of SetRansacParameters (:127-137), host libm as the reference: float
// epsilon, std::pow(float, int) and std::log in double, N == minInliers -> 1. A quotient that is
// no positive int (epsilon >= 1, or 0) is what the reference's x86 build converts to INT_MIN.
inline int sim3_ransac_iterations(int N, double probability, int minInliers, int maxIterations) {
  const float epsilon = (float)minInliers / N;
  int nIterations;
  if (minInliers == N) {
    nIterations = 1;
  } else {
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
    nIterations = v >= 1.0 && v <= 2147483647.0 ? (int)v : INT_MIN;
  }
  return std::max(1, std::min(nIterations, maxIterations));
}

// DUtils::Random::RandomInt (DUtils/Random.cpp:47-50) on the C library's rand().
inline int reference_random_int(int min, int max) {
  const int d = max - min + 1;
  return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

// The reference class's surface over the views. The constructor does the gather of :64-105
// (mvnIndices1 and the skip rules: no map point on either side, a bad one, GetIndexInKeyFrame < 0)
// and, like the reference's, evaluates nothing. SetRansacParameters draws the WHOLE schedule with
// the functor -- in the order the reference would consume the draws for this solver alone; several
// interleaved solvers consume rand() in another global order than the reference's lazy draws,
// which is why the draws are an input of the C ABI -- and makes the one synchronous call.
// iterate / find then replay :142-217 from the per-hypothesis counts and the events. The
// constructor's default parameters (0.99, 6, 300) are evaluated by the first iterate if
// SetRansacParameters was never called.
class Sim3SolverCore {
 public:
  using RandomInt = std::function<int(int, int)>;

  Sim3SolverCore(int kf1_index, int kf2_index, const KeyFrameView* kfs, const MapPointView* mps,
                 const int32_t* vpMatched12, int n_matched, const float K1[4], const float K2[4],
                 const float* sigma2_1, const float* sigma2_2, int nlevels, bool bFixScale,
                 RandomInt random_int = reference_random_int)
      : mN1_(n_matched), fix_scale_(bFixScale), nlevels_(nlevels),
        sigma2_1_(sigma2_1, sigma2_1 + nlevels), sigma2_2_(sigma2_2, sigma2_2 + nlevels),
        random_int_(std::move(random_int)) {
    std::memcpy(K1_, K1, sizeof K1_);
    std::memcpy(K2_, K2, sizeof K2_);
    const KeyFrameView& kf1 = kfs[kf1_index];
    const KeyFrameView& kf2 = kfs[kf2_index];
    auto index_in = [&](int m, int kf) {  // MapPoint::GetIndexInKeyFrame
      for (int o = 0; o < mps[m].n_obs; ++o)
        if (mps[m].obs[o].keyframe == kf) return (int)mps[m].obs[o].keypoint;
      return -1;
    };
    for (int i1 = 0; i1 < n_matched; ++i1) {
      const int m2 = vpMatched12[i1];
      if (m2 < 0) continue;
      const int m1 = kf1.map_points[i1];
      if (m1 < 0) continue;
      if (mps[m1].bad || mps[m2].bad) continue;
      const int i_kf1 = index_in(m1, kf1_index), i_kf2 = index_in(m2, kf2_index);
      if (i_kf1 < 0 || i_kf2 < 0) continue;
      const slamgpu_keypoint& kp1 = kf1.undist_kps[i_kf1];
      const slamgpu_keypoint& kp2 = kf2.undist_kps[i_kf2];
      slamgpu_sim3_match c;
      for (int r = 0; r < 3; ++r) {
        c.x1c[r] = cv_gemm_row(kf1.Tcw, r, mps[m1].xyz);
        c.x2c[r] = cv_gemm_row(kf2.Tcw, r, mps[m2].xyz);
      }
      c.u1 = kp1.x, c.v1 = kp1.y, c.u2 = kp2.x, c.v2 = kp2.y;
      c.octave1 = kp1.octave;
      c.octave2 = kp2.octave;
      matches_.push_back(c);
      indices1_.push_back(i1);
    }
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    prob_ = probability, min_inliers_ = minInliers, max_its_arg_ = maxIterations;
    const int N = (int)matches_.size();
    max_its_ = sim3_ransac_iterations(N, probability, minInliers, maxIterations);
    iterations_ = 0;
    evaluated_ = true;
    draws_.clear();
    hyp_.clear();
    bits_.clear();
    events_.clear();
    if (N < minInliers) return;  // iterate returns at once (:151-154): nothing is drawn
    if (N < 3) throw std::runtime_error("slamgpu: Sim3Solver needs 3 correspondences");
    for (int k = 0; k < max_its_; ++k)
      for (int i = 0; i < 3; ++i) draws_.push_back(random_int_(0, N - 1 - i));
    words_ = SLAMGPU_SIM3_MASK_WORDS(N);
    hyp_.resize(max_its_);
    bits_.resize((size_t)max_its_ * words_);
    events_.resize(max_its_);
    int ne = 0;
    throw_if(slamgpu_sim3_ransac(K1_, K2_, sigma2_1_.data(), sigma2_2_.data(), nlevels_,
                                 matches_.data(), N, draws_.data(), max_its_, minInliers,
                                 fix_scale_ ? 1 : 0, hyp_.data(), bits_.data(), events_.data(),
                                 &ne),
             slamgpu_sim3solver_last_error);
    events_.resize(ne);
  }

  // iterate (:142-211): the 0-based iteration whose transform the reference returns (T12 below
  // gives the matrix), or -1 for its empty cv::Mat.
  int iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    if (!evaluated_) SetRansacParameters(prob_, min_inliers_, max_its_arg_);
    bNoMore = false;
    vbInliers.assign(mN1_, false);
    nInliers = 0;
    const int N = (int)matches_.size();
    if (N < min_inliers_) {
      bNoMore = true;
      return -1;
    }
    const int start = iterations_;
    const int end = std::min(max_its_, start + std::max(nIterations, 0));
    size_t j = 0;
    while (j < events_.size() && events_[j] < start) ++j;
    if (j < events_.size() && events_[j] < end) {
      const int k = events_[j];
      iterations_ = k + 1;
      nInliers = hyp_[k].n_inliers;
      for (int i = 0; i < N; ++i)
        if (bits_[(size_t)k * words_ + i / 64] >> (i % 64) & 1) vbInliers[indices1_[i]] = true;
      return k;
    }
    iterations_ = end;
    if (iterations_ >= max_its_) bNoMore = true;
    return -1;
  }
  // find (:213-217)
  int find(std::vector<bool>& vbInliers12, int& nInliers) {
    if (!evaluated_) SetRansacParameters(prob_, min_inliers_, max_its_arg_);
    bool flag;
    return iterate(max_its_, flag, vbInliers12, nInliers);
  }

  // mT12i of iteration k, 4x4 row-major: [ms12i * mR12i | mt12i; 0 0 0 1] (:325-330).
  void T12(int k, float T[16]) const {
    const slamgpu_sim3_hyp& h = hyp_[k];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[4 * r + c] = h.s12 * h.R12[3 * r + c];
      T[4 * r + 3] = h.t12[r];
      T[12 + r] = 0.0f;
    }
    T[15] = 1.0f;
  }

  // mBestRotation / mBestTranslation / mBestScale as the reference leaves them, also after a call
  // that returned nothing: the last iteration, among those run, that reached the running maximum
  // (the >= of :186). false while the reference's matrices are still empty.
  bool GetEstimatedRotation(float R[9]) const {
    const int k = best();
    if (k >= 0) std::memcpy(R, hyp_[k].R12, sizeof(float) * 9);
    return k >= 0;
  }
  bool GetEstimatedTranslation(float t[3]) const {
    const int k = best();
    if (k >= 0) std::memcpy(t, hyp_[k].t12, sizeof(float) * 3);
    return k >= 0;
  }
  float GetEstimatedScale() const {
    const int k = best();
    return k >= 0 ? hyp_[k].s12 : 0.0f;
  }

  const std::vector<slamgpu_sim3_match>& matches() const { return matches_; }
  const std::vector<int32_t>& indices1() const { return indices1_; }  // mvnIndices1
  const std::vector<int32_t>& draws() const { return draws_; }
  const slamgpu_sim3_hyp& hypothesis(int k) const { return hyp_[k]; }
  int max_iterations() const { return max_its_; }  // the effective mRansacMaxIts

 private:
  int best() const {
    int k = -1, n = 0;
    for (int i = 0; i < iterations_ && i < (int)hyp_.size(); ++i)
      if (hyp_[i].n_inliers >= n) n = hyp_[i].n_inliers, k = i;
    return k;
  }

  int mN1_;
  bool fix_scale_;
  int nlevels_;
  float K1_[4], K2_[4];
  std::vector<float> sigma2_1_, sigma2_2_;
  RandomInt random_int_;
  std::vector<slamgpu_sim3_match> matches_;
  std::vector<int32_t> indices1_;
  double prob_ = 0.99;
  int min_inliers_ = 6, max_its_arg_ = 300, max_its_ = 300;
  bool evaluated_ = false;
  int iterations_ = 0;  // mnIterations
  int words_ = 0;
  std::vector<int32_t> draws_, events_;
  std::vector<slamgpu_sim3_hyp> hyp_;
  std::vector<uint64_t> bits_;
};

// ---- PnPsolver (src/solvers/pnp_solver.h, pnp_solver.cpp), Tracker::Relocalization
// (tracker.cpp:826-991) ---------------------------------------------------------------------------
// The effective mRansacMinInliers and mRansacMaxIts of SetRansacParameters (:87-105), host libm
// as the reference: int(N * float epsilon), the two lower bounds, the float epsilon raised to
// minInliers / N, std::pow(float, int) and std::log in double, N == minInliers -> 1. A quotient
// that is no positive int is what the reference's x86 build converts to INT_MIN. The sample is
// four points: any other minSet throws.
struct PnpRansacParameters {
  int min_inliers, max_its;
};
inline PnpRansacParameters pnp_ransac_parameters(int N, double probability, int minInliers,
                                                 int maxIterations, int minSet, float epsilon) {
  if (minSet != 4)
    throw std::invalid_argument("slamgpu: PnPsolver minSet " + std::to_string(minSet) +
                                " is not supported, the sample is 4 points");
  int nMinInliers = (int)(N * epsilon);
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
  int nIterations;
  if (nMinInliers == N) {
    nIterations = 1;
  } else {
    const double v =
        std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
    nIterations = v >= 1.0 && v <= 2147483647.0 ? (int)v : INT_MIN;
  }
  return {nMinInliers, std::max(1, std::min(nIterations, maxIterations))};
}

// The reference class's surface over the views. The constructor does the gather of :32-54
// (mvP2D, the octave mvSigma2 is looked up with, mvP3Dw, mvKeyPointIndices; map points that are
// absent or bad are skipped) and, unlike the reference's, evaluates nothing: the default
// parameters (0.99, 8, 300, 4, 0.4, 5.991) are evaluated by the first iterate if
// SetRansacParameters was never called. SetRansacParameters draws the WHOLE schedule with the
// functor -- in the order the reference would consume the draws for this solver alone (see
// Sim3SolverCore) -- and makes the one synchronous call. iterate / find then replay :112-211 from
// the counts, the running bests, the refined rows and the events. The loop of :135 runs while
// mnIterations < mRansacMaxIts OR the call's own count < nIterations, so a call that starts near
// the end runs past the schedule: the core appends draws and evaluates the longer schedule again
// (the prefix is the same draws, hence the same rows; nothing is carried in).
class PnPSolverCore {
 public:
  using RandomInt = std::function<int(int, int)>;

  PnPSolverCore(const FrameView& F, const MapPointView* mps, const int32_t* vpMapPointMatches,
                int n_matches, const float K[4], const float* sigma2, int nlevels,
                RandomInt random_int = reference_random_int)
      : n_kp_(n_matches), nlevels_(nlevels), sigma2_(sigma2, sigma2 + nlevels),
        random_int_(std::move(random_int)) {
    std::memcpy(K_, K, sizeof K_);
    for (int i = 0; i < n_matches; ++i) {
      const int mp = vpMapPointMatches[i];
      if (mp < 0 || mps[mp].bad) continue;
      const slamgpu_keypoint& kp = F.undist_kps[i];
      slamgpu_pnp_match c;
      c.xw[0] = mps[mp].xyz[0], c.xw[1] = mps[mp].xyz[1], c.xw[2] = mps[mp].xyz[2];
      c.u = kp.x, c.v = kp.y;
      c.octave = kp.octave;
      matches_.push_back(c);
      indices_.push_back(i);
    }
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300,
                           int minSet = 4, float epsilon = 0.4f, float th2 = 5.991f) {
    prob_ = probability, min_inliers_arg_ = minInliers, max_its_arg_ = maxIterations;
    min_set_ = minSet, epsilon_ = epsilon, th2_ = th2;
    const int N = (int)matches_.size();
    const PnpRansacParameters p =
        pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon);
    min_inliers_ = p.min_inliers, max_its_ = p.max_its;
    iterations_ = 0;
    evaluated_ = true;
    draws_.clear();
    hyp_.clear(), refined_.clear(), bits_.clear(), refined_bits_.clear(), events_.clear();
    if (N < min_inliers_) return;  // iterate returns at once (:126-130): nothing is drawn
    extend(max_its_);
  }

  // iterate (:118-211). true when a pose is returned: Tcw (4x4 row-major) is mRefinedTcw, or
  // mBestTcw at exhaustion; false for the reference's empty cv::Mat.
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
               float Tcw[16]) {
    if (!evaluated_)
      SetRansacParameters(prob_, min_inliers_arg_, max_its_arg_, min_set_, epsilon_, th2_);
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    const int N = (int)matches_.size();
    if (N < min_inliers_) {
      bNoMore = true;
      return false;
    }
    const int start = iterations_;
    const int end = std::max(max_its_, start + std::max(nIterations, 0));  // the || of :135
    for (;;) {
      size_t j = 0;
      while (j < events_.size() && events_[j] < start) ++j;
      if (j < events_.size() && events_[j] < end) {
        const int k = events_[j], b = hyp_[k].best;
        iterations_ = k + 1;
        give(refined_[b], &refined_bits_[(size_t)b * words_], vbInliers, nInliers, Tcw);
        return true;
      }
      if ((int)hyp_.size() >= end) break;
      extend(end);
    }
    iterations_ = end;  // >= mRansacMaxIts (:194-196)
    bNoMore = true;
    const int b = hyp_[end - 1].best;
    if (b < 0) return false;  // mnBestInliers < mRansacMinInliers
    give(hyp_[b], &bits_[(size_t)b * words_], vbInliers, nInliers, Tcw);
    return true;
  }
  // find (:112-116)
  bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
    if (!evaluated_)
      SetRansacParameters(prob_, min_inliers_arg_, max_its_arg_, min_set_, epsilon_, th2_);
    bool flag;
    return iterate(max_its_, flag, vbInliers, nInliers, Tcw);
  }

  const std::vector<slamgpu_pnp_match>& matches() const { return matches_; }
  const std::vector<int32_t>& indices() const { return indices_; }  // mvKeyPointIndices
  const std::vector<int32_t>& draws() const { return draws_; }
  int min_inliers() const { return min_inliers_; }    // the effective mRansacMinInliers
  int max_iterations() const { return max_its_; }     // the effective mRansacMaxIts
  int iterations() const { return iterations_; }      // mnIterations
  int device_calls() const { return device_calls_; }  // 1, and one more per schedule extension

 private:
  // Draws up to n_its iterations and evaluates the schedule.
  void extend(int n_its) {
    if (n_its > SLAMGPU_PNP_RANSAC_MAX_ITS)
      throw std::runtime_error("slamgpu: PnPsolver " + std::to_string(n_its) +
                               " iterations > SLAMGPU_PNP_RANSAC_MAX_ITS");
    const int N = (int)matches_.size();
    for (int k = (int)draws_.size() / 4; k < n_its; ++k)
      for (int i = 0; i < 4; ++i) draws_.push_back(random_int_(0, N - 1 - i));
    words_ = SLAMGPU_PNP_MASK_WORDS(N);
    hyp_.assign(n_its, slamgpu_pnp_hyp{});
    refined_.assign(n_its, slamgpu_pnp_hyp{});
    bits_.assign((size_t)n_its * words_, 0);
    refined_bits_.assign((size_t)n_its * words_, 0);
    events_.assign(n_its, 0);
    int ne = 0;
    ++device_calls_;
    throw_if(slamgpu_pnp_ransac(K_, sigma2_.data(), nlevels_, th2_, matches_.data(), N,
                                draws_.data(), n_its, min_inliers_, hyp_.data(), bits_.data(),
                                refined_.data(), refined_bits_.data(), events_.data(), &ne),
             slamgpu_pnpsolver_last_error);
    events_.resize(ne);
  }

  void give(const slamgpu_pnp_hyp& h, const uint64_t* bits, std::vector<bool>& vbInliers,
            int& nInliers, float Tcw[16]) const {
    nInliers = h.n_inliers;
    vbInliers.assign(n_kp_, false);
    for (size_t i = 0; i < matches_.size(); ++i)
      if (bits[i / 64] >> (i % 64) & 1) vbInliers[indices_[i]] = true;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Tcw[4 * r + c] = h.Rcw[3 * r + c];
      Tcw[4 * r + 3] = h.tcw[r];
      Tcw[12 + r] = 0.0f;
    }
    Tcw[15] = 1.0f;
  }

  int n_kp_, nlevels_;
  float K_[4];
  std::vector<float> sigma2_;
  RandomInt random_int_;
  std::vector<slamgpu_pnp_match> matches_;
  std::vector<int32_t> indices_;
  double prob_ = 0.99;
  int min_inliers_arg_ = 8, max_its_arg_ = 300, min_set_ = 4;
  float epsilon_ = 0.4f, th2_ = 5.991f;
  int min_inliers_ = 8, max_its_ = 300;
  bool evaluated_ = false;
  int iterations_ = 0;  // mnIterations
  int words_ = 0, device_calls_ = 0;
  std::vector<int32_t> draws_, events_;
  std::vector<slamgpu_pnp_hyp> hyp_, refined_;
  std::vector<uint64_t> bits_, refined_bits_;
};

// ---- Monocular Initializer (include/slamgpu_initializer.h) --------------------------------------

// DUtils::Random::SeedRandOnce(int) (DUtils/Random.cpp:38-45): srand(seed) the first time in the
// process.
inline void seed_rand_once(int seed) {
  static bool already_seeded = false;
  if (!already_seeded) {
    std::srand(seed);
    already_seeded = true;
  }
}

// The reference's Initializer (src/util/initializer.h) over plain arrays: keys = the undistorted
// keypoint positions (x, y) of a frame. Initialize draws the schedule as initializer.cpp:60-77
// does (SeedRandOnce(0), then eight RandomInt per iteration), makes the ONE synchronous device call
// and replays :92-98 and the tails of ReconstructH (:693-735) / ReconstructF (:495-565) from its
// outputs. R21 (3x3 row-major), t21, vP3D ([n1][3]) and vbTriangulated are written only when it
// returns true, as the reference's are.
class InitializerCore {
 public:
  using RandomInt = std::function<int(int, int)>;

  InitializerCore(const float* keys1, int n1, const float K[4], float sigma = 1.0f,
                  int iterations = 200, RandomInt random_int = reference_random_int)
      : keys1_(keys1, keys1 + 2 * (size_t)n1), n1_(n1), sigma_(sigma), iterations_(iterations),
        random_int_(std::move(random_int)) {
    std::memcpy(K_, K, sizeof K_);
  }

  bool Initialize(const float* keys2, int n2, const std::vector<int>& vMatches12, float R21[9],
                  float t21[3], std::vector<float>& vP3D, std::vector<bool>& vbTriangulated,
                  float minParallax = 1.0f, int minTriangulated = 50) {
    if ((int)vMatches12.size() != n1_)
      throw std::runtime_error("slamgpu: Initializer: one vMatches12 entry per key of frame 1");
    std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
    int N = 0;
    for (int m : m12) N += m >= 0;
    seed_rand_once(0);
    draws_.clear();
    for (int it = 0; it < iterations_; ++it)
      for (int j = 0; j < 8; ++j) draws_.push_back(random_int_(0, N - 1 - j));
    const size_t words = SLAMGPU_INIT_MASK_WORDS(n1_), its = (size_t)std::max(iterations_, 1);
    hyp_.assign(2 * its, slamgpu_init_hyp{});
    bits_.assign(2 * its * words, 0);
    std::vector<int32_t> pairs(2 * (size_t)n1_);
    std::vector<uint64_t> good(SLAMGPU_INIT_MAX_MOTIONS * words);
    std::vector<float> p3d((size_t)SLAMGPU_INIT_MAX_MOTIONS * 3 * n1_);
    ++device_calls_;
    throw_if(slamgpu_init_ransac(keys1_.data(), m12.data(), n1_, keys2, n2, K_, sigma_,
                                 draws_.data(), iterations_, hyp_.data(), bits_.data(), &result_,
                                 pairs.data(), motion_, good.data(), p3d.data()),
             slamgpu_initializer_last_error);
    const int model = result_.model, nm = result_.n_motions, b = result_.best[model];
    if (b < 0 || nm == 0) return false;  // an empty mask (:160), or the early return of :601
    const uint64_t* hb = &bits_[((size_t)model * iterations_ + b) * words];
    int Nin = 0;
    for (int i = 0; i < result_.n; ++i) Nin += (int)(hb[i / 64] >> (i % 64) & 1);
    float parallax[SLAMGPU_INIT_MAX_MOTIONS];
    for (int i = 0; i < nm; ++i)
      parallax[i] = motion_[i].n_good > 0
                        ? (float)(std::acos((double)motion_[i].cos_parallax) * 180 /
                                  3.1415926535897932384626433832795)
                        : 0.0f;
    int chosen = -1;
    if (model == SLAMGPU_INIT_MODEL_F) {
      int maxGood = 0, nsimilar = 0;
      for (int i = 0; i < 4; ++i) maxGood = std::max(maxGood, motion_[i].n_good);
      const int nMinGood = std::max(static_cast<int>(0.9 * Nin), minTriangulated);
      for (int i = 0; i < 4; ++i)
        if (motion_[i].n_good > 0.7 * maxGood) nsimilar++;
      if (maxGood < nMinGood || nsimilar > 1) return false;
      for (int i = 0; i < 4 && chosen < 0; ++i)
        if (maxGood == motion_[i].n_good) chosen = i;  // the else-if chain: the first that ties
      if (!(parallax[chosen] > minParallax)) return false;
    } else {
      int bestGood = 0, secondBestGood = 0;
      float bestParallax = -1;
      for (int i = 0; i < nm; ++i) {
        const int nGood = motion_[i].n_good;
        if (nGood > bestGood) {
          secondBestGood = bestGood;
          bestGood = nGood;
          chosen = i;
          bestParallax = parallax[i];
        } else if (nGood > secondBestGood) {
          secondBestGood = nGood;
        }
      }
      if (!(secondBestGood < 0.75 * bestGood && bestParallax >= minParallax &&
            bestGood > minTriangulated && bestGood > 0.9 * Nin))
        return false;
    }
    std::memcpy(R21, motion_[chosen].R, sizeof motion_[chosen].R);
    std::memcpy(t21, motion_[chosen].t, sizeof motion_[chosen].t);
    vP3D.assign(p3d.begin() + (size_t)chosen * 3 * n1_, p3d.begin() + (size_t)(chosen + 1) * 3 * n1_);
    vbTriangulated.assign(n1_, false);
    for (int i = 0; i < n1_; ++i)
      if (good[(size_t)chosen * words + i / 64] >> (i % 64) & 1) vbTriangulated[i] = true;
    return true;
  }

  const slamgpu_init_result& result() const { return result_; }  // of the last Initialize
  const std::vector<int32_t>& draws() const { return draws_; }
  int device_calls() const { return device_calls_; }

 private:
  std::vector<float> keys1_;
  int n1_;
  float K_[4], sigma_;
  int iterations_;
  RandomInt random_int_;
  std::vector<int32_t> draws_;
  std::vector<slamgpu_init_hyp> hyp_;
  std::vector<uint64_t> bits_;
  slamgpu_init_result result_{};
  slamgpu_init_motion motion_[SLAMGPU_INIT_MAX_MOTIONS] = {};
  int device_calls_ = 0;
};

// ---- Optimizer::BundleAdjustment (optimizer.cpp:33-207), GlobalBundleAdjustemnt (:18-31) ----
// Vertices: every keyframe that is not bad (fixed when Id() == 0), every map point that is not
// bad with its observations in GetObservations() order, skipping bad keyframes. A point left
// with no edge is still a vertex here and stays where it is (the device leaves points without
// observations out of the system, as :149-152 does).
inline LocalBaGraph gather_global_bundle_adjustment(const KeyFrameView* kfs, int n_kf,
                                                    const MapPointView* mps, int n_mp) {
  LocalBaGraph g;
  std::vector<int32_t> vertex_of(n_kf, -1);
  for (int k = 0; k < n_kf; ++k) {
    if (kfs[k].bad) continue;
    vertex_of[k] = (int32_t)g.keyframe.size();
    g.keyframe.push_back(k);
    g.kf_Tcw.insert(g.kf_Tcw.end(), kfs[k].Tcw, kfs[k].Tcw + 16);
    g.kf_mode.push_back(kfs[k].id == 0 ? SLAMGPU_KF_LOCAL_FIXED : SLAMGPU_KF_LOCAL);
  }
  g.n_local = (int)g.keyframe.size();
  g.point_obs_start.push_back(0);
  for (int m = 0; m < n_mp; ++m) {
    if (mps[m].bad) continue;
    g.map_point.push_back(m);
    g.points.insert(g.points.end(), mps[m].xyz, mps[m].xyz + 3);
    for (int o = 0; o < mps[m].n_obs; ++o) {
      const ObsRef r = mps[m].obs[o];
      if (kfs[r.keyframe].bad) continue;
      const slamgpu_keypoint& kp = kfs[r.keyframe].undist_kps[r.keypoint];
      slamgpu_ba_obs e;
      e.keyframe = vertex_of[r.keyframe];
      e.u = kp.x;
      e.v = kp.y;
      e.ur = kfs[r.keyframe].right_coords[r.keypoint];
      e.octave = kp.octave;
      g.obs.push_back(e);
      g.obs_ref.push_back(r);
    }
    g.point_obs_start.push_back((int32_t)g.obs.size());
  }
  return g;
}
// The whole call: gather, solve (optimised keyframe poses and point positions written into the
// graph: the caller stores them as the reference's :170-206 does), LM iterations run.
inline int global_bundle_adjustment(LocalBaGraph& g, const slamgpu_camera& cam,
                                    const float* inv_sigma2, int nlevels, int n_iterations,
                                    bool robust, const volatile bool* stop_flag) {
  int its = 0;
  throw_if(slamgpu_global_bundle_adjustment(&cam, inv_sigma2, nlevels, g.kf_Tcw.data(),
                                            g.kf_mode.data(), (int)g.keyframe.size(),
                                            g.points.data(), (int)g.map_point.size(),
                                            g.point_obs_start.data(), g.obs.data(), n_iterations,
                                            robust ? 1 : 0, stop_flag, &its),
           slamgpu_optimizer_last_error);
  return its;
}

// ---- the LoopCloser's three Sim3 matchers (slamgpu_loopmatch.h) ----------------------------------
// The decomposed transforms stay with the caller's OpenCV arithmetic: Scw as the reference splits
// it at orb_matcher.cpp:393-397 / :965-969, S12 as :1103-1105 makes sR12, sR21 and t21.
struct ScwBlocks {
  float Rcw[9], tcw[3], Ow[3];
};
struct Sim3Blocks {
  float sR12[9], t12[3], sR21[9], t21[3];
};

inline slamgpu_kf loop_kf(const KeyFrameView& v, const KeyFrameFeatures& f, const float* Rcw,
                          const float* tcw, const float* Ow) {
  slamgpu_kf k;
  std::memset(&k, 0, sizeof(k));
  k.kps = v.undist_kps;
  k.desc = f.desc;
  k.n = v.n_kps;
  for (int i = 0; i < 9; ++i) k.Rcw[i] = Rcw[i];
  for (int i = 0; i < 3; ++i) {
    k.tcw[i] = tcw[i];
    k.Ow[i] = Ow ? Ow[i] : 0.0f;
  }
  return k;
}
// The keyframe at its own pose (SearchBySim3 reads GetRotation() / GetTranslation()).
inline slamgpu_kf loop_kf(const KeyFrameView& v, const KeyFrameFeatures& f) {
  float R[9], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = v.Tcw[4 * r + c];
    t[r] = v.Tcw[4 * r + 3];
  }
  return loop_kf(v, f, R, t, f.Ow);
}

// Map point m as the matchers read it (m < 0: an empty record with skip set).
inline slamgpu_fuse_point loop_point(const MapPointView* mps, const MapPointGeometry* geom, int m,
                                     bool skip) {
  slamgpu_fuse_point q;
  std::memset(&q, 0, sizeof(q));
  q.skip = m < 0 || skip;
  if (m < 0) return q;
  std::memcpy(q.xyz, mps[m].xyz, sizeof(q.xyz));
  std::memcpy(q.normal, geom[m].normal, sizeof(q.normal));
  q.min_dist = geom[m].min_dist;
  q.max_dist = geom[m].max_dist;
  std::memcpy(q.desc, mps[m].desc, 32);
  return q;
}

// ---- OrbMatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (orb_matcher.cpp:956-1079),
// LoopCloser::SearchAndFuse (loop_closer.cpp:484, th = 4). replace[i] = the map point the caller
// writes into vpReplacePoint[i] (-1: leave it); added = the (point, keypoint) pairs of
// pMP->AddObservation(pKF, idx); pKF->AddMapPoint(pMP, idx), in order.
struct FuseSim3Result {
  int nfused = 0;
  std::vector<int32_t> replace;
  std::vector<std::pair<int32_t, int32_t>> added;
};
// The tail :1061-1075 over the candidate search's result. `slot` is the keyframe's map point per
// keypoint (updated by the AddMapPoint calls). A point that is bad or sits in a slot by now is
// passed over: inside one call that restates spAlreadyFound (nothing in the loop makes a point
// bad), across a SearchAndFuse batch it is the re-check the earlier keyframes' Replace calls need.
inline FuseSim3Result fuse_sim3_apply(const int32_t* best_idx, const int32_t* points,
                                      int n_points, const uint8_t* bad,
                                      std::vector<int32_t>& slot,
                                      const std::vector<uint8_t>& in_kf_at_entry) {
  FuseSim3Result res;
  res.replace.assign(n_points > 0 ? n_points : 0, -1);
  for (int i = 0; i < n_points; ++i) {
    const int m = points[i];
    if (m < 0 || bad[m] || in_kf_at_entry[i] || best_idx[i] < 0) continue;
    const int j = best_idx[i], cur = slot[j];
    if (cur >= 0) {
      if (!bad[cur]) res.replace[i] = cur;
    } else {
      slot[j] = m;
      res.added.emplace_back(m, j);
    }
    res.nfused++;
  }
  return res;
}
inline FuseSim3Result fuse_sim3(const KeyFrameView& kf, const KeyFrameFeatures& kff,
                                const ScwBlocks& scw, const MapPointView* mps,
                                const MapPointGeometry* geom, const int32_t* points, int n_points,
                                float th, const slamgpu_camera& cam, const slamgpu_levels& lv,
                                const slamgpu_kf_grid& grid) {
  // spAlreadyFound = pKF->GetMapPoints() (:972)
  auto in_kf = [&](int m) {
    for (int i = 0; i < kf.n_kps; ++i)
      if (kf.map_points[i] == m) return true;
    return false;
  };
  std::vector<slamgpu_fuse_point> pts(n_points > 0 ? n_points : 1);
  std::vector<uint8_t> found(n_points > 0 ? n_points : 1), bad(1);
  int max_m = -1;
  for (int i = 0; i < n_points; ++i) max_m = points[i] > max_m ? points[i] : max_m;
  for (int i = 0; i < kf.n_kps; ++i) max_m = kf.map_points[i] > max_m ? kf.map_points[i] : max_m;
  bad.assign(max_m + 2, 0);
  for (int m = 0; m <= max_m; ++m) bad[m] = mps[m].bad;
  for (int i = 0; i < n_points; ++i) {
    const int m = points[i];
    found[i] = m >= 0 && in_kf(m);
    pts[i] = loop_point(mps, geom, m, m >= 0 && (mps[m].bad || found[i]));
  }
  const slamgpu_kf k = loop_kf(kf, kff, scw.Rcw, scw.tcw, scw.Ow);
  std::vector<int32_t> best(n_points > 0 ? n_points : 1), dist(n_points > 0 ? n_points : 1);
  int nf = 0;
  throw_if(slamgpu_fuse_sim3(&k, pts.data(), n_points, th, &cam, &lv, &grid, best.data(),
                             dist.data(), &nf),
           slamgpu_loopmatch_last_error);
  std::vector<int32_t> slot(kf.map_points, kf.map_points + kf.n_kps);
  return fuse_sim3_apply(best.data(), points, n_points, bad.data(), slot, found);
}

// ---- OrbMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (orb_matcher.cpp:384-497),
// LoopCloser::ComputeSim3 (loop_closer.cpp:441, th = 10). vpMatched: map point index per
// keypoint (-1 = none), updated in place as :490 does. Returns nmatches.
inline int search_by_projection_sim3(const KeyFrameView& kf, const KeyFrameFeatures& kff,
                                     const ScwBlocks& scw, const MapPointView* mps,
                                     const MapPointGeometry* geom, const int32_t* points,
                                     int n_points, int32_t* vpMatched, float th,
                                     const slamgpu_camera& cam, const slamgpu_levels& lv,
                                     const slamgpu_kf_grid& grid) {
  const int n = kf.n_kps;
  std::vector<uint8_t> matched_in(n > 0 ? n : 1);
  for (int j = 0; j < n; ++j) matched_in[j] = vpMatched[j] >= 0;
  auto already_found = [&](int m) {  // spAlreadyFound (:400-401)
    for (int j = 0; j < n; ++j)
      if (vpMatched[j] == m) return true;
    return false;
  };
  std::vector<slamgpu_fuse_point> pts(n_points > 0 ? n_points : 1);
  for (int i = 0; i < n_points; ++i) {
    const int m = points[i];
    pts[i] = loop_point(mps, geom, m, m >= 0 && (mps[m].bad || already_found(m)));
  }
  const slamgpu_kf k = loop_kf(kf, kff, scw.Rcw, scw.tcw, scw.Ow);
  std::vector<int32_t> kp_point(n > 0 ? n : 1), point_kp(n_points > 0 ? n_points : 1);
  int nm = 0;
  throw_if(slamgpu_search_by_projection_sim3(&k, pts.data(), n_points, matched_in.data(), th,
                                             &cam, &lv, &grid, kp_point.data(), point_kp.data(),
                                             &nm),
           slamgpu_loopmatch_last_error);
  for (int j = 0; j < n; ++j)
    if (kp_point[j] >= 0) vpMatched[j] = points[kp_point[j]];
  return nm;
}

// ---- OrbMatcher::SearchBySim3 (orb_matcher.cpp:1081-1310), LoopCloser::ComputeSim3
// (loop_closer.cpp:382, th = 7.5). vpMatches12: pKF2's map point index per pKF1 feature (-1 =
// none), updated in place where both directions agree (:1291-1307). Returns nFound.
inline int search_by_sim3(int kf1_index, int kf2_index, const KeyFrameView* kfs,
                          const KeyFrameFeatures& f1, const KeyFrameFeatures& f2,
                          const MapPointView* mps, const MapPointGeometry* geom,
                          int32_t* vpMatches12, const Sim3Blocks& s, float th,
                          const slamgpu_camera& cam, const slamgpu_levels& lv,
                          const slamgpu_kf_grid& grid) {
  const KeyFrameView& kf1 = kfs[kf1_index];
  const KeyFrameView& kf2 = kfs[kf2_index];
  const int n1 = kf1.n_kps, n2 = kf2.n_kps;
  std::vector<slamgpu_fuse_point> mp1(n1 > 0 ? n1 : 1), mp2(n2 > 0 ? n2 : 1);
  std::vector<uint8_t> already1(n1 > 0 ? n1 : 1, 0), already2(n2 > 0 ? n2 : 1, 0);
  for (int i = 0; i < n1; ++i) {
    const int m = kf1.map_points[i];
    mp1[i] = loop_point(mps, geom, m, m >= 0 && mps[m].bad);
  }
  for (int i = 0; i < n2; ++i) {
    const int m = kf2.map_points[i];
    mp2[i] = loop_point(mps, geom, m, m >= 0 && mps[m].bad);
  }
  for (int i = 0; i < n1; ++i) {  // :1116-1126
    const int m = vpMatches12[i];
    if (m < 0) continue;
    already1[i] = 1;
    for (int o = 0; o < mps[m].n_obs; ++o)  // GetIndexInKeyFrame(pKF2)
      if (mps[m].obs[o].keyframe == kf2_index) {
        const int idx2 = mps[m].obs[o].keypoint;
        if (idx2 >= 0 && idx2 < n2) already2[idx2] = 1;
        break;
      }
  }
  const slamgpu_kf k1 = loop_kf(kf1, f1), k2 = loop_kf(kf2, f2);
  std::vector<int32_t> match12(n1 > 0 ? n1 : 1), vn1(n1 > 0 ? n1 : 1), vn2(n2 > 0 ? n2 : 1);
  int nfound = 0;
  throw_if(slamgpu_search_by_sim3(&k1, &k2, mp1.data(), mp2.data(), already1.data(),
                                  already2.data(), s.sR12, s.t12, s.sR21, s.t21, th, &cam, &lv,
                                  &grid, match12.data(), vn1.data(), vn2.data(), &nfound),
           slamgpu_loopmatch_last_error);
  for (int i = 0; i < n1; ++i)
    if (match12[i] >= 0) vpMatches12[i] = kf2.map_points[match12[i]];
  return nfound;
}

// ---- OrbMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>&
// sAlreadyFound, th, ORBdist) (orb_matcher.cpp:1455-1582), Tracker::Relocalization
// (tracker.cpp:938-960: (10, 100), then (3, 64)). Runs on the frame the context holds.

struct RelocInput {
  std::vector<slamgpu_reloc_query> queries;  // one per keyframe keypoint, keypoint order
  slamgpu_reloc_pose pose;
};

// Ow = -Rcw.t() * tcw (:1461) for callers without their own cv::Mat arithmetic: the products and
// their sum in double, rounded to float once. The library itself takes Ow as given
// (slamgpu_reloc_pose): a caller with OpenCV passes what its own expression gave.
inline void reloc_camera_center(const float* Tcw, float* Ow) {
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int r = 0; r < 3; ++r) s += (double)Tcw[4 * r + k] * (double)Tcw[4 * r + 3];
    Ow[k] = (float)-s;
  }
}

// pKF->GetMapPointMatches() in keypoint order (:1469-1477): a slot that is null, bad or in
// already_found (map point indices: sAlreadyFound at entry) becomes a skip record. mp_id is the
// map point's index, so the frame's map point array is the call's map_point argument as it is.
inline RelocInput gather_search_by_projection_reloc(const FrameView& current, const KeyFrameView& kf,
                                                    const MapPointView* mps,
                                                    const MapPointGeometry* geom,
                                                    const int32_t* already_found, int n_found,
                                                    const float* Ow, float th, int orb_dist,
                                                    bool check_ori) {
  RelocInput in;
  in.queries.resize(kf.n_kps > 0 ? kf.n_kps : 0);
  std::vector<int32_t> found(already_found, already_found + n_found);
  std::sort(found.begin(), found.end());
  for (int i = 0; i < kf.n_kps; ++i) {
    slamgpu_reloc_query& q = in.queries[i];
    std::memset(&q, 0, sizeof q);
    const int m = kf.map_points[i];
    q.skip = m < 0 || mps[m].bad || std::binary_search(found.begin(), found.end(), m);
    if (q.skip) continue;
    std::memcpy(q.xyz, mps[m].xyz, sizeof q.xyz);
    q.max_dist = geom[m].max_dist;
    q.min_dist = geom[m].min_dist;
    q.kf_angle = kf.undist_kps[i].angle;
    q.mp_id = m;
    std::memcpy(q.desc, mps[m].desc, 32);
  }
  slamgpu_reloc_pose& p = in.pose;
  std::memset(&p, 0, sizeof p);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.Rcw[3 * r + c] = current.Tcw[4 * r + c];
    p.tcw[r] = current.Tcw[4 * r + 3];
    p.Ow[r] = Ow[r];
  }
  p.th = th;
  p.orb_dist = orb_dist;
  p.check_ori = check_ori ? 1 : 0;
  return in;
}

// CurrentFrame.SetMapPoint(bestIdx2, pMP) / SetMapPoint(idx, nullptr) (:1543, :1574): the slots
// the call returns are map point indices already (mp_id = index); copies them into the frame's
// array and returns how many slots hold a point now that did not at entry.
inline int apply_search_by_projection_reloc(const int32_t* slot, int32_t* current_map_points, int n) {
  int assigned = 0;
  for (int i = 0; i < n; ++i) {
    if (slot[i] >= 0 && current_map_points[i] < 0) ++assigned;
    current_map_points[i] = slot[i];
  }
  return assigned;
}

// The whole call on frame `frame` of the context's last frame / frontend call; current_map_points
// (the frame's map point index per keypoint, -1 = none) is in/out. Returns nmatches; throws on a
// device error.
inline int search_by_projection_reloc(slamgpu_ctx* ctx, int frame, const FrameView& current,
                                      const KeyFrameView& kf, const MapPointView* mps,
                                      const MapPointGeometry* geom, const int32_t* already_found,
                                      int n_found, const float* Ow, float th, int orb_dist,
                                      bool check_ori, int32_t* current_map_points,
                                      slamgpu_reloc_pose* pose_used = nullptr) {
  const RelocInput in = gather_search_by_projection_reloc(current, kf, mps, geom, already_found,
                                                          n_found, Ow, th, orb_dist, check_ori);
  if (pose_used) *pose_used = in.pose;
  std::vector<int32_t> slot(current_map_points, current_map_points + current.n_kps);
  std::vector<uint8_t> blocked(current.n_kps > 0 ? current.n_kps : 1);
  int nm = 0;
  const int rc = slamgpu_search_by_projection_reloc(ctx, frame, in.queries.data(),
                                                    (int)in.queries.size(), &in.pose, slot.data(),
                                                    blocked.data(), current.n_kps, &nm);
  if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") + slamgpu_last_error(ctx));
  apply_search_by_projection_reloc(slot.data(), current_map_points, current.n_kps);
  return nm;
}

// One step of relocalization_refine as it ran, for tests and logs.
struct RelocRefineStep {
  enum Kind : int32_t { kPoseOptimization = 0, kSearch = 1 };
  int32_t kind;
  int32_t result;                      // nGood of the optimization / nadditional of the search
  float Tcw_in[16], Tcw_out[16];
  slamgpu_reloc_pose pose;             // the search's pose record (zero for an optimization)
  std::vector<int32_t> found;          // the search's sAlreadyFound
  std::vector<int32_t> map_points_in;  // the frame's slots before the step ...
  std::vector<int32_t> map_points_out; // ... and after it (outliers not yet cleared)
  std::vector<uint8_t> outlier_out;    // the frame's outlier flags after the step
};

// Tracker::Relocalization's refinement of one candidate (tracker.cpp:924-975), after the PnP
// inliers were set as the frame's map points and sFound (:915-922): PoseOptimization; with fewer
// than 10 inliers the candidate is dropped; outliers cleared; with fewer than 50 the (10, 100)
// search and, if that brings the count to 50, PoseOptimization; with 30 < nGood < 50 sFound
// rebuilt from the frame's slots, the (3, 64) search and, if that brings the count to 50, the
// final PoseOptimization and clearing. Tcw[16], map_points[n] and outlier[n] of `current` are
// updated in place through the three mutable pointers (current.Tcw / .map_points / .outlier must
// point at the same arrays). Returns nGood: the caller accepts the candidate iff nGood >= 50.
inline int relocalization_refine(slamgpu_ctx* ctx, int frame, const slamgpu_camera& cam,
                                 const float* inv_sigma2, int nlevels, const FrameView& current,
                                 float* Tcw, int32_t* map_points, uint8_t* outlier,
                                 const KeyFrameView& kf, const MapPointView* mps,
                                 const MapPointGeometry* geom, std::vector<int32_t> found,
                                 bool check_ori, std::vector<RelocRefineStep>* trace = nullptr,
                                 const std::function<void(const float*, float*)>& center =
                                     reloc_camera_center) {
  if (current.Tcw != Tcw || current.map_points != map_points || current.outlier != outlier)
    throw std::invalid_argument("relocalization_refine: `current` must view the mutable arrays");
  const int n = current.n_kps;
  auto begin_step = [&](int kind) {
    RelocRefineStep s;
    s.kind = kind;
    s.result = 0;
    std::memcpy(s.Tcw_in, Tcw, sizeof s.Tcw_in);
    std::memset(&s.pose, 0, sizeof s.pose);
    s.map_points_in.assign(map_points, map_points + n);
    return s;
  };
  auto end_step = [&](RelocRefineStep& s, int result) {
    s.result = result;
    std::memcpy(s.Tcw_out, Tcw, sizeof s.Tcw_out);
    s.map_points_out.assign(map_points, map_points + n);
    s.outlier_out.assign(outlier, outlier + n);
    if (trace) trace->push_back(std::move(s));
  };
  auto pose_optimization = [&]() {
    RelocRefineStep s = begin_step(RelocRefineStep::kPoseOptimization);
    const PoseGraph g = gather_pose_optimization(current, mps);
    std::vector<uint8_t> edge_outlier(g.edges.size() + 1, 0);
    int n_inliers = 0;
    if (slamgpu_pose_optimization(&cam, inv_sigma2, nlevels, g.edges.data(), (int)g.edges.size(),
                                  Tcw, edge_outlier.data(), &n_inliers) != SLAMGPU_OK)
      throw std::runtime_error(std::string("slamgpu: ") + slamgpu_optimizer_last_error());
    apply_pose_optimization(g, edge_outlier.data(), outlier);
    end_step(s, n_inliers);
    return n_inliers;
  };
  auto clear_outliers = [&]() {
    for (int io = 0; io < n; ++io)
      if (outlier[io]) map_points[io] = -1;
  };
  auto search = [&](float th, int orb_dist) {
    RelocRefineStep s = begin_step(RelocRefineStep::kSearch);
    s.found = found;
    float Ow[3];
    center(Tcw, Ow);
    const int nm = search_by_projection_reloc(ctx, frame, current, kf, mps, geom, found.data(),
                                              (int)found.size(), Ow, th, orb_dist, check_ori,
                                              map_points, &s.pose);
    end_step(s, nm);
    return nm;
  };

  int nGood = pose_optimization();
  if (nGood < 10) return nGood;
  clear_outliers();
  if (nGood < 50) {
    int nadditional = search(10.0f, 100);
    if (nadditional + nGood >= 50) {
      nGood = pose_optimization();
      if (nGood > 30 && nGood < 50) {
        found.clear();
        for (int ip = 0; ip < n; ++ip)
          if (map_points[ip] >= 0) found.push_back(map_points[ip]);
        nadditional = search(3.0f, 64);
        if (nGood + nadditional >= 50) {
          nGood = pose_optimization();
          clear_outliers();
        }
      }
    }
  }
  return nGood;
}

// ---- OrbMatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
// (orb_matcher.cpp:264-382), Tracker::MonocularInitialization (tracker.cpp:297-364). F2 is the
// frame the context holds (slamgpu_frame_mono); F1 is the initial frame the caller kept.

// One query per keypoint of F1, in keypoint order (the query index is i1): the undistorted
// keypoint's angle and octave and descriptor row i1. FrameView carries no descriptors, so they
// come beside it (F1.GetDescriptors(), n_kps x 32 bytes).
inline std::vector<slamgpu_init_query> gather_search_for_initialization(const FrameView& F1,
                                                                        const uint8_t* descriptors) {
  std::vector<slamgpu_init_query> q(F1.n_kps > 0 ? F1.n_kps : 0);
  for (int i = 0; i < F1.n_kps; ++i) {
    std::memset(&q[i], 0, sizeof q[i]);
    q[i].angle = F1.undist_kps[i].angle;
    q[i].octave = F1.undist_kps[i].octave;
    std::memcpy(q[i].desc, descriptors + (size_t)i * 32, 32);
  }
  return q;
}

// The whole call: prev_matched ([n1][2], vbPrevMatched) is in/out, matches12 ([n1], vnMatches12)
// out. Returns nmatches; throws on an error.
inline int search_for_initialization(slamgpu_ctx* ctx, int frame, const FrameView& F1,
                                     const uint8_t* descriptors, float* prev_matched,
                                     int32_t* matches12, int window_size, float nnratio,
                                     bool check_ori) {
  const std::vector<slamgpu_init_query> q = gather_search_for_initialization(F1, descriptors);
  slamgpu_init_search p;
  std::memset(&p, 0, sizeof p);
  p.nnratio = nnratio;
  p.window_size = window_size;
  p.check_ori = check_ori ? 1 : 0;
  int nm = 0;
  const int rc = slamgpu_search_for_initialization(ctx, frame, q.data(), (int)q.size(), &p,
                                                   prev_matched, matches12, &nm);
  if (rc != SLAMGPU_OK) throw std::runtime_error(std::string("slamgpu: ") + slamgpu_last_error(ctx));
  return nm;
}

// ---- KeyframeDatabase queries (include/slamgpu_kfdb.h), LoopCloser::DetectLoop
// (src/core/loop_closer.cpp:194-297) -------------------------------------------------------------
// The id lists of slamgpu_kfdb_detect_loop_candidates for keyframe `cur` of the keyframe array:
// connected = GetConnectedKeyFrames() (the caller's set, as keyframe indices, in any order),
// covisible = GetVectorCovisibleKeyFrames() with the bad ones dropped (loop_closer.cpp:215-218),
// both as KeyFrame::Id()s, which are the database's slots.
struct LoopQueryIds {
  int32_t kf_id;
  std::vector<int32_t> connected, covisible;
};
inline LoopQueryIds gather_detect_loop_candidates(int cur, const KeyFrameView* kfs,
                                                  const int32_t* connected, int n_connected) {
  LoopQueryIds q;
  q.kf_id = (int32_t)kfs[cur].id;
  for (int i = 0; i < n_connected; i++) q.connected.push_back((int32_t)kfs[connected[i]].id);
  for (int i = 0; i < kfs[cur].n_covisible; i++) {
    const KeyFrameView& k = kfs[kfs[cur].covisible[i]];
    if (!k.bad) q.covisible.push_back((int32_t)k.id);
  }
  return q;
}

// One synchronous query with the gathered lists; returns the candidate ids in the reference's
// order and *min_score. Throws on an error.
inline std::vector<int32_t> detect_loop_candidates(slamgpu_kfdb* db, const LoopQueryIds& q,
                                                   int max_keyframes, float* min_score) {
  std::vector<int32_t> cand((size_t)max_keyframes);
  int n = 0;
  throw_if(slamgpu_kfdb_detect_loop_candidates(db, q.kf_id, q.connected.data(),
                                               (int)q.connected.size(), q.covisible.data(),
                                               (int)q.covisible.size(), min_score, cand.data(), &n,
                                               nullptr, nullptr),
           slamgpu_kfdb_last_error);
  cand.resize((size_t)n);
  return cand;
}

// The rest of DetectLoop on the host: the consistency groups of loop_closer.cpp:239-296 kept as
// sorted sets of keyframe ids, the way Sim3SolverCore replays iterate / find. The caller's
// DetectLoop becomes
//   if (core.too_soon(id)) { db add(id); return false; }                              // :204-208
//   cand = detect_loop_candidates(...);
//   r = core.update(cand.data(), cand.size(), connected_of);  db add(id);   // :227-232, :289
//   return r.detected;   // consistent_enough_candidates_ = r.consistent_enough
// Every exit adds the current keyframe to the database: Result::add_current_keyframe is true on
// all of them and early_exit() says so for the first.
class LoopDetectorCore {
 public:
  using Group = std::pair<std::vector<int32_t>, int>;  // ConsistentGroup: (sorted ids, counter)
  struct Result {
    std::vector<int32_t> consistent_enough;  // consistent_enough_candidates_, in candidate order
    bool add_current_keyframe;               // keyframe_db_->add(current_keyframe_)
    bool detected;                           // DetectLoop's return value
  };

  explicit LoopDetectorCore(int covisibility_consistency_threshold = 3)
      : threshold_(covisibility_consistency_threshold) {}

  int64_t last_loop_kf_id = 0;  // last_loop_kf_id_: the caller sets it where CorrectLoop does

  // loop_closer.cpp:204: fewer than 10 keyframes since the last loop -- no query at all.
  bool too_soon(int64_t kf_id) const { return kf_id < last_loop_kf_id + 10; }
  static Result early_exit() { return Result{{}, true, false}; }

  // connected_of(id, out): appends GetConnectedKeyFrames() of candidate `id` to out (any order).
  template <class ConnectedOf>
  Result update(const int32_t* candidates, int n, ConnectedOf connected_of) {
    Result r{{}, true, false};
    if (n == 0) {  // :227-232
      groups_.clear();
      return r;
    }
    std::vector<Group> current;
    std::vector<bool> visited(groups_.size(), false);
    for (int c = 0; c < n; c++) {
      std::vector<int32_t> group;
      connected_of(candidates[c], group);
      group.push_back(candidates[c]);
      std::sort(group.begin(), group.end());
      group.erase(std::unique(group.begin(), group.end()), group.end());
      bool has_enough = false, consistent_for_some = false;
      for (size_t g = 0; g < groups_.size(); g++) {
        const std::vector<int32_t>& prev = groups_[g].first;
        bool consistent = false;
        for (int32_t id : group)
          if (std::binary_search(prev.begin(), prev.end(), id)) {
            consistent = true;
            consistent_for_some = true;
            break;
          }
        if (!consistent) continue;
        const int n_current = groups_[g].second + 1;
        if (!visited[g]) {  // :267-270: a previous group is extended once per query
          current.emplace_back(group, n_current);
          visited[g] = true;
        }
        if (n_current >= threshold_ && !has_enough) {
          r.consistent_enough.push_back(candidates[c]);
          has_enough = true;
        }
      }
      if (!consistent_for_some) current.emplace_back(group, 0);  // :280-282
    }
    groups_ = std::move(current);  // :286
    r.detected = !r.consistent_enough.empty();
    return r;
  }

  const std::vector<Group>& groups() const { return groups_; }

 private:
  int threshold_;
  std::vector<Group> groups_;
};

}  // namespace slamgpu_adapter
