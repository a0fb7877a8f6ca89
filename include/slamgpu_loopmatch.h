/*
 * slamgpu_loopmatch.h -- C ABI of the LoopCloser's three Sim3 matchers (libslamgpu.so), drop-in
 * for (paths relative to the reference repository root):
 *   OrbMatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 *     src/orb_features/orb_matcher.cpp:1081-1310; caller LoopCloser::ComputeSim3
 *     (src/core/loop_closer.cpp:382, th = 7.5)
 *   OrbMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)   orb_matcher.cpp:384-497;
 *     caller LoopCloser::ComputeSim3 (loop_closer.cpp:441, th = 10)
 *   OrbMatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)            orb_matcher.cpp:956-1079;
 *     caller LoopCloser::SearchAndFuse (loop_closer.cpp:484, th = 4)
 * None of the three applies the reprojection chi-square gates of the plain Fuse, and none reads
 * the stereo right coordinate (slamgpu_kf.u_right may be NULL here).
 *
 * The caller passes the DECOMPOSED transforms as floats, computed with its own cv::Mat
 * arithmetic (orb_matcher.cpp:393-397, :965-969, :1103-1105): Rcw, tcw, Ow of the two Scw calls
 * in the slamgpu_kf; sR12, t12, sR21, t21 of SearchBySim3 in the pair record. The library takes
 * no position on MatExpr rounding.
 *
 * Conventions as slamgpu_kfmatch.h, whose slamgpu_kf, slamgpu_fuse_point, slamgpu_levels,
 * slamgpu_kf_grid and slamgpu_camera are reused: POD types, caller-owned buffers, 0 or a negative
 * SLAMGPU_E* code with the message in slamgpu_loopmatch_last_error() (per thread; the same
 * string slamgpu_kfmatch_last_error() returns). The synchronous calls take host pointers and
 * stage through the calling thread's device buffer; the *_device calls take device pointers and a
 * hipStream_t, never allocate and return without synchronising. n <= SLAMGPU_KF_MAX_FEATURES
 * per keyframe (the synchronous calls reject more; a *_device call flags the job, see below).
 * A keypoint whose octave is outside [0, 255) never matches in a *_device call.
 */
#ifndef SLAMGPU_LOOPMATCH_H_
#define SLAMGPU_LOOPMATCH_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu_kfmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) --------------------------------------------- */
/* The candidate search (:979-1059) for every point; kf->Rcw / tcw / Ow = the decomposed Scw.
 * pts[i].skip = isBad() || spAlreadyFound.count(pMP) (the snapshot of :972). best_idx[i] = the
 * keypoint point i fuses into (bestDist <= TH_LOW) or -1, best_dist[i] = bestDist (256 if no
 * candidate; the reference's INT_MAX never escapes the loop). *nfused = #(best_idx >= 0). The
 * adapter then walks the points in order doing :1061-1075 (slamgpu_adapters.hpp). */
int slamgpu_fuse_sim3(const slamgpu_kf* kf, const slamgpu_fuse_point* pts, int n_pts, float th,
                      const slamgpu_camera* cam, const slamgpu_levels* lv,
                      const slamgpu_kf_grid* grid, int32_t* best_idx, int32_t* best_dist,
                      int* nfused);

/* Batched over n_kfs keyframes x ONE shared point array (SearchAndFuse offers the same
 * loop_map_points_ to every corrected keyframe; the 80-byte records are not replicated).
 * d_skip: optional [n_kfs][n_pts] bytes, "isBad() or already in keyframe k"; NULL = use
 * d_pts[i].skip for every keyframe. Outputs [n_kfs][n_pts]. A keyframe with n outside
 * [0, SLAMGPU_KF_MAX_FEATURES] gets best_idx = -1, best_dist = 256 everywhere. */
int slamgpu_fuse_sim3_device(const slamgpu_kf* d_kfs, int n_kfs, const slamgpu_fuse_point* d_pts,
                             int n_pts, const uint8_t* d_skip, float th,
                             const slamgpu_camera* cam, const slamgpu_levels* lv,
                             const slamgpu_kf_grid* grid, int32_t* d_best_idx,
                             int32_t* d_best_dist, void* stream);

/* ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) ----------------------------------- */
/* matched_in[idx] = vpMatched[idx] != nullptr when the call starts (kf->n bytes). pts[i].skip =
 * isBad() || spAlreadyFound.count(pMP). The points are committed in order, exactly as the
 * reference's loop (:406-494): point i takes its best candidate (first strict minimum in
 * GetFeaturesInArea order) among the keypoints neither matched at entry nor claimed by a point
 * before it, and claims it when the distance is <= TH_LOW.
 * kp_point[idx] = the index of the point that claimed keypoint idx, or -1 (keypoints matched at
 * entry stay -1: vpMatched[idx] is unchanged there); point_kp[i] = the keypoint point i claimed
 * or -1; *nmatches = the reference's return value. */
int slamgpu_search_by_projection_sim3(const slamgpu_kf* kf, const slamgpu_fuse_point* pts,
                                      int n_pts, const uint8_t* matched_in, float th,
                                      const slamgpu_camera* cam, const slamgpu_levels* lv,
                                      const slamgpu_kf_grid* grid, int32_t* kp_point,
                                      int32_t* point_kp, int* nmatches);

/* One independent job of the batched call: points d_pts[pt_begin .. pt_begin + n_pts) into
 * d_kfs[kf]; its keypoint rows (matched_in, kp_point) start at kp_begin. 16 bytes. */
typedef struct {
  int32_t kf;
  int32_t pt_begin, n_pts;
  int32_t kp_begin;
} slamgpu_sbp_job;

/* The candidates of distance <= TH_LOW the scan keeps per point for the in-order resolve; a
 * point that runs out of them while more exist is searched again at its place in the order. */
#define SLAMGPU_SBP_KEEP 3

/* Bytes of d_scratch for a point array of n_pts_total records. */
size_t slamgpu_search_by_projection_sim3_scratch_bytes(int n_pts_total);

/* n_pts_total / n_kp_total = the lengths of d_pts / d_point_kp and of d_matched_in / d_kp_point;
 * max_job_pts >= every job's n_pts (it sizes the launch). Job j writes d_point_kp[pt_begin ..),
 * d_kp_point[kp_begin .. kp_begin + n) (point indices relative to pt_begin) and d_nmatches[j]
 * (-1, and nothing else, when the job's ranges leave the arrays, n_pts > max_job_pts or the
 * keyframe's n is outside [0, SLAMGPU_KF_MAX_FEATURES]). Point ranges of different jobs must
 * not overlap (the scratch rows are per point). */
int slamgpu_search_by_projection_sim3_device(
    const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_pts, int n_pts_total,
    const slamgpu_sbp_job* d_jobs, int n_jobs, int max_job_pts, const uint8_t* d_matched_in,
    int n_kp_total, float th, const slamgpu_camera* cam, const slamgpu_levels* lv,
    const slamgpu_kf_grid* grid, int32_t* d_kp_point, int32_t* d_point_kp, int32_t* d_nmatches,
    void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- SearchBySim3 --------------------------------------------------------------------------- */
/* mp1[i] / mp2[i]: one record per feature of kf1 / kf2 (GetMapPointMatches()), skip = !pMP ||
 * isBad(); normal is unused. kf->Rcw / tcw = GetRotation() / GetTranslation() (Ow unused).
 * already1 / already2 = vbAlreadyMatched1 / 2 (:1113-1126): such features are skipped as sources
 * only. sR12 (row-major), t12, sR21, t21 as the reference computes them at :1103-1105.
 * cam / lv / grid are shared by the two keyframes (one camera).
 * vn_match1[i1] / vn_match2[i2] = vnMatch1 / vnMatch2 (:1128-1289); match12[i1] = the kf2
 * feature whose map point the reference writes into vpMatches12[i1] (:1291-1307), or -1;
 * *nfound = the return value. */
int slamgpu_search_by_sim3(const slamgpu_kf* kf1, const slamgpu_kf* kf2,
                           const slamgpu_fuse_point* mp1, const slamgpu_fuse_point* mp2,
                           const uint8_t* already1, const uint8_t* already2, const float* sR12,
                           const float* t12, const float* sR21, const float* t21, float th,
                           const slamgpu_camera* cam, const slamgpu_levels* lv,
                           const slamgpu_kf_grid* grid, int32_t* match12, int32_t* vn_match1,
                           int32_t* vn_match2, int* nfound);

/* A keyframe pair of the batched call: d_kfs[kf1] against d_kfs[kf2], whose per-feature map
 * point records start at d_mp[mp1_begin] / d_mp[mp2_begin]. 112 bytes. */
typedef struct {
  int32_t kf1, kf2;
  int32_t mp1_begin, mp2_begin;
  float sR12[9], t12[3];
  float sR21[9], t21[3];
} slamgpu_sim3_pair;

/* Pair p reads d_already1 / d_already2 + p * stride and writes d_match12 / d_vn_match1 /
 * d_vn_match2 + p * stride and d_nfound[p] (-1, and nothing else, when a keyframe's n is outside
 * [0, min(stride, SLAMGPU_KF_MAX_FEATURES)] or an mp range leaves [0, n_mp_total)). */
int slamgpu_search_by_sim3_device(const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_mp,
                                  int n_mp_total, const slamgpu_sim3_pair* d_pairs, int n_pairs,
                                  const uint8_t* d_already1, const uint8_t* d_already2,
                                  int64_t stride, float th, const slamgpu_camera* cam,
                                  const slamgpu_levels* lv, const slamgpu_kf_grid* grid,
                                  int32_t* d_match12, int32_t* d_vn_match1,
                                  int32_t* d_vn_match2, int32_t* d_nfound, void* stream);

const char* slamgpu_loopmatch_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_LOOPMATCH_H_ */
