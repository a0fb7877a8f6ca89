/*
 * slamgpu_kfmatch.h -- C ABI of the keyframe-rate matchers the LocalMapper runs before
 * LocalBundleAdjustment (libslamgpu.so). SURVEY.md section 8(f) row 3, drop-in for (paths
 * relative to the reference repository root):
 *   OrbMatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
 *     src/orb_features/orb_matcher.cpp:634-802 (+ CheckDistEpipolarLine :114-131);
 *     caller LocalMapper::CreateNewMapPoints (src/core/local_mapper.cpp)
 *   OrbMatcher::Fuse(pKF, vpMapPoints, th)  orb_matcher.cpp:804-954 (+ MapPoint::PredictScale
 *     src/data/map_point.cpp:366-381, KeyFrame::GetFeaturesInArea keyframe.cpp:442-476);
 *     caller LocalMapper::SearchInNeighbors
 * Conventions as slamgpu.h: POD types, caller-owned buffers, 0 or a negative SLAMGPU_E* code
 * with the message in slamgpu_kfmatch_last_error() (per thread). The synchronous calls stage
 * through the calling thread's device buffer (see slamgpu_bow.h); the *_device calls take device pointers and a hipStream_t,
 * never allocate and return without synchronising.
 */
#ifndef SLAMGPU_KFMATCH_H_
#define SLAMGPU_KFMATCH_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMGPU_KF_MAX_FEATURES 4096

/* The per-level tables a KeyFrame copies from its extractor: log_scale_factor (float
 * log(scaleFactor)), scale_factors, level_sigma_sq, inv_level_sigma_sq (keyframe.h:167-170). */
typedef struct {
  int32_t nlevels;
  float log_scale_factor;
  float scale[32];
  float sigma2[32];
  float inv_sigma2[32];
} slamgpu_levels;

/* KeyFrame::min_x_ .. max_y_ (ints, keyframe.cpp:14-15) and grid_element_width_ / _height_ of
 * the 64 x 48 keypoint grid (Frame::AssignFeaturesToGrid frame.cpp:234-248). */
typedef struct {
  float min_x, max_x, min_y, max_y;
  float cell_w, cell_h;
} slamgpu_kf_grid;

/* One keyframe as the matchers read it: host pointers in the synchronous calls, device pointers
 * in the *_device calls. 128 bytes. */
typedef struct {
  const slamgpu_keypoint* kps; /* [n] undistorted_keypoints                                */
  const uint8_t* desc;         /* [n][32] descriptors                                       */
  const float* u_right;        /* [n] right_coords (< 0: monocular)                         */
  const uint8_t* has_mp;       /* [n] GetMapPoint(i) != NULL (SearchForTriangulation)       */
  const uint32_t* nodes;       /* FeatureVector: [n_nodes] ascending (SearchForTriangulation) */
  const int32_t* node_start;   /* [n_nodes + 1]                                             */
  const uint32_t* node_feats;  /* [node_start[n_nodes]]                                     */
  int32_t n, n_nodes;
  float Rcw[9];                /* GetRotation(), row-major                                  */
  float tcw[3];                /* GetTranslation()                                          */
  float Ow[3];                 /* GetCameraCenter()                                         */
  float pad;
} slamgpu_kf;

/* ---- SearchForTriangulation --------------------------------------------------------------- */
/* match12[i] = vMatches12[i] (the pKF2 keypoint matched to pKF1 keypoint i, or -1); the
 * reference's vMatchedPairs = the (i, match12[i]) with match12[i] >= 0, ascending i.
 * cam = pKF2's fx, fy, cx, cy (bf unused); lv = pKF2's level tables; F12 row-major. */
int slamgpu_search_for_triangulation(const slamgpu_kf* kf1, const slamgpu_kf* kf2,
                                     const float* F12, const slamgpu_camera* cam,
                                     const slamgpu_levels* lv, int only_stereo, int check_ori,
                                     int32_t* match12, int* nmatches);

/* A keyframe pair of a batched call: d_kfs[kf1] against d_kfs[kf2]. 48 bytes. */
typedef struct {
  int32_t kf1, kf2;
  float F12[9];
  int32_t only_stereo;
} slamgpu_tri_pair;

/* Pair p writes d_match12 + p * match_stride and d_nmatches[p] (-1 if a keyframe exceeds
 * SLAMGPU_KF_MAX_FEATURES, or its FeatureVector names a feature >= n, or a candidate keypoint's
 * octave is outside [0, nlevels): such a pair's match row is left partly written). */
int slamgpu_search_for_triangulation_device(const slamgpu_kf* d_kfs,
                                            const slamgpu_tri_pair* d_pairs, int n_pairs,
                                            const slamgpu_camera* cam, const slamgpu_levels* lv,
                                            int check_ori, int32_t* d_match12,
                                            int64_t match_stride, int32_t* d_nmatches,
                                            void* stream);

/* ---- Fuse ------------------------------------------------------------------------------------ */
/* A map point offered to Fuse(pKF, vpMapPoints, th). 80 bytes. */
typedef struct {
  float xyz[3];     /* GetWorldPos()                                                    */
  float normal[3];  /* GetNormal()                                                      */
  float min_dist;   /* min_dist_ (GetMinDistanceInvariance() = 0.8f * min_dist_)        */
  float max_dist;   /* max_dist_ (GetMaxDistanceInvariance() = 1.2f * max_dist_)        */
  int32_t skip;     /* !pMP || isBad() || IsInKeyFrame(pKF) when the call starts         */
  int32_t pad[3];
  uint8_t desc[32]; /* GetDescriptor()                                                  */
} slamgpu_fuse_point;

/* The candidate search of Fuse (:821-928) for every point: best_idx[i] = the keypoint point i
 * fuses into (bestDist <= TH_LOW), else -1; best_dist[i] = bestDist (256 if no candidate).
 * *nfused = #(best_idx >= 0). The adapter then walks the points in order and, re-checking
 * isBad() / IsInKeyFrame(pKF) (earlier Replace calls can change them), does the reference's
 * Replace / AddObservation (:931-949). cam = pKF's fx, fy, cx, cy, mbf. */
int slamgpu_fuse(const slamgpu_kf* kf, const slamgpu_fuse_point* pts, int n_pts, float th,
                 const slamgpu_camera* cam, const slamgpu_levels* lv, const slamgpu_kf_grid* grid,
                 int32_t* best_idx, int32_t* best_dist, int* nfused);

/* Batched: point i is fused into d_kfs[d_point_kf[i]]. */
int slamgpu_fuse_device(const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_pts,
                        const int32_t* d_point_kf, int n_pts, float th,
                        const slamgpu_camera* cam, const slamgpu_levels* lv,
                        const slamgpu_kf_grid* grid, int32_t* d_best_idx, int32_t* d_best_dist,
                        void* stream);

/* ---- CreateNewMapPoints --------------------------------------------------------------------- */
/* LocalMapper::CreateNewMapPoints (src/core/local_mapper.cpp:258-492) for one current keyframe and
 * its neighbours, in order: SearchForTriangulation against neighbour k on the current has_mp, the
 * triangulation and the six acceptance tests of :332-471 for every matched pair in ascending idx1,
 * and has_mp[idx1] = 1 for every accepted pair before neighbour k + 1 is searched. The baseline
 * tests (:290-304) stay with the caller: a neighbour that fails them is passed with skip = 1. */

/* Per-keypoint status of one neighbour: 0 = no match, 1 .. 3 = accepted (the source of the point),
 * negative = the test of the reference that dropped the pair. */
#define SLAMGPU_NP_DLT 1               /* linear triangulation (:375-392)                     */
#define SLAMGPU_NP_STEREO1 2           /* UnprojectStereo of the current keyframe (:394-396)  */
#define SLAMGPU_NP_STEREO2 3           /* UnprojectStereo of the neighbour (:397-399)         */
#define SLAMGPU_NP_W_ZERO (-1)         /* x3D(3) == 0 (:387)                                  */
#define SLAMGPU_NP_LOW_PARALLAX (-2)   /* no stereo and very low parallax (:400-402)          */
#define SLAMGPU_NP_BEHIND1 (-3)        /* z <= 0 in the current keyframe (:407)               */
#define SLAMGPU_NP_BEHIND2 (-4)        /* z <= 0 in the neighbour (:412)                      */
#define SLAMGPU_NP_REPROJ1_STEREO (-5) /* :428                                                */
#define SLAMGPU_NP_REPROJ1_MONO (-6)   /* :432                                                */
#define SLAMGPU_NP_REPROJ2_STEREO (-7) /* :449                                                */
#define SLAMGPU_NP_REPROJ2_MONO (-8)   /* :453                                                */
#define SLAMGPU_NP_DIST_ZERO (-9)      /* :462                                                */
#define SLAMGPU_NP_SCALE (-10)         /* scale consistency (:469)                            */
#define SLAMGPU_NP_NO_DEPTH (-11)      /* UnprojectStereo of a depth <= 0 (keyframe.cpp:489)  */
#define SLAMGPU_NP_MALFORMED (-12)     /* match >= n2, or an octave outside [0, nlevels)      */

typedef struct {              /* what CreateNewMapPoints reads beyond slamgpu_kf            */
  const float* depth;         /* [n] depths                                                  */
  const slamgpu_keypoint* raw_kps; /* [n] keypoints (UnprojectStereo); NULL = kf.kps         */
  slamgpu_camera cam;         /* fx fy cx cy mbf of this keyframe                            */
  float mb;
} slamgpu_kf_stereo;

typedef struct {              /* one neighbour of one job                                    */
  int32_t kf2;                /* index into d_kfs / d_kf_stereo                              */
  float F12[9];               /* ComputeFundamentalMatrix(current, neighbour), row-major     */
  int32_t skip;               /* the baseline test failed: no search, status row all 0       */
  int32_t first_obs;          /* whose descriptor the new points get: 0 = the current
                                 keyframe's, 1 = the neighbour's (the keyframe that comes
                                 first in the new MapPoint's std::map<KeyFrame*, size_t>)    */
} slamgpu_newpoints_nbor;

typedef struct {              /* one current keyframe                                        */
  int32_t kf1, first_nbor, n_nbors; /* neighbours d_nbors[first_nbor .. first_nbor + n_nbors) */
  uint8_t* has_mp1;           /* == d_kfs[kf1].has_mp, written in place                      */
} slamgpu_newpoints_job;

typedef struct {              /* where new point i of a job came from                        */
  int32_t neighbour;          /* 0 .. n_nbors - 1                                            */
  int32_t idx1, idx2;         /* the keypoints of the current keyframe and of the neighbour  */
  int32_t source;             /* SLAMGPU_NP_DLT / _STEREO1 / _STEREO2                        */
} slamgpu_new_point;

size_t slamgpu_create_new_map_points_scratch_bytes(int n_jobs, int max_nbors);

/* Every job's chain, enqueued on `stream`: one preparing launch, then for k = 0 .. max_nbors - 1
 * the search and the triangulation of neighbour k of every job (2 * max_nbors + 1 launches, no
 * synchronisation, no allocation). Jobs must not share a kf1; a neighbour's has_mp is only read.
 * cam: fx fy cx cy of the neighbours, as SearchForTriangulation reads them; lv: the level tables
 * of all keyframes (ratioFactor = 1.5f * scale[1]).
 * Outputs of job j: d_n_new[j]; d_points / d_new + j * point_stride, the new points in the
 * reference's order (neighbour, then ascending idx1), d_points ready for slamgpu_fuse_device;
 * d_status + (j * max_nbors + k) * status_stride, the status of every keypoint of kf1 against
 * neighbour k (rows k >= n_nbors are not written). point_stride and status_stride >= n of kf1.
 * d_n_new[j] = -1 when a search of the job reported -1 (slamgpu_search_for_triangulation_device) or
 * point_stride is too small: the job stops there, and what it wrote for that and the later
 * neighbours is undefined. */
int slamgpu_create_new_map_points_device(
    const slamgpu_kf* d_kfs, const slamgpu_kf_stereo* d_kf_stereo,
    const slamgpu_newpoints_job* d_jobs, int n_jobs, const slamgpu_newpoints_nbor* d_nbors,
    int max_nbors, const slamgpu_camera* cam, const slamgpu_levels* lv, int check_ori,
    int32_t* d_n_new, slamgpu_fuse_point* d_points, slamgpu_new_point* d_new, int64_t point_stride,
    int8_t* d_status, int64_t status_stride, void* d_scratch, size_t scratch_bytes, void* stream);

/* One job, synchronous, host pointers: kfs[0] / st[0] the current keyframe, kfs[1 + k] / st[1 + k]
 * neighbour k (nbors[k].kf2 is ignored; at most 64 neighbours). has_mp1 [n1], in and out: the
 * current keyframe's flags at entry (kfs[0].has_mp is not read), the updated ones at return.
 * points / news [n1], status [n_nbors][n1]. *n_new = -1 as above. */
int slamgpu_create_new_map_points(const slamgpu_kf* kfs, const slamgpu_kf_stereo* st,
                                  const slamgpu_newpoints_nbor* nbors, int n_nbors,
                                  const slamgpu_camera* cam, const slamgpu_levels* lv, int check_ori,
                                  uint8_t* has_mp1, slamgpu_fuse_point* points,
                                  slamgpu_new_point* news, int8_t* status, int* n_new);

const char* slamgpu_kfmatch_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_KFMATCH_H_ */
