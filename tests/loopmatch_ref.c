/*
 * tests/loopmatch_ref.c -- CPU restatement of the LoopCloser's three Sim3 matchers (TEST
 * INFRASTRUCTURE ONLY; built on demand by tests/loopmatch_ref.py against oracle/liborb_oracle.so):
 *   src/orb_features/orb_matcher.cpp:384-497    SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
 *   src/orb_features/orb_matcher.cpp:956-1079   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) -- the
 *                                               candidate search (:979-1059)
 *   src/orb_features/orb_matcher.cpp:1081-1310  SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 *   src/data/map_point.cpp:356-381              Get{Min,Max}DistanceInvariance, PredictScale
 *   src/data/keyframe.cpp:442-476, :494-496     KeyFrame::GetFeaturesInArea, IsInImage
 * stated statement by statement; GetFeaturesInArea, PredictScale, DescriptorDistance and
 * std::log(float) are the oracle's (oc_features_in_area, oc_predict_scale,
 * oc_descriptor_distance, oc_logf inside oc_predict_scale).
 *
 * Float rules assumed (those of oracle/kfmatch_oracle.c; built with -ffp-contract=off): the
 * Release build contracts u = fx*x + cx, v = fy*y + cy to fma(fx, x, cx), fma(fy, y, cy); OpenCV
 * does not contract: Rcw*X + tcw, sR21*p + t21 and sR12*p + t12 are its small gemm, a float dot
 * plus a (double) add; cv::norm of a 3-vector is a double sum of squares, its sqrt rounded to
 * float; Mat::dot is a double sum of exact products. invz = 1.0/z (:998, :1150, :1230, a double
 * division rounded to float) equals the float division 1.0f/z (53 >= 2*24 + 2 bits: the double
 * rounding is innocuous); :425 is a float division as written. None of the three methods applies
 * the chi-square reprojection gates of the plain Fuse (:880-905) or reads the right coordinate.
 *
 * The transforms arrive DECOMPOSED (Rcw, tcw, Ow of Scw at :393-397 / :965-969; sR12, t12, sR21,
 * t21 at :1103-1105): the caller's own cv::Mat arithmetic makes them, this file takes no
 * position on MatExpr rounding.
 *
 * PARITY STATUS: "parity unpinned" against the reference binary (OpenCV / DBoW2 absent; no
 * fixtures). Pinned by tests/test_loopmatch_ref.py against an independent pure-Python
 * restatement.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/orb_oracle.h"

/* OpenCV small gemm row: (float)((double)(float dot) + (double)c). */
static inline float gemm_row(const float* R, int r, const float* x, float c) {
  const float dot = R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2];
  return (float)((double)dot + (double)c);
}

static inline float norm3(const float* p) {
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += (double)p[k] * (double)p[k];
  return (float)sqrt(s);
}

typedef struct {
  const oc_keypoint* kps;
  const uint8_t* desc;
  int n;
  const oc_grid_geom* g;
  float fx, fy, cx, cy;
  const float* scale;
  int nlevels;
  float log_scale_factor;
} lr_kf;

/* :415-456 / :988-1030: everything between GetWorldPos() and GetFeaturesInArea() of the two Scw
 * methods. Returns the candidate count (0 also when a gate rejects the point). */
static int scw_candidates(const lr_kf* K, const float* Rcw, const float* tcw, const float* Ow,
                          const oc_fuse_point* P, float th, int* level, int* cand) {
  const float xc = gemm_row(Rcw, 0, P->xyz, tcw[0]);
  const float yc = gemm_row(Rcw, 1, P->xyz, tcw[1]);
  const float zc = gemm_row(Rcw, 2, P->xyz, tcw[2]);
  if (zc < 0.0f) return 0;
  const float invz = 1.0f / zc;
  const float x = xc * invz, y = yc * invz;
  const float u = fmaf(K->fx, x, K->cx), v = fmaf(K->fy, y, K->cy);
  if (!(u >= K->g->min_x && u < K->g->max_x && v >= K->g->min_y && v < K->g->max_y)) return 0;
  const float maxDistance = 1.2f * P->max_dist, minDistance = 0.8f * P->min_dist;
  const float PO[3] = {P->xyz[0] - Ow[0], P->xyz[1] - Ow[1], P->xyz[2] - Ow[2]};
  const float dist = norm3(PO);
  if (dist < minDistance || dist > maxDistance) return 0;
  double dot = 0.0;
  for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)P->normal[k];
  if (dot < 0.5 * (double)dist) return 0;
  const int nPredictedLevel = oc_predict_scale(P->max_dist, dist, K->log_scale_factor, K->nlevels);
  const float radius = th * K->scale[nPredictedLevel];
  *level = nPredictedLevel;
  return oc_features_in_area(K->g, K->kps, K->n, u, v, radius, -1, -1, cand, K->n + 1);
}

/* Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :979-1059 + the bestDist <= TH_LOW test of :1061.
 * pts[i].skip = isBad() || spAlreadyFound.count(pMP). best_dist 256 when no candidate. */
int lr_fuse_sim3(const oc_keypoint* kps, const uint8_t* desc, int n, const oc_grid_geom* g,
                 const float* Rcw, const float* tcw, const float* Ow, float fx, float fy, float cx,
                 float cy, const float* scale, int nlevels, float log_scale_factor,
                 const oc_fuse_point* pts, int n_pts, float th, int32_t* best_idx,
                 int32_t* best_dist) {
  const int TH_LOW = 50;
  const lr_kf K = {kps, desc, n, g, fx, fy, cx, cy, scale, nlevels, log_scale_factor};
  int nFused = 0;
  int* cand = (int*)malloc(sizeof(int) * (size_t)(n + 1));
  for (int iMP = 0; iMP < n_pts; iMP++) {
    const oc_fuse_point* P = &pts[iMP];
    best_idx[iMP] = -1;
    best_dist[iMP] = 256;
    if (P->skip) continue;
    int nPredictedLevel = 0;
    const int nc = scw_candidates(&K, Rcw, tcw, Ow, P, th, &nPredictedLevel, cand);
    if (nc == 0) continue;
    int bestDist = 0x7fffffff, bestIdx = -1;
    for (int c = 0; c < nc; c++) {
      const int idx = cand[c];
      const int kpLevel = kps[idx].octave;
      if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
      const int dist = oc_descriptor_distance(P->desc, desc + (size_t)idx * 32);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx = idx;
      }
    }
    if (bestIdx >= 0) best_dist[iMP] = bestDist;
    if (bestDist <= TH_LOW) {
      best_idx[iMP] = bestIdx;
      nFused++;
    }
  }
  free(cand);
  return nFused;
}

/* SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :406-494. matched_in[idx] = vpMatched[idx]
 * != nullptr at entry; kp_point[idx] = the point that wrote vpMatched[idx] (:490) or -1;
 * point_kp[i] = the keypoint point i claimed or -1. passed_over[i] (test instrumentation) = how
 * many candidates of distance <= TH_LOW, of the right octave, point i skipped at :469 because a
 * point before it had claimed them (keypoints matched at entry are not counted). */
int lr_search_by_projection_sim3(const oc_keypoint* kps, const uint8_t* desc, int n,
                                 const oc_grid_geom* g, const float* Rcw, const float* tcw,
                                 const float* Ow, float fx, float fy, float cx, float cy,
                                 const float* scale, int nlevels, float log_scale_factor,
                                 const oc_fuse_point* pts, int n_pts, const uint8_t* matched_in,
                                 float th, int32_t* kp_point, int32_t* point_kp,
                                 int32_t* passed_over) {
  const int TH_LOW = 50;
  const lr_kf K = {kps, desc, n, g, fx, fy, cx, cy, scale, nlevels, log_scale_factor};
  int nmatches = 0;
  int* cand = (int*)malloc(sizeof(int) * (size_t)(n + 1));
  uint8_t* vpMatched = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));
  for (int j = 0; j < n; j++) {
    vpMatched[j] = matched_in[j] != 0;
    kp_point[j] = -1;
  }
  for (int iMP = 0; iMP < n_pts; iMP++) {
    const oc_fuse_point* P = &pts[iMP];
    point_kp[iMP] = -1;
    passed_over[iMP] = 0;
    if (P->skip) continue;
    int nPredictedLevel = 0;
    const int nc = scw_candidates(&K, Rcw, tcw, Ow, P, th, &nPredictedLevel, cand);
    if (nc == 0) continue;
    int bestDist = 256, bestIdx = -1;
    for (int c = 0; c < nc; c++) {
      const int idx = cand[c];
      const int kpLevel = kps[idx].octave;
      if (vpMatched[idx]) {
        if (!matched_in[idx] && kpLevel >= nPredictedLevel - 1 && kpLevel <= nPredictedLevel &&
            oc_descriptor_distance(P->desc, desc + (size_t)idx * 32) <= TH_LOW)
          passed_over[iMP]++;
        continue;
      }
      if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
      const int dist = oc_descriptor_distance(P->desc, desc + (size_t)idx * 32);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx = idx;
      }
    }
    if (bestDist <= TH_LOW) {
      vpMatched[bestIdx] = 1;
      kp_point[bestIdx] = iMP;
      point_kp[iMP] = bestIdx;
      nmatches++;
    }
  }
  free(vpMatched);
  free(cand);
  return nmatches;
}

/* One direction of SearchBySim3 (:1132-1209 with A = 1, B = 2; :1212-1289 with A = 2, B = 1):
 * the points of keyframe A (camera pose RAw, tAw) through sR, t into keyframe B. */
static void sim3_direction(const lr_kf* B, const float* RAw, const float* tAw, const float* sR,
                           const float* t, const oc_fuse_point* mpA, const uint8_t* alreadyA,
                           int nA, float th, int32_t* vnMatch, int* cand) {
  const int TH_HIGH = 100;
  for (int i = 0; i < nA; i++) {
    const oc_fuse_point* P = &mpA[i];
    vnMatch[i] = -1;
    if (P->skip || alreadyA[i]) continue;
    const float p3Dc1[3] = {gemm_row(RAw, 0, P->xyz, tAw[0]), gemm_row(RAw, 1, P->xyz, tAw[1]),
                            gemm_row(RAw, 2, P->xyz, tAw[2])};
    const float p3Dc2[3] = {gemm_row(sR, 0, p3Dc1, t[0]), gemm_row(sR, 1, p3Dc1, t[1]),
                            gemm_row(sR, 2, p3Dc1, t[2])};
    if (p3Dc2[2] < 0.0f) continue;
    const float invz = 1.0f / p3Dc2[2];
    const float x = p3Dc2[0] * invz, y = p3Dc2[1] * invz;
    const float u = fmaf(B->fx, x, B->cx), v = fmaf(B->fy, y, B->cy);
    if (!(u >= B->g->min_x && u < B->g->max_x && v >= B->g->min_y && v < B->g->max_y)) continue;
    const float maxDistance = 1.2f * P->max_dist, minDistance = 0.8f * P->min_dist;
    const float dist3D = norm3(p3Dc2);
    if (dist3D < minDistance || dist3D > maxDistance) continue;
    const int nPredictedLevel =
        oc_predict_scale(P->max_dist, dist3D, B->log_scale_factor, B->nlevels);
    const float radius = th * B->scale[nPredictedLevel];
    const int nc = oc_features_in_area(B->g, B->kps, B->n, u, v, radius, -1, -1, cand, B->n + 1);
    if (nc == 0) continue;
    int bestDist = 0x7fffffff, bestIdx = -1;
    for (int c = 0; c < nc; c++) {
      const int idx = cand[c];
      const int octave = B->kps[idx].octave;
      if (octave < nPredictedLevel - 1 || octave > nPredictedLevel) continue;
      const int dist = oc_descriptor_distance(P->desc, B->desc + (size_t)idx * 32);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx = idx;
      }
    }
    if (bestDist <= TH_HIGH) vnMatch[i] = bestIdx;
  }
}

/* SearchBySim3 :1081-1310. T1w / T2w = R (row-major) then t of GetRotation() / GetTranslation().
 * match12[i1] = the kf2 feature whose map point :1303 writes into vpMatches12[i1], or -1. */
int lr_search_by_sim3(const oc_keypoint* k1, const uint8_t* d1, int n1, const oc_keypoint* k2,
                      const uint8_t* d2, int n2, const oc_grid_geom* g, const float* T1w,
                      const float* T2w, const oc_fuse_point* mp1, const oc_fuse_point* mp2,
                      const uint8_t* already1, const uint8_t* already2, const float* sR12,
                      const float* t12, const float* sR21, const float* t21, float fx, float fy,
                      float cx, float cy, const float* scale, int nlevels, float log_scale_factor,
                      float th, int32_t* match12, int32_t* vnMatch1, int32_t* vnMatch2) {
  const lr_kf K1 = {k1, d1, n1, g, fx, fy, cx, cy, scale, nlevels, log_scale_factor};
  const lr_kf K2 = {k2, d2, n2, g, fx, fy, cx, cy, scale, nlevels, log_scale_factor};
  int* cand = (int*)malloc(sizeof(int) * (size_t)((n1 > n2 ? n1 : n2) + 1));
  sim3_direction(&K2, T1w, T1w + 9, sR21, t21, mp1, already1, n1, th, vnMatch1, cand);
  sim3_direction(&K1, T2w, T2w + 9, sR12, t12, mp2, already2, n2, th, vnMatch2, cand);
  free(cand);
  int nFound = 0;
  for (int i1 = 0; i1 < n1; i1++) {
    match12[i1] = -1;
    const int idx2 = vnMatch1[i1];
    if (idx2 >= 0) {
      const int idx1 = vnMatch2[idx2];
      if (idx1 == i1) {
        match12[i1] = idx2;
        nFound++;
      }
    }
  }
  return nFound;
}
