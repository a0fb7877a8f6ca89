/*
 * tests/relocmatch_ref.c -- CPU restatement of the relocalisation matcher (TEST INFRASTRUCTURE
 * ONLY; built on demand by tests/relocmatch_ref.py against oracle/liborb_oracle.so):
 *   src/orb_features/orb_matcher.cpp:1455-1582  SearchByProjection(CurrentFrame, pKF,
 *                                               sAlreadyFound, th, ORBdist)
 *   src/orb_features/orb_matcher.cpp:1584-1625  ComputeThreeMaxima
 *   src/data/map_point.cpp:356-364, :382-396    Get{Min,Max}DistanceInvariance, PredictScale(Frame*)
 *   src/data/frame.cpp:348-403                  Frame::GetFeaturesInArea (oc_features_in_area)
 * stated statement by statement; GetFeaturesInArea, DescriptorDistance and std::log(float) are the
 * oracle's (oc_features_in_area, oc_descriptor_distance, oc_logf).
 *
 * Float rules assumed (built with -ffp-contract=off): Rcw*x3Dw + tcw is OpenCV's small gemm, a
 * float dot plus a (double) add; invzc = 1.0 / z is a double division rounded to float; the
 * Release build contracts u = fx*xc*invzc + cx to fma(fx*xc, invzc, cx) (the association the
 * frame-to-frame overload's restatement, oracle/matcher_oracle.c, uses for the same expression);
 * cv::norm of a 3-vector is a double sum of squares, its sqrt rounded to float;
 * Get{Max,Min}DistanceInvariance are 1.2f * max_dist_ and 0.8f * min_dist_; PredictScale is
 * ceil(logf(max_dist_ / dist) / log_scale_factor) in float, clamped to [0, nlevels - 1]. Ow arrives
 * from the caller (the caller's cv::Mat arithmetic makes -Rcw.t()*tcw; this file takes no position
 * on MatExpr rounding).
 *
 * Undefined in the reference, defined here (and in the device path): a query whose invzc, u, v,
 * dist3D or max_dist / dist3D is not finite, or whose ratio is <= 0, reaches a float -> int
 * conversion of NaN / infinity in GetFeaturesInArea or PredictScale; such a query matches nothing
 * and writes nothing.
 *
 * PARITY STATUS: "parity unpinned" against the reference binary (OpenCV absent; no fixtures).
 * Pinned by tests/test_relocmatch_ref.py against an independent pure-Python restatement.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/orb_oracle.h"

#define RR_HISTO_LENGTH 30

/* == slamgpu_reloc_query, 64 B */
typedef struct {
  float xyz[3];
  float max_dist, min_dist; /* max_dist_ / min_dist_ as stored */
  float kf_angle;           /* pKF->undistorted_keypoints[i].angle */
  int32_t mp_id;
  int32_t skip;             /* !pMP || pMP->isBad() || sAlreadyFound.count(pMP) */
  uint8_t desc[32];
} rr_query;

static inline float gemm_row(const float* R, int r, const float* x, float c) {
  const float dot = R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2];
  return (float)((double)dot + (double)c);
}

static inline float norm3(const float* p) {
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += (double)p[k] * (double)p[k];
  return (float)sqrt(s);
}

/* map_point[n]: the frame's map point slots, in/out (-1 = nullptr). query_kp[nq]: the keypoint
 * query i set at :1543 (-1 none; kept when the rotation tail clears the slot again).
 * passed_over[nq] (test instrumentation): how many candidates of distance <= orb_dist query i
 * skipped at :1526 because a query before it in this call had taken them (slots occupied at
 * entry are not counted). *n_removed: the slots the tail :1571-1578 cleared. Returns nmatches. */
int rr_search_by_projection_reloc(const oc_keypoint* kps, const uint8_t* desc, int n,
                                  const oc_grid_geom* g, float fx, float fy, float cx, float cy,
                                  const float* scale, int nlevels, float log_scale_factor,
                                  const float* Rcw, const float* tcw, const float* Ow, float th,
                                  int orb_dist, int check_ori, const rr_query* queries, int nq,
                                  int32_t* map_point, int32_t* query_kp, int32_t* passed_over,
                                  int32_t* n_removed) {
  int nmatches = 0;
  int* rotHist[RR_HISTO_LENGTH];
  int rotCount[RR_HISTO_LENGTH];
  for (int i = 0; i < RR_HISTO_LENGTH; i++) {
    rotHist[i] = (int*)malloc(sizeof(int) * (size_t)(nq > 0 ? nq : 1));
    rotCount[i] = 0;
  }
  const float factor = 1.0f / RR_HISTO_LENGTH;
  int* vIndices2 = (int*)malloc(sizeof(int) * (size_t)(n + 1));
  uint8_t* at_entry = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));
  for (int j = 0; j < n; j++) at_entry[j] = map_point[j] >= 0;
  *n_removed = 0;

  for (int i = 0; i < nq; i++) {
    const rr_query* pMP = &queries[i];
    query_kp[i] = -1;
    passed_over[i] = 0;
    if (pMP->skip) continue;

    const float xc = gemm_row(Rcw, 0, pMP->xyz, tcw[0]);
    const float yc = gemm_row(Rcw, 1, pMP->xyz, tcw[1]);
    const float zc = gemm_row(Rcw, 2, pMP->xyz, tcw[2]);
    const float invzc = (float)(1.0 / (double)zc);

    const float u = fmaf(fx * xc, invzc, cx);
    const float v = fmaf(fy * yc, invzc, cy);
    if (!isfinite(invzc) || !isfinite(u) || !isfinite(v)) continue; /* defined here */

    if (u < g->min_x || u > g->max_x) continue;
    if (v < g->min_y || v > g->max_y) continue;

    const float PO[3] = {pMP->xyz[0] - Ow[0], pMP->xyz[1] - Ow[1], pMP->xyz[2] - Ow[2]};
    const float dist3D = norm3(PO);
    if (!isfinite(dist3D)) continue; /* defined here */

    const float maxDistance = 1.2f * pMP->max_dist;
    const float minDistance = 0.8f * pMP->min_dist;
    if (dist3D < minDistance || dist3D > maxDistance) continue;

    /* PredictScale(dist3D, &CurrentFrame) */
    const float ratio = pMP->max_dist / dist3D;
    if (!isfinite(ratio) || !(ratio > 0.0f)) continue; /* defined here */
    int nPredictedLevel = (int)ceilf(oc_logf(ratio) / log_scale_factor);
    if (nPredictedLevel < 0) {
      nPredictedLevel = 0;
    } else if (nPredictedLevel >= nlevels) {
      nPredictedLevel = nlevels - 1;
    }

    const float radius = th * scale[nPredictedLevel];
    const int nc = oc_features_in_area(g, kps, n, u, v, radius, nPredictedLevel - 1,
                                       nPredictedLevel + 1, vIndices2, n + 1);
    if (nc == 0) continue;

    int bestDist = 256;
    int bestIdx2 = -1;
    for (int c = 0; c < nc; c++) {
      const int i2 = vIndices2[c];
      if (map_point[i2] >= 0) {
        if (!at_entry[i2] && oc_descriptor_distance(pMP->desc, desc + (size_t)i2 * 32) <= orb_dist)
          passed_over[i]++;
        continue;
      }
      const int dist = oc_descriptor_distance(pMP->desc, desc + (size_t)i2 * 32);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx2 = i2;
      }
    }

    /* orb_dist <= 256 and bestDist starts at 256: with orb_dist == 256 and no free candidate the
     * reference would SetMapPoint(-1, ...); the C ABI's range [0, 256] keeps the test, the index
     * check states what an out-of-range vector write cannot */
    if (bestDist <= orb_dist && bestIdx2 >= 0) {
      map_point[bestIdx2] = pMP->mp_id;
      query_kp[i] = bestIdx2;
      ++nmatches;
      if (check_ori) {
        float rot = pMP->kf_angle - kps[bestIdx2].angle;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == RR_HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < RR_HISTO_LENGTH) rotHist[bin][rotCount[bin]++] = bestIdx2;
      }
    }
  }

  if (check_ori) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < RR_HISTO_LENGTH; i++) {
      const int s = rotCount[i];
      if (s > max1) {
        max3 = max2;
        max2 = max1;
        max1 = s;
        ind3 = ind2;
        ind2 = ind1;
        ind1 = i;
      } else if (s > max2) {
        max3 = max2;
        max2 = s;
        ind3 = ind2;
        ind2 = i;
      } else if (s > max3) {
        max3 = s;
        ind3 = i;
      }
    }
    if (max2 < 0.1f * (float)max1) {
      ind2 = -1;
      ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
      ind3 = -1;
    }
    for (int i = 0; i < RR_HISTO_LENGTH; i++) {
      if (i != ind1 && i != ind2 && i != ind3) {
        for (int j = 0; j < rotCount[i]; j++) {
          map_point[rotHist[i][j]] = -1;
          --nmatches;
          ++*n_removed;
        }
      }
    }
  }

  free(at_entry);
  free(vIndices2);
  for (int i = 0; i < RR_HISTO_LENGTH; i++) free(rotHist[i]);
  return nmatches;
}

#ifdef RELOCMATCH_REF_MAIN
/* Stand-alone driver for a sanitizer build (address + undefined): a pseudo-random frame on the
 * KITTI-size grid, queries placed on its keypoints (with occupied slots, skips, duplicates and
 * the defined-UB records: NaN / infinite coordinates, zero depth, zero max_dist), both stages
 * (10, 100) and (3, 64), with and without the rotation check. Prints the counts. */
#include <stdio.h>

static uint32_t rng_state = 12345u;
static uint32_t rnd(void) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}
static float frand(void) { return (float)(rnd() & 0xffff) / 65536.0f; }

int main(void) {
  enum { N = 1500, NQ = 2 * N + 8 };
  oc_grid_geom g;
  oc_grid_geom_init(&g, 1241, 376);
  const float fx = 718.856f, fy = 718.856f, cx = 607.1928f, cy = 185.2157f;
  float scale[8];
  scale[0] = 1.0f;
  for (int l = 1; l < 8; l++) scale[l] = (float)((double)scale[l - 1] * 1.2);
  const float lsf = oc_logf(1.2f);
  oc_keypoint* kps = (oc_keypoint*)calloc(N, sizeof(oc_keypoint));
  uint8_t* desc = (uint8_t*)malloc((size_t)N * 32);
  rr_query* q = (rr_query*)calloc(NQ, sizeof(rr_query));
  int32_t* mp = (int32_t*)malloc(sizeof(int32_t) * N);
  int32_t* qk = (int32_t*)malloc(sizeof(int32_t) * NQ);
  int32_t* po = (int32_t*)malloc(sizeof(int32_t) * NQ);
  for (int i = 0; i < N; i++) {
    kps[i].x = 20.0f + frand() * 1200.0f;
    kps[i].y = 20.0f + frand() * 330.0f;
    kps[i].octave = (int32_t)(rnd() % 8);
    kps[i].angle = frand() * 360.0f;
    for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = (uint8_t)rnd();
  }
  const float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0.01f, -0.02f, 0.03f};
  const float Ow[3] = {-0.01f, 0.02f, -0.03f};
  for (int i = 0; i < NQ; i++) {
    const int j = i % N;
    const float z = 5.0f + frand() * 40.0f;
    q[i].xyz[0] = (kps[j].x - cx) * z / fx + Ow[0];
    q[i].xyz[1] = (kps[j].y - cy) * z / fy + Ow[1];
    q[i].xyz[2] = z + Ow[2];
    q[i].max_dist = z * scale[kps[j].octave];
    q[i].min_dist = q[i].max_dist / scale[7];
    q[i].kf_angle = kps[j].angle + (i % 7 == 0 ? 90.0f : 3.0f * frand());
    q[i].mp_id = i;
    q[i].skip = (i % 11) == 0;
    memcpy(q[i].desc, desc + (size_t)j * 32, 32);
    for (int b = 0; b < (int)(rnd() % 12); b++) q[i].desc[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
  }
  q[NQ - 1].xyz[0] = NAN;
  q[NQ - 2].xyz[1] = INFINITY;
  q[NQ - 3].xyz[2] = Ow[2] - tcw[2]; /* zc == 0 -> invzc infinite */
  q[NQ - 4].max_dist = 0.0f;
  q[NQ - 4].min_dist = 0.0f;
  q[NQ - 5].max_dist = INFINITY;
  q[NQ - 6].xyz[2] = -q[NQ - 6].xyz[2]; /* behind the camera */
  q[NQ - 7].max_dist = NAN;
  q[NQ - 8].xyz[0] = 3.0e38f;
  for (int ori = 0; ori < 2; ori++) {
    for (int j = 0; j < N; j++) mp[j] = (j % 5 == 0) ? 100000 + j : -1;
    int rem = 0;
    const int a = rr_search_by_projection_reloc(kps, desc, N, &g, fx, fy, cx, cy, scale, 8, lsf, Rcw,
                                                tcw, Ow, 10.0f, 100, ori, q, NQ, mp, qk, po, &rem);
    int passed = 0;
    for (int i = 0; i < NQ; i++) passed += po[i] > 0;
    int rem2 = 0;
    const int b = rr_search_by_projection_reloc(kps, desc, N, &g, fx, fy, cx, cy, scale, 8, lsf, Rcw,
                                                tcw, Ow, 3.0f, 64, ori, q, NQ, mp, qk, po, &rem2);
    printf("check_ori %d: (10,100) nmatches %d removed %d passed-over queries %d; (3,64) nmatches %d "
           "removed %d\n", ori, a, rem, passed, b, rem2);
  }
  free(po);
  free(qk);
  free(mp);
  free(q);
  free(desc);
  free(kps);
  return 0;
}
#endif
