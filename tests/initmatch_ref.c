/*
 * tests/initmatch_ref.c -- CPU restatement of the monocular initialisation matcher (TEST
 * INFRASTRUCTURE ONLY; built on demand by tests/initmatch_ref.py against oracle/liborb_oracle.so):
 *   src/orb_features/orb_matcher.cpp:264-382    SearchForInitialization(F1, F2, vbPrevMatched,
 *                                               vnMatches12, windowSize)
 *   src/orb_features/orb_matcher.cpp:1584-1625  ComputeThreeMaxima
 *   src/data/frame.cpp:348-403                  Frame::GetFeaturesInArea (oc_features_in_area)
 * stated statement by statement; GetFeaturesInArea and DescriptorDistance are the oracle's
 * (oc_features_in_area, oc_descriptor_distance).
 *
 * Float rules (built with -ffp-contract=off): the window's half side is (float)windowSize (the
 * int argument converts at the call, frame.cpp:348); the ratio test :323 compares (float)bestDist
 * with the float product (float)bestDist2 * mfNNratio, bestDist2 possibly INT_MAX (2^31 as a
 * float); rot and the bin are the float expressions of :337-342.
 *
 * Undefined in the reference, defined here (and in the device path): a vbPrevMatched entry that is
 * not finite reaches a float -> int conversion of NaN / infinity in GetFeaturesInArea; such a query
 * matches nothing and its neighbours are unaffected.
 *
 * PARITY STATUS: "parity unpinned" against the reference binary (OpenCV absent; no fixtures).
 * Pinned by tests/test_initmatch_ref.py against an independent pure-Python restatement and by
 * constructed cases whose expected outputs follow from the cited lines.
 */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/orb_oracle.h"

#define IR_HISTO_LENGTH 30
#define IR_TH_LOW 50

/* == slamgpu_init_query, 64 B */
typedef struct {
  float angle;
  int32_t octave;
  int32_t pad[6];
  uint8_t desc[32];
} ir_query;

/* kps2 / desc2 [n2]: F2's undistorted keypoints and descriptors; queries[n1]: F1's;
 * prev_matched[n1][2] in/out; matches12[n1] out. Diagnostics (test instrumentation):
 * accept_kp[n1] the keypoint query i1 was matched to when it was accepted (-1 never accepted;
 * kept when the match is later taken over or removed), counts[0] the candidates skipped by
 * :306-307, counts[1] the take-overs (:325-329), counts[2] the matches the histogram tail
 * removed (:366-370), counts[3] the largest candidate list. Returns nmatches. */
int ir_search_for_initialization(const oc_keypoint* kps2, const uint8_t* desc2, int n2,
                                 const oc_grid_geom* g, const ir_query* queries, int n1,
                                 float nnratio, int window_size, int check_ori,
                                 float* prev_matched, int32_t* matches12, int32_t* accept_kp,
                                 int32_t* counts) {
  int nmatches = 0;
  int* rotHist[IR_HISTO_LENGTH];
  int rotCount[IR_HISTO_LENGTH];
  for (int i = 0; i < IR_HISTO_LENGTH; i++) {
    rotHist[i] = (int*)malloc(sizeof(int) * (size_t)(n1 > 0 ? n1 : 1));
    rotCount[i] = 0;
  }
  const float factor = 1.0f / IR_HISTO_LENGTH;
  int* vIndices2 = (int*)malloc(sizeof(int) * (size_t)(n2 + 1));
  int* vMatchedDistance = (int*)malloc(sizeof(int) * (size_t)(n2 + 1));
  int* vnMatches21 = (int*)malloc(sizeof(int) * (size_t)(n2 + 1));
  for (int j = 0; j < n2; j++) {
    vMatchedDistance[j] = INT_MAX;
    vnMatches21[j] = -1;
  }
  for (int i = 0; i < n1; i++) {
    matches12[i] = -1;
    accept_kp[i] = -1;
  }
  counts[0] = counts[1] = counts[2] = counts[3] = 0;

  for (int i1 = 0; i1 < n1; i1++) {
    const ir_query* kp1 = &queries[i1];
    const int level1 = kp1->octave;
    if (level1 > 0) continue;

    const float px = prev_matched[2 * i1], py = prev_matched[2 * i1 + 1];
    if (!isfinite(px) || !isfinite(py)) continue; /* defined here */
    const int nc = oc_features_in_area(g, kps2, n2, px, py, (float)window_size, level1, level1,
                                       vIndices2, n2 + 1);
    if (nc == 0) continue;
    if (nc > counts[3]) counts[3] = nc;

    int bestDist = INT_MAX;
    int bestDist2 = INT_MAX;
    int bestIdx2 = -1;
    for (int c = 0; c < nc; c++) {
      const int i2 = vIndices2[c];
      const int dist = oc_descriptor_distance(kp1->desc, desc2 + (size_t)i2 * 32);
      if (vMatchedDistance[i2] <= dist) {
        counts[0]++;
        continue;
      }
      if (dist < bestDist) {
        bestDist2 = bestDist;
        bestDist = dist;
        bestIdx2 = i2;
      } else if (dist < bestDist2) {
        bestDist2 = dist;
      }
    }

    if (bestDist <= IR_TH_LOW) {
      if ((float)bestDist < (float)bestDist2 * nnratio) {
        if (vnMatches21[bestIdx2] >= 0) {
          matches12[vnMatches21[bestIdx2]] = -1;
          nmatches--;
          counts[1]++;
        }
        matches12[i1] = bestIdx2;
        vnMatches21[bestIdx2] = i1;
        vMatchedDistance[bestIdx2] = bestDist;
        accept_kp[i1] = bestIdx2;
        nmatches++;

        if (check_ori) {
          float rot = kp1->angle - kps2[bestIdx2].angle;
          if (rot < 0.0) rot += 360.0f;
          int bin = (int)roundf(rot * factor);
          if (bin == IR_HISTO_LENGTH) bin = 0;
          if (bin >= 0 && bin < IR_HISTO_LENGTH) rotHist[bin][rotCount[bin]++] = i1;
        }
      }
    }
  }

  if (check_ori) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < IR_HISTO_LENGTH; i++) {
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
    for (int i = 0; i < IR_HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int j = 0; j < rotCount[i]; j++) {
        const int idx1 = rotHist[i][j];
        if (matches12[idx1] >= 0) {
          matches12[idx1] = -1;
          nmatches--;
          counts[2]++;
        }
      }
    }
  }

  for (int i1 = 0; i1 < n1; i1++)
    if (matches12[i1] >= 0) {
      prev_matched[2 * i1] = kps2[matches12[i1]].x;
      prev_matched[2 * i1 + 1] = kps2[matches12[i1]].y;
    }

  free(vnMatches21);
  free(vMatchedDistance);
  free(vIndices2);
  for (int i = 0; i < IR_HISTO_LENGTH; i++) free(rotHist[i]);
  return nmatches;
}

#ifdef INITMATCH_REF_MAIN
/* Stand-alone driver for a sanitizer build (address + undefined): a pseudo-random frame on the
 * KITTI-size grid, F1 = F2 moved by a few pixels with bits flipped (every third keypoint a copy of
 * its neighbour's descriptor, so keypoints are contested and taken over), non-finite vbPrevMatched
 * entries, windows off the grid, both window sizes, with and without the rotation check, n1 = 0
 * and n2 = 0. Prints the counts. */
#include <stdio.h>

static uint32_t rng_state = 12345u;
static uint32_t rnd(void) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}
static float frand(void) { return (float)(rnd() & 0xffff) / 65536.0f; }

int main(void) {
  enum { N = 1200 };
  oc_grid_geom g;
  oc_grid_geom_init(&g, 1241, 376);
  oc_keypoint* kps = (oc_keypoint*)calloc(N, sizeof(oc_keypoint));
  uint8_t* desc = (uint8_t*)malloc((size_t)N * 32);
  ir_query* q = (ir_query*)calloc(N, sizeof(ir_query));
  float* prev = (float*)malloc(sizeof(float) * 2 * N);
  int32_t* m12 = (int32_t*)malloc(sizeof(int32_t) * N);
  int32_t* ak = (int32_t*)malloc(sizeof(int32_t) * N);
  for (int i = 0; i < N; i++) {
    kps[i].x = 20.0f + frand() * 1200.0f;
    kps[i].y = 20.0f + frand() * 330.0f;
    kps[i].octave = (int32_t)(rnd() % 3);
    kps[i].angle = frand() * 360.0f;
    for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = (uint8_t)rnd();
  }
  for (int i = 0; i < N; i++) {
    const int j = (i % 3 == 2) ? i - 1 : i;
    q[i].angle = kps[j].angle + (i % 37 == 0 ? 90.0f : 3.0f * frand());
    if (q[i].angle >= 360.0f) q[i].angle -= 360.0f;
    q[i].octave = kps[i].octave;
    memcpy(q[i].desc, desc + (size_t)j * 32, 32);
    const int flips = (int)(rnd() % 30);
    for (int b = 0; b < flips; b++) q[i].desc[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
  }
  for (int ws = 0; ws < 2; ws++)
    for (int ori = 0; ori < 2; ori++) {
      for (int i = 0; i < N; i++) {
        const int j = (i % 3 == 2) ? i - 1 : i;
        prev[2 * i] = kps[j].x + 4.0f * frand() - 2.0f;
        prev[2 * i + 1] = kps[j].y + 4.0f * frand() - 2.0f;
      }
      prev[0] = NAN;
      prev[3] = INFINITY;
      prev[4] = -INFINITY;
      prev[6] = -5000.0f;
      prev[9] = 9000.0f;
      int32_t cnt[4];
      const int nm = ir_search_for_initialization(kps, desc, N, &g, q, N, ws ? 0.9f : 1.5f,
                                                  ws ? 100 : 30, ori, prev, m12, ak, cnt);
      int held = 0;
      for (int i = 0; i < N; i++) held += m12[i] >= 0;
      printf("window %d check_ori %d: nmatches %d (held %d) skipped %d take-overs %d removed %d "
             "max candidates %d\n", ws ? 100 : 30, ori, nm, held, cnt[0], cnt[1], cnt[2], cnt[3]);
      if (nm != held) return 1;
    }
  int32_t cnt[4];
  if (ir_search_for_initialization(kps, desc, N, &g, q, 0, 0.9f, 100, 1, prev, m12, ak, cnt) != 0)
    return 1;
  if (ir_search_for_initialization(kps, desc, 0, &g, q, N, 0.9f, 100, 1, prev, m12, ak, cnt) != 0)
    return 1;
  free(ak);
  free(m12);
  free(prev);
  free(q);
  free(desc);
  free(kps);
  return 0;
}
#endif
