// kfmatch.hip -- the keyframe-rate matchers of the LocalMapper on gfx950 (include/slamgpu_kfmatch.h).
//
//   search_tri   OrbMatcher::SearchForTriangulation (src/orb_features/orb_matcher.cpp:634-802):
//                one workgroup per keyframe pair, a wave per pKF1 FeatureVector entry (the
//                reference never marks vbMatched2, so the pKF1 features are independent), the
//                node's pKF2 candidates across lanes. The kept candidate is the last passing one
//                of minimal distance in node order (`dist > bestDist` skips, :717): the wave
//                minimum of (distance << 16 | ~position).
//   fuse         the candidate search of OrbMatcher::Fuse(pKF, vpMapPoints, th) (:804-928): a wave
//                per map point; projection, image / distance / viewing-angle gates and
//                PredictScale (glibc logf) on uniform values, then every keypoint of the keyframe
//                across lanes, in GetFeaturesInArea order (grid cell x-major, then index): the
//                first strict minimum is the minimum of (distance, cell, index).
// Float semantics follow oracle/kfmatch_oracle.c (the Release build's contractions as explicit
// fmaf, OpenCV's double sums). The rules shared with the other matchers (descriptor distance,
// Fuse's gate chain, grid cells, candidate keys, the rotation histogram) are orbmatch_device.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kfmatch_common.h"

namespace slamgpu {
namespace {

static_assert(sizeof(slamgpu_tri_pair) == 48, "slamgpu_tri_pair layout");

__device__ __forceinline__ int node_find(const uint32_t* nodes, int nn, uint32_t key) {
  int lo = 0, hi = nn;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nodes[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < nn && nodes[lo] == key) ? lo : -1;
}

// ---------------------------------------------------------------------------------------
constexpr int kTriWaves = 8;

__global__ __launch_bounds__(64 * kTriWaves) void search_tri_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_tri_pair* __restrict__ pairs,
    slamgpu_camera cam, slamgpu_levels lv, int check_ori, int32_t* __restrict__ match,
    int64_t match_stride, int32_t* __restrict__ nmatches) {
  __shared__ int8_t s_bin[kMaxFeat];
  __shared__ int s_hist[kRotWords<kTriWaves>], s_bad;
  const int pair = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const slamgpu_tri_pair P = pairs[pair];
  const slamgpu_kf& A = kfs[P.kf1];
  const slamgpu_kf& B = kfs[P.kf2];
  const int na = A.n, nb = B.n;
  if (na < 0 || nb < 0 || na > kMaxFeat || nb > kMaxFeat) {
    if (tid == 0) nmatches[pair] = -1;
    return;
  }
  int32_t* out = match + (int64_t)pair * match_stride;
  for (int i = tid; i < na; i += 64 * kTriWaves) {
    out[i] = -1;
    s_bin[i] = -1;
  }
  if (tid < kHisto) s_hist[tid] = 0;
  if (tid == 0) s_bad = 0;
  // epipole of pKF1's centre in pKF2 (:643-649)
  const float c2x = gemm_row(B.Rcw, A.Ow, B.tcw[0]);
  const float c2y = gemm_row(B.Rcw + 3, A.Ow, B.tcw[1]);
  const float c2z = gemm_row(B.Rcw + 6, A.Ow, B.tcw[2]);
  const float invz = 1.0f / c2z;
  const float ex = fmaf(cam.fx * c2x, invz, cam.cx), ey = fmaf(cam.fy * c2y, invz, cam.cy);
  const float* F = P.F12;
  __syncthreads();
  const int n_entries = A.n_nodes > 0 ? A.node_start[A.n_nodes] : 0;
  int acc = 0;
  for (int p = wid; p < n_entries; p += kTriWaves) {
    int lo = 0, hi = A.n_nodes;  // node of entry p: last ia with node_start[ia] <= p
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (A.node_start[mid] <= p) lo = mid;
      else hi = mid;
    }
    const int ib = node_find(B.nodes, B.n_nodes, A.nodes[lo]);
    if (ib < 0) continue;
    const int idx1 = (int)A.node_feats[p];
    if ((unsigned)idx1 >= (unsigned)na) {  // malformed FeatureVector: flag the pair, touch nothing
      s_bad = 1;
      continue;
    }
    if (A.has_mp[idx1]) continue;
    const bool st1 = A.u_right[idx1] >= 0;
    if (P.only_stereo && !st1) continue;
    const slamgpu_keypoint kp1 = A.kps[idx1];
    // epipolar line of kp1 in pKF2 (CheckDistEpipolarLine :117-119)
    const float la = fmaf(kp1.x, F[0], kp1.y * F[3]) + F[6];
    const float lb = fmaf(kp1.x, F[1], kp1.y * F[4]) + F[7];
    const float lc = fmaf(kp1.x, F[2], kp1.y * F[5]) + F[8];
    const float den = fmaf(la, la, lb * lb);
    const uint8_t* d1 = A.desc + (int64_t)idx1 * 32;
    const int b0 = B.node_start[ib], nbn = B.node_start[ib + 1] - b0;
    uint32_t best = 0xffffffffu;
    for (int c = lane; c < nbn; c += 64) {
      const int idx2 = (int)B.node_feats[b0 + c];
      if ((unsigned)idx2 >= (unsigned)nb) {
        s_bad = 1;
        continue;
      }
      if (B.has_mp[idx2]) continue;
      const bool st2 = B.u_right[idx2] >= 0;
      if (P.only_stereo && !st2) continue;
      const int dist = hamming32(d1, B.desc + (int64_t)idx2 * 32);
      if (dist > kThLow) continue;
      const slamgpu_keypoint kp2 = B.kps[idx2];
      if ((unsigned)kp2.octave >= (unsigned)lv.nlevels) {
        s_bad = 1;
        continue;
      }
      if (!st1 && !st2) {
        const float dx = ex - kp2.x, dy = ey - kp2.y;
        if (fmaf(dx, dx, dy * dy) < 100.0f * lv.scale[kp2.octave]) continue;
      }
      if (den == 0) continue;
      const float num = fmaf(la, kp2.x, lb * kp2.y) + lc;
      const float dsqr = num * num / den;
      if (!((double)dsqr < 3.84 * (double)lv.sigma2[kp2.octave])) continue;
      best = min(best, (uint32_t)dist << 16 | (uint32_t)(0xffff - c));
    }
    best = wave_min(best);
    if (best == 0xffffffffu) continue;
    if (lane == 0) {
      const int idx2 = (int)B.node_feats[b0 + (0xffff - (int)(best & 0xffffu))];
      out[idx1] = idx2;
      if (check_ori) {
        const int bin = rot_bin(kp1.angle, B.kps[idx2].angle);
        s_bin[idx1] = (int8_t)bin;
        atomicAdd(&s_hist[bin], 1);
      }
    }
    acc++;
  }
  const int nm = rot_filter_count<kTriWaves>(acc, check_ori, s_hist, s_bin, na, out);
  if (tid == 0) nmatches[pair] = s_bad ? -1 : nm;
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fuse_kernel(const slamgpu_kf* __restrict__ kfs,
                                                   const slamgpu_fuse_point* __restrict__ pts,
                                                   const int32_t* __restrict__ point_kf,
                                                   int n_pts, float th, slamgpu_camera cam,
                                                   slamgpu_levels lv, slamgpu_kf_grid g,
                                                   int32_t* __restrict__ best_idx,
                                                   int32_t* __restrict__ best_dist) {
  const int i = blockIdx.x * 4 + wave_id();
  if (i >= n_pts) return;
  const int lane = lane_id();
  const slamgpu_fuse_point& P = pts[i];
  int out_idx = -1, out_dist = 256;
  const int kfi = point_kf ? point_kf[i] : 0;
  const slamgpu_kf& K = kfs[kfi];
  const int n = min(K.n, kMaxFeat);
  do {
    if (P.skip) break;
    Proj pr;
    if (!project_scw(K, P, th, cam, lv, g, &pr)) break;
    const float u = pr.u, v = pr.v, r = pr.r;
    const int lvl = pr.lvl;
    const float urp = fmaf(-cam.bf, pr.invz, u);
    uint64_t best = kNoKey;
    for (int j = lane; j < n; j += 64) {
      const slamgpu_keypoint kp = K.kps[j];
      // the window test also drops off-grid and non-finite kps; only a cell inside the window
      // becomes an int, and the row is worked out only for a keypoint in the window's columns
      const float fx = cell_coord(kp.x, g.min_x, g.cell_w);
      if (!(fx >= (float)pr.cx0 && fx <= (float)pr.cx1)) continue;
      const float fy = cell_coord(kp.y, g.min_y, g.cell_h);
      if (!(fy >= (float)pr.cy0 && fy <= (float)pr.cy1)) continue;
      const int px = (int)fx, py = (int)fy;
      const float dxk = kp.x - u, dyk = kp.y - v;
      if (!(fabsf(dxk) < r && fabsf(dyk) < r)) continue;
      const int kl = kp.octave;
      if (kl < lvl - 1 || kl > lvl) continue;
      const float ex = u - kp.x, ey = v - kp.y;
      const float kr = K.u_right[j];
      if (kr >= 0) {
        const float er = urp - kr;
        const float e2 = fmaf(er, er, fmaf(ex, ex, ey * ey));
        if ((double)(e2 * lv.inv_sigma2[kl]) > 7.8) continue;
      } else {
        const float e2 = fmaf(ex, ex, ey * ey);
        if ((double)(e2 * lv.inv_sigma2[kl]) > 5.99) continue;
      }
      const uint32_t dist = (uint32_t)hamming32(P.desc, K.desc + (int64_t)j * 32);
      const uint64_t key = cand_key(dist, px * kGridRows + py, j);
      best = best < key ? best : key;
    }
    best = wave_min(best);
    if (best == kNoKey) break;
    out_dist = key_dist(best);
    if (out_dist <= kThLow) out_idx = key_idx(best);
  } while (false);
  if (lane == 0) {
    best_idx[i] = out_idx;
    best_dist[i] = out_dist;
  }
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

const char* slamgpu_kfmatch_last_error(void) { return t_kf_err.c_str(); }

int slamgpu_search_for_triangulation_device(const slamgpu_kf* d_kfs,
                                            const slamgpu_tri_pair* d_pairs, int n_pairs,
                                            const slamgpu_camera* cam, const slamgpu_levels* lv,
                                            int check_ori, int32_t* d_match12,
                                            int64_t match_stride, int32_t* d_nmatches,
                                            void* stream) {
  if (n_pairs < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "n_pairs %d < 0", n_pairs);
  if (n_pairs == 0) return 0;
  if (!d_kfs || !d_pairs || !d_match12 || !d_nmatches || !cam)
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_levels(lv)) return r;
  hipLaunchKernelGGL(search_tri_kernel, dim3(n_pairs), dim3(64 * kTriWaves), 0,
                     static_cast<hipStream_t>(stream), d_kfs, d_pairs, *cam, *lv,
                     check_ori ? 1 : 0, d_match12, match_stride, d_nmatches);
  HIPCHECK(t_kf_err, hipGetLastError());
  return 0;
}

int slamgpu_search_for_triangulation(const slamgpu_kf* kf1, const slamgpu_kf* kf2,
                                     const float* F12, const slamgpu_camera* cam,
                                     const slamgpu_levels* lv, int only_stereo, int check_ori,
                                     int32_t* match12, int* nmatches) {
  if (int r = check_kf(kf1, true, "kf1")) return r;
  if (int r = check_kf(kf2, true, "kf2")) return r;
  if (int r = check_levels(lv)) return r;
  if (!F12 || !cam || !nmatches || (kf1->n > 0 && !match12))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  StageLease S(t_kf_err);
  StageLayout L;
  const int n[2] = {kf1->n, kf2->n}, n_nodes[2] = {kf1->n_nodes, kf2->n_nodes};
  const int n_feats[2] = {n_nodes[0] > 0 ? kf1->node_start[n_nodes[0]] : 0,
                          n_nodes[1] > 0 ? kf2->node_start[n_nodes[1]] : 0};
  const TriLayout t = layout_search_tri(L, n, n_nodes, n_feats);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const slamgpu_kf dk[2] = {upload_kf(S, *kf1, t.kf[0]), upload_kf(S, *kf2, t.kf[1])};
  slamgpu_tri_pair pr{};
  pr.kf1 = 0;
  pr.kf2 = 1;
  for (int i = 0; i < 9; i++) pr.F12[i] = F12[i];
  pr.only_stereo = only_stereo ? 1 : 0;
  HIPCHECK(t_kf_err, S.upload(t.kfs, dk, sizeof(dk)));
  HIPCHECK(t_kf_err, S.upload(t.pair, &pr, sizeof(pr)));
  if (int r = slamgpu_search_for_triangulation_device(
          S.at<slamgpu_kf>(t.kfs), S.at<slamgpu_tri_pair>(t.pair), 1, cam, lv, check_ori,
          S.at<int32_t>(t.match), 0, S.at<int32_t>(t.nmatches), st))
    return r;
  int32_t nm = 0;
  HIPCHECK(t_kf_err, S.download(&nm, t.nmatches, 4));
  HIPCHECK(t_kf_err, S.download(match12, t.match, (size_t)kf1->n * 4));
  HIPCHECK(t_kf_err, hipStreamSynchronize(st));
  *nmatches = nm;
  return 0;
}

int slamgpu_fuse_device(const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_pts,
                        const int32_t* d_point_kf, int n_pts, float th,
                        const slamgpu_camera* cam, const slamgpu_levels* lv,
                        const slamgpu_kf_grid* grid, int32_t* d_best_idx, int32_t* d_best_dist,
                        void* stream) {
  if (n_pts < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "n_pts %d < 0", n_pts);
  if (n_pts == 0) return 0;
  if (!d_kfs || !d_pts || !d_best_idx || !d_best_dist || !cam || !grid)
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_levels(lv)) return r;
  if (int r = check_grid(grid)) return r;
  hipLaunchKernelGGL(fuse_kernel, dim3((n_pts + 3) / 4), dim3(256), 0,
                     static_cast<hipStream_t>(stream), d_kfs, d_pts, d_point_kf, n_pts, th, *cam,
                     *lv, *grid, d_best_idx, d_best_dist);
  HIPCHECK(t_kf_err, hipGetLastError());
  return 0;
}

int slamgpu_fuse(const slamgpu_kf* kf, const slamgpu_fuse_point* pts, int n_pts, float th,
                 const slamgpu_camera* cam, const slamgpu_levels* lv, const slamgpu_kf_grid* grid,
                 int32_t* best_idx, int32_t* best_dist, int* nfused) {
  if (int r = check_kf(kf, false, "kf")) return r;
  if (int r = check_levels(lv)) return r;
  if (n_pts < 0 || !cam || !grid || !nfused || (n_pts > 0 && (!pts || !best_idx || !best_dist)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "bad arguments");
  for (int j = 0; j < kf->n; j++)
    if (kf->kps[j].octave >= lv->nlevels)
      return t_kf_err.fail(SLAMGPU_EINVAL, "keypoint %d octave %d >= nlevels", j, kf->kps[j].octave);
  *nfused = 0;
  if (n_pts == 0) return 0;
  StageLease S(t_kf_err);
  StageLayout L;
  const FuseLayout f = layout_fuse(L, kKfStereo, kf->n, n_pts);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const slamgpu_kf dk = upload_kf(S, *kf, f.kf);
  HIPCHECK(t_kf_err, S.upload(f.kfs, &dk, sizeof(dk)));
  HIPCHECK(t_kf_err, S.upload(f.pts, pts, (size_t)n_pts * sizeof(slamgpu_fuse_point)));
  if (int r = slamgpu_fuse_device(S.at<slamgpu_kf>(f.kfs), S.at<slamgpu_fuse_point>(f.pts), nullptr,
                                  n_pts, th, cam, lv, grid, S.at<int32_t>(f.best_idx),
                                  S.at<int32_t>(f.best_dist), st))
    return r;
  HIPCHECK(t_kf_err, S.download(best_idx, f.best_idx, (size_t)n_pts * 4));
  HIPCHECK(t_kf_err, S.download(best_dist, f.best_dist, (size_t)n_pts * 4));
  HIPCHECK(t_kf_err, hipStreamSynchronize(st));
  int nf = 0;
  for (int i = 0; i < n_pts; i++) nf += best_idx[i] >= 0;
  *nfused = nf;
  return 0;
}

}  // extern "C"
