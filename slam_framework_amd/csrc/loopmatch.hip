// loopmatch.hip -- the LoopCloser's three Sim3 matchers on gfx950 (include/slamgpu_loopmatch.h).
//
//   fuse_sim3     the candidate search of OrbMatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
//                 (src/orb_features/orb_matcher.cpp:956-1079), n_kfs keyframes x one shared point
//                 array.
//   sbp_scan +    OrbMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:384-497).
//   sbp_resolve   The scan keeps, per point, its first kKeep candidates of distance <= TH_LOW in
//                 (distance, GetFeaturesInArea order) order and their total count, among the
//                 keypoints not matched at entry; a one-wave resolve commits the claims in point
//                 order (64 points a round, iterated to the fixed point; a point whose kept
//                 candidates are all taken while more exist is rescanned alone, at its place).
//   sim3_scan +   OrbMatcher::SearchBySim3 (:1081-1310): both projection directions in one launch,
//   sim3_mutual   then the agreement check and count.
//
// All scans share one shape: a workgroup takes one (keyframe, chunk of 64 points), stages the
// keyframe's x, y and (grid cell, octave, excluded) once in LDS (48 KB) and each wave walks its
// points: gates on wave-uniform values, keypoints across lanes, the descriptor fetched only for
// a keypoint that passed the window and octave tests. The winner is the wave minimum of
// (distance, cell, index), cells in GetFeaturesInArea's x-major order: the reference's first
// strict minimum. None of the three applies Fuse's chi-square gates or reads u_right.
// Float semantics follow oracle/kfmatch_oracle.c (explicit fmaf for u, v; OpenCV's gemm row as a
// float dot plus a double add; cv::norm and Mat::dot as double sums; glibc logf); the gates
// (project_scw and its parts), the descriptor distance and the candidate keys are
// orbmatch_device.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slamgpu_loopmatch.h"
#include "kfmatch_common.h"

namespace slamgpu {
namespace {

static_assert(sizeof(slamgpu_sbp_job) == 16, "slamgpu_sbp_job layout");
static_assert(sizeof(slamgpu_sim3_pair) == 112, "slamgpu_sim3_pair layout");

constexpr int kScanWaves = 8, kChunk = 64;  // waves and points per workgroup
constexpr int kKeep = SLAMGPU_SBP_KEEP;     // kept candidates per point (SearchByProjection)
static_assert(kKeep == 3, "sbp_resolve_kernel holds the kept candidates in three registers");
constexpr int kRow = kKeep + 1;             // scratch row: total count, then the kept keypoints

struct KpLds {
  float x[kMaxFeat];
  float y[kMaxFeat];
  uchar4 c[kMaxFeat];  // cell column (255: in no cell), cell row, octave (255: none), excluded
};

__device__ __forceinline__ void stage_kps(KpLds& S, const slamgpu_kf& K, int n,
                                          const slamgpu_kf_grid& g, const uint8_t* excl, int tid,
                                          int nthreads) {
  for (int j = tid; j < n; j += nthreads) {
    const slamgpu_keypoint kp = K.kps[j];
    int px, py;
    const bool on = pos_in_grid(kp.x, kp.y, g.min_x, g.min_y, g.cell_w, g.cell_h, &px, &py);
    const int o = kp.octave;
    S.x[j] = kp.x;
    S.y[j] = kp.y;
    S.c[j] = make_uchar4(on ? px : 255, on ? py : 255, (o >= 0 && o < 255) ? o : 255,
                         (excl && excl[j]) ? 1 : 0);
  }
}

// The gates of SearchBySim3 :1142-1173 (and :1222-1253): source keyframe A's point into the
// other camera through sR, t; the range is measured on the camera-frame point; no viewing angle.
__device__ __forceinline__ bool project_sim3(const slamgpu_kf& A, const float* sR, const float* t,
                                             const slamgpu_fuse_point& P, float th,
                                             const slamgpu_camera& cam, const slamgpu_levels& lv,
                                             const slamgpu_kf_grid& g, Proj* o) {
  float p1[3];
  p1[0] = gemm_row(A.Rcw, P.xyz, A.tcw[0]);
  p1[1] = gemm_row(A.Rcw + 3, P.xyz, A.tcw[1]);
  p1[2] = gemm_row(A.Rcw + 6, P.xyz, A.tcw[2]);
  const float xc = gemm_row(sR, p1, t[0]);
  const float yc = gemm_row(sR + 3, p1, t[1]);
  const float zc = gemm_row(sR + 6, p1, t[2]);
  if (!proj_uv(xc, yc, zc, cam, g, o)) return false;
  const float dist3D = norm3(xc, yc, zc);
  if (!in_range(P, dist3D)) return false;
  return proj_window(P, dist3D, th, lv, g, o);
}

// Wave scan of the staged keyframe: the minimum candidate key (distance, cell, index) over the
// keypoints inside the window, of octave lvl - 1 or lvl, not excluded, not in `claimed` (LDS
// bitmap or NULL) and with key > floor (kNoKey: no floor). *n_low (if non-NULL) receives the
// number of such keypoints, floor aside, of distance <= TH_LOW.
__device__ __forceinline__ uint64_t scan_kps(const KpLds& S, int n, const Proj& p, const Desc& d,
                                             const uint8_t* kdesc, const uint32_t* claimed,
                                             uint64_t floor, int* n_low) {
  const int lane = lane_id();
  uint64_t best = kNoKey;
  int low = 0;
  for (int j = lane; j < n; j += 64) {
    const uchar4 c = S.c[j];
    const int px = c.x, py = c.y, kl = c.z;
    if (c.w || px < p.cx0 || px > p.cx1 || py < p.cy0 || py > p.cy1) continue;
    if (kl < p.lvl - 1 || kl > p.lvl) continue;
    if (!(fabsf(S.x[j] - p.u) < p.r && fabsf(S.y[j] - p.v) < p.r)) continue;
    if (claimed && (claimed[j >> 5] >> (j & 31) & 1u)) continue;
    const uint32_t dist = (uint32_t)hamming(d, kdesc + (int64_t)j * 32);
    low += dist <= (uint32_t)kThLow;
    const uint64_t key = cand_key(dist, px * kGridRows + py, j);
    if (floor != kNoKey && key <= floor) continue;
    best = best < key ? best : key;
  }
  if (n_low) *n_low = wave_sum(low);
  return wave_min(best);
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kScanWaves) void fuse_sim3_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_fuse_point* __restrict__ pts,
    const uint8_t* __restrict__ skip, int n_pts, float th, slamgpu_camera cam, slamgpu_levels lv,
    slamgpu_kf_grid g, int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  __shared__ KpLds S;
  const int kfi = blockIdx.y, lane = lane_id(), wid = wave_id();
  const slamgpu_kf& K = kfs[kfi];
  const int n = (K.n < 0 || K.n > kMaxFeat) ? 0 : K.n;
  stage_kps(S, K, n, g, nullptr, threadIdx.x, 64 * kScanWaves);
  __syncthreads();
  const int base = blockIdx.x * kChunk, end = min(base + kChunk, n_pts);
  const int64_t row = (int64_t)kfi * n_pts;
  for (int i = base + wid; i < end; i += kScanWaves) {
    const slamgpu_fuse_point& P = pts[i];
    int out_idx = -1, out_dist = 256;
    Proj pr;
    const bool skipped = skip ? skip[row + i] != 0 : P.skip != 0;
    if (n > 0 && !skipped && project_scw(K, P, th, cam, lv, g, &pr)) {
      const uint64_t best = scan_kps(S, n, pr, load_desc(P.desc), K.desc, nullptr, kNoKey, nullptr);
      if (best != kNoKey) {
        out_dist = key_dist(best);
        if (out_dist <= kThLow) out_idx = key_idx(best);
      }
    }
    if (lane == 0) {
      best_idx[row + i] = out_idx;
      best_dist[row + i] = out_dist;
    }
  }
}

// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool sbp_job_ok(const slamgpu_sbp_job& J, const slamgpu_kf& K,
                                           int n_pts_total, int n_kp_total, int max_job_pts) {
  return K.n >= 0 && K.n <= kMaxFeat && J.pt_begin >= 0 && J.n_pts >= 0 &&
         J.n_pts <= max_job_pts && (int64_t)J.pt_begin + J.n_pts <= n_pts_total &&
         J.kp_begin >= 0 && (int64_t)J.kp_begin + K.n <= n_kp_total;
}

__global__ __launch_bounds__(64 * kScanWaves) void sbp_scan_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_fuse_point* __restrict__ pts,
    int n_pts_total, const slamgpu_sbp_job* __restrict__ jobs, int max_job_pts,
    const uint8_t* __restrict__ matched_in, int n_kp_total, float th, slamgpu_camera cam,
    slamgpu_levels lv, slamgpu_kf_grid g, int32_t* __restrict__ scratch) {
  __shared__ KpLds S;
  const slamgpu_sbp_job J = jobs[blockIdx.y];
  if (J.kf < 0) return;
  const slamgpu_kf& K = kfs[J.kf];
  if (!sbp_job_ok(J, K, n_pts_total, n_kp_total, max_job_pts)) return;
  const int base = blockIdx.x * kChunk, end = min(base + kChunk, J.n_pts);
  if (base >= end) return;
  const int n = K.n, lane = lane_id(), wid = wave_id();
  stage_kps(S, K, n, g, matched_in + J.kp_begin, threadIdx.x, 64 * kScanWaves);
  __syncthreads();
  for (int i = base + wid; i < end; i += kScanWaves) {
    const slamgpu_fuse_point& P = pts[J.pt_begin + i];
    int32_t* row = scratch + (int64_t)(J.pt_begin + i) * kRow;
    int total = 0, mine = -1;  // lane k keeps candidate k
    Proj pr;
    if (n > 0 && !P.skip && project_scw(K, P, th, cam, lv, g, &pr)) {
      const Desc d = load_desc(P.desc);
      uint64_t key = scan_kps(S, n, pr, d, K.desc, nullptr, kNoKey, &total);
      const int nk = min(total, kKeep);
      for (int k = 0; k < nk; k++) {  // the total candidates <= TH_LOW are the first in key order
        if (k > 0) key = scan_kps(S, n, pr, d, K.desc, nullptr, key, nullptr);
        if (lane == k) mine = key_idx(key);
      }
    }
    if (lane == 0) row[0] = total;
    if (lane < kKeep) row[1 + lane] = mine;
  }
}

__global__ __launch_bounds__(64) void sbp_resolve_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_fuse_point* __restrict__ pts,
    int n_pts_total, const slamgpu_sbp_job* __restrict__ jobs, int max_job_pts,
    const uint8_t* __restrict__ matched_in, int n_kp_total, float th, slamgpu_camera cam,
    slamgpu_levels lv, slamgpu_kf_grid g, const int32_t* __restrict__ scratch,
    int32_t* __restrict__ kp_point, int32_t* __restrict__ point_kp,
    int32_t* __restrict__ nmatches) {
  __shared__ KpLds S;
  __shared__ uint32_t s_claimed[kMaxFeat / 32];
  const int job = blockIdx.x, lane = threadIdx.x;
  const slamgpu_sbp_job J = jobs[job];
  const bool ok = J.kf >= 0 && sbp_job_ok(J, kfs[J.kf < 0 ? 0 : J.kf], n_pts_total, n_kp_total,
                                          max_job_pts);
  if (!ok) {
    if (lane == 0) nmatches[job] = -1;
    return;
  }
  const slamgpu_kf& K = kfs[J.kf];
  const int n = K.n, n_pts = J.n_pts;
  const uint8_t* min_ = matched_in + J.kp_begin;
  int32_t* kpp = kp_point + J.kp_begin;
  int32_t* pkp = point_kp + J.pt_begin;
  for (int w = lane; w < kMaxFeat / 32; w += 64) {  // claimed starts as "matched at entry"
    uint32_t bits = 0;
    for (int b = 0; b < 32; b++) {
      const int j = w * 32 + b;
      if (j < n && min_[j]) bits |= 1u << b;
    }
    s_claimed[w] = bits;
  }
  for (int j = lane; j < n; j += 64) kpp[j] = -1;
  stage_kps(S, K, n, g, nullptr, lane, 64);
  __syncthreads();
  int nm = 0;  // lane-partial
  int start = 0;
  while (start < n_pts) {
    const int m = min(64, n_pts - start);
    const bool active = lane < m;
    int total = 0, k0 = -1, k1 = -1, k2 = -1;
    if (active) {
      const int32_t* row = scratch + (int64_t)(J.pt_begin + start + lane) * kRow;
      total = row[0];
      k0 = row[1];
      k1 = row[2];
      k2 = row[3];
    }
    const int nk = min(total, kKeep);
    int ptr = 0, cur = -1;
    // Fixed point: every lane holds its first kept candidate that is neither claimed by an
    // earlier round nor held by a lower lane. A lane only ever advances: the candidate it leaves
    // stays held by some lower lane from then on (that lane leaves it only to a still lower one).
    for (;;) {
      for (;;) {
        cur = ptr == 0 ? k0 : ptr == 1 ? k1 : k2;
        if (ptr >= nk) {
          cur = -1;
          break;
        }
        if ((unsigned)cur >= (unsigned)n || (s_claimed[cur >> 5] >> (cur & 31) & 1u)) ptr++;
        else break;
      }
      const int tag = cur >= 0 ? cur : -1 - lane;
      bool lose = false;
      for (int l = 0; l < 63; l++) {
        const int o = __shfl(tag, l, 64);
        lose |= l < lane && o == tag;
      }
      if (lose) ptr++;
      if (__ballot(lose) == 0) break;
    }
    // A lane that ran out of kept candidates while more exist must be rescanned at its place;
    // the lanes below the first such one are final.
    const uint64_t ex = __ballot(active && cur < 0 && total > kKeep);
    const int e = ex ? __ffsll((unsigned long long)ex) - 1 : 64;
    const int ncommit = min(e, m);
    if (lane < ncommit) {
      pkp[start + lane] = cur;
      if (cur >= 0) {
        atomicOr(&s_claimed[cur >> 5], 1u << (cur & 31));
        kpp[cur] = start + lane;
        nm++;
      }
    }
    __syncthreads();
    start += ncommit;
    if (e < m) {  // wave-uniform
      const slamgpu_fuse_point& P = pts[J.pt_begin + start];
      Proj pr;
      int got = -1;
      if (!P.skip && project_scw(K, P, th, cam, lv, g, &pr)) {
        const uint64_t key =
            scan_kps(S, n, pr, load_desc(P.desc), K.desc, s_claimed, kNoKey, nullptr);
        if (key != kNoKey && key_dist(key) <= kThLow) got = key_idx(key);
      }
      if (lane == 0) {
        pkp[start] = got;
        if (got >= 0) {
          s_claimed[got >> 5] |= 1u << (got & 31);
          kpp[got] = start;
          nm++;
        }
      }
      __syncthreads();
      start++;
    }
  }
  nm = wave_sum(nm);
  if (lane == 0) nmatches[job] = nm;
}

// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool sim3_pair_ok(const slamgpu_sim3_pair& P,
                                             const slamgpu_kf* __restrict__ kfs, int n_mp_total,
                                             int64_t stride) {
  if (P.kf1 < 0 || P.kf2 < 0) return false;
  const int n1 = kfs[P.kf1].n, n2 = kfs[P.kf2].n;
  const int64_t cap = stride < kMaxFeat ? stride : kMaxFeat;
  return n1 >= 0 && n2 >= 0 && n1 <= cap && n2 <= cap && P.mp1_begin >= 0 && P.mp2_begin >= 0 &&
         (int64_t)P.mp1_begin + n1 <= n_mp_total && (int64_t)P.mp2_begin + n2 <= n_mp_total;
}

// grid (chunks, direction, pair): direction 0 projects kf1's points into kf2, 1 the reverse.
__global__ __launch_bounds__(64 * kScanWaves) void sim3_scan_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_fuse_point* __restrict__ mp, int n_mp_total,
    const slamgpu_sim3_pair* __restrict__ pairs, const uint8_t* __restrict__ already1,
    const uint8_t* __restrict__ already2, int64_t stride, float th, slamgpu_camera cam,
    slamgpu_levels lv, slamgpu_kf_grid g, int32_t* __restrict__ vn1, int32_t* __restrict__ vn2) {
  __shared__ KpLds S;
  const int pair = blockIdx.z, dir = blockIdx.y, lane = lane_id(), wid = wave_id();
  const slamgpu_sim3_pair& P = pairs[pair];
  if (!sim3_pair_ok(P, kfs, n_mp_total, stride)) return;
  const slamgpu_kf& A = kfs[dir ? P.kf2 : P.kf1];  // source of the points
  const slamgpu_kf& B = kfs[dir ? P.kf1 : P.kf2];  // searched keyframe
  const int na = A.n, nb = B.n;
  const int base = blockIdx.x * kChunk, end = min(base + kChunk, na);
  if (base >= end) return;
  const slamgpu_fuse_point* src = mp + (dir ? P.mp2_begin : P.mp1_begin);
  const uint8_t* already = (dir ? already2 : already1) + (int64_t)pair * stride;
  int32_t* out = (dir ? vn2 : vn1) + (int64_t)pair * stride;
  const float* sR = dir ? P.sR12 : P.sR21;
  const float* t = dir ? P.t12 : P.t21;
  stage_kps(S, B, nb, g, nullptr, threadIdx.x, 64 * kScanWaves);
  __syncthreads();
  for (int i = base + wid; i < end; i += kScanWaves) {
    const slamgpu_fuse_point& X = src[i];
    int res = -1;
    Proj pr;
    if (nb > 0 && !X.skip && !already[i] && project_sim3(A, sR, t, X, th, cam, lv, g, &pr)) {
      const uint64_t best =
          scan_kps(S, nb, pr, load_desc(X.desc), B.desc, nullptr, kNoKey, nullptr);
      if (best != kNoKey && key_dist(best) <= kThHigh) res = key_idx(best);
    }
    if (lane == 0) out[i] = res;
  }
}

__global__ __launch_bounds__(256) void sim3_mutual_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_sim3_pair* __restrict__ pairs,
    int n_mp_total, int64_t stride, const int32_t* __restrict__ vn1,
    const int32_t* __restrict__ vn2, int32_t* __restrict__ match12,
    int32_t* __restrict__ nfound) {
  __shared__ int s_cnt[4];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const slamgpu_sim3_pair& P = pairs[pair];
  if (!sim3_pair_ok(P, kfs, n_mp_total, stride)) {
    if (tid == 0) nfound[pair] = -1;
    return;
  }
  const int n1 = kfs[P.kf1].n, n2 = kfs[P.kf2].n;
  const int32_t* a = vn1 + (int64_t)pair * stride;
  const int32_t* b = vn2 + (int64_t)pair * stride;
  int32_t* out = match12 + (int64_t)pair * stride;
  int cnt = 0;
  for (int i1 = tid; i1 < n1; i1 += 256) {
    const int idx2 = a[i1];
    const bool hit = idx2 >= 0 && idx2 < n2 && b[idx2] == i1;
    out[i1] = hit ? idx2 : -1;
    cnt += hit;
  }
  cnt = wave_sum(cnt);
  if (lane_id() == 0) s_cnt[wave_id()] = cnt;
  __syncthreads();
  if (tid == 0) nfound[pair] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

int check_common(const slamgpu_camera* cam, const slamgpu_levels* lv,
                 const slamgpu_kf_grid* grid) {
  if (!cam || !grid) return t_kf_err.fail(SLAMGPU_EINVAL, "NULL camera or grid");
  if (int r = check_levels(lv)) return r;
  return check_grid(grid);
}

// The Sim3 matchers never read u_right; has_mp and the FeatureVector neither.
int check_kf_loop(const slamgpu_kf* k, const slamgpu_levels* lv, const char* name) {
  if (!k) return t_kf_err.fail(SLAMGPU_EINVAL, "%s is NULL", name);
  if (k->n < 0 || k->n > kMaxFeat)
    return t_kf_err.fail(SLAMGPU_EINVAL, "%s: n %d outside [0, %d]", name, k->n, kMaxFeat);
  if (k->n > 0 && (!k->kps || !k->desc)) return t_kf_err.fail(SLAMGPU_EINVAL, "%s: NULL keypoint arrays", name);
  for (int j = 0; j < k->n; j++)
    if (k->kps[j].octave < 0 || k->kps[j].octave >= lv->nlevels)
      return t_kf_err.fail(SLAMGPU_EINVAL, "%s: keypoint %d octave %d outside [0, nlevels)", name, j,
                  k->kps[j].octave);
  return 0;
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

const char* slamgpu_loopmatch_last_error(void) { return t_kf_err.c_str(); }

int slamgpu_fuse_sim3_device(const slamgpu_kf* d_kfs, int n_kfs, const slamgpu_fuse_point* d_pts,
                             int n_pts, const uint8_t* d_skip, float th,
                             const slamgpu_camera* cam, const slamgpu_levels* lv,
                             const slamgpu_kf_grid* grid, int32_t* d_best_idx,
                             int32_t* d_best_dist, void* stream) {
  if (n_kfs < 0 || n_pts < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "n_kfs %d or n_pts %d < 0", n_kfs, n_pts);
  if (n_kfs == 0 || n_pts == 0) return 0;
  if (n_kfs > 65535) return t_kf_err.fail(SLAMGPU_EINVAL, "n_kfs %d > 65535", n_kfs);
  if (!d_kfs || !d_pts || !d_best_idx || !d_best_dist) return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_common(cam, lv, grid)) return r;
  hipLaunchKernelGGL(fuse_sim3_kernel, dim3((n_pts + kChunk - 1) / kChunk, n_kfs),
                     dim3(64 * kScanWaves), 0, static_cast<hipStream_t>(stream), d_kfs, d_pts,
                     d_skip, n_pts, th, *cam, *lv, *grid, d_best_idx, d_best_dist);
  HIPCHECK(t_kf_err, hipGetLastError());
  return 0;
}

int slamgpu_fuse_sim3(const slamgpu_kf* kf, const slamgpu_fuse_point* pts, int n_pts, float th,
                      const slamgpu_camera* cam, const slamgpu_levels* lv,
                      const slamgpu_kf_grid* grid, int32_t* best_idx, int32_t* best_dist,
                      int* nfused) {
  if (int r = check_common(cam, lv, grid)) return r;
  if (int r = check_kf_loop(kf, lv, "kf")) return r;
  if (n_pts < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "n_pts %d < 0", n_pts);
  if (!nfused || (n_pts > 0 && (!pts || !best_idx || !best_dist)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  *nfused = 0;
  if (n_pts == 0) return 0;
  const size_t pbytes = (size_t)n_pts * sizeof(slamgpu_fuse_point), obytes = (size_t)n_pts * 4;
  StageLease S(t_kf_err);
  StageLayout L;
  const FuseLayout f = layout_fuse(L, kKfLoop, kf->n, n_pts);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const slamgpu_kf dk = upload_kf(S, *kf, f.kf);
  HIPCHECK(t_kf_err, S.upload(f.kfs, &dk, sizeof(dk)));
  HIPCHECK(t_kf_err, S.upload(f.pts, pts, pbytes));
  if (int r = slamgpu_fuse_sim3_device(S.at<slamgpu_kf>(f.kfs), 1, S.at<slamgpu_fuse_point>(f.pts),
                                       n_pts, nullptr, th, cam, lv, grid, S.at<int32_t>(f.best_idx),
                                       S.at<int32_t>(f.best_dist), st))
    return r;
  HIPCHECK(t_kf_err, S.download(best_idx, f.best_idx, obytes));
  HIPCHECK(t_kf_err, S.download(best_dist, f.best_dist, obytes));
  HIPCHECK(t_kf_err, hipStreamSynchronize(st));
  int nf = 0;
  for (int i = 0; i < n_pts; i++) nf += best_idx[i] >= 0;
  *nfused = nf;
  return 0;
}

size_t slamgpu_search_by_projection_sim3_scratch_bytes(int n_pts_total) {
  return n_pts_total > 0 ? (size_t)n_pts_total * kRow * sizeof(int32_t) : 0;
}

int slamgpu_search_by_projection_sim3_device(
    const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_pts, int n_pts_total,
    const slamgpu_sbp_job* d_jobs, int n_jobs, int max_job_pts, const uint8_t* d_matched_in,
    int n_kp_total, float th, const slamgpu_camera* cam, const slamgpu_levels* lv,
    const slamgpu_kf_grid* grid, int32_t* d_kp_point, int32_t* d_point_kp, int32_t* d_nmatches,
    void* d_scratch, size_t scratch_bytes, void* stream) {
  if (n_jobs < 0 || n_pts_total < 0 || n_kp_total < 0 || max_job_pts < 0)
    return t_kf_err.fail(SLAMGPU_EINVAL, "negative count");
  if (n_jobs == 0) return 0;
  if (n_jobs > 65535) return t_kf_err.fail(SLAMGPU_EINVAL, "n_jobs %d > 65535", n_jobs);
  if (!d_kfs || !d_jobs || !d_nmatches || (n_pts_total > 0 && (!d_pts || !d_point_kp || !d_scratch)) ||
      (n_kp_total > 0 && (!d_matched_in || !d_kp_point)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (scratch_bytes < slamgpu_search_by_projection_sim3_scratch_bytes(n_pts_total))
    return t_kf_err.fail(SLAMGPU_EINVAL, "scratch_bytes %zu < %zu", scratch_bytes,
                slamgpu_search_by_projection_sim3_scratch_bytes(n_pts_total));
  if (int r = check_common(cam, lv, grid)) return r;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (max_job_pts > 0)
    hipLaunchKernelGGL(sbp_scan_kernel, dim3((max_job_pts + kChunk - 1) / kChunk, n_jobs),
                       dim3(64 * kScanWaves), 0, st, d_kfs, d_pts, n_pts_total, d_jobs,
                       max_job_pts, d_matched_in, n_kp_total, th, *cam, *lv, *grid,
                       static_cast<int32_t*>(d_scratch));
  hipLaunchKernelGGL(sbp_resolve_kernel, dim3(n_jobs), dim3(64), 0, st, d_kfs, d_pts, n_pts_total,
                     d_jobs, max_job_pts, d_matched_in, n_kp_total, th, *cam, *lv, *grid,
                     static_cast<const int32_t*>(d_scratch), d_kp_point, d_point_kp, d_nmatches);
  HIPCHECK(t_kf_err, hipGetLastError());
  return 0;
}

int slamgpu_search_by_projection_sim3(const slamgpu_kf* kf, const slamgpu_fuse_point* pts,
                                      int n_pts, const uint8_t* matched_in, float th,
                                      const slamgpu_camera* cam, const slamgpu_levels* lv,
                                      const slamgpu_kf_grid* grid, int32_t* kp_point,
                                      int32_t* point_kp, int* nmatches) {
  if (int r = check_common(cam, lv, grid)) return r;
  if (int r = check_kf_loop(kf, lv, "kf")) return r;
  if (n_pts < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "n_pts %d < 0", n_pts);
  if (!nmatches || (n_pts > 0 && (!pts || !point_kp)) || (kf->n > 0 && (!matched_in || !kp_point)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  *nmatches = 0;
  if (n_pts == 0 || kf->n == 0) {
    for (int i = 0; i < n_pts; i++) point_kp[i] = -1;
    for (int j = 0; j < kf->n; j++) kp_point[j] = -1;
    return 0;
  }
  const int n = kf->n;
  const size_t pbytes = (size_t)n_pts * sizeof(slamgpu_fuse_point);
  const size_t sbytes = slamgpu_search_by_projection_sim3_scratch_bytes(n_pts);
  StageLease S(t_kf_err);
  StageLayout L;
  const SbpSim3Layout l = layout_sbp_sim3(L, n, n_pts, sbytes);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const slamgpu_kf dk = upload_kf(S, *kf, l.kf);
  const slamgpu_sbp_job job{0, 0, n_pts, 0};
  HIPCHECK(t_kf_err, S.upload(l.kfs, &dk, sizeof(dk)));
  HIPCHECK(t_kf_err, S.upload(l.pts, pts, pbytes));
  HIPCHECK(t_kf_err, S.upload(l.job, &job, sizeof(job)));
  HIPCHECK(t_kf_err, S.upload(l.matched_in, matched_in, (size_t)n));
  if (int r = slamgpu_search_by_projection_sim3_device(
          S.at<slamgpu_kf>(l.kfs), S.at<slamgpu_fuse_point>(l.pts), n_pts,
          S.at<slamgpu_sbp_job>(l.job), 1, n_pts, S.at<uint8_t>(l.matched_in), n, th, cam, lv, grid,
          S.at<int32_t>(l.kp_point), S.at<int32_t>(l.point_kp), S.at<int32_t>(l.nmatches),
          S.at<char>(l.scratch), sbytes, st))
    return r;
  int32_t nm = 0;
  HIPCHECK(t_kf_err, S.download(kp_point, l.kp_point, (size_t)n * 4));
  HIPCHECK(t_kf_err, S.download(point_kp, l.point_kp, (size_t)n_pts * 4));
  HIPCHECK(t_kf_err, S.download(&nm, l.nmatches, 4));
  HIPCHECK(t_kf_err, hipStreamSynchronize(st));
  if (nm < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "job rejected on the device");
  *nmatches = nm;
  return 0;
}

int slamgpu_search_by_sim3_device(const slamgpu_kf* d_kfs, const slamgpu_fuse_point* d_mp,
                                  int n_mp_total, const slamgpu_sim3_pair* d_pairs, int n_pairs,
                                  const uint8_t* d_already1, const uint8_t* d_already2,
                                  int64_t stride, float th, const slamgpu_camera* cam,
                                  const slamgpu_levels* lv, const slamgpu_kf_grid* grid,
                                  int32_t* d_match12, int32_t* d_vn_match1,
                                  int32_t* d_vn_match2, int32_t* d_nfound, void* stream) {
  if (n_pairs < 0 || n_mp_total < 0 || stride < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "negative count");
  if (n_pairs == 0) return 0;
  if (n_pairs > 65535) return t_kf_err.fail(SLAMGPU_EINVAL, "n_pairs %d > 65535", n_pairs);
  if (!d_kfs || !d_pairs || !d_nfound ||
      (stride > 0 && (!d_mp || !d_already1 || !d_already2 || !d_match12 || !d_vn_match1 ||
                      !d_vn_match2)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_common(cam, lv, grid)) return r;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t cap = stride < kMaxFeat ? stride : kMaxFeat;
  if (cap > 0)
    hipLaunchKernelGGL(sim3_scan_kernel, dim3((int)((cap + kChunk - 1) / kChunk), 2, n_pairs),
                       dim3(64 * kScanWaves), 0, st, d_kfs, d_mp, n_mp_total, d_pairs, d_already1,
                       d_already2, stride, th, *cam, *lv, *grid, d_vn_match1, d_vn_match2);
  hipLaunchKernelGGL(sim3_mutual_kernel, dim3(n_pairs), dim3(256), 0, st, d_kfs, d_pairs,
                     n_mp_total, stride, d_vn_match1, d_vn_match2, d_match12, d_nfound);
  HIPCHECK(t_kf_err, hipGetLastError());
  return 0;
}

int slamgpu_search_by_sim3(const slamgpu_kf* kf1, const slamgpu_kf* kf2,
                           const slamgpu_fuse_point* mp1, const slamgpu_fuse_point* mp2,
                           const uint8_t* already1, const uint8_t* already2, const float* sR12,
                           const float* t12, const float* sR21, const float* t21, float th,
                           const slamgpu_camera* cam, const slamgpu_levels* lv,
                           const slamgpu_kf_grid* grid, int32_t* match12, int32_t* vn_match1,
                           int32_t* vn_match2, int* nfound) {
  if (int r = check_common(cam, lv, grid)) return r;
  if (int r = check_kf_loop(kf1, lv, "kf1")) return r;
  if (int r = check_kf_loop(kf2, lv, "kf2")) return r;
  const int n1 = kf1->n, n2 = kf2->n;
  if (!nfound || !sR12 || !t12 || !sR21 || !t21 ||
      (n1 > 0 && (!mp1 || !already1 || !match12 || !vn_match1)) ||
      (n2 > 0 && (!mp2 || !already2 || !vn_match2)))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  *nfound = 0;
  if (n1 == 0 || n2 == 0) {
    for (int i = 0; i < n1; i++) match12[i] = vn_match1[i] = -1;
    for (int i = 0; i < n2; i++) vn_match2[i] = -1;
    return 0;
  }
  const int stride = n1 > n2 ? n1 : n2;
  StageLease S(t_kf_err);
  StageLayout L;
  const SearchSim3Layout l = layout_search_sim3(L, n1, n2);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t st = S.stream();
  const slamgpu_kf dk[2] = {upload_kf(S, *kf1, l.kf[0]), upload_kf(S, *kf2, l.kf[1])};
  slamgpu_sim3_pair pr{};
  pr.kf1 = 0;
  pr.kf2 = 1;
  pr.mp1_begin = 0;
  pr.mp2_begin = n1;
  for (int i = 0; i < 9; i++) {
    pr.sR12[i] = sR12[i];
    pr.sR21[i] = sR21[i];
  }
  for (int i = 0; i < 3; i++) {
    pr.t12[i] = t12[i];
    pr.t21[i] = t21[i];
  }
  const size_t pt = sizeof(slamgpu_fuse_point);
  HIPCHECK(t_kf_err, S.upload(l.kfs, dk, sizeof(dk)));
  HIPCHECK(t_kf_err, S.upload(l.mp, mp1, (size_t)n1 * pt));
  HIPCHECK(t_kf_err, S.upload(l.mp + (size_t)n1 * pt, mp2, (size_t)n2 * pt));
  HIPCHECK(t_kf_err, S.upload(l.pair, &pr, sizeof(pr)));
  HIPCHECK(t_kf_err, S.upload(l.already1, already1, (size_t)n1));
  HIPCHECK(t_kf_err, S.upload(l.already2, already2, (size_t)n2));
  if (int r = slamgpu_search_by_sim3_device(
          S.at<slamgpu_kf>(l.kfs), S.at<slamgpu_fuse_point>(l.mp), n1 + n2,
          S.at<slamgpu_sim3_pair>(l.pair), 1, S.at<uint8_t>(l.already1), S.at<uint8_t>(l.already2),
          stride, th, cam, lv, grid, S.at<int32_t>(l.match12), S.at<int32_t>(l.vn_match1),
          S.at<int32_t>(l.vn_match2), S.at<int32_t>(l.nfound), st))
    return r;
  int32_t nf = 0;
  HIPCHECK(t_kf_err, S.download(match12, l.match12, (size_t)n1 * 4));
  HIPCHECK(t_kf_err, S.download(vn_match1, l.vn_match1, (size_t)n1 * 4));
  HIPCHECK(t_kf_err, S.download(vn_match2, l.vn_match2, (size_t)n2 * 4));
  HIPCHECK(t_kf_err, S.download(&nf, l.nfound, 4));
  HIPCHECK(t_kf_err, hipStreamSynchronize(st));
  if (nf < 0) return t_kf_err.fail(SLAMGPU_EINVAL, "pair rejected on the device");
  *nfound = nf;
  return 0;
}

}  // extern "C"
