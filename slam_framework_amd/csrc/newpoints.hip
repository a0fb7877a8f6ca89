// newpoints.hip -- LocalMapper::CreateNewMapPoints (src/core/local_mapper.cpp:258-492) on gfx950:
// the chain over the neighbour keyframes without a trip through the host
// (include/slamgpu_kfmatch.h).
//
//   np_prepare   the slamgpu_tri_pair of every (neighbour k, job) in scratch, n_new = 0.
//   search_tri   kfmatch.hip's kernel through slamgpu_search_for_triangulation_device, neighbour k
//                of every job in one launch, on the has_mp the step before left.
//   new_points   one workgroup per job: a lane per keypoint of the current keyframe with a match
//                runs :335-471 (rays, the stereo / DLT / skip branch, depth, reprojection and scale
//                tests) and builds the MapPoint of :474-485; the accepted ones are compacted in
//                ascending idx1 by a workgroup scan (the order is the reference's), has_mp is set.
// A skipped or absent neighbour still gets a search (the launch is one per k for all jobs): its
// pair is (kf1, kf1) with F12 = 0, which matches nothing, and its row is not read.
// Float semantics follow tests/newpoints_ref.c line by line (DESIGN.md "CreateNewMapPoints"): the
// Initializer's cv::Mat rules, the Release build's fma association written out, the stereo
// parallax as (d^2 - h^2) / (d^2 + h^2) in double.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jacobi_svd.h"
#include "kfmatch_common.h"

namespace slamgpu {
namespace {

static_assert(sizeof(slamgpu_kf_stereo) == 40, "slamgpu_kf_stereo layout");
static_assert(sizeof(slamgpu_newpoints_nbor) == 48, "slamgpu_newpoints_nbor layout");
static_assert(sizeof(slamgpu_newpoints_job) == 24, "slamgpu_newpoints_job layout");
static_assert(sizeof(slamgpu_new_point) == 16, "slamgpu_new_point layout");

constexpr int kNpThreads = 512;
constexpr int kNpSweeps = 6;  // tools/newpoints_jacobi_sweeps.py: settled after 4, plus two

__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }

// y = R^T x under the cv::Mat product rule: a double sum over ascending k, rounded once.
__device__ __forceinline__ void rotate_t(const float* R, const float* x, float* y) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) acc += (double)R[3 * k + i] * (double)x[k];
    y[i] = (float)acc;
  }
}

__device__ __forceinline__ double dot3d(const float* a, const float* b) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) acc += (double)a[k] * (double)b[k];
  return acc;
}

// cos(2 * atan2(mb / 2, depth)) (:362, :365) by the project's identity.
__device__ __forceinline__ float cos_stereo(float mb, float depth) {
  const float h = fdiv(mb, 2.0f);
  const double hh = (double)h * (double)h, dd = (double)depth * (double)depth;
  return (float)((dd - hh) / (dd + hh));
}

// The null vector of the DLT matrix (:376-385), rounded to float. Out of line: the FP64 4 x 4
// Jacobi is the register peak of the kernel and only the lanes of the DLT branch pay for it.
__device__ __noinline__ void dlt_null_vector(const float* xn1, const slamgpu_kf& K1,
                                             const float* xn2, const slamgpu_kf& K2, float* x) {
  float A[16];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float a0 = c < 3 ? K1.Rcw[c] : K1.tcw[0], a1 = c < 3 ? K1.Rcw[3 + c] : K1.tcw[1],
                a2 = c < 3 ? K1.Rcw[6 + c] : K1.tcw[2];
    const float b0 = c < 3 ? K2.Rcw[c] : K2.tcw[0], b1 = c < 3 ? K2.Rcw[3 + c] : K2.tcw[1],
                b2 = c < 3 ? K2.Rcw[6 + c] : K2.tcw[2];
    A[c] = xn1[0] * a2 - a0;
    A[4 + c] = xn1[1] * a2 - a1;
    A[8 + c] = xn2[0] * b2 - b0;
    A[12 + c] = xn2[1] * b2 - b1;
  }
  double d[4], vt[16], ut[16];
  svd_lane<4, kNpSweeps>(A, d, vt, ut);
#pragma unroll
  for (int r = 0; r < 4; r++) x[r] = (float)vt[12 + r];
}

// KeyFrame::UnprojectStereo (keyframe.cpp:478-492); Twc = [Rcw^T | Ow].
__device__ __forceinline__ bool unproject_stereo(const slamgpu_kf& K, const slamgpu_kf_stereo& S,
                                                 int i, float* x3D) {
  const float z = S.depth[i];
  if (!(z > 0)) return false;
  const slamgpu_keypoint* raw = S.raw_kps ? S.raw_kps : K.kps;
  const float u = raw[i].x, v = raw[i].y;
  const float invfx = fdiv(1.0f, S.cam.fx), invfy = fdiv(1.0f, S.cam.fy);
  const float c[3] = {(u - S.cam.cx) * z * invfx, (v - S.cam.cy) * z * invfy, z};
  float r[3];
  rotate_t(K.Rcw, c, r);
#pragma unroll
  for (int k = 0; k < 3; k++) x3D[k] = r[k] + K.Ow[k];
  return true;
}

// What a lane keeps of its new MapPoint until the scan has placed it.
struct NewPoint {
  float xyz[3], normal[3], min_dist, max_dist;
};

// One pair (:335-485): the status, and the point when it is positive.
__device__ __forceinline__ int pair_one(const slamgpu_kf& K1, const slamgpu_kf_stereo& S1,
                                        const slamgpu_kf& K2, const slamgpu_kf_stereo& S2,
                                        int idx1, int idx2, const slamgpu_levels& lv,
                                        NewPoint* out) {
  if ((unsigned)idx2 >= (unsigned)K2.n) return SLAMGPU_NP_MALFORMED;
  const slamgpu_keypoint kp1 = K1.kps[idx1], kp2 = K2.kps[idx2];
  if ((unsigned)kp1.octave >= (unsigned)lv.nlevels || (unsigned)kp2.octave >= (unsigned)lv.nlevels)
    return SLAMGPU_NP_MALFORMED;
  const float ur1 = K1.u_right[idx1], ur2 = K2.u_right[idx2];
  const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
  const slamgpu_camera c1 = S1.cam, c2 = S2.cam;

  // :347-355
  const float xn1[3] = {(kp1.x - c1.cx) * fdiv(1.0f, c1.fx), (kp1.y - c1.cy) * fdiv(1.0f, c1.fy),
                        1.0f};
  const float xn2[3] = {(kp2.x - c2.cx) * fdiv(1.0f, c2.fx), (kp2.y - c2.cy) * fdiv(1.0f, c2.fy),
                        1.0f};
  float ray1[3], ray2[3];
  rotate_t(K1.Rcw, xn1, ray1);
  rotate_t(K2.Rcw, xn2, ray2);
  const float cosRays = (float)(dot3d(ray1, ray2) / (__builtin_sqrt(dot3d(ray1, ray1)) *
                                                     __builtin_sqrt(dot3d(ray2, ray2))));

  // :357-369
  float cosSt = cosRays + 1;
  float cosSt1 = cosSt, cosSt2 = cosSt;
  if (st1) cosSt1 = cos_stereo(S1.mb, S1.depth[idx1]);
  else if (st2) cosSt2 = cos_stereo(S2.mb, S2.depth[idx2]);
  cosSt = cosSt2 < cosSt1 ? cosSt2 : cosSt1;

  float x3D[3];
  int source;
  if (cosRays < cosSt && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {  // :372-374
    float x[4];
    dlt_null_vector(xn1, K1, xn2, K2, x);
    if (x[3] == 0) return SLAMGPU_NP_W_ZERO;
    const float s = (float)(1.0 / (double)x[3]);
#pragma unroll
    for (int k = 0; k < 3; k++) x3D[k] = x[k] * s;
    source = SLAMGPU_NP_DLT;
  } else if (st1 && cosSt1 < cosSt2) {
    if (!unproject_stereo(K1, S1, idx1, x3D)) return SLAMGPU_NP_NO_DEPTH;
    source = SLAMGPU_NP_STEREO1;
  } else if (st2 && cosSt2 < cosSt1) {
    if (!unproject_stereo(K2, S2, idx2, x3D)) return SLAMGPU_NP_NO_DEPTH;
    source = SLAMGPU_NP_STEREO2;
  } else {
    return SLAMGPU_NP_LOW_PARALLAX;
  }

  // :406-414
  const float z1 = (float)(dot3d(K1.Rcw + 6, x3D) + (double)K1.tcw[2]);
  if (z1 <= 0) return SLAMGPU_NP_BEHIND1;
  const float z2 = (float)(dot3d(K2.Rcw + 6, x3D) + (double)K2.tcw[2]);
  if (z2 <= 0) return SLAMGPU_NP_BEHIND2;

  // :417-435
  const float sig1 = lv.sigma2[kp1.octave];
  const float x1 = (float)(dot3d(K1.Rcw, x3D) + (double)K1.tcw[0]);
  const float y1 = (float)(dot3d(K1.Rcw + 3, x3D) + (double)K1.tcw[1]);
  const float u1 = fdiv(c1.fx * x1, z1) + c1.cx;
  const float v1 = fdiv(c1.fy * y1, z1) + c1.cy;
  const float ex1 = u1 - kp1.x, ey1 = v1 - kp1.y;
  if (st1) {
    const float u1r = u1 - fdiv(c1.bf, z1);
    const float er1 = u1r - ur1;
    if ((double)fmaf(er1, er1, fmaf(ex1, ex1, ey1 * ey1)) > 7.8 * (double)sig1)
      return SLAMGPU_NP_REPROJ1_STEREO;
  } else {
    if ((double)fmaf(ex1, ex1, ey1 * ey1) > 5.991 * (double)sig1) return SLAMGPU_NP_REPROJ1_MONO;
  }

  // :438-456; :447 reads the current keyframe's mbf
  const float sig2 = lv.sigma2[kp2.octave];
  const float x2 = (float)(dot3d(K2.Rcw, x3D) + (double)K2.tcw[0]);
  const float y2 = (float)(dot3d(K2.Rcw + 3, x3D) + (double)K2.tcw[1]);
  const float u2 = fdiv(c2.fx * x2, z2) + c2.cx;
  const float v2 = fdiv(c2.fy * y2, z2) + c2.cy;
  const float ex2 = u2 - kp2.x, ey2 = v2 - kp2.y;
  if (st2) {
    const float u2r = u2 - fdiv(c1.bf, z2);
    const float er2 = u2r - ur2;
    if (fmaf(er2, er2, fmaf(ex2, ex2, ey2 * ey2)) > 7.8f * sig2) return SLAMGPU_NP_REPROJ2_STEREO;
  } else {
    if ((double)fmaf(ex2, ex2, ey2 * ey2) > 5.991 * (double)sig2) return SLAMGPU_NP_REPROJ2_MONO;
  }

  // :459-471
  const float n1[3] = {x3D[0] - K1.Ow[0], x3D[1] - K1.Ow[1], x3D[2] - K1.Ow[2]};
  const float n2[3] = {x3D[0] - K2.Ow[0], x3D[1] - K2.Ow[1], x3D[2] - K2.Ow[2]};
  const double nd1 = __builtin_sqrt(dot3d(n1, n1)), nd2 = __builtin_sqrt(dot3d(n2, n2));
  const float dist1 = (float)nd1, dist2 = (float)nd2;
  if (dist1 == 0 || dist2 == 0) return SLAMGPU_NP_DIST_ZERO;
  const float ratioDist = fdiv(dist2, dist1);
  const float ratioFactor = 1.5f * lv.scale[lv.nlevels > 1 ? 1 : 0];
  const float ratioOctave = fdiv(lv.scale[kp1.octave], lv.scale[kp2.octave]);
  if (ratioDist * ratioFactor < ratioOctave || fdiv(ratioDist, ratioFactor) > ratioOctave)
    return SLAMGPU_NP_SCALE;

  // the MapPoint after :474-485 (map_point.cpp:311-354 with two observations)
  const float s1 = (float)(1.0 / nd1), s2 = (float)(1.0 / nd2);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    out->xyz[k] = x3D[k];
    float normal = 0.0f;
    normal = normal + n1[k] * s1;
    normal = normal + n2[k] * s2;
    out->normal[k] = normal * 0.5f;
  }
  out->max_dist = dist1 * lv.scale[kp1.octave];
  out->min_dist = fdiv(out->max_dist, lv.scale[lv.nlevels - 1]);
  return source;
}

// The rank of this thread among the threads of the workgroup whose flag is set, in thread order
// (lanes before it in its wave, then the waves before that), and their number. No atomics: the
// order of the output is the reference's.
__device__ __forceinline__ void block_rank(bool flag, int* s_count, int* before, int* total) {
  const int lane = lane_id(), wid = wave_id();
  const unsigned long long votes = __ballot(flag);
  __syncthreads();  // the counts of the scan before this one have been read
  if (lane == 0) s_count[wid] = __popcll(votes);
  __syncthreads();
  int b = __popcll(votes & ((1ull << lane) - 1ull)), t = 0;
#pragma unroll
  for (int w = 0; w < kNpThreads / 64; w++) {
    b += w < wid ? s_count[w] : 0;
    t += s_count[w];
  }
  *before = b;
  *total = t;
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void np_prepare_kernel(
    const slamgpu_newpoints_job* __restrict__ jobs, int n_jobs,
    const slamgpu_newpoints_nbor* __restrict__ nbors, int max_nbors,
    slamgpu_tri_pair* __restrict__ pairs, int32_t* __restrict__ n_new) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_jobs * max_nbors) return;
  const int k = t / n_jobs, j = t % n_jobs;
  const slamgpu_newpoints_job J = jobs[j];
  slamgpu_tri_pair P;
  P.kf1 = P.kf2 = J.kf1;
  for (int i = 0; i < 9; i++) P.F12[i] = 0.0f;
  P.only_stereo = 0;
  if (k < J.n_nbors) {
    const slamgpu_newpoints_nbor& N = nbors[J.first_nbor + k];
    if (!N.skip) {
      P.kf2 = N.kf2;
      for (int i = 0; i < 9; i++) P.F12[i] = N.F12[i];
    }
  }
  pairs[t] = P;
  if (k == 0) n_new[j] = 0;
}

__global__ __launch_bounds__(kNpThreads) void new_points_kernel(
    const slamgpu_kf* __restrict__ kfs, const slamgpu_kf_stereo* __restrict__ kst,
    const slamgpu_newpoints_job* __restrict__ jobs, const slamgpu_newpoints_nbor* __restrict__ nbors,
    int k, int max_nbors, slamgpu_levels lv, const int32_t* __restrict__ match,
    const int32_t* __restrict__ nmatches, int32_t* __restrict__ n_new,
    slamgpu_fuse_point* __restrict__ points, slamgpu_new_point* __restrict__ news,
    int64_t point_stride, int8_t* __restrict__ status, int64_t status_stride) {
  __shared__ int s_count[kNpThreads / 64];
  __shared__ uint16_t s_idx1[kMaxFeat];  // the keypoints with a match, ascending
  const int job = blockIdx.x, tid = threadIdx.x;
  const slamgpu_newpoints_job J = jobs[job];
  if (k >= J.n_nbors) return;
  int n_cur = n_new[job];
  if (n_cur < 0) return;
  const slamgpu_newpoints_nbor& N = nbors[J.first_nbor + k];
  const slamgpu_kf& K1 = kfs[J.kf1];
  const int n1 = K1.n;
  // a search that reported -1 (n1 outside [0, kMaxFeat] among its reasons), or rows too short
  if ((!N.skip && nmatches[job] < 0) || n1 < 0 || n1 > kMaxFeat || n1 > status_stride) {
    if (tid == 0) n_new[job] = -1;
    return;
  }
  int8_t* st_row = status + ((int64_t)job * max_nbors + k) * status_stride;
  if (N.skip) {
    for (int i = tid; i < n1; i += kNpThreads) st_row[i] = 0;
    return;
  }
  const slamgpu_kf& K2 = kfs[N.kf2];
  const slamgpu_kf_stereo& S1 = kst[J.kf1];
  const slamgpu_kf_stereo& S2 = kst[N.kf2];
  const int32_t* m12 = match + (int64_t)job * kMaxFeat;
  slamgpu_fuse_point* pts = points + (int64_t)job * point_stride;
  slamgpu_new_point* nws = news + (int64_t)job * point_stride;
  // the matched keypoints first, so that the pair routine runs on full waves
  int n_matched = 0;
  for (int base = 0; base < n1; base += kNpThreads) {
    const int i = base + tid;
    const bool matched = i < n1 && m12[i] >= 0;
    if (i < n1 && !matched) st_row[i] = 0;
    int before, total;
    block_rank(matched, s_count, &before, &total);
    if (matched) s_idx1[n_matched + before] = (uint16_t)i;
    n_matched += total;
  }
  __syncthreads();
  for (int base = 0; base < n_matched; base += kNpThreads) {
    int st = 0, idx2 = -1, i = -1;
    NewPoint p;
    if (base + tid < n_matched) {
      i = s_idx1[base + tid];
      idx2 = m12[i];
      st = pair_one(K1, S1, K2, S2, i, idx2, lv, &p);
      st_row[i] = (int8_t)st;
    }
    int before, total;
    block_rank(st > 0, s_count, &before, &total);
    if ((int64_t)n_cur + total > point_stride) {
      if (tid == 0) n_new[job] = -1;
      return;
    }
    if (st > 0) {
      slamgpu_fuse_point& o = pts[n_cur + before];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        o.xyz[c] = p.xyz[c];
        o.normal[c] = p.normal[c];
        o.pad[c] = 0;
      }
      o.min_dist = p.min_dist;
      o.max_dist = p.max_dist;
      o.skip = 0;
      const Desc d = load_desc(N.first_obs ? K2.desc + (int64_t)idx2 * 32 : K1.desc + (int64_t)i * 32);
      uint4* od = reinterpret_cast<uint4*>(o.desc);
      od[0] = d.a;
      od[1] = d.b;
      slamgpu_new_point& q = nws[n_cur + before];
      q.neighbour = k;
      q.idx1 = i;
      q.idx2 = idx2;
      q.source = st;
      J.has_mp1[i] = 1;
    }
    n_cur += total;
  }
  if (tid == 0) n_new[job] = n_cur;
}

struct NpScratch {
  size_t pairs, match, nmatches, size;
};
inline NpScratch np_scratch(size_t n_jobs, size_t max_nbors) {
  StageLayout L;
  NpScratch s;
  s.pairs = L.take<slamgpu_tri_pair>(n_jobs * max_nbors);
  s.match = L.take<int32_t>(n_jobs * kMaxFeat);
  s.nmatches = L.take<int32_t>(n_jobs);
  s.size = L.size();
  return s;
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

size_t slamgpu_create_new_map_points_scratch_bytes(int n_jobs, int max_nbors) {
  if (n_jobs <= 0 || max_nbors <= 0) return 0;
  return np_scratch((size_t)n_jobs, (size_t)max_nbors).size;
}

int slamgpu_create_new_map_points_device(
    const slamgpu_kf* d_kfs, const slamgpu_kf_stereo* d_kf_stereo,
    const slamgpu_newpoints_job* d_jobs, int n_jobs, const slamgpu_newpoints_nbor* d_nbors,
    int max_nbors, const slamgpu_camera* cam, const slamgpu_levels* lv, int check_ori,
    int32_t* d_n_new, slamgpu_fuse_point* d_points, slamgpu_new_point* d_new, int64_t point_stride,
    int8_t* d_status, int64_t status_stride, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (n_jobs < 0 || max_nbors < 0)
    return t_kf_err.fail(SLAMGPU_EINVAL, "n_jobs %d or max_nbors %d < 0", n_jobs, max_nbors);
  if (n_jobs == 0) return 0;
  if (!d_kfs || !d_kf_stereo || !d_jobs || !d_n_new || !cam)
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_levels(lv)) return r;
  if (point_stride < 0 || status_stride < 0)
    return t_kf_err.fail(SLAMGPU_EINVAL, "negative stride");
  if (max_nbors > 0 && (!d_nbors || !d_points || !d_new || !d_status || !d_scratch))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if ((uintptr_t)d_points % 16 || (uintptr_t)d_scratch % 16)
    return t_kf_err.fail(SLAMGPU_EINVAL, "d_points and d_scratch must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (max_nbors == 0) {
    HIPCHECK(t_kf_err, hipMemsetAsync(d_n_new, 0, (size_t)n_jobs * 4, st));
    return 0;
  }
  const NpScratch s = np_scratch((size_t)n_jobs, (size_t)max_nbors);
  if (scratch_bytes < s.size)
    return t_kf_err.fail(SLAMGPU_EINVAL, "scratch: %zu bytes given, %zu needed", scratch_bytes,
                         s.size);
  char* base = static_cast<char*>(d_scratch);
  slamgpu_tri_pair* pairs = reinterpret_cast<slamgpu_tri_pair*>(base + s.pairs);
  int32_t* match = reinterpret_cast<int32_t*>(base + s.match);
  int32_t* nmatches = reinterpret_cast<int32_t*>(base + s.nmatches);
  const int n_pairs = n_jobs * max_nbors;
  hipLaunchKernelGGL(np_prepare_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, d_jobs,
                     n_jobs, d_nbors, max_nbors, pairs, d_n_new);
  HIPCHECK(t_kf_err, hipGetLastError());
  for (int k = 0; k < max_nbors; k++) {
    if (int r = slamgpu_search_for_triangulation_device(d_kfs, pairs + (size_t)k * n_jobs, n_jobs,
                                                        cam, lv, check_ori, match, kMaxFeat,
                                                        nmatches, stream))
      return r;
    hipLaunchKernelGGL(new_points_kernel, dim3(n_jobs), dim3(kNpThreads), 0, st, d_kfs,
                       d_kf_stereo, d_jobs, d_nbors, k, max_nbors, *lv, match, nmatches, d_n_new,
                       d_points, d_new, point_stride, d_status, status_stride);
    HIPCHECK(t_kf_err, hipGetLastError());
  }
  return 0;
}

int slamgpu_create_new_map_points(const slamgpu_kf* kfs, const slamgpu_kf_stereo* st,
                                  const slamgpu_newpoints_nbor* nbors, int n_nbors,
                                  const slamgpu_camera* cam, const slamgpu_levels* lv, int check_ori,
                                  uint8_t* has_mp1, slamgpu_fuse_point* points,
                                  slamgpu_new_point* news, int8_t* status, int* n_new) {
  if (n_nbors < 0 || n_nbors > 64)
    return t_kf_err.fail(SLAMGPU_EINVAL, "n_nbors %d outside [0, 64]", n_nbors);
  if (!kfs || !st || !cam || !n_new || (n_nbors > 0 && !nbors))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (int r = check_levels(lv)) return r;
  const int n_kfs = 1 + n_nbors;
  slamgpu_kf hk[65];
  for (int i = 0; i < n_kfs; i++) hk[i] = kfs[i];
  hk[0].has_mp = has_mp1;
  for (int i = 0; i < n_kfs; i++) {
    if (int r = check_kf(&hk[i], true, i ? "neighbour" : "kf1")) return r;
    if (hk[i].n > 0 && !st[i].depth)
      return t_kf_err.fail(SLAMGPU_EINVAL, "keyframe %d: NULL depth", i);
  }
  const int n1 = hk[0].n;
  if (n1 > 0 && n_nbors > 0 && (!points || !news || !status))
    return t_kf_err.fail(SLAMGPU_EINVAL, "NULL output");
  *n_new = 0;
  if (n_nbors == 0) return 0;

  StageLease S(t_kf_err);
  StageLayout L;
  KfPlace place[65];
  size_t depth_at[65], raw_at[65];
  for (int i = 0; i < n_kfs; i++) {
    const int nn = hk[i].n_nodes;
    place[i] = place_kf(L, kKfFeatureVector, hk[i].n, nn, nn > 0 ? hk[i].node_start[nn] : 0);
    depth_at[i] = L.take<float>(hk[i].n);
    raw_at[i] = st[i].raw_kps ? L.take<slamgpu_keypoint>(hk[i].n) : kNoSlot;
  }
  const size_t at_kfs = L.take<slamgpu_kf>(n_kfs), at_st = L.take<slamgpu_kf_stereo>(n_kfs);
  const size_t at_job = L.take<slamgpu_newpoints_job>(1);
  const size_t at_nbors = L.take<slamgpu_newpoints_nbor>(n_nbors);
  const size_t at_n_new = L.take<int32_t>(1);
  const size_t at_points = L.take<slamgpu_fuse_point>(n1), at_news = L.take<slamgpu_new_point>(n1);
  const size_t at_status = L.take((size_t)n_nbors * n1);
  const size_t scratch_bytes = slamgpu_create_new_map_points_scratch_bytes(1, n_nbors);
  const size_t at_scratch = L.take(scratch_bytes);
  if (int r = S.reserve(L.size())) return r;
  hipStream_t stream = S.stream();

  slamgpu_kf dk[65];
  slamgpu_kf_stereo ds[65];
  slamgpu_newpoints_nbor hn[64];
  for (int i = 0; i < n_kfs; i++) {
    dk[i] = upload_kf(S, hk[i], place[i]);
    ds[i] = st[i];
    HIPCHECK(t_kf_err, S.upload(depth_at[i], st[i].depth, (size_t)hk[i].n * 4));
    ds[i].depth = S.at<float>(depth_at[i]);
    if (raw_at[i] != kNoSlot) {
      HIPCHECK(t_kf_err, S.upload(raw_at[i], st[i].raw_kps, (size_t)hk[i].n * sizeof(slamgpu_keypoint)));
      ds[i].raw_kps = S.at<slamgpu_keypoint>(raw_at[i]);
    }
  }
  for (int k = 0; k < n_nbors; k++) {
    hn[k] = nbors[k];
    hn[k].kf2 = 1 + k;
  }
  slamgpu_newpoints_job job{};
  job.kf1 = 0;
  job.first_nbor = 0;
  job.n_nbors = n_nbors;
  job.has_mp1 = const_cast<uint8_t*>(dk[0].has_mp);
  HIPCHECK(t_kf_err, S.upload(at_kfs, dk, sizeof(slamgpu_kf) * n_kfs));
  HIPCHECK(t_kf_err, S.upload(at_st, ds, sizeof(slamgpu_kf_stereo) * n_kfs));
  HIPCHECK(t_kf_err, S.upload(at_job, &job, sizeof(job)));
  HIPCHECK(t_kf_err, S.upload(at_nbors, hn, sizeof(slamgpu_newpoints_nbor) * n_nbors));
  if (int r = slamgpu_create_new_map_points_device(
          S.at<slamgpu_kf>(at_kfs), S.at<slamgpu_kf_stereo>(at_st),
          S.at<slamgpu_newpoints_job>(at_job), 1, S.at<slamgpu_newpoints_nbor>(at_nbors), n_nbors,
          cam, lv, check_ori, S.at<int32_t>(at_n_new), S.at<slamgpu_fuse_point>(at_points),
          S.at<slamgpu_new_point>(at_news), n1, S.at<int8_t>(at_status), n1,
          S.at<char>(at_scratch), scratch_bytes, stream))
    return r;
  int32_t nn = 0;
  HIPCHECK(t_kf_err, S.download(&nn, at_n_new, 4));
  HIPCHECK(t_kf_err, S.download(status, at_status, (size_t)n_nbors * n1));
  HIPCHECK(t_kf_err, S.download(has_mp1, place[0].has_mp, (size_t)n1));
  HIPCHECK(t_kf_err, hipStreamSynchronize(stream));
  *n_new = nn;
  if (nn > 0) {
    HIPCHECK(t_kf_err, S.download(points, at_points, (size_t)nn * sizeof(slamgpu_fuse_point)));
    HIPCHECK(t_kf_err, S.download(news, at_news, (size_t)nn * sizeof(slamgpu_new_point)));
    HIPCHECK(t_kf_err, hipStreamSynchronize(stream));
  }
  return 0;
}

}  // extern "C"
