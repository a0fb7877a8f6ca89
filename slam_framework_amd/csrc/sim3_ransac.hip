// sim3_ransac.hip -- the loop closer's RANSAC Sim3 solver (include/slamgpu_sim3solver.h): every
// hypothesis of every candidate in one launch, then the iterations at which the reference's
// Sim3Solver::iterate (src/solvers/sim3solver.cpp:142-211) would return.
//
//   sim3_hyp_kernel    grid (ceil(max_its / 4), jobs), 4 waves per workgroup, ONE WAVE PER
//                      HYPOTHESIS. The wave resolves its three draws to correspondence indices
//                      (the swap-and-pop of :173-179, on every lane), solves Horn once -- every
//                      lane holds the same transform, the FP64 Jacobi costs a wave the same
//                      whether one lane or 64 run it -- and strides over the correspondences 64 at
//                      a time: one lane per correspondence, the ballot of err1 < max1 && err2 <
//                      max2 is the mask word (one 8-byte store by lane 0), its popcount the count.
//                      No per-correspondence bytes, no atomics, no LDS: a job's records are a few
//                      KB that all its waves read from L2 (4096 x 48 B would not fit LDS anyway),
//                      and a lane's three loads consume its 48-byte record whole.
//   sim3_event_kernel  one wave per job: exclusive prefix maximum over the <= 300 counts in
//                      chunks of 64 (shuffles), the predicate of :186-195, ballot compaction.
//
// Both kernels validate the job the same way first (ranges, n, n_its, every draw), so an invalid
// job writes n_events = -1 and nothing else.
//
// Arithmetic: DESIGN.md "RANSAC Sim3 solver"; tests/sim3solver_ref.c restates it on the CPU and
// the two are compared bit for bit. The library is built -ffp-contract=off; nothing here turns
// contraction back on (the one fma is the reference's own, u = fx * x + cx). The draw checks, the
// swap-and-pop, the mask word and the compaction are ransac_device.h's, as in the other solvers;
// the angle of the two-sided Jacobi is jacobi_angle of jacobi_svd.h, as in their one-sided one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/slamgpu_sim3solver.h"
#include "device_math.h"
#include "host_stage.h"
#include "jacobi_svd.h"
#include "ransac_device.h"
#include "stage_layout.h"

namespace slamgpu {
namespace {

constexpr int kHypWaves = 4;       // hypotheses (waves) per workgroup
constexpr int kJacobiSweeps = 8;   // 6 found on the CPU, plus two

struct RansacParams {
  float K1[4], K2[4];
  float thr1[SLAMGPU_MAX_LEVELS], thr2[SLAMGPU_MAX_LEVELS];  // (float)(size_t)(9.210 * sigma2)
  int nlevels;
};

__device__ __forceinline__ bool job_ranges_ok(const slamgpu_sim3_ransac_job& J,
                                              int n_matches_total, int n_draws_total, int max_n,
                                              int max_its) {
  if (J.n < 3 || J.n > max_n || J.n > SLAMGPU_SIM3_MAX_MATCHES) return false;
  if (J.n_its < 1 || J.n_its > max_its) return false;
  if (J.match_begin < 0 || (int64_t)J.match_begin + J.n > (int64_t)n_matches_total) return false;
  if (J.draw_begin < 0 || (int64_t)J.draw_begin + 3 * (int64_t)J.n_its > (int64_t)n_draws_total)
    return false;
  return true;
}

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return a0 * b0 + a1 * b1 + a2 * b2;
}

// One Jacobi rotation on the pair (P, Q) of the symmetric A, accumulated into V.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  double t, c, s;
  jacobi_angle((A[Q][Q] - A[P][P]) / (2.0 * apq), t, c, s);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k == P || k == Q) continue;
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = A[P][k] = c * akp - s * akq;
    A[k][Q] = A[Q][k] = s * akp + c * akq;
  }
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

struct Transform {
  float T12[12], T21[12];  // rows [sR | t]
};

// ComputeSim3 (:230-341) on the sample P1 / P2 (row-major 3x3, column i = point i).
__device__ __forceinline__ void compute_sim3(const float (&P1)[9], const float (&P2)[9],
                                             int fix_scale, float (&R)[9], float (&t)[3], float& s12,
                                             Transform& T) {
  const float third = (float)(1.0 / 3.0);
  float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[3 * r] + P1[3 * r + 1]) + P1[3 * r + 2]) * third;
    O2[r] = ((P2[3 * r] + P2[3 * r + 1]) + P2[3 * r + 2]) * third;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      Pr1[3 * r + i] = P1[3 * r + i] - O1[r];
      Pr2[3 * r + i] = P2[3 * r + i] - O2[r];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      M[3 * i + j] = dot3(Pr2[3 * i], Pr2[3 * i + 1], Pr2[3 * i + 2], Pr1[3 * j], Pr1[3 * j + 1],
                          Pr1[3 * j + 2]);
  const float N11 = M[0] + M[4] + M[8];
  const float N12 = M[5] - M[7];
  const float N13 = M[6] - M[2];
  const float N14 = M[1] - M[3];
  const float N22 = M[0] - M[4] - M[8];
  const float N23 = M[1] + M[3];
  const float N24 = M[6] + M[2];
  const float N33 = -M[0] + M[4] - M[8];
  const float N34 = M[5] + M[7];
  const float N44 = -M[0] - M[4] + M[8];
  double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24},
                    {N13, N23, N33, N34}, {N14, N24, N34, N44}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
  for (int sw = 0; sw < kJacobiSweeps; sw++) {
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<0, 3>(A, V);
    jacobi_rotate<1, 2>(A, V);
    jacobi_rotate<1, 3>(A, V);
    jacobi_rotate<2, 3>(A, V);
  }
  // the largest eigenvalue, lowest index on a tie (a NaN never wins)
  double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0], best = A[0][0];
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (A[i][i] > best) {
      best = A[i][i];
      w = V[0][i];
      x = V[1][i];
      y = V[2][i];
      z = V[3][i];
    }
  const double nrm = __builtin_sqrt(w * w + x * x + y * y + z * z);
  w = w / nrm;
  x = x / nrm;
  y = y / nrm;
  z = z / nrm;
  R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  R[1] = (float)(2.0 * (x * y - w * z));
  R[2] = (float)(2.0 * (x * z + w * y));
  R[3] = (float)(2.0 * (x * y + w * z));
  R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  R[5] = (float)(2.0 * (y * z - w * x));
  R[6] = (float)(2.0 * (x * z - w * y));
  R[7] = (float)(2.0 * (y * z + w * x));
  R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
  float s = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float p3 = dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[j], Pr2[3 + j], Pr2[6 + j]);
        const float a = Pr1[3 * i + j] * p3, b = p3 * p3;
        nom += (double)a;
        den += (double)b;
      }
    s = (float)(nom / den);
  }
  s12 = s;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float d = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], O2[0], O2[1], O2[2]);
    t[r] = (float)((double)(-s) * (double)d + (double)O1[r]);
  }
  const float inv = (float)(1.0 / (double)s);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      T.T12[4 * r + c] = s * R[3 * r + c];
      T.T21[4 * r + c] = R[3 * c + r] * inv;
    }
#pragma unroll
  for (int r = 0; r < 3; r++) {
    T.T12[4 * r + 3] = t[r];
    T.T21[4 * r + 3] = -dot3(T.T21[4 * r], T.T21[4 * r + 1], T.T21[4 * r + 2], t[0], t[1], t[2]);
  }
}

// FromCameraToImage (:424-428).
__device__ __forceinline__ void to_image(float X, float Y, float Z, const float (&K)[4], float& u,
                                         float& v) {
  const float invz = 1.0f / Z;
  const float x = X * invz, y = Y * invz;
  u = __builtin_fmaf(K[0], x, K[2]);
  v = __builtin_fmaf(K[1], y, K[3]);
}

// Project (:402-407): the small gemm row, a float dot plus a double add.
__device__ __forceinline__ void project(const float (&T)[12], const float (&X)[3],
                                        const float (&K)[4], float& u, float& v) {
  float P[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float d = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2];
    P[r] = (float)((double)d + (double)T[4 * r + 3]);
  }
  to_image(P[0], P[1], P[2], K, u, v);
}

__global__ __launch_bounds__(64 * kHypWaves) void sim3_hyp_kernel(
    const slamgpu_sim3_match* __restrict__ matches, int n_matches_total,
    const int32_t* __restrict__ draws, int n_draws_total,
    const slamgpu_sim3_ransac_job* __restrict__ jobs, int max_n, int max_its, RansacParams P,
    slamgpu_sim3_hyp* __restrict__ hyp, uint64_t* __restrict__ inlier_bits) {
  const int job = blockIdx.y;
  const slamgpu_sim3_ransac_job J = jobs[job];
  if (!job_ranges_ok(J, n_matches_total, n_draws_total, max_n, max_its)) return;
  const int32_t* jd = draws + J.draw_begin;
  int bad = 0;
  for (int i = threadIdx.x; i < 3 * J.n_its; i += 64 * kHypWaves)
    bad |= !draw_in_range<3>(jd[i], i, J.n);
  if (__syncthreads_or(bad)) return;
  const int k = blockIdx.x * kHypWaves + wave_id();
  if (k >= J.n_its) return;
  const int n = J.n, lane = lane_id();
  const slamgpu_sim3_match* m = matches + J.match_begin;
  int idx[3];  // the sample (:173-179), the same on every lane
  resolve_sample<3>(jd + 3 * k, n, idx);
  float P1[9], P2[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      P1[3 * r + i] = m[idx[i]].x1c[r];
      P2[3 * r + i] = m[idx[i]].x2c[r];
    }
  float R[9], t[3], s12;
  Transform T;
  compute_sim3(P1, P2, J.fix_scale, R, t, s12, T);

  const int words = (max_n + 63) >> 6;
  const size_t row = (size_t)job * max_its + k;
  uint64_t* bits = inlier_bits + row * words;
  int cnt = 0;
  for (int w = 0; w < words; w++) {
    const int i = w * 64 + lane;
    bool in = false;
    if (i < n) {
      const slamgpu_sim3_match c = m[i];
      const int o1 = c.octave1, o2 = c.octave2;
      float u11, v11, u22, v22, u21, v21, u12, v12;
      to_image(c.x1c[0], c.x1c[1], c.x1c[2], P.K1, u11, v11);  // mvP1im1
      to_image(c.x2c[0], c.x2c[1], c.x2c[2], P.K2, u22, v22);  // mvP2im2
      project(T.T12, c.x2c, P.K1, u21, v21);                    // vP2im1
      project(T.T21, c.x1c, P.K2, u12, v12);                    // vP1im2
      const float d1x = u11 - u21, d1y = v11 - v21;
      const float d2x = u12 - u22, d2y = v12 - v22;
      const float err1 = d1x * d1x + d1y * d1y;
      const float err2 = d2x * d2x + d2y * d2y;
      if (o1 >= 0 && o1 < P.nlevels && o2 >= 0 && o2 < P.nlevels)
        in = err1 < P.thr1[o1] && err2 < P.thr2[o2];
    }
    cnt += store_mask_word(in, bits + w, lane);
  }
  if (lane == 0) {
    slamgpu_sim3_hyp h;
#pragma unroll
    for (int i = 0; i < 9; i++) h.R12[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) h.t12[i] = t[i];
    h.s12 = s12;
    h.n_inliers = cnt;
    h.pad[0] = h.pad[1] = 0;
    hyp[row] = h;
  }
}

__global__ __launch_bounds__(64) void sim3_event_kernel(
    const int32_t* __restrict__ draws, int n_matches_total, int n_draws_total,
    const slamgpu_sim3_ransac_job* __restrict__ jobs, int max_n, int max_its,
    const slamgpu_sim3_hyp* __restrict__ hyp, int32_t* __restrict__ events,
    int32_t* __restrict__ n_events) {
  const int job = blockIdx.x, lane = lane_id();
  const slamgpu_sim3_ransac_job J = jobs[job];
  if (!job_ranges_ok(J, n_matches_total, n_draws_total, max_n, max_its) ||
      !draws_ok<3>(draws + J.draw_begin, J.n_its, J.n, lane)) {
    if (lane == 0) n_events[job] = -1;
    return;
  }
  const slamgpu_sim3_hyp* jh = hyp + (size_t)job * max_its;
  int32_t* je = events + (size_t)job * max_its;
  int carry = 0, ne = 0;  // mnBestInliers, events so far
  for (int base = 0; base < J.n_its; base += 64) {
    const int k = base + lane;
    const int v = k < J.n_its ? jh[k].n_inliers : -1;
    int inc = v;  // inclusive prefix maximum of the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off, 64);
      if (lane >= off) inc = o > inc ? o : inc;
    }
    const int prev = __shfl_up(inc, 1, 64);
    const int excl = lane == 0 ? carry : (prev > carry ? prev : carry);
    const bool ev = k < J.n_its && v >= excl && v > J.min_inliers;
    const int slot = compact_slot(__ballot(ev), ne);
    if (ev) je[slot] = k;
    const int last = __shfl(inc, 63, 64);
    carry = last > carry ? last : carry;
  }
  if (lane == 0) n_events[job] = ne;
}

int make_params(const float K1[4], const float K2[4], const float* sigma2_1, const float* sigma2_2,
                int nlevels, RansacParams* P) {
  if (!K1 || !K2 || !sigma2_1 || !sigma2_2)
    return t_s3_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (nlevels < 1 || nlevels > SLAMGPU_MAX_LEVELS)
    return t_s3_err.fail(SLAMGPU_EINVAL, "nlevels %d outside [1, %d]", nlevels, SLAMGPU_MAX_LEVELS);
  for (int i = 0; i < 4; i++) {
    P->K1[i] = K1[i];
    P->K2[i] = K2[i];
  }
  for (int l = 0; l < SLAMGPU_MAX_LEVELS; l++) P->thr1[l] = P->thr2[l] = 0.0f;
  for (int l = 0; l < nlevels; l++) {
    // mvnMaxError* is a std::vector<size_t> (sim3solver.h:74-75): the product is truncated
    const double a = 9.210 * (double)sigma2_1[l], b = 9.210 * (double)sigma2_2[l];
    if (!(a >= 0.0 && a < 1e15 && b >= 0.0 && b < 1e15))
      return t_s3_err.fail(SLAMGPU_EINVAL, "sigma2 of level %d is negative, NaN or too large", l);
    P->thr1[l] = (float)(size_t)a;
    P->thr2[l] = (float)(size_t)b;
  }
  P->nlevels = nlevels;
  return 0;
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

const char* slamgpu_sim3solver_last_error(void) { return t_s3_err.c_str(); }

int slamgpu_sim3_ransac_device(const float K1[4], const float K2[4], const float* sigma2_1,
                               const float* sigma2_2, int nlevels,
                               const slamgpu_sim3_match* d_matches, int n_matches_total,
                               const int32_t* d_draws, int n_draws_total,
                               const slamgpu_sim3_ransac_job* d_jobs, int n_jobs, int max_n,
                               int max_its, slamgpu_sim3_hyp* d_hyp, uint64_t* d_inlier_bits,
                               int32_t* d_events, int32_t* d_n_events, void* stream) {
  RansacParams P;
  if (int r = make_params(K1, K2, sigma2_1, sigma2_2, nlevels, &P)) return r;
  if (n_jobs < 0 || n_matches_total < 0 || n_draws_total < 0)
    return t_s3_err.fail(SLAMGPU_EINVAL, "negative count");
  if (n_jobs == 0) return 0;
  if (n_jobs > 65535) return t_s3_err.fail(SLAMGPU_EINVAL, "n_jobs %d > 65535", n_jobs);
  if (max_its < 1 || max_its > SLAMGPU_SIM3_RANSAC_MAX_ITS)
    return t_s3_err.fail(SLAMGPU_EINVAL, "max_its %d outside [1, SLAMGPU_SIM3_RANSAC_MAX_ITS (%d)]",
                         max_its, SLAMGPU_SIM3_RANSAC_MAX_ITS);
  if (max_n < 1 || max_n > SLAMGPU_SIM3_MAX_MATCHES)
    return t_s3_err.fail(SLAMGPU_ECAP, "max_n %d outside [1, SLAMGPU_SIM3_MAX_MATCHES (%d)]", max_n,
                         SLAMGPU_SIM3_MAX_MATCHES);
  if (!d_jobs || !d_hyp || !d_inlier_bits || !d_events || !d_n_events ||
      (n_matches_total > 0 && !d_matches) || (n_draws_total > 0 && !d_draws))
    return t_s3_err.fail(SLAMGPU_EINVAL, "NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sim3_hyp_kernel, dim3((max_its + kHypWaves - 1) / kHypWaves, n_jobs),
                     dim3(64 * kHypWaves), 0, st, d_matches, n_matches_total, d_draws,
                     n_draws_total, d_jobs, max_n, max_its, P, d_hyp, d_inlier_bits);
  hipLaunchKernelGGL(sim3_event_kernel, dim3(n_jobs), dim3(64), 0, st, d_draws, n_matches_total,
                     n_draws_total, d_jobs, max_n, max_its, d_hyp, d_events, d_n_events);
  HIPCHECK(t_s3_err, hipGetLastError());
  return 0;
}

int slamgpu_sim3_ransac(const float K1[4], const float K2[4], const float* sigma2_1,
                        const float* sigma2_2, int nlevels, const slamgpu_sim3_match* matches,
                        int n, const int32_t* draws, int n_its, int min_inliers, int fix_scale,
                        slamgpu_sim3_hyp* hyp, uint64_t* inlier_bits, int32_t* events,
                        int* n_events) {
  if (!matches || !draws || !hyp || !inlier_bits || !events || !n_events)
    return t_s3_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (n > SLAMGPU_SIM3_MAX_MATCHES)
    return t_s3_err.fail(SLAMGPU_ECAP, "%d matches > SLAMGPU_SIM3_MAX_MATCHES (%d)", n,
                         SLAMGPU_SIM3_MAX_MATCHES);
  if (n < 3) return t_s3_err.fail(SLAMGPU_EINVAL, "%d matches < 3", n);
  if (n_its < 1 || n_its > SLAMGPU_SIM3_RANSAC_MAX_ITS)
    return t_s3_err.fail(SLAMGPU_EINVAL, "n_its %d outside [1, SLAMGPU_SIM3_RANSAC_MAX_ITS (%d)]",
                         n_its, SLAMGPU_SIM3_RANSAC_MAX_ITS);
  if (int r = check_draws<3>(t_s3_err, draws, n_its, n)) return r;
  const size_t words = SLAMGPU_SIM3_MASK_WORDS(n);
  StageLease S(t_s3_err);
  StageLayout L;
  const Sim3RansacLayout l = layout_sim3_ransac(L, n, n_its);
  if (int r = S.reserve(L.size())) return r;
  const slamgpu_sim3_ransac_job job{0, n, 0, n_its, min_inliers, fix_scale ? 1 : 0};
  HIPCHECK(t_s3_err, S.upload(l.matches, matches, (size_t)n * sizeof(slamgpu_sim3_match)));
  HIPCHECK(t_s3_err, S.upload(l.draws, draws, (size_t)n_its * 3 * sizeof(int32_t)));
  HIPCHECK(t_s3_err, S.upload(l.job, &job, sizeof(job)));
  if (int r = slamgpu_sim3_ransac_device(
          K1, K2, sigma2_1, sigma2_2, nlevels, S.at<slamgpu_sim3_match>(l.matches), n,
          S.at<int32_t>(l.draws), 3 * n_its, S.at<slamgpu_sim3_ransac_job>(l.job), 1, n, n_its,
          S.at<slamgpu_sim3_hyp>(l.hyp), S.at<uint64_t>(l.bits), S.at<int32_t>(l.events),
          S.at<int32_t>(l.n_events), S.stream()))
    return r;
  int32_t ne = 0;
  HIPCHECK(t_s3_err, S.download(hyp, l.hyp, (size_t)n_its * sizeof(slamgpu_sim3_hyp)));
  HIPCHECK(t_s3_err, S.download(inlier_bits, l.bits, (size_t)n_its * words * sizeof(uint64_t)));
  HIPCHECK(t_s3_err, S.download(events, l.events, (size_t)n_its * sizeof(int32_t)));
  HIPCHECK(t_s3_err, S.download(&ne, l.n_events, sizeof(ne)));
  HIPCHECK(t_s3_err, hipStreamSynchronize(S.stream()));
  if (ne < 0) return t_s3_err.fail(SLAMGPU_EINVAL, "job rejected on the device");
  *n_events = ne;
  return 0;
}

}  // extern "C"
