// init_ransac.hip -- the monocular Initializer (include/slamgpu_initializer.h): every homography
// and fundamental hypothesis of Initializer::Initialize (src/util/initializer.cpp:22-101), the
// choice between the two models and CheckRT of every motion hypothesis of the chosen one.
//
//   init_prep_kernel    one wave per job. Validates the job (ranges, matches12, N >= 8, every
//                       draw), compacts vMatches12 into mvMatches12 (ballot compaction, :35-44)
//                       and runs Normalize (:753-801) of both frames: four lanes carry the four
//                       float sums, each in index order.
//   init_hyp_kernel     grid (max_its, 2 models, jobs), one 64-lane wave per hypothesis. Lane 0
//                       resolves the eight draws (swap-and-pop of :64-76), lanes 0..7 write the
//                       rows of A, the wave runs the 16 x 9 or 8 x 9 SVD cooperatively in LDS and
//                       every lane finishes the 3 x 3 algebra redundantly (rank 2 for F,
//                       denormalisation, H's inverse). The matches are scored 64 at a time: the
//                       lanes compute the terms, which are then added in the reference's order
//                       (lane by lane, image 1 then image 2); the ballot is the mask word.
//   init_select_kernel  one wave per job: the best of each model (prefix maximum, strict >, scores
//                       > 0, NaN never wins), RH, the model, and its 8 (H) or 4 (F) motions.
//   init_check_rt_kernel  grid (8 motions, jobs), 256 lanes, one lane per inlier with its own
//                       4 x 4 SVD. vbGood is built in LDS, nGood counted, and the cosine at rank
//                       min(50, nGood - 1) found by a bitwise search over order-preserving keys.
//
// Every kernel after the first reads the job's status from its result row (same stream), so a
// rejected job writes status = -1 and nothing else.
//
// Arithmetic: DESIGN.md "Monocular Initializer"; tests/initializer_ref.c restates it on the CPU
// and the two are compared bit for bit. Float division and square root are written through double
// (exact: 53 >= 2 * 24 + 2). The library is built -ffp-contract=off; nothing here turns
// contraction back on. The 16 x 9 and 8 x 9 SVDs are svd_lds of jacobi_svd.h, shared with
// pnp_ransac.hip, the 3 x 3 and 4 x 4 ones its one-lane svd_lane, with this solver's own sweep
// count. The draw checks, the swap-and-pop, the mask word, the compaction and the best of a wave
// are ransac_device.h's, as in the other solvers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/slamgpu_initializer.h"
#include "device_math.h"
#include "host_stage.h"
#include "jacobi_svd.h"
#include "ransac_device.h"
#include "stage_layout.h"

namespace slamgpu {
namespace {

constexpr int kSweeps = 10;     // tools/init_jacobi_sweeps.py settles after 8, plus two
constexpr int kRtThreads = 256;
constexpr int kMotions = SLAMGPU_INIT_MAX_MOTIONS;

__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float fsqrt(float a) { return (float)__builtin_sqrt((double)a); }

// ---- the one SVD -------------------------------------------------------------------------------

struct SvdLds {
  double A[144], V[81];
  int idx[8];
};

// cv::SVD::compute of a 3 x 3 CV_32F Mat: w, u, vt as float.
__device__ __noinline__ void svd3(const float* A, float* w, float* u, float* vt) {
  double d[3], vtd[9], utd[9];
  svd_lane<3, kSweeps>(A, d, vtd, utd);
  for (int k = 0; k < 3; k++) {
    w[k] = (float)d[k];
    for (int r = 0; r < 3; r++) {
      vt[3 * k + r] = (float)vtd[3 * k + r];
      u[3 * r + k] = (float)utd[3 * k + r];
    }
  }
}

// ---- cv::Mat arithmetic ------------------------------------------------------------------------

// C (M x N) = A (M x K) B (K x N): double accumulation over ascending k from 0.0, one rounding.
template <int M, int K, int N>
__device__ __forceinline__ void matmul(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double acc = 0.0;
#pragma unroll
      for (int l = 0; l < K; l++) acc += (double)A[i * K + l] * (double)B[l * N + j];
      C[i * N + j] = (float)acc;
    }
}

__device__ __forceinline__ double det3(const float* a) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6],
               a7 = a[7], a8 = a[8];
  return a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6) + a2 * (a3 * a7 - a4 * a6);
}

__device__ __forceinline__ void inv3(const float* a, float* o) {
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

__device__ __forceinline__ void transpose3(const float* a, float* o) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) o[3 * i + j] = a[3 * j + i];
}

// v / cv::norm(v): the norm in double, the reciprocal rounded to float.
__device__ __forceinline__ void normalize3(float* v) {
  const double n = __builtin_sqrt((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1] +
                                  (double)v[2] * (double)v[2]);
  const float s = (float)(1.0 / n);
#pragma unroll
  for (int i = 0; i < 3; i++) v[i] = v[i] * s;
}

__device__ __forceinline__ void k_matrix(const float* K, float* Km) {
  Km[0] = K[0], Km[1] = 0.0f, Km[2] = K[2];
  Km[3] = 0.0f, Km[4] = K[1], Km[5] = K[3];
  Km[6] = 0.0f, Km[7] = 0.0f, Km[8] = 1.0f;
}

__device__ __forceinline__ void t_matrix(const float* nm, float* T) {  // :796-800
  T[0] = nm[2], T[1] = 0.0f, T[2] = -nm[0] * nm[2];
  T[3] = 0.0f, T[4] = nm[3], T[5] = -nm[1] * nm[3];
  T[6] = 0.0f, T[7] = 0.0f, T[8] = 1.0f;
}

// ---- init_prep_kernel --------------------------------------------------------------------------

__device__ __forceinline__ bool job_ranges_ok(const slamgpu_init_job& J, int n_keys1_total,
                                              int n_keys2_total, int n_draws_total, int max_n1,
                                              int max_its) {
  if (J.n1 < 8 || J.n1 > max_n1 || J.n1 > SLAMGPU_INIT_MAX_KEYS) return false;
  if (J.n2 < 1 || J.n2 > SLAMGPU_INIT_MAX_KEYS) return false;
  if (J.n_its < 1 || J.n_its > max_its) return false;
  if (J.key1_begin < 0 || (int64_t)J.key1_begin + J.n1 > (int64_t)n_keys1_total) return false;
  if (J.key2_begin < 0 || (int64_t)J.key2_begin + J.n2 > (int64_t)n_keys2_total) return false;
  if (J.draw_begin < 0 || (int64_t)J.draw_begin + 8 * (int64_t)J.n_its > (int64_t)n_draws_total)
    return false;
  return true;
}

// One of Normalize's float sums over all n keys in index order: coordinate c, about `mean` when
// dev is set (:763-782).
__device__ __forceinline__ float key_sum(const float* keys, int n, int c, bool dev, float mean) {
  float s = 0;
  for (int i = 0; i < n; i++) {
    const float x = keys[2 * i + c];
    s += dev ? __builtin_fabsf(x - mean) : x;
  }
  return s;
}

__global__ __launch_bounds__(64) void init_prep_kernel(
    const float* __restrict__ keys1, const int32_t* __restrict__ matches12, int n_keys1_total,
    const float* __restrict__ keys2, int n_keys2_total, const int32_t* __restrict__ draws,
    int n_draws_total, const slamgpu_init_job* __restrict__ jobs, int max_n1, int max_its,
    slamgpu_init_result* __restrict__ result, int32_t* __restrict__ pairs) {
  const int job = blockIdx.x, lane = lane_id();
  const slamgpu_init_job J = jobs[job];
  slamgpu_init_result* res = result + job;
  if (!job_ranges_ok(J, n_keys1_total, n_keys2_total, n_draws_total, max_n1, max_its)) {
    if (lane == 0) res->status = -1;
    return;
  }
  const int32_t* m12 = matches12 + J.key1_begin;
  int n = 0, bad = 0;
  for (int base = 0; base < J.n1; base += 64) {
    const int i = base + lane;
    const int m = i < J.n1 ? m12[i] : -1;
    bad |= m < -1 || m >= J.n2;
    n += __popcll(__ballot(m >= 0));
  }
  if (n < 8 || __ballot(bad) != 0 || !draws_ok<8>(draws + J.draw_begin, J.n_its, n, lane)) {
    if (lane == 0) res->status = -1;
    return;
  }
  // mvMatches12 (:35-44)
  int32_t* jp = pairs + (size_t)job * max_n1 * 2;
  int c = 0;
  for (int base = 0; base < J.n1; base += 64) {
    const int i = base + lane;
    const int m = i < J.n1 ? m12[i] : -1;
    const int at = compact_slot(__ballot(m >= 0), c);
    if (m >= 0) {
      jp[2 * at] = i;
      jp[2 * at + 1] = m;
    }
  }
  // Normalize: lane = 2 * frame + coordinate
  if (lane < 4) {
    const float* keys =
        lane < 2 ? keys1 + 2 * (size_t)J.key1_begin : keys2 + 2 * (size_t)J.key2_begin;
    const int nk = lane < 2 ? J.n1 : J.n2, co = lane & 1;
    const float mean = fdiv(key_sum(keys, nk, co, false, 0.0f), (float)nk);
    const float meanDev = fdiv(key_sum(keys, nk, co, true, mean), (float)nk);
    res->norm[4 * (lane >> 1) + co] = mean;
    res->norm[4 * (lane >> 1) + 2 + co] = fdiv(1.0f, meanDev);
  }
  if (lane == 0) {
    res->status = 0;
    res->n = n;
    res->pad[0] = res->pad[1] = res->pad[2] = 0;
  }
}

// ---- init_hyp_kernel ---------------------------------------------------------------------------

struct Match {
  float u1, v1, u2, v2;
};

// The two terms of CheckHomography (:336-366) for one match; false = chiSquare > th.
__device__ __forceinline__ void terms_h(const float* H21, const float* H12, const Match& P,
                                        float invSigmaSquare, float& t1, float& t2, bool& in) {
  const float th = 5.991f;
  const float w2in1inv = fdiv(1.0f, H12[6] * P.u2 + H12[7] * P.v2 + H12[8]);
  const float u2in1 = (H12[0] * P.u2 + H12[1] * P.v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * P.u2 + H12[4] * P.v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (P.u1 - u2in1) * (P.u1 - u2in1) + (P.v1 - v2in1) * (P.v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  const float w1in2inv = fdiv(1.0f, H21[6] * P.u1 + H21[7] * P.v1 + H21[8]);
  const float u1in2 = (H21[0] * P.u1 + H21[1] * P.v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * P.u1 + H21[4] * P.v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (P.u2 - u1in2) * (P.u2 - u1in2) + (P.v2 - v1in2) * (P.v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  const bool out1 = chiSquare1 > th, out2 = chiSquare2 > th;
  t1 = out1 ? 0.0f : th - chiSquare1;
  t2 = out2 ? 0.0f : th - chiSquare2;
  in = !out1 && !out2;
}

// The two terms of CheckFundamental (:414-448).
__device__ __forceinline__ void terms_f(const float* F, const Match& P, float invSigmaSquare,
                                        float& t1, float& t2, bool& in) {
  const float th = 3.841f, thScore = 5.991f;
  const float a2 = F[0] * P.u1 + F[1] * P.v1 + F[2];
  const float b2 = F[3] * P.u1 + F[4] * P.v1 + F[5];
  const float c2 = F[6] * P.u1 + F[7] * P.v1 + F[8];
  const float num2 = a2 * P.u2 + b2 * P.v2 + c2;
  const float squareDist1 = fdiv(num2 * num2, a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  const float a1 = F[0] * P.u2 + F[3] * P.v2 + F[6];
  const float b1 = F[1] * P.u2 + F[4] * P.v2 + F[7];
  const float c1 = F[2] * P.u2 + F[5] * P.v2 + F[8];
  const float num1 = a1 * P.u1 + b1 * P.v1 + c1;
  const float squareDist2 = fdiv(num1 * num1, a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  const bool out1 = chiSquare1 > th, out2 = chiSquare2 > th;
  t1 = out1 ? 0.0f : thScore - chiSquare1;
  t2 = out2 ? 0.0f : thScore - chiSquare2;
  in = !out1 && !out2;
}

__global__ __launch_bounds__(64) void init_hyp_kernel(
    const float* __restrict__ keys1, const float* __restrict__ keys2,
    const int32_t* __restrict__ draws, const slamgpu_init_job* __restrict__ jobs, int max_n1,
    int max_its, const slamgpu_init_result* __restrict__ result,
    const int32_t* __restrict__ pairs, slamgpu_init_hyp* __restrict__ hyp,
    uint64_t* __restrict__ bits) {
  __shared__ SvdLds S;
  const int job = blockIdx.z, model = blockIdx.y, k = blockIdx.x, lane = lane_id();
  const slamgpu_init_result* res = result + job;
  if (res->status != 0) return;
  const slamgpu_init_job J = jobs[job];
  if (k >= J.n_its) return;
  const int n = res->n;
  float nm[8];
#pragma unroll
  for (int i = 0; i < 8; i++) nm[i] = res->norm[i];
  const float* k1 = keys1 + 2 * (size_t)J.key1_begin;
  const float* k2 = keys2 + 2 * (size_t)J.key2_begin;
  const int32_t* jp = pairs + (size_t)job * max_n1 * 2;
  if (lane == 0) resolve_sample<8>(draws + J.draw_begin + 8 * k, n, S.idx);  // :64-76
  __syncthreads();
  if (lane < 8) {  // the rows of A (:215-242, :258-274) from the normalised points (:777-793)
    const int a = jp[2 * S.idx[lane]], b = jp[2 * S.idx[lane] + 1];
    const float u1 = (k1[2 * a] - nm[0]) * nm[2], v1 = (k1[2 * a + 1] - nm[1]) * nm[3];
    const float u2 = (k2[2 * b] - nm[4]) * nm[6], v2 = (k2[2 * b + 1] - nm[5]) * nm[7];
    if (model == SLAMGPU_INIT_MODEL_H) {
      double* r0 = S.A + 18 * lane;
      double* r1 = r0 + 9;
      r0[0] = 0.0, r0[1] = 0.0, r0[2] = 0.0, r0[3] = -u1, r0[4] = -v1, r0[5] = -1.0;
      r0[6] = v2 * u1, r0[7] = v2 * v1, r0[8] = v2;
      r1[0] = u1, r1[1] = v1, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0;
      r1[6] = -u2 * u1, r1[7] = -u2 * v1, r1[8] = -u2;
    } else {
      double* r = S.A + 9 * lane;
      r[0] = u2 * u1, r[1] = u2 * v1, r[2] = u2, r[3] = v2 * u1, r[4] = v2 * v1, r[5] = v2;
      r[6] = u1, r[7] = v1, r[8] = 1.0;
    }
  }
  __syncthreads();
  double d[9];
  int ord[9];
  if (model == SLAMGPU_INIT_MODEL_H)
    svd_lds<16, 9, kSweeps>(S, lane, d, ord);
  else
    svd_lds<8, 9, kSweeps>(S, lane, d, ord);
  float Mn[9], T1[9], T2[9], tmp[9], M[9], Minv[9];
#pragma unroll
  for (int c = 0; c < 9; c++) Mn[c] = (float)S.V[c * 9 + ord[8]];  // vt.row(8)
  t_matrix(nm, T1);
  t_matrix(nm + 4, T2);
  if (model == SLAMGPU_INIT_MODEL_H) {
    float T2inv[9];
    inv3(T2, T2inv);  // :114
    matmul<3, 3, 3>(T2inv, Mn, tmp);
    matmul<3, 3, 3>(tmp, T1, M);  // :140
    inv3(M, Minv);                // :141
  } else {
    float w[3], u[9], vt[9], uw[9], T2t[9];
    svd3(Mn, w, u, vt);
    const float D[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, 0.0f};  // w[2] = 0 (:284)
    matmul<3, 3, 3>(u, D, uw);
    matmul<3, 3, 3>(uw, vt, Mn);
    transpose3(T2, T2t);  // :167
    matmul<3, 3, 3>(T2t, Mn, tmp);
    matmul<3, 3, 3>(tmp, T1, M);  // :194
  }
  const float invSigmaSquare = fdiv(1.0f, J.sigma * J.sigma);
  const int words = SLAMGPU_INIT_MASK_WORDS(max_n1);
  const size_t row = ((size_t)job * 2 + model) * max_its + k;
  uint64_t* hb = bits + row * words;
  float score = 0;
  for (int w = 0; w < words; w++) {
    const int i = w * 64 + lane;
    float t1 = 0.0f, t2 = 0.0f;
    bool in = false;
    if (i < n) {
      const int a = jp[2 * i], b = jp[2 * i + 1];
      const Match P = {k1[2 * a], k1[2 * a + 1], k2[2 * b], k2[2 * b + 1]};
      if (model == SLAMGPU_INIT_MODEL_H)
        terms_h(M, Minv, P, invSigmaSquare, t1, t2, in);
      else
        terms_f(M, P, invSigmaSquare, t1, t2, in);
    }
    store_mask_word(in, hb + w, lane);
    // score += th - chi in match order, image 1 then image 2. A term that the reference skips is
    // +0 here: the score is never -0, so adding it changes nothing.
    if (w * 64 < n) {
#pragma unroll 8
      for (int l = 0; l < 64; l++) {
        score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t1), l));
        score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t2), l));
      }
    }
  }
  if (lane == 0) {
    slamgpu_init_hyp h;
#pragma unroll
    for (int c = 0; c < 9; c++) h.M[c] = M[c];
    h.score = score;
    h.pad[0] = h.pad[1] = 0;
    hyp[row] = h;
  }
}

// ---- init_select_kernel ------------------------------------------------------------------------

// DecomposeE (:924-944). The left singular vectors of E are the right ones of E^T; v_k =
// E^T u_k / d_k for k = 0, 1 and v_2 = v_0 x v_1 (at rank 2 the third column of A V is noise).
__device__ __forceinline__ void decompose_e(const float* E, float* R1, float* R2, float* t) {
  float Et[9], u[9], vt[9], tmp[9];
  double d[3], vtd[9], utd[9], v[3][3];
  transpose3(E, Et);
  svd_lane<3, kSweeps>(Et, d, vtd, utd);
  for (int k = 0; k < 2; k++)
    for (int r = 0; r < 3; r++) v[k][r] = utd[3 * k + r];
  v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1];
  v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2];
  v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
  for (int k = 0; k < 3; k++)
    for (int r = 0; r < 3; r++) {
      u[3 * r + k] = (float)vtd[3 * k + r];
      vt[3 * k + r] = (float)v[k][r];
    }
  t[0] = u[2], t[1] = u[5], t[2] = u[8];
  normalize3(t);
  const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float Wt[9];
  transpose3(W, Wt);
  matmul<3, 3, 3>(u, W, tmp);
  matmul<3, 3, 3>(tmp, vt, R1);
  if (det3(R1) < 0)
    for (int i = 0; i < 9; i++) R1[i] = -R1[i];
  matmul<3, 3, 3>(u, Wt, tmp);
  matmul<3, 3, 3>(tmp, vt, R2);
  if (det3(R2) < 0)
    for (int i = 0; i < 9; i++) R2[i] = -R2[i];
}

__device__ __forceinline__ slamgpu_init_motion make_motion(const float* R, const float* t,
                                                           bool negate_t) {
  slamgpu_init_motion m;
  for (int i = 0; i < 9; i++) m.R[i] = R[i];
  for (int i = 0; i < 3; i++) m.t[i] = negate_t ? -t[i] : t[i];
  m.n_good = 0;
  m.cos_parallax = 0.0f;
  m.pad[0] = m.pad[1] = 0;
  return m;
}

// The four motions of ReconstructF (:475-493).
__device__ __noinline__ int motions_f(const float* F21, const float* K, slamgpu_init_motion* m) {
  float Km[9], Kt[9], tmp[9], E[9], R1[9], R2[9], t[3];
  k_matrix(K, Km);
  transpose3(Km, Kt);
  matmul<3, 3, 3>(Kt, F21, tmp);
  matmul<3, 3, 3>(tmp, Km, E);
  decompose_e(E, R1, R2, t);
  for (int i = 0; i < 4; i++) m[i] = make_motion(i & 1 ? R2 : R1, t, (i & 2) != 0);
  return 4;
}

// The eight motions of ReconstructH (:588-690), or 0 for the early return of :601.
__device__ __noinline__ int motions_h(const float* H21, const float* K, slamgpu_init_motion* m) {
  float Km[9], invK[9], tmp[9], A[9], w[3], U[9], Vt[9];
  k_matrix(K, Km);
  inv3(Km, invK);
  matmul<3, 3, 3>(invK, H21, tmp);
  matmul<3, 3, 3>(tmp, Km, A);
  svd3(A, w, U, Vt);
  const float s = (float)(det3(U) * det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)fdiv(d1, d2) < 1.00001 || (double)fdiv(d2, d3) < 1.00001) return 0;
  const float aux1 = fsqrt(fdiv(d1 * d1 - d2 * d2, d1 * d1 - d3 * d3));
  const float aux3 = fsqrt(fdiv(d2 * d2 - d3 * d3, d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = fdiv(fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 + d3) * d2);
  const float ctheta = fdiv(d2 * d2 + d1 * d3, (d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = fdiv(fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 - d3) * d2);
  const float cphi = fdiv(d1 * d3 - d2 * d2, (d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  float sU[9];
  for (int i = 0; i < 9; i++) sU[i] = s * U[i];
#pragma unroll 1
  for (int i = 0; i < 8; i++) {
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tp[3], R[9], t[3];
    if (i < 4) {
      Rp[0] = ctheta, Rp[2] = -stheta[i], Rp[6] = stheta[i], Rp[8] = ctheta;
      tp[0] = x1[i], tp[1] = 0.0f, tp[2] = -x3[i];
      for (int j = 0; j < 3; j++) tp[j] = tp[j] * (d1 - d3);
    } else {
      Rp[0] = cphi, Rp[2] = sphi[i - 4], Rp[4] = -1.0f, Rp[6] = sphi[i - 4], Rp[8] = -cphi;
      tp[0] = x1[i - 4], tp[1] = 0.0f, tp[2] = x3[i - 4];
      for (int j = 0; j < 3; j++) tp[j] = tp[j] * (d1 + d3);
    }
    matmul<3, 3, 3>(sU, Rp, tmp);
    matmul<3, 3, 3>(tmp, Vt, R);
    matmul<3, 3, 1>(U, tp, t);
    normalize3(t);
    m[i] = make_motion(R, t, false);
  }
  return 8;
}

__global__ __launch_bounds__(64) void init_select_kernel(
    const slamgpu_init_job* __restrict__ jobs, int max_its,
    slamgpu_init_result* __restrict__ result, const slamgpu_init_hyp* __restrict__ hyp,
    slamgpu_init_motion* __restrict__ motion) {
  const int job = blockIdx.x, lane = lane_id();
  slamgpu_init_result* res = result + job;
  if (res->status != 0) return;
  const slamgpu_init_job J = jobs[job];
  float S[2];
  int best[2];
  for (int model = 0; model < 2; model++) {
    const slamgpu_init_hyp* jh = hyp + ((size_t)job * 2 + model) * max_its;
    float bs = 0.0f;  // score = 0.0 (:117, :170): only a greater score wins, a NaN never does
    int bi = -1;
    for (int k = lane; k < J.n_its; k += 64) {
      const float s = jh[k].score;
      if (s > bs) {
        bs = s;
        bi = k;
      }
    }
    wave_first_best(bs, bi);
    S[model] = bs;
    best[model] = bi;
  }
  const float RH = fdiv(S[0], S[0] + S[1]);  // :92
  const int model = (double)RH > 0.40 ? SLAMGPU_INIT_MODEL_H : SLAMGPU_INIT_MODEL_F;
  int n_motions = 0;
  if (lane == 0) {
    if (best[model] >= 0) {
      const slamgpu_init_hyp h = hyp[((size_t)job * 2 + model) * max_its + best[model]];
      slamgpu_init_motion* jm = motion + (size_t)job * kMotions;
      n_motions = model == SLAMGPU_INIT_MODEL_H ? motions_h(h.M, J.K, jm) : motions_f(h.M, J.K, jm);
    }
    res->best[0] = best[0];
    res->best[1] = best[1];
    res->SH = S[0];
    res->SF = S[1];
    res->RH = RH;
    res->model = model;
    res->n_motions = n_motions;
  }
}

// ---- init_check_rt_kernel ----------------------------------------------------------------------

// Ascending keys = ascending cosines, NaN last.
__device__ __forceinline__ uint32_t cos_key(float c) {
  if (c != c) return 0xFFFFFFFFu;
  const uint32_t b = (uint32_t)__float_as_int(c);
  return b & 0x80000000u ? ~b : b | 0x80000000u;
}

__device__ __forceinline__ float key_cos(uint32_t k) {
  if (k == 0xFFFFFFFFu) return __int_as_float(0x7FC00000);
  return __int_as_float((int)(k & 0x80000000u ? k & 0x7FFFFFFFu : ~k));
}

// Triangulate (:738-751).
__device__ __noinline__ void triangulate(const float* kp1, const float* kp2, const float* P1,
                                         const float* P2, float* x3D) {
  float A[16];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    A[c] = kp1[0] * P1[8 + c] - P1[c];
    A[4 + c] = kp1[1] * P1[8 + c] - P1[4 + c];
    A[8 + c] = kp2[0] * P2[8 + c] - P2[c];
    A[12 + c] = kp2[1] * P2[8 + c] - P2[4 + c];
  }
  double d[4], vt[16], ut[16];
  svd_lane<4, kSweeps>(A, d, vt, ut);
  const float x[4] = {(float)vt[12], (float)vt[13], (float)vt[14], (float)vt[15]};
  const float s = (float)(1.0 / (double)x[3]);
#pragma unroll
  for (int i = 0; i < 3; i++) x3D[i] = x[i] * s;
}

__device__ __forceinline__ bool finite_f(float x) {
  return (__float_as_int(x) & 0x7F800000) != 0x7F800000;
}

struct RtLds {
  uint32_t keys[SLAMGPU_INIT_MAX_KEYS];
  unsigned long long good[SLAMGPU_INIT_MASK_WORDS(SLAMGPU_INIT_MAX_KEYS)];
  int n_good;
  int below[32];
};

__global__ __launch_bounds__(kRtThreads) void init_check_rt_kernel(
    const float* __restrict__ keys1, const int32_t* __restrict__ matches12,
    const float* __restrict__ keys2, const slamgpu_init_job* __restrict__ jobs, int max_n1,
    int max_its, const slamgpu_init_result* __restrict__ result, const int32_t* __restrict__ pairs,
    const uint64_t* __restrict__ bits, slamgpu_init_motion* __restrict__ motion,
    uint64_t* __restrict__ good_bits, float* __restrict__ p3d) {
  __shared__ RtLds S;
  const int job = blockIdx.y, mi = blockIdx.x, tid = threadIdx.x;
  const slamgpu_init_result* res = result + job;
  if (res->status != 0 || mi >= res->n_motions) return;
  const slamgpu_init_job J = jobs[job];
  const int n = res->n, n1 = J.n1, words = SLAMGPU_INIT_MASK_WORDS(max_n1);
  const float* k1 = keys1 + 2 * (size_t)J.key1_begin;
  const float* k2 = keys2 + 2 * (size_t)J.key2_begin;
  const int32_t* m12 = matches12 + J.key1_begin;
  const int32_t* jp = pairs + (size_t)job * max_n1 * 2;
  const uint64_t* hb =
      bits + (((size_t)job * 2 + res->model) * max_its + res->best[res->model]) * words;
  slamgpu_init_motion* mo = motion + (size_t)job * kMotions + mi;
  float* p3 = p3d + ((size_t)job * kMotions + mi) * max_n1 * 3;
  for (int w = tid; w < words; w += kRtThreads) S.good[w] = 0;
  if (tid < 32) S.below[tid] = 0;
  if (tid == 0) S.n_good = 0;
  __syncthreads();
  float R[9], t[3], Km[9], P1[12], Rt[12], P2[12], Rtn[9], O2[3];
  for (int i = 0; i < 9; i++) R[i] = mo->R[i];
  for (int i = 0; i < 3; i++) t[i] = mo->t[i];
  const float fx = J.K[0], fy = J.K[1], cx = J.K[2], cy = J.K[3];
  k_matrix(J.K, Km);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      P1[4 * i + j] = Km[3 * i + j];
      Rt[4 * i + j] = R[3 * i + j];
      Rtn[3 * i + j] = -R[3 * j + i];
    }
    P1[4 * i + 3] = 0.0f;
    Rt[4 * i + 3] = t[i];
  }
  matmul<3, 3, 4>(Km, Rt, P2);   // :838
  matmul<3, 3, 1>(Rtn, t, O2);   // :840
  const float th2 = 4.0f * (J.sigma * J.sigma);  // :490, :707
  // vP3D of the keys without a match; the matched ones are written below, each by its own lane
  for (int i = tid; i < n1; i += kRtThreads)
    if (m12[i] < 0) p3[3 * i] = p3[3 * i + 1] = p3[3 * i + 2] = 0.0f;
  for (int i = tid; i < n; i += kRtThreads) {
    const int i1 = jp[2 * i];
    float p[3] = {0.0f, 0.0f, 0.0f};
    bool good = false;
    float cosParallax = 0.0f;
    if (hb[i >> 6] >> (i & 63) & 1) {
      const float kp1[2] = {k1[2 * i1], k1[2 * i1 + 1]};
      const float kp2[2] = {k2[2 * jp[2 * i + 1]], k2[2 * jp[2 * i + 1] + 1]};
      float p2[3];
      triangulate(kp1, kp2, P1, P2, p);
      good = finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]);
      if (good) {
        const float dist1 = (float)__builtin_sqrt((double)p[0] * (double)p[0] +
                                                  (double)p[1] * (double)p[1] +
                                                  (double)p[2] * (double)p[2]);
        const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};
        const float dist2 = (float)__builtin_sqrt((double)n2[0] * (double)n2[0] +
                                                  (double)n2[1] * (double)n2[1] +
                                                  (double)n2[2] * (double)n2[2]);
        const double dot = (double)p[0] * (double)n2[0] + (double)p[1] * (double)n2[1] +
                           (double)p[2] * (double)n2[2];
        cosParallax = (float)(dot / (double)(dist1 * dist2));
        const bool low = (double)cosParallax < 0.99998;
        if (p[2] <= 0 && low) good = false;
        matmul<3, 3, 1>(R, p, p2);  // :876
        for (int j = 0; j < 3; j++) p2[j] = p2[j] + t[j];
        if (p2[2] <= 0 && low) good = false;
        const float invZ1 = fdiv(1.0f, p[2]);
        const float im1x = fx * p[0] * invZ1 + cx;
        const float im1y = fy * p[1] * invZ1 + cy;
        const float squareError1 =
            (im1x - kp1[0]) * (im1x - kp1[0]) + (im1y - kp1[1]) * (im1y - kp1[1]);
        if (squareError1 > th2) good = false;
        const float invZ2 = fdiv(1.0f, p2[2]);
        const float im2x = fx * p2[0] * invZ2 + cx;
        const float im2y = fy * p2[1] * invZ2 + cy;
        const float squareError2 =
            (im2x - kp2[0]) * (im2x - kp2[0]) + (im2y - kp2[1]) * (im2y - kp2[1]);
        if (squareError2 > th2) good = false;
      }
    }
    if (good) {
      S.keys[atomicAdd(&S.n_good, 1)] = cos_key(cosParallax);
      if ((double)cosParallax < 0.99998) atomicOr(&S.good[i1 >> 6], 1ull << (i1 & 63));
    }
    p3[3 * i1] = good ? p[0] : 0.0f;
    p3[3 * i1 + 1] = good ? p[1] : 0.0f;
    p3[3 * i1 + 2] = good ? p[2] : 0.0f;
  }
  __syncthreads();
  const int nGood = S.n_good;
  for (int w = tid; w < words; w += kRtThreads) {
    good_bits[((size_t)job * kMotions + mi) * words + w] = S.good[w];
  }
  // the key at rank idx of the ascending keys: the greatest K with #(key < K) <= idx
  uint32_t key = 0;
  if (nGood > 0) {
    const int idx = nGood - 1 < 50 ? nGood - 1 : 50;
    for (int b = 31; b >= 0; b--) {
      const uint32_t trial = key | (1u << b);
      int c = 0;
      for (int i = tid; i < nGood; i += kRtThreads) c += S.keys[i] < trial;
      if (c) atomicAdd(&S.below[b], c);
      __syncthreads();
      if (S.below[b] <= idx) key = trial;
    }
  }
  if (tid == 0) {
    mo->n_good = nGood;
    mo->cos_parallax = nGood > 0 ? key_cos(key) : 0.0f;
  }
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

const char* slamgpu_initializer_last_error(void) { return t_init_err.c_str(); }

int slamgpu_init_ransac_device(const float* d_keys1, const int32_t* d_matches12, int n_keys1_total,
                               const float* d_keys2, int n_keys2_total, const int32_t* d_draws,
                               int n_draws_total, const slamgpu_init_job* d_jobs, int n_jobs,
                               int max_n1, int max_its, slamgpu_init_hyp* d_hyp, uint64_t* d_bits,
                               slamgpu_init_result* d_result, int32_t* d_pairs,
                               slamgpu_init_motion* d_motion, uint64_t* d_good_bits, float* d_p3d,
                               void* stream) {
  if (n_jobs < 0 || n_keys1_total < 0 || n_keys2_total < 0 || n_draws_total < 0)
    return t_init_err.fail(SLAMGPU_EINVAL, "negative count");
  if (n_jobs == 0) return 0;
  if (n_jobs > 65535) return t_init_err.fail(SLAMGPU_EINVAL, "n_jobs %d > 65535", n_jobs);
  if (max_its < 1 || max_its > SLAMGPU_INIT_MAX_ITS)
    return t_init_err.fail(SLAMGPU_EINVAL, "max_its %d outside [1, SLAMGPU_INIT_MAX_ITS (%d)]",
                           max_its, SLAMGPU_INIT_MAX_ITS);
  if (max_n1 < 1 || max_n1 > SLAMGPU_INIT_MAX_KEYS)
    return t_init_err.fail(SLAMGPU_ECAP, "max_n1 %d outside [1, SLAMGPU_INIT_MAX_KEYS (%d)]",
                           max_n1, SLAMGPU_INIT_MAX_KEYS);
  if (!d_jobs || !d_hyp || !d_bits || !d_result || !d_pairs || !d_motion || !d_good_bits ||
      !d_p3d || (n_keys1_total > 0 && (!d_keys1 || !d_matches12)) ||
      (n_keys2_total > 0 && !d_keys2) || (n_draws_total > 0 && !d_draws))
    return t_init_err.fail(SLAMGPU_EINVAL, "NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(init_prep_kernel, dim3(n_jobs), dim3(64), 0, st, d_keys1, d_matches12,
                     n_keys1_total, d_keys2, n_keys2_total, d_draws, n_draws_total, d_jobs, max_n1,
                     max_its, d_result, d_pairs);
  hipLaunchKernelGGL(init_hyp_kernel, dim3(max_its, 2, n_jobs), dim3(64), 0, st, d_keys1, d_keys2,
                     d_draws, d_jobs, max_n1, max_its, d_result, d_pairs, d_hyp, d_bits);
  hipLaunchKernelGGL(init_select_kernel, dim3(n_jobs), dim3(64), 0, st, d_jobs, max_its, d_result,
                     d_hyp, d_motion);
  hipLaunchKernelGGL(init_check_rt_kernel, dim3(kMotions, n_jobs), dim3(kRtThreads), 0, st, d_keys1,
                     d_matches12, d_keys2, d_jobs, max_n1, max_its, d_result, d_pairs, d_bits,
                     d_motion, d_good_bits, d_p3d);
  HIPCHECK(t_init_err, hipGetLastError());
  return 0;
}

int slamgpu_init_ransac(const float* keys1, const int32_t* matches12, int n1, const float* keys2,
                        int n2, const float K[4], float sigma, const int32_t* draws, int n_its,
                        slamgpu_init_hyp* hyp, uint64_t* bits, slamgpu_init_result* result,
                        int32_t* pairs, slamgpu_init_motion* motion, uint64_t* good_bits,
                        float* p3d) {
  if (!keys1 || !matches12 || !keys2 || !K || !draws || !hyp || !bits || !result || !pairs ||
      !motion || !good_bits || !p3d)
    return t_init_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (n1 > SLAMGPU_INIT_MAX_KEYS || n2 > SLAMGPU_INIT_MAX_KEYS)
    return t_init_err.fail(SLAMGPU_ECAP, "%d / %d keys > SLAMGPU_INIT_MAX_KEYS (%d)", n1, n2,
                           SLAMGPU_INIT_MAX_KEYS);
  if (n1 < 8 || n2 < 1) return t_init_err.fail(SLAMGPU_EINVAL, "%d / %d keys: too few", n1, n2);
  if (n_its < 1 || n_its > SLAMGPU_INIT_MAX_ITS)
    return t_init_err.fail(SLAMGPU_EINVAL, "n_its %d outside [1, SLAMGPU_INIT_MAX_ITS (%d)]", n_its,
                           SLAMGPU_INIT_MAX_ITS);
  int n = 0;
  for (int i = 0; i < n1; i++) {
    if (matches12[i] < -1 || matches12[i] >= n2)
      return t_init_err.fail(SLAMGPU_EINVAL, "matches12[%d] = %d outside [-1, %d)", i, matches12[i],
                             n2);
    n += matches12[i] >= 0;
  }
  if (n < 8) return t_init_err.fail(SLAMGPU_EINVAL, "%d matches < 8", n);
  if (int r = check_draws<8>(t_init_err, draws, n_its, n)) return r;
  const size_t words = SLAMGPU_INIT_MASK_WORDS(n1);
  StageLease S(t_init_err);
  StageLayout L;
  const InitRansacLayout l = layout_init_ransac(L, n1, n2, n_its);
  if (int r = S.reserve(L.size())) return r;
  const slamgpu_init_job job{0, n1, 0, n2, 0, n_its, {K[0], K[1], K[2], K[3]}, sigma, 0};
  HIPCHECK(t_init_err, S.upload(l.keys1, keys1, (size_t)n1 * 2 * sizeof(float)));
  HIPCHECK(t_init_err, S.upload(l.matches12, matches12, (size_t)n1 * sizeof(int32_t)));
  HIPCHECK(t_init_err, S.upload(l.keys2, keys2, (size_t)n2 * 2 * sizeof(float)));
  HIPCHECK(t_init_err, S.upload(l.draws, draws, (size_t)n_its * 8 * sizeof(int32_t)));
  HIPCHECK(t_init_err, S.upload(l.job, &job, sizeof(job)));
  if (int r = slamgpu_init_ransac_device(
          S.at<float>(l.keys1), S.at<int32_t>(l.matches12), n1, S.at<float>(l.keys2), n2,
          S.at<int32_t>(l.draws), 8 * n_its, S.at<slamgpu_init_job>(l.job), 1, n1, n_its,
          S.at<slamgpu_init_hyp>(l.hyp), S.at<uint64_t>(l.bits),
          S.at<slamgpu_init_result>(l.result), S.at<int32_t>(l.pairs),
          S.at<slamgpu_init_motion>(l.motion), S.at<uint64_t>(l.good_bits), S.at<float>(l.p3d),
          S.stream()))
    return r;
  slamgpu_init_result res;
  HIPCHECK(t_init_err, S.download(&res, l.result, sizeof(res)));
  HIPCHECK(t_init_err, hipStreamSynchronize(S.stream()));
  if (res.status != 0) return t_init_err.fail(SLAMGPU_EINVAL, "job rejected on the device");
  const size_t nm = (size_t)res.n_motions;
  HIPCHECK(t_init_err, S.download(hyp, l.hyp, (size_t)2 * n_its * sizeof(slamgpu_init_hyp)));
  HIPCHECK(t_init_err, S.download(bits, l.bits, (size_t)2 * n_its * words * sizeof(uint64_t)));
  HIPCHECK(t_init_err, S.download(pairs, l.pairs, (size_t)res.n * 2 * sizeof(int32_t)));
  HIPCHECK(t_init_err, S.download(motion, l.motion, nm * sizeof(slamgpu_init_motion)));
  HIPCHECK(t_init_err, S.download(good_bits, l.good_bits, nm * words * sizeof(uint64_t)));
  HIPCHECK(t_init_err, S.download(p3d, l.p3d, nm * (size_t)n1 * 3 * sizeof(float)));
  HIPCHECK(t_init_err, hipStreamSynchronize(S.stream()));
  *result = res;
  return 0;
}

}  // extern "C"
