// pnp_ransac.hip -- the relocalisation's RANSAC EPnP solver (include/slamgpu_pnpsolver.h): every
// hypothesis of every candidate, Refine() of every running best, and the iterations at which the
// reference's PnPsolver::iterate (src/solvers/pnp_solver.cpp:118-211) would return.
//
//   pnp_hyp_kernel     grid (max_its, jobs), one 64-lane wave per hypothesis. The wave resolves its
//                      four draws (the swap-and-pop of :144-154), runs EPnP on the sample and
//                      strides over the correspondences 64 at a time: the ballot of CheckInliers
//                      is the mask word, its popcount the count.
//   pnp_refine_kernel  grid (max_its, jobs). The wave finds the running best after its iteration
//                      (prefix maximum, strict >, counts >= min_inliers), records it in the
//                      hypothesis row and leaves unless its own iteration is that best; otherwise
//                      it compacts the mask to an index list in LDS, runs EPnP over those
//                      correspondences and CheckInliers over all of them.
//   pnp_event_kernel   one wave per job: ballot compaction of the iterations with
//                      n_k >= min_inliers whose best's refined count is > min_inliers.
//
// EPnP is ONE wave-cooperative routine for both kernels (n = 4 and n = the inlier count), so the
// arithmetic exists once. Sums over correspondences: lane l adds the points l, l + 64, ...
// ascending from 0.0, the 64 partials go through LDS and are added ascending from 0.0. Every SVD
// (3x3 PCA, 3x3 inverse, 12x12 MtM, 6x3 / 6x4 / 6x5 least squares, 3x3 ABt) is the same cyclic
// one-sided Jacobi on a matrix held in LDS. A sweep visits the column pairs in round-robin order;
// the (up to 6) pairs of a round share no column, so a group of 10 lanes takes each: every lane of
// the group forms the pair's three dot products and the rotation, then the rows of A and V are
// dealt over the group. (Measured against one pair at a time, one lane per row, in row-major pair
// order: DESIGN.md.) The small serial parts (L_6x10, the betas, Gauss-Newton, qr_solve) run
// redundantly on every lane.
//
// All three kernels validate the job the same way first (ranges, n, n_its, min_inliers, every
// draw), so an invalid job writes n_events = -1 and nothing else.
//
// Arithmetic: DESIGN.md "RANSAC EPnP solver"; tests/pnpsolver_ref.c restates it on the CPU and
// the two are compared bit for bit. The library is built -ffp-contract=off; nothing here turns
// contraction back on. The SVD is svd_lds of jacobi_svd.h; the draw checks, the swap-and-pop, the
// mask word, the compaction and the best of a wave are ransac_device.h's, as in the other solvers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/slamgpu_pnpsolver.h"
#include "device_math.h"
#include "host_stage.h"
#include "jacobi_svd.h"
#include "ransac_device.h"
#include "stage_layout.h"

namespace slamgpu {
namespace {

constexpr int kSweeps = 15;   // tools/pnp_jacobi_sweeps.py settles after 13, plus two
constexpr int kMtmSums = 78;  // upper triangle of the 12 x 12 MtM

struct PnpParams {
  double fu, fv, uc, vc;
  float thr[SLAMGPU_MAX_LEVELS];  // sigma2[level] * th2 in float (:109)
  int nlevels;
};

// The LDS of one wave.
struct WaveLds {
  double part[kMtmSums * 64];  // partial sums, [entry][lane]
  double tot[kMtmSums];
  double A[144], V[144];       // the matrix under the Jacobi rotations and the rotations' product
  int sel[SLAMGPU_PNP_MAX_MATCHES];
};

__device__ __forceinline__ bool job_ranges_ok(const slamgpu_pnp_ransac_job& J, int n_matches_total,
                                              int n_draws_total, int max_n, int max_its) {
  if (J.n < 4 || J.n > max_n || J.n > SLAMGPU_PNP_MAX_MATCHES) return false;
  if (J.n_its < 1 || J.n_its > max_its) return false;
  if (J.min_inliers < 4) return false;
  if (J.match_begin < 0 || (int64_t)J.match_begin + J.n > (int64_t)n_matches_total) return false;
  if (J.draw_begin < 0 || (int64_t)J.draw_begin + 4 * (int64_t)J.n_its > (int64_t)n_draws_total)
    return false;
  return true;
}

// One wave validates the whole job.
__device__ __forceinline__ bool job_ok(const slamgpu_pnp_ransac_job& J, const int32_t* draws,
                                       int n_matches_total, int n_draws_total, int max_n,
                                       int max_its, int lane) {
  return job_ranges_ok(J, n_matches_total, n_draws_total, max_n, max_its) &&
         draws_ok<4>(draws + J.draw_begin, J.n_its, J.n, lane);
}

// ---- sums over correspondences ---------------------------------------------------------------

// part[e] of every lane -> tot[e] of every lane, the 64 partials added in lane order (not the
// butterfly wave_sum of device_math.h, whose order of additions is another).
template <int K>
__device__ __forceinline__ void ordered_wave_sum(WaveLds& S, const double (&part)[K],
                                                 double (&tot)[K], int lane) {
#pragma unroll
  for (int e = 0; e < K; e++) S.part[e * 64 + lane] = part[e];
  __syncthreads();
  for (int e = lane; e < K; e += 64) {
    double t = 0.0;
    for (int l = 0; l < 64; l++) t += S.part[e * 64 + l];
    S.tot[e] = t;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < K; e++) tot[e] = S.tot[e];
}

// ---- the one SVD: svd_lds of jacobi_svd.h ------------------------------------------------------

// x (N) from the SVD in S.A / S.V / d / ord: least squares, minimum norm when rank-deficient.
template <int M, int N>
__device__ __forceinline__ void svd_backsolve(const WaveLds& S, const double* d, const int* ord,
                                              const double* b, double* x) {
  double sum = 0.0;
  for (int k = 0; k < N; k++) sum += d[k];
  const double thr = 2.0 * 2.220446049250313e-16 * sum;
  for (int i = 0; i < N; i++) x[i] = 0.0;
  for (int k = 0; k < N; k++) {
    if (!(d[k] > thr)) continue;
    const int j = ord[k];
    double ub = 0.0;
    for (int r = 0; r < M; r++) ub += (S.A[r * N + j] / d[k]) * b[r];
    const double w = ub / d[k];
    for (int i = 0; i < N; i++) x[i] += S.V[i * N + j] * w;
  }
}

// Lane 0 places a private matrix in S.A; everyone waits for it.
template <int COUNT>
__device__ __forceinline__ void put_A(WaveLds& S, const double* a, int lane) {
  __syncthreads();  // earlier readers of S.A are done
  if (lane == 0)
    for (int i = 0; i < COUNT; i++) S.A[i] = a[i];
  __syncthreads();
}

// cvSolve(L, Rho, x, CV_SVD) for the 6 x N systems of find_betas_approx_*.
template <int N>
__device__ __forceinline__ void lstsq6(WaveLds& S, int lane, const double* l, const double* rho,
                                       double* x) {
  double d[N];
  int ord[N];
  put_A<6 * N>(S, l, lane);
  svd_lds<6, N, kSweeps>(S, lane, d, ord);
  svd_backsolve<6, N>(S, d, ord, rho, x);
}

// ---- EPnP --------------------------------------------------------------------------------------

struct Epnp {
  const slamgpu_pnp_match* m;
  int n;
  double fu, fv, uc, vc;
  double cws[4][3], ccs[4][3], cc_inv[9];
  double v4[4][12];  // ut rows 11, 10, 9, 8
  double l_6x10[60], rho[6];
};

__device__ __forceinline__ double dot(const double* v1, const double* v2) {
  return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2];
}

__device__ __forceinline__ double dist2(const double* p1, const double* p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) +
         (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

struct Point {
  double w[3], u, v;
};

__device__ __forceinline__ Point point_of(const Epnp& E, const WaveLds& S, int i) {
  const slamgpu_pnp_match c = E.m[S.sel[i]];
  return {{(double)c.xw[0], (double)c.xw[1], (double)c.xw[2]}, (double)c.u, (double)c.v};
}

__device__ __forceinline__ void alphas_of(const Epnp& E, const Point& P, double (&a)[4]) {
  const double* ci = E.cc_inv;
#pragma unroll
  for (int j = 0; j < 3; j++)
    a[1 + j] = ci[3 * j] * (P.w[0] - E.cws[0][0]) + ci[3 * j + 1] * (P.w[1] - E.cws[0][1]) +
               ci[3 * j + 2] * (P.w[2] - E.cws[0][2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

__device__ __forceinline__ void pcs_of(const Epnp& E, const Point& P, bool flip, double (&pc)[3]) {
  double a[4];
  alphas_of(E, P, a);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    pc[j] = a[0] * E.ccs[0][j] + a[1] * E.ccs[1][j] + a[2] * E.ccs[2][j] + a[3] * E.ccs[3][j];
    if (flip) pc[j] = -pc[j];
  }
}

__device__ __noinline__ void choose_control_points(Epnp& E, WaveLds& S, int lane) {
  const int n = E.n;
  double p3[3] = {0.0, 0.0, 0.0}, t3[3];
  for (int i = lane; i < n; i += 64) {
    const Point P = point_of(E, S, i);
#pragma unroll
    for (int j = 0; j < 3; j++) p3[j] += P.w[j];
  }
  ordered_wave_sum<3>(S, p3, t3, lane);
#pragma unroll
  for (int j = 0; j < 3; j++) E.cws[0][j] = t3[j] / n;
  double p6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t6[6];
  for (int i = lane; i < n; i += 64) {
    const Point P = point_of(E, S, i);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = a; b < 3; b++, e++) p6[e] += (P.w[a] - E.cws[0][a]) * (P.w[b] - E.cws[0][b]);
  }
  ordered_wave_sum<6>(S, p6, t6, lane);
  const double pw0tpw0[9] = {t6[0], t6[1], t6[2], t6[1], t6[3], t6[4], t6[2], t6[4], t6[5]};
  double dc[3];
  int ord[3];
  put_A<9>(S, pw0tpw0, lane);
  svd_lds<3, 3, kSweeps>(S, lane, dc, ord);
  for (int i = 1; i < 4; i++) {
    const double k = __builtin_sqrt(dc[i - 1] / n);
    for (int j = 0; j < 3; j++) E.cws[i][j] = E.cws[0][j] + k * S.V[j * 3 + ord[i - 1]];
  }
}

__device__ __noinline__ void compute_cc_inv(Epnp& E, WaveLds& S, int lane) {
  double cc[9], d[3];
  int ord[3];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = E.cws[j][i] - E.cws[0][i];
  put_A<9>(S, cc, lane);
  svd_lds<3, 3, kSweeps>(S, lane, d, ord);
  for (int j = 0; j < 3; j++) {
    double e[3] = {0.0, 0.0, 0.0}, x[3];
    e[j] = 1.0;
    svd_backsolve<3, 3>(S, d, ord, e, x);
    for (int i = 0; i < 3; i++) E.cc_inv[3 * i + j] = x[i];
  }
}

// MtM into S.A, then its eigenvectors: E.v4 = the four of the smallest eigenvalues.
__device__ __noinline__ void compute_mtm_eig(Epnp& E, WaveLds& S, int lane) {
  double part[kMtmSums], tot[kMtmSums];
#pragma unroll
  for (int e = 0; e < kMtmSums; e++) part[e] = 0.0;
  for (int i = lane; i < E.n; i += 64) {
    const Point P = point_of(E, S, i);
    double as[4], M1[12], M2[12];
    alphas_of(E, P, as);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      M1[3 * k] = as[k] * E.fu;
      M1[3 * k + 1] = 0.0;
      M1[3 * k + 2] = as[k] * (E.uc - P.u);
      M2[3 * k] = 0.0;
      M2[3 * k + 1] = as[k] * E.fv;
      M2[3 * k + 2] = as[k] * (E.vc - P.v);
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 12; a++)
#pragma unroll
      for (int b = a; b < 12; b++, e++) {
        part[e] += M1[a] * M1[b];
        part[e] += M2[a] * M2[b];
      }
  }
  ordered_wave_sum<kMtmSums>(S, part, tot, lane);
  // S.tot still holds the 78 sums: entry (a, b), a <= b, is at 12 a - a (a - 1) / 2 + b - a
  for (int t = lane; t < 144; t += 64) {
    int a = t / 12, b = t % 12;
    if (a > b) {
      const int tmp = a;
      a = b;
      b = tmp;
    }
    S.A[t] = S.tot[12 * a - a * (a - 1) / 2 + b - a];
  }
  __syncthreads();
  double d[12];
  int ord[12];
  svd_lds<12, 12, kSweeps>(S, lane, d, ord);
  for (int i = 0; i < 4; i++)
    for (int c = 0; c < 12; c++) E.v4[i][c] = S.V[c * 12 + ord[11 - i]];
}

__device__ __noinline__ void compute_L_6x10_rho(Epnp& E) {
  double dv[4][6][3];
  for (int i = 0; i < 4; i++) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      dv[i][j][0] = E.v4[i][3 * a] - E.v4[i][3 * b];
      dv[i][j][1] = E.v4[i][3 * a + 1] - E.v4[i][3 * b + 1];
      dv[i][j][2] = E.v4[i][3 * a + 2] - E.v4[i][3 * b + 2];
      b++;
      if (b > 3) {
        a++;
        b = a + 1;
      }
    }
  }
  for (int i = 0; i < 6; i++) {
    double* row = E.l_6x10 + 10 * i;
    row[0] = dot(dv[0][i], dv[0][i]);
    row[1] = 2.0 * dot(dv[0][i], dv[1][i]);
    row[2] = dot(dv[1][i], dv[1][i]);
    row[3] = 2.0 * dot(dv[0][i], dv[2][i]);
    row[4] = 2.0 * dot(dv[1][i], dv[2][i]);
    row[5] = dot(dv[2][i], dv[2][i]);
    row[6] = 2.0 * dot(dv[0][i], dv[3][i]);
    row[7] = 2.0 * dot(dv[1][i], dv[3][i]);
    row[8] = 2.0 * dot(dv[2][i], dv[3][i]);
    row[9] = dot(dv[3][i], dv[3][i]);
  }
  E.rho[0] = dist2(E.cws[0], E.cws[1]);
  E.rho[1] = dist2(E.cws[0], E.cws[2]);
  E.rho[2] = dist2(E.cws[0], E.cws[3]);
  E.rho[3] = dist2(E.cws[1], E.cws[2]);
  E.rho[4] = dist2(E.cws[1], E.cws[3]);
  E.rho[5] = dist2(E.cws[2], E.cws[3]);
}

__device__ __noinline__ void find_betas_approx_1(const Epnp& E, WaveLds& S, int lane,
                                                 double* betas) {
  double l[24], b4[4];
  for (int i = 0; i < 6; i++) {
    l[4 * i] = E.l_6x10[10 * i];
    l[4 * i + 1] = E.l_6x10[10 * i + 1];
    l[4 * i + 2] = E.l_6x10[10 * i + 3];
    l[4 * i + 3] = E.l_6x10[10 * i + 6];
  }
  lstsq6<4>(S, lane, l, E.rho, b4);
  if (b4[0] < 0) {
    betas[0] = __builtin_sqrt(-b4[0]);
    betas[1] = -b4[1] / betas[0];
    betas[2] = -b4[2] / betas[0];
    betas[3] = -b4[3] / betas[0];
  } else {
    betas[0] = __builtin_sqrt(b4[0]);
    betas[1] = b4[1] / betas[0];
    betas[2] = b4[2] / betas[0];
    betas[3] = b4[3] / betas[0];
  }
}

__device__ __noinline__ void find_betas_approx_2(const Epnp& E, WaveLds& S, int lane,
                                                 double* betas) {
  double l[18], b3[3];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 3; j++) l[3 * i + j] = E.l_6x10[10 * i + j];
  lstsq6<3>(S, lane, l, E.rho, b3);
  if (b3[0] < 0) {
    betas[0] = __builtin_sqrt(-b3[0]);
    betas[1] = (b3[2] < 0) ? __builtin_sqrt(-b3[2]) : 0.0;
  } else {
    betas[0] = __builtin_sqrt(b3[0]);
    betas[1] = (b3[2] > 0) ? __builtin_sqrt(b3[2]) : 0.0;
  }
  if (b3[1] < 0) betas[0] = -betas[0];
  betas[2] = 0.0;
  betas[3] = 0.0;
}

__device__ __noinline__ void find_betas_approx_3(const Epnp& E, WaveLds& S, int lane,
                                                 double* betas) {
  double l[30], b5[5];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 5; j++) l[5 * i + j] = E.l_6x10[10 * i + j];
  lstsq6<5>(S, lane, l, E.rho, b5);
  if (b5[0] < 0) {
    betas[0] = __builtin_sqrt(-b5[0]);
    betas[1] = (b5[2] < 0) ? __builtin_sqrt(-b5[2]) : 0.0;
  } else {
    betas[0] = __builtin_sqrt(b5[0]);
    betas[1] = (b5[2] > 0) ? __builtin_sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) betas[0] = -betas[0];
  betas[2] = b5[3] / betas[0];
  betas[3] = 0.0;
}

// qr_solve (:813-903) for the 6 x 4 system. On a zero column it returns early and x stays as it
// was. The scan for eta reads A[k][k] twice and never the last row, as the reference's does.
__device__ __forceinline__ void qr_solve(double* pA, double* pb, double* pX) {
  constexpr int nr = 6, nc = 4;
  double A1[6], A2[6];
  for (int k = 0; k < nc; k++) {
    double eta = __builtin_fabs(pA[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {
      const double elt = __builtin_fabs(pA[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) return;
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      pA[i * nc + k] *= inv_eta;
      sum += pA[i * nc + k] * pA[i * nc + k];
    }
    double sigma = __builtin_sqrt(sum);
    if (pA[k * nc + k] < 0) sigma = -sigma;
    pA[k * nc + k] += sigma;
    A1[k] = sigma * pA[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double s2 = 0;
      for (int i = k; i < nr; i++) s2 += pA[i * nc + k] * pA[i * nc + j];
      const double tau = s2 / A1[k];
      for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {
    double tau = 0;
    for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
    tau /= A1[j];
    for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
  }
  pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
    pX[i] = (pb[i] - sum) / A2[i];
  }
}

__device__ __noinline__ void gauss_newton(const Epnp& E, double* betas) {
  double a[24], b[6], x[4] = {0.0, 0.0, 0.0, 0.0};
  const double* rho = E.rho;
#pragma unroll 1
  for (int k = 0; k < 5; k++) {
    for (int i = 0; i < 6; i++) {
      const double* rowL = E.l_6x10 + i * 10;
      double* rowA = a + i * 4;
      rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
      rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
      rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
      rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
      b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] +
                       rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                       rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                       rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                       rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
    }
    qr_solve(a, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// compute_R_and_t (:604-615): ccs, the sign from the first correspondence, estimate_R_and_t and
// the reprojection error. R row-major.
__device__ __noinline__ double compute_R_and_t(Epnp& E, WaveLds& S, int lane, const double* betas,
                                               double* R, double* t) {
  const int n = E.n;
  for (int i = 0; i < 4; i++) E.ccs[i][0] = E.ccs[i][1] = E.ccs[i][2] = 0.0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) E.ccs[j][k] += betas[i] * E.v4[i][3 * j + k];
  double first[3];
  pcs_of(E, point_of(E, S, 0), false, first);
  const bool flip = first[2] < 0.0;
  double p6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t6[6];
  for (int i = lane; i < n; i += 64) {
    const Point P = point_of(E, S, i);
    double pc[3];
    pcs_of(E, P, flip, pc);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      p6[j] += pc[j];
      p6[3 + j] += P.w[j];
    }
  }
  ordered_wave_sum<6>(S, p6, t6, lane);
  double pc0[3], pw0[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    pc0[j] = t6[j] / n;
    pw0[j] = t6[3 + j] / n;
  }
  double p9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, abt[9];
  for (int i = lane; i < n; i += 64) {
    const Point P = point_of(E, S, i);
    double pc[3];
    pcs_of(E, P, flip, pc);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int c = 0; c < 3; c++) p9[3 * j + c] += (pc[j] - pc0[j]) * (P.w[c] - pw0[c]);
  }
  ordered_wave_sum<9>(S, p9, abt, lane);
  double d[3];
  int ord[3];
  put_A<9>(S, abt, lane);
  svd_lds<3, 3, kSweeps>(S, lane, d, ord);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      R[3 * i + j] = (S.A[i * 3 + ord[0]] / d[0]) * S.V[j * 3 + ord[0]] +
                     (S.A[i * 3 + ord[1]] / d[1]) * S.V[j * 3 + ord[1]] +
                     (S.A[i * 3 + ord[2]] / d[2]) * S.V[j * 3 + ord[2]];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] -
                     R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  t[0] = pc0[0] - dot(R, pw0);
  t[1] = pc0[1] - dot(R + 3, pw0);
  t[2] = pc0[2] - dot(R + 6, pw0);
  double p1[1] = {0.0}, t1[1];
  for (int i = lane; i < n; i += 64) {
    const Point P = point_of(E, S, i);
    const double Xc = dot(R, P.w) + t[0];
    const double Yc = dot(R + 3, P.w) + t[1];
    const double inv_Zc = 1.0 / (dot(R + 6, P.w) + t[2]);
    const double ue = E.uc + E.fu * Xc * inv_Zc;
    const double ve = E.vc + E.fv * Yc * inv_Zc;
    p1[0] += __builtin_sqrt((P.u - ue) * (P.u - ue) + (P.v - ve) * (P.v - ve));
  }
  ordered_wave_sum<1>(S, p1, t1, lane);
  return t1[0] / n;
}

// compute_pose (:430-478) over the correspondences m[S.sel[0 .. n)]. Every lane returns the same
// R (row-major) and t.
__device__ __noinline__ void compute_pose(const slamgpu_pnp_match* m, int n, const PnpParams& P,
                                          WaveLds& S, int lane, double* R, double* t) {
  Epnp E;
  E.m = m;
  E.n = n;
  E.fu = P.fu;
  E.fv = P.fv;
  E.uc = P.uc;
  E.vc = P.vc;
  choose_control_points(E, S, lane);
  compute_cc_inv(E, S, lane);
  compute_mtm_eig(E, S, lane);
  compute_L_6x10_rho(E);
  double betas[4], Rs[4][9], ts[4][3], rep_errors[4];
  find_betas_approx_1(E, S, lane, betas);
  gauss_newton(E, betas);
  rep_errors[1] = compute_R_and_t(E, S, lane, betas, Rs[1], ts[1]);
  find_betas_approx_2(E, S, lane, betas);
  gauss_newton(E, betas);
  rep_errors[2] = compute_R_and_t(E, S, lane, betas, Rs[2], ts[2]);
  find_betas_approx_3(E, S, lane, betas);
  gauss_newton(E, betas);
  rep_errors[3] = compute_R_and_t(E, S, lane, betas, Rs[3], ts[3]);
  int N = 1;
  if (rep_errors[2] < rep_errors[1]) N = 2;
  if (rep_errors[3] < rep_errors[N]) N = 3;
  for (int i = 0; i < 9; i++) R[i] = Rs[N][i];
  for (int i = 0; i < 3; i++) t[i] = ts[N][i];
}

// CheckInliers (:261-292) over all n correspondences: the mask words and the count.
__device__ __forceinline__ int check_inliers(const slamgpu_pnp_match* m, int n, int words,
                                             const PnpParams& P, const double* R, const double* t,
                                             int lane, uint64_t* bits) {
  int cnt = 0;
  for (int w = 0; w < words; w++) {
    const int i = w * 64 + lane;
    bool in = false;
    if (i < n) {
      const slamgpu_pnp_match c = m[i];
      const float x = c.xw[0], y = c.xw[1], z = c.xw[2];
      const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
      const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
      const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
      const double ue = P.uc + P.fu * Xc * invZc;
      const double ve = P.vc + P.fv * Yc * invZc;
      const float distX = (float)(c.u - ue);
      const float distY = (float)(c.v - ve);
      const float error2 = distX * distX + distY * distY;
      const int o = c.octave;
      if (o >= 0 && o < P.nlevels) in = error2 < P.thr[o];
    }
    cnt += store_mask_word(in, bits + w, lane);
  }
  return cnt;
}

__device__ __forceinline__ slamgpu_pnp_hyp make_hyp(const double* R, const double* t, int cnt,
                                                    int best) {
  slamgpu_pnp_hyp h;
#pragma unroll
  for (int i = 0; i < 9; i++) h.Rcw[i] = (float)R[i];
#pragma unroll
  for (int i = 0; i < 3; i++) h.tcw[i] = (float)t[i];
  h.n_inliers = cnt;
  h.best = best;
  h.pad[0] = h.pad[1] = 0;
  return h;
}

__global__ __launch_bounds__(64) void pnp_hyp_kernel(
    const slamgpu_pnp_match* __restrict__ matches, int n_matches_total,
    const int32_t* __restrict__ draws, int n_draws_total,
    const slamgpu_pnp_ransac_job* __restrict__ jobs, int max_n, int max_its, PnpParams P,
    slamgpu_pnp_hyp* __restrict__ hyp, uint64_t* __restrict__ inlier_bits) {
  __shared__ WaveLds S;
  const int job = blockIdx.y, k = blockIdx.x, lane = lane_id();
  const slamgpu_pnp_ransac_job J = jobs[job];
  if (!job_ok(J, draws, n_matches_total, n_draws_total, max_n, max_its, lane)) return;
  if (k >= J.n_its) return;
  const int n = J.n;
  const slamgpu_pnp_match* m = matches + J.match_begin;
  if (lane == 0) resolve_sample<4>(draws + J.draw_begin + 4 * k, n, S.sel);  // :144-154
  __syncthreads();
  double R[9], t[3];
  compute_pose(m, 4, P, S, lane, R, t);
  const int words = (max_n + 63) >> 6;
  const size_t row = (size_t)job * max_its + k;
  const int cnt = check_inliers(m, n, words, P, R, t, lane, inlier_bits + row * words);
  if (lane == 0) hyp[row] = make_hyp(R, t, cnt, -1);  // best: pnp_refine_kernel
}

__global__ __launch_bounds__(64) void pnp_refine_kernel(
    const slamgpu_pnp_match* __restrict__ matches, int n_matches_total,
    const int32_t* __restrict__ draws, int n_draws_total,
    const slamgpu_pnp_ransac_job* __restrict__ jobs, int max_n, int max_its, PnpParams P,
    slamgpu_pnp_hyp* hyp, const uint64_t* __restrict__ inlier_bits,
    slamgpu_pnp_hyp* __restrict__ refined, uint64_t* __restrict__ refined_bits) {
  __shared__ WaveLds S;
  const int job = blockIdx.y, k = blockIdx.x, lane = lane_id();
  const slamgpu_pnp_ransac_job J = jobs[job];
  if (!job_ok(J, draws, n_matches_total, n_draws_total, max_n, max_its, lane)) return;
  if (k >= J.n_its) return;
  const int n = J.n, words = (max_n + 63) >> 6;
  const slamgpu_pnp_match* m = matches + J.match_begin;
  slamgpu_pnp_hyp* jh = hyp + (size_t)job * max_its;
  // the running best after iteration k: the first iteration among 0 .. k that holds the largest
  // count, of those with count >= min_inliers
  int bc = -1, bi = -1;
  for (int j = lane; j <= k; j += 64) {
    const int c = jh[j].n_inliers;
    if (c >= J.min_inliers && c > bc) {
      bc = c;
      bi = j;
    }
  }
  wave_first_best(bc, bi);
  const size_t row = (size_t)job * max_its + k;
  if (lane == 0) jh[k].best = bi;
  uint64_t* rb = refined_bits + row * words;
  if (bi != k) {
    for (int w = lane; w < words; w += 64) rb[w] = 0;
    const double zero[9] = {};
    if (lane == 0) refined[row] = make_hyp(zero, zero, -1, -1);
    return;
  }
  // Refine (:213-258): the inliers of the best, in ascending order
  const uint64_t* kb = inlier_bits + row * words;
  int ns = 0;
  for (int w = 0; w < (n + 63) >> 6; w++) {
    const uint64_t mask = kb[w];
    const int slot = compact_slot(mask, ns);
    if (mask >> lane & 1) S.sel[slot] = w * 64 + lane;
  }
  __syncthreads();
  double R[9], t[3];
  compute_pose(m, ns, P, S, lane, R, t);
  const int cnt = check_inliers(m, n, words, P, R, t, lane, rb);
  if (lane == 0) refined[row] = make_hyp(R, t, cnt, k);
}

__global__ __launch_bounds__(64) void pnp_event_kernel(
    const int32_t* __restrict__ draws, int n_matches_total, int n_draws_total,
    const slamgpu_pnp_ransac_job* __restrict__ jobs, int max_n, int max_its,
    const slamgpu_pnp_hyp* __restrict__ hyp, const slamgpu_pnp_hyp* __restrict__ refined,
    int32_t* __restrict__ events, int32_t* __restrict__ n_events) {
  const int job = blockIdx.x, lane = lane_id();
  const slamgpu_pnp_ransac_job J = jobs[job];
  if (!job_ok(J, draws, n_matches_total, n_draws_total, max_n, max_its, lane)) {
    if (lane == 0) n_events[job] = -1;
    return;
  }
  const slamgpu_pnp_hyp* jh = hyp + (size_t)job * max_its;
  const slamgpu_pnp_hyp* jr = refined + (size_t)job * max_its;
  int32_t* je = events + (size_t)job * max_its;
  int ne = 0;
  for (int base = 0; base < J.n_its; base += 64) {
    const int k = base + lane;
    bool ev = false;
    if (k < J.n_its && jh[k].n_inliers >= J.min_inliers) {
      const int b = jh[k].best;  // >= 0: iteration k itself reached min_inliers
      ev = b >= 0 && b <= k && jr[b].n_inliers > J.min_inliers;
    }
    const int slot = compact_slot(__ballot(ev), ne);
    if (ev) je[slot] = k;
  }
  if (lane == 0) n_events[job] = ne;
}

int make_params(const float K[4], const float* sigma2, int nlevels, float th2, PnpParams* P) {
  if (!K || !sigma2) return t_pnp_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (nlevels < 1 || nlevels > SLAMGPU_MAX_LEVELS)
    return t_pnp_err.fail(SLAMGPU_EINVAL, "nlevels %d outside [1, %d]", nlevels,
                          SLAMGPU_MAX_LEVELS);
  P->fu = K[0];
  P->fv = K[1];
  P->uc = K[2];
  P->vc = K[3];
  for (int l = 0; l < SLAMGPU_MAX_LEVELS; l++) P->thr[l] = 0.0f;
  for (int l = 0; l < nlevels; l++) P->thr[l] = sigma2[l] * th2;  // mvMaxError (:109)
  P->nlevels = nlevels;
  return 0;
}

}  // namespace
}  // namespace slamgpu

using namespace slamgpu;

extern "C" {

const char* slamgpu_pnpsolver_last_error(void) { return t_pnp_err.c_str(); }

int slamgpu_pnp_ransac_device(const float K[4], const float* sigma2, int nlevels, float th2,
                              const slamgpu_pnp_match* d_matches, int n_matches_total,
                              const int32_t* d_draws, int n_draws_total,
                              const slamgpu_pnp_ransac_job* d_jobs, int n_jobs, int max_n,
                              int max_its, slamgpu_pnp_hyp* d_hyp, uint64_t* d_inlier_bits,
                              slamgpu_pnp_hyp* d_refined, uint64_t* d_refined_bits,
                              int32_t* d_events, int32_t* d_n_events, void* stream) {
  PnpParams P;
  if (int r = make_params(K, sigma2, nlevels, th2, &P)) return r;
  if (n_jobs < 0 || n_matches_total < 0 || n_draws_total < 0)
    return t_pnp_err.fail(SLAMGPU_EINVAL, "negative count");
  if (n_jobs == 0) return 0;
  if (n_jobs > 65535) return t_pnp_err.fail(SLAMGPU_EINVAL, "n_jobs %d > 65535", n_jobs);
  if (max_its < 1 || max_its > SLAMGPU_PNP_RANSAC_MAX_ITS)
    return t_pnp_err.fail(SLAMGPU_EINVAL, "max_its %d outside [1, SLAMGPU_PNP_RANSAC_MAX_ITS (%d)]",
                          max_its, SLAMGPU_PNP_RANSAC_MAX_ITS);
  if (max_n < 1 || max_n > SLAMGPU_PNP_MAX_MATCHES)
    return t_pnp_err.fail(SLAMGPU_ECAP, "max_n %d outside [1, SLAMGPU_PNP_MAX_MATCHES (%d)]", max_n,
                          SLAMGPU_PNP_MAX_MATCHES);
  if (!d_jobs || !d_hyp || !d_inlier_bits || !d_refined || !d_refined_bits || !d_events ||
      !d_n_events || (n_matches_total > 0 && !d_matches) || (n_draws_total > 0 && !d_draws))
    return t_pnp_err.fail(SLAMGPU_EINVAL, "NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(max_its, n_jobs);
  hipLaunchKernelGGL(pnp_hyp_kernel, grid, dim3(64), 0, st, d_matches, n_matches_total, d_draws,
                     n_draws_total, d_jobs, max_n, max_its, P, d_hyp, d_inlier_bits);
  hipLaunchKernelGGL(pnp_refine_kernel, grid, dim3(64), 0, st, d_matches, n_matches_total, d_draws,
                     n_draws_total, d_jobs, max_n, max_its, P, d_hyp, d_inlier_bits, d_refined,
                     d_refined_bits);
  hipLaunchKernelGGL(pnp_event_kernel, dim3(n_jobs), dim3(64), 0, st, d_draws, n_matches_total,
                     n_draws_total, d_jobs, max_n, max_its, d_hyp, d_refined, d_events, d_n_events);
  HIPCHECK(t_pnp_err, hipGetLastError());
  return 0;
}

int slamgpu_pnp_ransac(const float K[4], const float* sigma2, int nlevels, float th2,
                       const slamgpu_pnp_match* matches, int n, const int32_t* draws, int n_its,
                       int min_inliers, slamgpu_pnp_hyp* hyp, uint64_t* inlier_bits,
                       slamgpu_pnp_hyp* refined, uint64_t* refined_bits, int32_t* events,
                       int* n_events) {
  if (!matches || !draws || !hyp || !inlier_bits || !refined || !refined_bits || !events ||
      !n_events)
    return t_pnp_err.fail(SLAMGPU_EINVAL, "NULL argument");
  if (n > SLAMGPU_PNP_MAX_MATCHES)
    return t_pnp_err.fail(SLAMGPU_ECAP, "%d matches > SLAMGPU_PNP_MAX_MATCHES (%d)", n,
                          SLAMGPU_PNP_MAX_MATCHES);
  if (n < 4) return t_pnp_err.fail(SLAMGPU_EINVAL, "%d matches < 4", n);
  if (n_its < 1 || n_its > SLAMGPU_PNP_RANSAC_MAX_ITS)
    return t_pnp_err.fail(SLAMGPU_EINVAL, "n_its %d outside [1, SLAMGPU_PNP_RANSAC_MAX_ITS (%d)]",
                          n_its, SLAMGPU_PNP_RANSAC_MAX_ITS);
  if (min_inliers < 4) return t_pnp_err.fail(SLAMGPU_EINVAL, "min_inliers %d < 4", min_inliers);
  if (int r = check_draws<4>(t_pnp_err, draws, n_its, n)) return r;
  const size_t words = SLAMGPU_PNP_MASK_WORDS(n);
  StageLease S(t_pnp_err);
  StageLayout L;
  const PnpRansacLayout l = layout_pnp_ransac(L, n, n_its);
  if (int r = S.reserve(L.size())) return r;
  const slamgpu_pnp_ransac_job job{0, n, 0, n_its, min_inliers, 0};
  HIPCHECK(t_pnp_err, S.upload(l.matches, matches, (size_t)n * sizeof(slamgpu_pnp_match)));
  HIPCHECK(t_pnp_err, S.upload(l.draws, draws, (size_t)n_its * 4 * sizeof(int32_t)));
  HIPCHECK(t_pnp_err, S.upload(l.job, &job, sizeof(job)));
  if (int r = slamgpu_pnp_ransac_device(
          K, sigma2, nlevels, th2, S.at<slamgpu_pnp_match>(l.matches), n, S.at<int32_t>(l.draws),
          4 * n_its, S.at<slamgpu_pnp_ransac_job>(l.job), 1, n, n_its,
          S.at<slamgpu_pnp_hyp>(l.hyp), S.at<uint64_t>(l.bits), S.at<slamgpu_pnp_hyp>(l.refined),
          S.at<uint64_t>(l.refined_bits), S.at<int32_t>(l.events), S.at<int32_t>(l.n_events),
          S.stream()))
    return r;
  int32_t ne = 0;
  const size_t rows = (size_t)n_its * sizeof(slamgpu_pnp_hyp);
  const size_t masks = (size_t)n_its * words * sizeof(uint64_t);
  HIPCHECK(t_pnp_err, S.download(hyp, l.hyp, rows));
  HIPCHECK(t_pnp_err, S.download(inlier_bits, l.bits, masks));
  HIPCHECK(t_pnp_err, S.download(refined, l.refined, rows));
  HIPCHECK(t_pnp_err, S.download(refined_bits, l.refined_bits, masks));
  HIPCHECK(t_pnp_err, S.download(events, l.events, (size_t)n_its * sizeof(int32_t)));
  HIPCHECK(t_pnp_err, S.download(&ne, l.n_events, sizeof(ne)));
  HIPCHECK(t_pnp_err, hipStreamSynchronize(S.stream()));
  if (ne < 0) return t_pnp_err.fail(SLAMGPU_EINVAL, "job rejected on the device");
  *n_events = ne;
  return 0;
}

}  // extern "C"
