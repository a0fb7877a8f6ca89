/* initializer_ref.c -- CPU restatement of the monocular Initializer (include/slamgpu_initializer.h,
 * csrc/init_ransac.hip): the contract the device is compared against bit for bit. It follows the
 * reference's Initializer (src/util/initializer.cpp) function by function; the line numbers in
 * the comments are that file's. What the reference leaves to OpenCV is stated here (DESIGN.md
 * "Monocular Initializer"):
 *   - data is float (CV_32F). A single + - * / sqrt of float operands that the reference evaluates
 *     in double and rounds to float IS the float operation (53 >= 2 * 24 + 2), so 1.0 / x,
 *     4.0 * mSigma2, sqrt(x) and the like are written as float operations;
 *   - every cv::SVDecomp / cv::SVD::compute is ONE routine, the cyclic one-sided Jacobi of the
 *     EPnP solver's "Linear algebra contract" in FP64 on the float entries widened to double,
 *     with a fixed sweep count; results are rounded to float once. Null vectors are columns of V;
 *   - DecomposeE needs a LEFT null vector: the routine runs on E^T, so that U of E is its V;
 *     v_k = E^T u_k / d_k for k = 0, 1 and v_2 = v_0 x v_1;
 *   - a cv::Mat product accumulates in double over ascending k from 0.0 and rounds to float once
 *     per product; a chain is evaluated left to right. 3 x 3 inv() and determinant are the closed
 *     (cofactor) form in double, rounded once. Mat / s multiplies by (float)(1.0 / s); cv::norm
 *     and Mat::dot accumulate in double;
 *   - comparisons against double literals (RH > 0.40, cosParallax < 0.99998, d1 / d2 < 1.00001)
 *     widen the float, as C++ does.
 * Built with the oracle Makefile's CFLAGS (-ffp-contract=off): no fused multiply-add anywhere.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define INIT_SWEEPS 10 /* tools/init_jacobi_sweeps.py settles after 8, plus two */
#define INIT_MAX_KEYS 8192
#define INIT_MAX_ITS 512
#define INIT_MAX_MOTIONS 8

typedef struct {
  float M[9]; /* H21i / F21i, row-major */
  float score;
  int32_t pad[2];
} init_hyp;

typedef struct {
  int32_t status, n; /* 0 / -1; N = mvMatches12.size() */
  int32_t best[2];   /* H, F: the winning iteration or -1 */
  float SH, SF, RH;
  int32_t model, n_motions; /* 0 = H (RH > 0.40), 1 = F */
  float norm[8];            /* meanX, meanY, sX, sY of frame 1, then of frame 2 */
  int32_t pad[3];
} init_result;

typedef struct {
  float R[9], t[3];
  int32_t n_good;
  float cos_parallax; /* the cosine at rank min(50, nGood - 1), 0 when nGood = 0 */
  int32_t pad[2];
} init_motion;

int init_jacobi_sweeps(void) { return INIT_SWEEPS; }

/* ---- the one SVD (tests/pnpsolver_ref.c: jacobi_columns, svd) ------------------------------ */

static void jacobi_columns(double* A, int m, int n, double* V, int sweeps) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  const int np = n + (n & 1);
  for (int sw = 0; sw < sweeps; sw++)
    for (int round = 0; round < np - 1; round++)
      for (int i = 0; i < np / 2; i++) {
        const int a = i == 0 ? np - 1 : (round + i) % (np - 1);
        const int b = i == 0 ? round : (round - i + np - 1) % (np - 1);
        if (a >= n || b >= n) continue; /* the bye */
        const int p = a < b ? a : b, q = a < b ? b : a;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < m; r++) {
          const double ap = A[r * n + p], aq = A[r * n + q];
          alpha += ap * ap;
          beta += aq * aq;
          gamma += ap * aq;
        }
        if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double root = sqrt(zeta * zeta + 1.0);
        const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : 1.0 / (zeta - root);
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        for (int r = 0; r < m; r++) {
          const double ap = A[r * n + p], aq = A[r * n + q];
          A[r * n + p] = c * ap - s * aq;
          A[r * n + q] = s * ap + c * aq;
        }
        for (int r = 0; r < n; r++) {
          const double vp = V[r * n + p], vq = V[r * n + q];
          V[r * n + p] = c * vp - s * vq;
          V[r * n + q] = s * vp + c * vq;
        }
      }
}

/* A = U diag(d) Vt of the float matrix A (m x n, m <= 16, n <= 9). d[n] descending (ties: lower
 * column first), vt[n][n] rows = right singular vectors (columns of V), ut[n][m] rows = columns
 * of A V over their norms. */
static void svd(const float* A_in, int m, int n, int sweeps, double* d, double* vt, double* ut) {
  double A[144], V[81], s[9];
  int ord[9];
  for (int i = 0; i < m * n; i++) A[i] = (double)A_in[i];
  jacobi_columns(A, m, n, V, sweeps);
  for (int j = 0; j < n; j++) {
    double sum = 0.0;
    for (int r = 0; r < m; r++) sum += A[r * n + j] * A[r * n + j];
    s[j] = sqrt(sum);
    ord[j] = j;
  }
  for (int i = 1; i < n; i++)
    for (int j = i; j > 0 && s[ord[j - 1]] < s[ord[j]]; j--) {
      const int tmp = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = tmp;
    }
  for (int k = 0; k < n; k++) {
    const int j = ord[k];
    d[k] = s[j];
    for (int r = 0; r < n; r++) vt[k * n + r] = V[r * n + j];
    for (int r = 0; r < m; r++) ut[k * m + r] = A[r * n + j] / s[j];
  }
}

void init_svd(const float* A, int m, int n, int sweeps, double* d, double* vt, double* ut) {
  svd(A, m, n, sweeps, d, vt, ut);
}

/* cv::SVD::compute(A, w, u, vt) of a 3 x 3 float Mat, all three results CV_32F. */
static void svd3(const float* A, int sweeps, float* w, float* u, float* vt) {
  double d[3], vtd[9], utd[9];
  svd(A, 3, 3, sweeps, d, vtd, utd);
  for (int k = 0; k < 3; k++) {
    w[k] = (float)d[k];
    for (int r = 0; r < 3; r++) {
      vt[3 * k + r] = (float)vtd[3 * k + r];
      u[3 * r + k] = (float)utd[3 * k + r];
    }
  }
}

void init_svd3(const float* A, int sweeps, float* w, float* u, float* vt) {
  svd3(A, sweeps, w, u, vt);
}

/* ---- cv::Mat arithmetic -------------------------------------------------------------------- */

/* C (m x n) = A (m x k) B (k x n) */
static void matmul(const float* A, const float* B, int m, int k, int n, float* C) {
  for (int i = 0; i < m; i++)
    for (int j = 0; j < n; j++) {
      double acc = 0.0;
      for (int l = 0; l < k; l++) acc += (double)A[i * k + l] * (double)B[l * n + j];
      C[i * n + j] = (float)acc;
    }
}

static double det3(const float* a) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6],
               a7 = a[7], a8 = a[8];
  return a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6) + a2 * (a3 * a7 - a4 * a6);
}

static void inv3(const float* a, float* o) {
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

void init_inv3(const float* a, float* o) { inv3(a, o); }
double init_det3(const float* a) { return det3(a); }

static void transpose3(const float* a, float* o) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) o[3 * i + j] = a[3 * j + i];
}

/* v / cv::norm(v) for a 3-vector */
static void normalize3(float* v) {
  const double n = sqrt((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1] +
                        (double)v[2] * (double)v[2]);
  const float s = (float)(1.0 / n);
  for (int i = 0; i < 3; i++) v[i] = v[i] * s;
}

static void k_matrix(const float* K, float* Km) {
  const float m[9] = {K[0], 0.0f, K[2], 0.0f, K[1], K[3], 0.0f, 0.0f, 1.0f};
  memcpy(Km, m, sizeof(m));
}

/* ---- Normalize (:753-801) ------------------------------------------------------------------- */

/* All n keys of the frame, in index order, in float. out = meanX, meanY, sX, sY. */
void init_normalize(const float* keys, int n, float* out) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) {
    meanX += keys[2 * i];
    meanY += keys[2 * i + 1];
  }
  meanX = meanX / n;
  meanY = meanY / n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    meanDevX += fabsf(keys[2 * i] - meanX);
    meanDevY += fabsf(keys[2 * i + 1] - meanY);
  }
  meanDevX = meanDevX / n;
  meanDevY = meanDevY / n;
  out[0] = meanX;
  out[1] = meanY;
  out[2] = 1.0f / meanDevX;
  out[3] = 1.0f / meanDevY;
}

static void t_matrix(const float* nm, float* T) { /* :796-800 */
  const float m[9] = {nm[2], 0.0f, -nm[0] * nm[2], 0.0f, nm[3], -nm[1] * nm[3], 0.0f, 0.0f, 1.0f};
  memcpy(T, m, sizeof(m));
}

static void normalized(const float* keys, int i, const float* nm, float* p) { /* :777-793 */
  p[0] = (keys[2 * i] - nm[0]) * nm[2];
  p[1] = (keys[2 * i + 1] - nm[1]) * nm[3];
}

/* ---- ComputeH21 (:208-249), ComputeF21 (:251-287) ----------------------------------------- */

void init_compute_h21(const float* p1, const float* p2, int sweeps, float* H) {
  float A[144];
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    float* r0 = A + 18 * i;
    float* r1 = r0 + 9;
    r0[0] = 0.0f, r0[1] = 0.0f, r0[2] = 0.0f, r0[3] = -u1, r0[4] = -v1, r0[5] = -1.0f;
    r0[6] = v2 * u1, r0[7] = v2 * v1, r0[8] = v2;
    r1[0] = u1, r1[1] = v1, r1[2] = 1.0f, r1[3] = 0.0f, r1[4] = 0.0f, r1[5] = 0.0f;
    r1[6] = -u2 * u1, r1[7] = -u2 * v1, r1[8] = -u2;
  }
  double d[9], vt[81], ut[144];
  svd(A, 16, 9, sweeps, d, vt, ut);
  for (int c = 0; c < 9; c++) H[c] = (float)vt[72 + c];
}

void init_compute_f21(const float* p1, const float* p2, int sweeps, float* F) {
  float A[72];
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    float* r = A + 9 * i;
    r[0] = u2 * u1, r[1] = u2 * v1, r[2] = u2, r[3] = v2 * u1, r[4] = v2 * v1, r[5] = v2;
    r[6] = u1, r[7] = v1, r[8] = 1.0f;
  }
  double d[9], vtd[81], utd[72];
  svd(A, 8, 9, sweeps, d, vtd, utd);
  float Fpre[9], w[3], u[9], vt[9], uw[9];
  for (int c = 0; c < 9; c++) Fpre[c] = (float)vtd[72 + c];
  svd3(Fpre, sweeps, w, u, vt);
  const float D[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, 0.0f}; /* w[2] = 0 (:284) */
  matmul(u, D, 3, 3, 3, uw);
  matmul(uw, vt, 3, 3, 3, F);
}

/* ---- CheckHomography (:289-375), CheckFundamental (:377-457) ------------------------------- */

/* pairs[i] = (first, second) of mvMatches12[i]. bits: ceil(n / 64) words are written. */
float init_check_homography(const float* H21, const float* H12, const float* keys1,
                            const float* keys2, const int32_t* pairs, int n, float sigma,
                            uint64_t* bits) {
  const float h11 = H21[0], h12 = H21[1], h13 = H21[2], h21 = H21[3], h22 = H21[4], h23 = H21[5],
              h31 = H21[6], h32 = H21[7], h33 = H21[8];
  const float h11inv = H12[0], h12inv = H12[1], h13inv = H12[2], h21inv = H12[3], h22inv = H12[4],
              h23inv = H12[5], h31inv = H12[6], h32inv = H12[7], h33inv = H12[8];
  float score = 0;
  const float th = 5.991f;
  const float invSigmaSquare = 1.0f / (sigma * sigma);
  for (int w = 0; w < (n + 63) / 64; w++) bits[w] = 0;
  for (int i = 0; i < n; i++) {
    int bIn = 1;
    const float u1 = keys1[2 * pairs[2 * i]], v1 = keys1[2 * pairs[2 * i] + 1];
    const float u2 = keys2[2 * pairs[2 * i + 1]], v2 = keys2[2 * pairs[2 * i + 1] + 1];
    const float w2in1inv = 1.0f / (h31inv * u2 + h32inv * v2 + h33inv);
    const float u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv;
    const float v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th)
      bIn = 0;
    else
      score += th - chiSquare1;
    const float w1in2inv = 1.0f / (h31 * u1 + h32 * v1 + h33);
    const float u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv;
    const float v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
      bIn = 0;
    else
      score += th - chiSquare2;
    if (bIn) bits[i >> 6] |= (uint64_t)1 << (i & 63);
  }
  return score;
}

float init_check_fundamental(const float* F21, const float* keys1, const float* keys2,
                             const int32_t* pairs, int n, float sigma, uint64_t* bits) {
  const float f11 = F21[0], f12 = F21[1], f13 = F21[2], f21 = F21[3], f22 = F21[4], f23 = F21[5],
              f31 = F21[6], f32 = F21[7], f33 = F21[8];
  float score = 0;
  const float th = 3.841f;
  const float thScore = 5.991f;
  const float invSigmaSquare = 1.0f / (sigma * sigma);
  for (int w = 0; w < (n + 63) / 64; w++) bits[w] = 0;
  for (int i = 0; i < n; i++) {
    int bIn = 1;
    const float u1 = keys1[2 * pairs[2 * i]], v1 = keys1[2 * pairs[2 * i] + 1];
    const float u2 = keys2[2 * pairs[2 * i + 1]], v2 = keys2[2 * pairs[2 * i + 1] + 1];
    const float a2 = f11 * u1 + f12 * v1 + f13;
    const float b2 = f21 * u1 + f22 * v1 + f23;
    const float c2 = f31 * u1 + f32 * v1 + f33;
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th)
      bIn = 0;
    else
      score += thScore - chiSquare1;
    const float a1 = f11 * u2 + f21 * v2 + f31;
    const float b1 = f12 * u2 + f22 * v2 + f32;
    const float c1 = f13 * u2 + f23 * v2 + f33;
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
      bIn = 0;
    else
      score += thScore - chiSquare2;
    if (bIn) bits[i >> 6] |= (uint64_t)1 << (i & 63);
  }
  return score;
}

/* ---- the sample (:62-77) -------------------------------------------------------------------- */

/* The eight draws of one iteration resolved by the swap-and-pop; 0 when one is out of range. */
int init_resolve(int n, const int* randi, int* idx) {
  int pos[8], val[8], size = n;
  for (int i = 0; i < 8; i++) {
    const int r = randi[i];
    if (r < 0 || r > size - 1) return 0;
    int at_r = r, at_back = size - 1;
    for (int j = 0; j < i; j++) { /* later writes win */
      if (pos[j] == r) at_r = val[j];
      if (pos[j] == size - 1) at_back = val[j];
    }
    idx[i] = at_r;
    pos[i] = r;
    val[i] = at_back;
    size--;
  }
  return 1;
}

/* ---- Triangulate (:738-751), CheckRT (:804-922) ------------------------------------------- */

/* P1, P2: 3 x 4 float. x3D: the three coordinates after the division by the fourth. */
void init_triangulate(const float* kp1, const float* kp2, const float* P1, const float* P2,
                      int sweeps, float* x3D) {
  float A[16];
  for (int c = 0; c < 4; c++) {
    A[c] = kp1[0] * P1[8 + c] - P1[c];
    A[4 + c] = kp1[1] * P1[8 + c] - P1[4 + c];
    A[8 + c] = kp2[0] * P2[8 + c] - P2[c];
    A[12 + c] = kp2[1] * P2[8 + c] - P2[4 + c];
  }
  double d[4], vt[16], ut[16];
  svd(A, 4, 4, sweeps, d, vt, ut);
  const float x[4] = {(float)vt[12], (float)vt[13], (float)vt[14], (float)vt[15]};
  const float s = (float)(1.0 / (double)x[3]);
  for (int i = 0; i < 3; i++) x3D[i] = x[i] * s;
}

static uint32_t cos_key(float c) { /* ascending order of the keys = ascending cosines, NaN last */
  uint32_t b;
  if (c != c) return 0xFFFFFFFFu;
  memcpy(&b, &c, 4);
  return b & 0x80000000u ? ~b : b | 0x80000000u;
}

static float key_cos(uint32_t k) {
  if (k == 0xFFFFFFFFu) return NAN;
  const uint32_t b = k & 0x80000000u ? k & 0x7FFFFFFFu : ~k;
  float c;
  memcpy(&c, &b, 4);
  return c;
}

static int cmp_u32(const void* a, const void* b) {
  const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return x < y ? -1 : x > y;
}

/* inlier_bits: vbMatchesInliers over the n matches. good_bits: vbGood over the n1 keys of frame
 * 1, ceil(n1 / 64) words; p3d[n1][3] (zero where nothing is written). Returns nGood;
 * *cos_parallax = the cosine at rank min(50, nGood - 1) ascending, 0 when nGood = 0. */
int init_check_rt(const float* R, const float* t, const float* keys1, int n1, const float* keys2,
                  const int32_t* pairs, int n, const uint64_t* inlier_bits, const float* K,
                  float th2, int sweeps, uint64_t* good_bits, float* p3d, float* cos_parallax) {
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  float Km[9], P1[12], Rt[12], P2[12], Rtn[9], O2[3];
  k_matrix(K, Km);
  for (int w = 0; w < (n1 + 63) / 64; w++) good_bits[w] = 0;
  memset(p3d, 0, sizeof(float) * 3 * (size_t)n1);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      P1[4 * i + j] = Km[3 * i + j];
      Rt[4 * i + j] = R[3 * i + j];
      Rtn[3 * i + j] = -R[3 * j + i];
    }
    P1[4 * i + 3] = 0.0f;
    Rt[4 * i + 3] = t[i];
  }
  matmul(Km, Rt, 3, 3, 4, P2);  /* :838 */
  matmul(Rtn, t, 3, 3, 1, O2);  /* :840 */
  uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(n > 0 ? n : 1));
  int nGood = 0;
  for (int i = 0; i < n; i++) {
    if (!(inlier_bits[i >> 6] >> (i & 63) & 1)) continue;
    const int i1 = pairs[2 * i];
    const float* kp1 = keys1 + 2 * i1;
    const float* kp2 = keys2 + 2 * pairs[2 * i + 1];
    float p[3], p2[3];
    init_triangulate(kp1, kp2, P1, P2, sweeps, p);
    if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) continue;
    const float dist1 = (float)sqrt((double)p[0] * (double)p[0] + (double)p[1] * (double)p[1] +
                                    (double)p[2] * (double)p[2]);
    const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};
    const float dist2 = (float)sqrt((double)n2[0] * (double)n2[0] + (double)n2[1] * (double)n2[1] +
                                    (double)n2[2] * (double)n2[2]);
    const double dot = (double)p[0] * (double)n2[0] + (double)p[1] * (double)n2[1] +
                       (double)p[2] * (double)n2[2];
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    if (p[2] <= 0 && (double)cosParallax < 0.99998) continue;
    matmul(R, p, 3, 3, 1, p2); /* :876 */
    for (int j = 0; j < 3; j++) p2[j] = p2[j] + t[j];
    if (p2[2] <= 0 && (double)cosParallax < 0.99998) continue;
    const float invZ1 = 1.0f / p[2];
    const float im1x = fx * p[0] * invZ1 + cx;
    const float im1y = fy * p[1] * invZ1 + cy;
    const float squareError1 =
        (im1x - kp1[0]) * (im1x - kp1[0]) + (im1y - kp1[1]) * (im1y - kp1[1]);
    if (squareError1 > th2) continue;
    const float invZ2 = 1.0f / p2[2];
    const float im2x = fx * p2[0] * invZ2 + cx;
    const float im2y = fy * p2[1] * invZ2 + cy;
    const float squareError2 =
        (im2x - kp2[0]) * (im2x - kp2[0]) + (im2y - kp2[1]) * (im2y - kp2[1]);
    if (squareError2 > th2) continue;
    keys[nGood++] = cos_key(cosParallax);
    memcpy(p3d + 3 * i1, p, sizeof(p));
    if ((double)cosParallax < 0.99998) good_bits[i1 >> 6] |= (uint64_t)1 << (i1 & 63);
  }
  *cos_parallax = 0.0f;
  if (nGood > 0) {
    qsort(keys, (size_t)nGood, sizeof(uint32_t), cmp_u32);
    *cos_parallax = key_cos(keys[nGood - 1 < 50 ? nGood - 1 : 50]);
  }
  free(keys);
  return nGood;
}

/* ---- DecomposeE (:924-944), the motions of ReconstructF (:475-483) and ReconstructH (:588-690) */

void init_decompose_e(const float* E, int sweeps, float* R1, float* R2, float* t) {
  float Et[9], u[9], vt[9], tmp[9];
  double d[3], vtd[9], utd[9], v[3][3];
  transpose3(E, Et);
  svd(Et, 3, 3, sweeps, d, vtd, utd); /* rows of vtd: the LEFT singular vectors of E */
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
  matmul(u, W, 3, 3, 3, tmp);
  matmul(tmp, vt, 3, 3, 3, R1);
  if (det3(R1) < 0)
    for (int i = 0; i < 9; i++) R1[i] = -R1[i];
  matmul(u, Wt, 3, 3, 3, tmp);
  matmul(tmp, vt, 3, 3, 3, R2);
  if (det3(R2) < 0)
    for (int i = 0; i < 9; i++) R2[i] = -R2[i];
}

/* The four motions of ReconstructF in its order: (R1, t), (R2, t), (R1, -t), (R2, -t). */
int init_motions_f(const float* F21, const float* K, int sweeps, init_motion* m) {
  float Km[9], Kt[9], tmp[9], E[9], R1[9], R2[9], t[3];
  k_matrix(K, Km);
  transpose3(Km, Kt);
  matmul(Kt, F21, 3, 3, 3, tmp);
  matmul(tmp, Km, 3, 3, 3, E);
  init_decompose_e(E, sweeps, R1, R2, t);
  for (int i = 0; i < 4; i++) {
    memset(&m[i], 0, sizeof(m[i]));
    memcpy(m[i].R, i & 1 ? R2 : R1, sizeof(R1));
    for (int j = 0; j < 3; j++) m[i].t[j] = i & 2 ? -t[j] : t[j];
  }
  return 4;
}

/* The eight motions of ReconstructH, or 0 for the early return of :601. */
int init_motions_h(const float* H21, const float* K, int sweeps, init_motion* m) {
  float Km[9], invK[9], tmp[9], A[9], w[3], U[9], Vt[9];
  k_matrix(K, Km);
  inv3(Km, invK);
  matmul(invK, H21, 3, 3, 3, tmp);
  matmul(tmp, Km, 3, 3, 3, A);
  svd3(A, sweeps, w, U, Vt);
  const float s = (float)(det3(U) * det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  float sU[9];
  for (int i = 0; i < 9; i++) sU[i] = s * U[i];
  for (int i = 0; i < 8; i++) {
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tp[3];
    if (i < 4) {
      Rp[0] = ctheta, Rp[2] = -stheta[i], Rp[6] = stheta[i], Rp[8] = ctheta;
      tp[0] = x1[i], tp[1] = 0.0f, tp[2] = -x3[i];
      for (int j = 0; j < 3; j++) tp[j] = tp[j] * (d1 - d3);
    } else {
      Rp[0] = cphi, Rp[2] = sphi[i - 4], Rp[4] = -1.0f, Rp[6] = sphi[i - 4], Rp[8] = -cphi;
      tp[0] = x1[i - 4], tp[1] = 0.0f, tp[2] = x3[i - 4];
      for (int j = 0; j < 3; j++) tp[j] = tp[j] * (d1 + d3);
    }
    memset(&m[i], 0, sizeof(m[i]));
    matmul(sU, Rp, 3, 3, 3, tmp);
    matmul(tmp, Vt, 3, 3, 3, m[i].R);
    matmul(U, tp, 3, 3, 1, m[i].t);
    normalize3(m[i].t);
  }
  return 8;
}

/* ---- the whole device call of one job ------------------------------------------------------ */

static int valid_job(int n1, int n2, const int32_t* matches12, const int* draws, int n_its,
                     int max_n1, int max_its, int* n_out) {
  if (n1 < 8 || n1 > max_n1 || n1 > INIT_MAX_KEYS || n2 < 1 || n2 > INIT_MAX_KEYS) return 0;
  if (n_its < 1 || n_its > max_its || max_its > INIT_MAX_ITS) return 0;
  int n = 0, idx[8];
  for (int i = 0; i < n1; i++) {
    if (matches12[i] < -1 || matches12[i] >= n2) return 0;
    n += matches12[i] >= 0;
  }
  if (n < 8) return 0;
  for (int k = 0; k < n_its; k++)
    if (!init_resolve(n, draws + 8 * k, idx)) return 0;
  *n_out = n;
  return 1;
}

/* The device call's layout: hyp[2][max_its], bits[2][max_its][words], pairs[max_n1][2],
 * motion[8], good_bits[8][words], p3d[8][max_n1][3], words = ceil(max_n1 / 64). Rows >= n_its,
 * pairs >= N, motions >= n_motions and p3d rows >= n1 are not written; an invalid job writes
 * result->status = -1 only. */
void init_ransac(const float* keys1, int n1, const float* keys2, int n2, const int32_t* matches12,
                 const float* K, float sigma, const int* draws, int n_its, int max_n1, int max_its,
                 init_hyp* hyp, uint64_t* bits, init_result* result, int32_t* pairs,
                 init_motion* motion, uint64_t* good_bits, float* p3d) {
  int n = 0;
  if (!valid_job(n1, n2, matches12, draws, n_its, max_n1, max_its, &n)) {
    result->status = -1;
    return;
  }
  const int words = (max_n1 + 63) / 64;
  init_result res;
  memset(&res, 0, sizeof(res));
  res.n = n;
  for (int i = 0, c = 0; i < n1; i++) /* :35-44 */
    if (matches12[i] >= 0) {
      pairs[2 * c] = i;
      pairs[2 * c + 1] = matches12[i];
      c++;
    }
  init_normalize(keys1, n1, res.norm);
  init_normalize(keys2, n2, res.norm + 4);
  float T1[9], T2[9], T2inv[9], T2t[9];
  t_matrix(res.norm, T1);
  t_matrix(res.norm + 4, T2);
  inv3(T2, T2inv);      /* :114 */
  transpose3(T2, T2t);  /* :167 */
  float best_score[2] = {0.0f, 0.0f};
  res.best[0] = res.best[1] = -1;
  for (int model = 0; model < 2; model++)
    for (int k = 0; k < n_its; k++) {
      int idx[8];
      float p1[16], p2[16], Mn[9], tmp[9], M[9], Minv[9];
      init_resolve(n, draws + 8 * k, idx);
      for (int j = 0; j < 8; j++) {
        normalized(keys1, pairs[2 * idx[j]], res.norm, p1 + 2 * j);
        normalized(keys2, pairs[2 * idx[j] + 1], res.norm + 4, p2 + 2 * j);
      }
      init_hyp* h = hyp + (size_t)model * max_its + k;
      uint64_t* hb = bits + ((size_t)model * max_its + k) * words;
      memset(h, 0, sizeof(*h));
      memset(hb, 0, sizeof(uint64_t) * (size_t)words);
      if (model == 0) {
        init_compute_h21(p1, p2, INIT_SWEEPS, Mn);
        matmul(T2inv, Mn, 3, 3, 3, tmp);
        matmul(tmp, T1, 3, 3, 3, M); /* :140 */
        inv3(M, Minv);               /* :141 */
        h->score = init_check_homography(M, Minv, keys1, keys2, pairs, n, sigma, hb);
      } else {
        init_compute_f21(p1, p2, INIT_SWEEPS, Mn);
        matmul(T2t, Mn, 3, 3, 3, tmp);
        matmul(tmp, T1, 3, 3, 3, M); /* :194 */
        h->score = init_check_fundamental(M, keys1, keys2, pairs, n, sigma, hb);
      }
      memcpy(h->M, M, sizeof(M));
      if (h->score > best_score[model]) { /* :145, :198 */
        best_score[model] = h->score;
        res.best[model] = k;
      }
    }
  res.SH = best_score[0];
  res.SF = best_score[1];
  res.RH = res.SH / (res.SH + res.SF); /* :92 */
  res.model = (double)res.RH > 0.40 ? 0 : 1;
  res.n_motions = 0;
  const int b = res.best[res.model];
  if (b >= 0) {
    const init_hyp* h = hyp + (size_t)res.model * max_its + b;
    const uint64_t* hb = bits + ((size_t)res.model * max_its + b) * words;
    res.n_motions = res.model == 0 ? init_motions_h(h->M, K, INIT_SWEEPS, motion)
                                   : init_motions_f(h->M, K, INIT_SWEEPS, motion);
    const float th2 = 4.0f * (sigma * sigma); /* :490, :707 */
    for (int i = 0; i < res.n_motions; i++) {
      memset(good_bits + (size_t)i * words, 0, sizeof(uint64_t) * (size_t)words);
      motion[i].n_good = init_check_rt(motion[i].R, motion[i].t, keys1, n1, keys2, pairs, n, hb, K,
                                       th2, INIT_SWEEPS, good_bits + (size_t)i * words,
                                       p3d + (size_t)i * max_n1 * 3, &motion[i].cos_parallax);
    }
  }
  *result = res;
}

/* ---- Initialize (:22-101) with the tails of ReconstructF (:495-565) / ReconstructH (:693-735) */

/* From the outputs of init_ransac. Returns 1 / 0; on 1 *chosen is the motion. */
int init_reconstruct(const init_result* res, const uint64_t* bits, int max_n1, int max_its,
                     const init_motion* motion, float minParallax, int minTriangulated,
                     int* chosen) {
  *chosen = -1;
  if (res->status != 0) return 0;
  const int b = res->best[res->model];
  if (b < 0 || res->n_motions == 0) return 0;
  const int words = (max_n1 + 63) / 64;
  const uint64_t* hb = bits + ((size_t)res->model * max_its + b) * words;
  int N = 0;
  for (int i = 0; i < res->n; i++) N += (int)(hb[i >> 6] >> (i & 63) & 1);
  float parallax[INIT_MAX_MOTIONS];
  for (int i = 0; i < res->n_motions; i++)
    parallax[i] = motion[i].n_good > 0
                      ? (float)(acos((double)motion[i].cos_parallax) * 180 /
                                3.1415926535897932384626433832795)
                      : 0.0f;
  if (res->model == 1) {
    int maxGood = 0, nsimilar = 0;
    for (int i = 0; i < 4; i++)
      if (motion[i].n_good > maxGood) maxGood = motion[i].n_good;
    const int t = (int)(0.9 * N);
    const int nMinGood = t > minTriangulated ? t : minTriangulated;
    for (int i = 0; i < 4; i++)
      if (motion[i].n_good > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return 0;
    for (int i = 0; i < 4; i++)
      if (maxGood == motion[i].n_good) { /* the else-if chain: the first that ties */
        if (parallax[i] > minParallax) {
          *chosen = i;
          return 1;
        }
        return 0;
      }
    return 0;
  }
  int bestGood = 0, secondBestGood = 0, bestIdx = -1;
  float bestParallax = -1;
  for (int i = 0; i < 8; i++) {
    const int nGood = motion[i].n_good;
    if (nGood > bestGood) {
      secondBestGood = bestGood;
      bestGood = nGood;
      bestIdx = i;
      bestParallax = parallax[i];
    } else if (nGood > secondBestGood) {
      secondBestGood = nGood;
    }
  }
  if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax &&
      bestGood > minTriangulated && bestGood > 0.9 * N) {
    *chosen = bestIdx;
    return 1;
  }
  return 0;
}
