/*
 * tests/sim3solver_ref.c -- CPU restatement of the loop closer's RANSAC Sim3 solver (TEST
 * INFRASTRUCTURE ONLY; built on demand by tests/sim3solver_ref.py with the oracle Makefile's
 * CFLAGS, no other library):
 *   src/solvers/sim3solver.cpp:142-217   iterate / find (the sequential state machine)
 *   src/solvers/sim3solver.cpp:219-341   ComputeCentroid, ComputeSim3 (Horn 1987)
 *   src/solvers/sim3solver.cpp:344-368   CheckInliers
 *   src/solvers/sim3solver.cpp:386-430   Project, FromCameraToImage
 * stated statement by statement under the arithmetic contract below. It shares no code with
 * csrc/: the sample is drawn from a literal copy of the index list (:166-180), the device uses a
 * closed form.
 *
 * The draws are an INPUT: per iteration the three values DUtils::Random::RandomInt returned.
 *
 * Float rules assumed (built with -ffp-contract=off), beyond those of tests/loopmatch_ref.c:
 *  - cv::reduce(P, C, 1, CV_REDUCE_SUM) of a 3x3 f32 matrix sums each row left to right in
 *    float; C = C / P.cols is a scale by the DOUBLE 1.0/3 that convertTo applies as the float
 *    (float)(1.0/3.0): C[r] = ((P[r][0] + P[r][1]) + P[r][2]) * (float)(1.0/3.0). Pr = P - C float.
 *  - M = Pr2 * Pr1.t() and P3 = mR12i * Pr2 are the small gemm: a float dot, terms left to right,
 *    no addend.
 *  - N11 .. N44 (:255-264) are float expressions of M's entries, left to right (the double
 *    variables only hold them), stored as float (:266-269).
 *  - cv::eigen (float, Jacobi in OpenCV) and atan2 / cv::Rodrigues are NOT restated: the
 *    eigenvector of the float-rounded N for its largest eigenvalue comes from a cyclic FP64
 *    Jacobi with a fixed sweep count (S3_JACOBI_SWEEPS sweeps over (0,1) (0,2) (0,3) (1,2) (1,3)
 *    (2,3); a pair whose off-diagonal is exactly 0 is skipped; + - * / sqrt only; largest
 *    eigenvalue, lowest index on a tie), normalised, and the rotation is formed from that unit
 *    quaternion directly in FP64 and rounded to float. The same matrix mathematically; q and -q
 *    agree; an exact identity gives I where the reference's vec / norm(vec) gives NaN.
 *  - nom = Pr1.dot(P3) and den = sum(P3^2) are double accumulations, in row-major order, of the
 *    products rounded to float; ms12i = (float)(nom / den).
 *  - mt12i = O1 - ms12i * mR12i * O2 is one gemm with alpha = -ms12i and the addend O1:
 *    t[r] = (float)((double)(-s) * (double)(float dot(R[r], O2)) + (double)O1[r]).
 *  - sR = ms12i * mR12i is the float product per entry; sRinv = (1.0 / ms12i) * mR12i.t() is
 *    the transpose scaled by the float (float)(1.0 / (double)ms12i); tinv = -sRinv * mt12i is a
 *    float dot, negated.
 *  - Project: Rcw * X + tcw is the small gemm row (float dot, double add, rounded to float);
 *    invz = 1 / z is a float division; x = X * invz; u = fx * x + cx is contracted by the
 *    Release build to fma(fx, x, cx), as in tests/loopmatch_ref.c. FromCameraToImage the same
 *    without the transform.
 *  - err = dx * dx + dy * dy in float (dist.dot(dist) of a 2-vector; not contracted: OpenCV).
 *  - mvnMaxError* is a std::vector<size_t> (sim3solver.h:74-75): the threshold is
 *    (float)(size_t)(9.210 * (double)sigma2[octave]). An octave outside [0, nlevels) (undefined
 *    behaviour in the reference) is never an inlier.
 *  - Degenerate samples propagate inf / NaN by IEEE rules; a NaN error is not an inlier.
 *
 * PARITY STATUS: "parity unpinned" against the reference binary (OpenCV absent; no fixtures).
 * Pinned by tests/test_sim3solver_ref.py against a pure-numpy model (np.linalg.eigh Horn, float64
 * projection) within rounding, and against a straightforward Python port of iterate().
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define S3_JACOBI_SWEEPS 8
#define S3_MAX_ITS 300
#define S3_MAX_MATCHES 4096

typedef struct {
  float x1c[3], x2c[3];
  float u1, v1, u2, v2;
  int32_t octave1, octave2;
} s3_match;

typedef struct {
  float R[9], t[3], s;
  int32_t n_inliers;
  int32_t pad[2];
} s3_hyp;

int s3_jacobi_sweeps(void) { return S3_JACOBI_SWEEPS; }

/* :166-180 on a literal copy of mvAllIndices. Returns 0 when a draw is out of its range. */
int s3_resolve(int n, const int32_t* randi, int32_t* idx) {
  if (n < 3) return 0;
  int* avail = (int*)malloc(sizeof(int) * (size_t)n);
  int size = n, ok = 1;
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int i = 0; i < 3 && ok; i++) {
    const int r = randi[i];
    if (r < 0 || r > size - 1) { ok = 0; break; }
    idx[i] = avail[r];
    avail[r] = avail[size - 1];
    size--;
  }
  free(avail);
  return ok;
}

/* Eigenvector (w, x, y, z; unit) of the symmetric float matrix N for its largest eigenvalue. */
void s3_eigvec(const float* Nf, int sweeps, double* q) {
  double A[4][4], V[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      A[i][j] = (double)Nf[4 * i + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sw = 0; sw < sweeps; sw++)
    for (int p = 0; p < 3; p++)
      for (int r = p + 1; r < 4; r++) {
        const double apq = A[p][r];
        if (apq == 0.0) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
        const double root = sqrt(theta * theta + 1.0);
        const double t = theta >= 0.0 ? 1.0 / (theta + root) : 1.0 / (theta - root);
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        for (int k = 0; k < 4; k++) {
          if (k == p || k == r) continue;
          const double akp = A[k][p], akq = A[k][r];
          A[k][p] = A[p][k] = c * akp - s * akq;
          A[k][r] = A[r][k] = s * akp + c * akq;
        }
        A[p][p] = A[p][p] - t * apq;
        A[r][r] = A[r][r] + t * apq;
        A[p][r] = A[r][p] = 0.0;
        for (int k = 0; k < 4; k++) {
          const double vkp = V[k][p], vkq = V[k][r];
          V[k][p] = c * vkp - s * vkq;
          V[k][r] = s * vkp + c * vkq;
        }
      }
  int best = 0;
  for (int i = 1; i < 4; i++)
    if (A[i][i] > A[best][best]) best = i;
  const double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double nrm = sqrt(w * w + x * x + y * y + z * z);
  q[0] = w / nrm;
  q[1] = x / nrm;
  q[2] = y / nrm;
  q[3] = z / nrm;
}

static inline float dot3(const float* a, int sa, const float* b, int sb) {
  return a[0] * b[0] + a[sa] * b[sb] + a[2 * sa] * b[2 * sb];
}

/* ComputeCentroid: P, Pr 3x3 row-major (column i = point i). */
static void centroid(const float* P, float* Pr, float* C) {
  const float third = (float)(1.0 / 3.0);
  for (int r = 0; r < 3; r++) {
    C[r] = ((P[3 * r] + P[3 * r + 1]) + P[3 * r + 2]) * third;
    for (int i = 0; i < 3; i++) Pr[3 * r + i] = P[3 * r + i] - C[r];
  }
}

typedef struct {
  float T12[12], T21[12]; /* [sR | t] rows of 4 */
} s3_transform;

/* ComputeSim3 (:230-341). N16 (optional): the float N, for the tests. */
static void compute_sim3(const float* P1, const float* P2, int fix_scale, int sweeps, s3_hyp* h,
                         s3_transform* T, float* N16) {
  float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
  centroid(P1, Pr1, O1);
  centroid(P2, Pr2, O2);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[3 * i + j] = dot3(Pr2 + 3 * i, 1, Pr1 + 3 * j, 1);
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
  const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24,
                       N13, N23, N33, N34, N14, N24, N34, N44};
  if (N16) memcpy(N16, N, sizeof(N));
  double q[4];
  s3_eigvec(N, sweeps, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  float* R = h->R;
  R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  R[1] = (float)(2.0 * (x * y - w * z));
  R[2] = (float)(2.0 * (x * z + w * y));
  R[3] = (float)(2.0 * (x * y + w * z));
  R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  R[5] = (float)(2.0 * (y * z - w * x));
  R[6] = (float)(2.0 * (x * z - w * y));
  R[7] = (float)(2.0 * (y * z + w * x));
  R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
  float P3[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) P3[3 * i + j] = dot3(R + 3 * i, 1, Pr2 + j, 3);
  float s = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int i = 0; i < 9; i++) {
      const float a = Pr1[i] * P3[i], b = P3[i] * P3[i];
      nom += (double)a;
      den += (double)b;
    }
    s = (float)(nom / den);
  }
  h->s = s;
  for (int r = 0; r < 3; r++) {
    const float d = dot3(R + 3 * r, 1, O2, 1);
    h->t[r] = (float)((double)(-s) * (double)d + (double)O1[r]);
  }
  const float inv = (float)(1.0 / (double)s);
  float sRinv[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      T->T12[4 * r + c] = s * R[3 * r + c];
      sRinv[3 * r + c] = R[3 * c + r] * inv;
      T->T21[4 * r + c] = sRinv[3 * r + c];
    }
  for (int r = 0; r < 3; r++) {
    T->T12[4 * r + 3] = h->t[r];
    T->T21[4 * r + 3] = -dot3(sRinv + 3 * r, 1, h->t, 1);
  }
}

static inline void to_image(const float* X, const float* K, float* uv) {
  const float invz = 1.0f / X[2];
  const float x = X[0] * invz, y = X[1] * invz;
  uv[0] = fmaf(K[0], x, K[2]);
  uv[1] = fmaf(K[1], y, K[3]);
}

static inline void project(const float* T, const float* X, const float* K, float* uv) {
  float P[3];
  for (int r = 0; r < 3; r++) {
    const float d = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2];
    P[r] = (float)((double)d + (double)T[4 * r + 3]);
  }
  to_image(P, K, uv);
}

float s3_threshold(float sigma2) { return (float)(size_t)(9.210 * (double)sigma2); }

/* One iteration: the sample idx[3], ComputeSim3, CheckInliers. bits[words] gets the mask. */
void s3_hypothesis(const s3_match* m, int n, const int32_t* idx, int fix_scale, const float* K1,
                   const float* K2, const float* sigma2_1, const float* sigma2_2, int nlevels,
                   int sweeps, s3_hyp* h, uint64_t* bits, int words, float* N16) {
  float P1[9], P2[9];
  for (int i = 0; i < 3; i++)
    for (int r = 0; r < 3; r++) {
      P1[3 * r + i] = m[idx[i]].x1c[r];
      P2[3 * r + i] = m[idx[i]].x2c[r];
    }
  s3_transform T;
  memset(h, 0, sizeof(*h));
  compute_sim3(P1, P2, fix_scale, sweeps, h, &T, N16);
  memset(bits, 0, sizeof(uint64_t) * (size_t)words);
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    float p1im1[2], p2im2[2], p2im1[2], p1im2[2];
    to_image(m[i].x1c, K1, p1im1);
    to_image(m[i].x2c, K2, p2im2);
    project(T.T12, m[i].x2c, K1, p2im1);
    project(T.T21, m[i].x1c, K2, p1im2);
    const float d1x = p1im1[0] - p2im1[0], d1y = p1im1[1] - p2im1[1];
    const float d2x = p1im2[0] - p2im2[0], d2y = p1im2[1] - p2im2[1];
    const float err1 = d1x * d1x + d1y * d1y;
    const float err2 = d2x * d2x + d2y * d2y;
    const int o1 = m[i].octave1, o2 = m[i].octave2;
    if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) continue;
    if (err1 < s3_threshold(sigma2_1[o1]) && err2 < s3_threshold(sigma2_2[o2])) {
      bits[i >> 6] |= (uint64_t)1 << (i & 63);
      cnt++;
    }
  }
  h->n_inliers = cnt;
}

/* ---- the solver object: SetRansacParameters' outcome (n_its, min_inliers) + iterate ---------- */
typedef struct {
  const s3_match* m;
  int n;
  float K1[4], K2[4];
  float sig1[64], sig2[64];
  int nlevels, fix_scale;
  const int32_t* draws;
  int n_its, min_inliers;
  int iterations;   /* mnIterations */
  int best_inliers; /* mnBestInliers */
  int has_best;
  s3_hyp best;      /* mBestRotation, mBestTranslation, mBestScale */
  int words;
  uint64_t *cur_bits, *best_bits; /* mvbInliersi, mvbBestInliers */
} s3_solver;

s3_solver* s3_create(const s3_match* m, int n, const float* K1, const float* K2,
                     const float* sigma2_1, const float* sigma2_2, int nlevels, int fix_scale,
                     const int32_t* draws, int n_its, int min_inliers) {
  s3_solver* S = (s3_solver*)calloc(1, sizeof(s3_solver));
  S->m = m;
  S->n = n;
  memcpy(S->K1, K1, 16);
  memcpy(S->K2, K2, 16);
  memcpy(S->sig1, sigma2_1, 4 * (size_t)nlevels);
  memcpy(S->sig2, sigma2_2, 4 * (size_t)nlevels);
  S->nlevels = nlevels;
  S->fix_scale = fix_scale;
  S->draws = draws;
  S->n_its = n_its;
  S->min_inliers = min_inliers;
  S->words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
  S->cur_bits = (uint64_t*)calloc((size_t)S->words, 8);
  S->best_bits = (uint64_t*)calloc((size_t)S->words, 8);
  return S;
}

void s3_destroy(s3_solver* S) {
  if (!S) return;
  free(S->cur_bits);
  free(S->best_bits);
  free(S);
}

/* iterate (:142-211). Returns the 0-based iteration whose transform is returned, or -1 (the empty
 * cv::Mat). inlier_bits[words]: mvbInliersi of that iteration (zero when nothing is returned). */
int s3_iterate(s3_solver* S, int n_iterations, int* no_more, int* n_inliers,
               uint64_t* inlier_bits) {
  *no_more = 0;
  *n_inliers = 0;
  memset(inlier_bits, 0, 8 * (size_t)S->words);
  if (S->n < S->min_inliers) {
    *no_more = 1;
    return -1;
  }
  int cur = 0;
  while (S->iterations < S->n_its && cur < n_iterations) {
    cur++;
    S->iterations++;
    const int k = S->iterations - 1;
    int32_t idx[3];
    s3_hyp h;
    if (!s3_resolve(S->n, S->draws + 3 * k, idx)) return -2;
    s3_hypothesis(S->m, S->n, idx, S->fix_scale, S->K1, S->K2, S->sig1, S->sig2, S->nlevels,
                  S3_JACOBI_SWEEPS, &h, S->cur_bits, S->words, NULL);
    if (h.n_inliers >= S->best_inliers) {
      memcpy(S->best_bits, S->cur_bits, 8 * (size_t)S->words);
      S->best_inliers = h.n_inliers;
      S->best = h;
      S->has_best = 1;
      if (h.n_inliers > S->min_inliers) {
        *n_inliers = h.n_inliers;
        memcpy(inlier_bits, S->cur_bits, 8 * (size_t)S->words);
        return k;
      }
    }
  }
  if (S->iterations >= S->n_its) *no_more = 1;
  return -1;
}

/* find (:213-217). */
int s3_find(s3_solver* S, int* n_inliers, uint64_t* inlier_bits) {
  int flag;
  return s3_iterate(S, S->n_its, &flag, n_inliers, inlier_bits);
}

/* GetEstimatedRotation / Translation / Scale; returns 0 while they are still empty. */
int s3_best(const s3_solver* S, s3_hyp* out) {
  *out = S->best;
  return S->has_best;
}

/* The whole schedule of one job, as the device call lays it out: hyp[n_its], bits[n_its][words],
 * events[], *n_events (-1 and nothing written for an invalid job). */
void s3_ransac(const s3_match* m, int n, const float* K1, const float* K2, const float* sigma2_1,
               const float* sigma2_2, int nlevels, int fix_scale, const int32_t* draws, int n_its,
               int max_its, int min_inliers, int words, s3_hyp* hyp, uint64_t* bits,
               int32_t* events, int32_t* n_events) {
  *n_events = -1;
  if (n < 3 || n > S3_MAX_MATCHES || n > 64 * words || n_its < 1 || n_its > max_its) return;
  int32_t idx[3];
  for (int k = 0; k < n_its; k++)
    if (!s3_resolve(n, draws + 3 * k, idx)) return;
  int best = 0, ne = 0;
  for (int k = 0; k < n_its; k++) {
    s3_resolve(n, draws + 3 * k, idx);
    s3_hypothesis(m, n, idx, fix_scale, K1, K2, sigma2_1, sigma2_2, nlevels, S3_JACOBI_SWEEPS,
                  hyp + k, bits + (size_t)k * words, words, NULL);
    if (hyp[k].n_inliers >= best) {
      best = hyp[k].n_inliers;
      if (hyp[k].n_inliers > min_inliers) events[ne++] = k;
    }
  }
  *n_events = ne;
}
