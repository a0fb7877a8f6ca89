/* newpoints_ref.c -- CPU restatement of the triangulation half of LocalMapper::CreateNewMapPoints
 * (include/slamgpu_kfmatch.h: slamgpu_create_new_map_points, csrc/newpoints.hip): the contract the
 * device is compared against bit for bit. It follows src/core/local_mapper.cpp:332-490 of the
 * reference for one (current, neighbour) pair and one match12 row, walking ascending idx1 (the
 * order of vMatchedIndices); the line numbers in the comments are that file's. Every `continue`
 * has its own status code. What the reference leaves to OpenCV and libm is stated here (DESIGN.md
 * "CreateNewMapPoints"):
 *   - cv::Mat rules of the monocular Initializer (tests/initializer_ref.c): a product accumulates
 *     in double over ascending k from 0.0 and rounds to float once, a chain is evaluated left to
 *     right; Mat / s multiplies by (float)(1.0 / s); cv::norm and Mat::dot accumulate in double;
 *     cv::SVD::compute is the cyclic one-sided Jacobi in FP64 with a fixed sweep count, the null
 *     vector a column of V rounded to float;
 *   - scalar float lines keep the association of the reference's Release build (GCC
 *     -ffp-contract=fast), each fma written out; a float division is the float division;
 *   - cos(2 * atan2(mb / 2, depth)) is (d^2 - h^2) / (d^2 + h^2) in double from the float h = mb / 2
 *     and the float d, rounded to float once. np_cos_stereo_libm is the literal float chain.
 * Built with the oracle Makefile's CFLAGS (-ffp-contract=off).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define NP_SWEEPS 6 /* tools/newpoints_jacobi_sweeps.py: settled after 4 at the latest, plus two */

/* status codes: 0 no match, 1 .. 3 the source of an accepted point, negative the failed test */
enum {
  NP_DLT = 1,          /* :375-392 */
  NP_STEREO1 = 2,      /* :394-396 UnprojectStereo(idx1) */
  NP_STEREO2 = 3,      /* :397-399 UnprojectStereo(idx2) */
  NP_W_ZERO = -1,      /* :387 */
  NP_LOW_PARALLAX = -2,/* :400-402 */
  NP_BEHIND1 = -3,     /* :407 */
  NP_BEHIND2 = -4,     /* :412 */
  NP_REPROJ1_STEREO = -5, /* :428 */
  NP_REPROJ1_MONO = -6,   /* :432 */
  NP_REPROJ2_STEREO = -7, /* :449 */
  NP_REPROJ2_MONO = -8,   /* :453 */
  NP_DIST_ZERO = -9,   /* :462 */
  NP_SCALE = -10,      /* :469 */
  NP_NO_DEPTH = -11,   /* keyframe.cpp:489: UnprojectStereo of a depth <= 0 returns an empty Mat */
  NP_MALFORMED = -12   /* match12 >= n2, or an octave outside [0, nlevels) */
};

typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} np_keypoint;

typedef struct {
  const np_keypoint* kps;     /* undistorted_keypoints */
  const np_keypoint* raw_kps; /* keypoints (UnprojectStereo); NULL = kps */
  const float* u_right;
  const float* depth;
  const uint8_t* desc;
  int32_t n, pad;
  float Rcw[9], tcw[3], Ow[3];
  float fx, fy, cx, cy, mbf, mb;
} np_kf;

typedef struct {
  float xyz[3], normal[3], min_dist, max_dist;
  int32_t skip, pad[3];
  uint8_t desc[32];
} np_fuse_point;

typedef struct {
  int32_t neighbour, idx1, idx2, source;
} np_new_point;

int np_jacobi_sweeps(void) { return NP_SWEEPS; }

/* ---- the one SVD (tests/initializer_ref.c: jacobi_columns, svd) for a 4 x 4 matrix ---------- */

static void jacobi_columns4(double* A, double* V, int sweeps) {
  const int n = 4;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sw = 0; sw < sweeps; sw++)
    for (int round = 0; round < n - 1; round++)
      for (int i = 0; i < n / 2; i++) {
        const int a = i == 0 ? n - 1 : (round + i) % (n - 1);
        const int b = i == 0 ? round : (round - i + n - 1) % (n - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < n; r++) {
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
        for (int r = 0; r < n; r++) {
          const double ap = A[r * n + p], aq = A[r * n + q];
          A[r * n + p] = c * ap - s * aq;
          A[r * n + q] = s * ap + c * aq;
          const double vp = V[r * n + p], vq = V[r * n + q];
          V[r * n + p] = c * vp - s * vq;
          V[r * n + q] = s * vp + c * vq;
        }
      }
}

/* vt.row(3) of cv::SVD::compute(A): the column of V whose A V column has the least norm (ties:
 * the later column), in double. */
static void null_vector4(const float* A_in, int sweeps, double* x) {
  double A[16], V[16], s[4];
  int ord[4];
  for (int i = 0; i < 16; i++) A[i] = (double)A_in[i];
  jacobi_columns4(A, V, sweeps);
  for (int j = 0; j < 4; j++) {
    double sum = 0.0;
    for (int r = 0; r < 4; r++) sum += A[r * 4 + j] * A[r * 4 + j];
    s[j] = sqrt(sum);
    ord[j] = j;
  }
  for (int i = 1; i < 4; i++)
    for (int j = i; j > 0 && s[ord[j - 1]] < s[ord[j]]; j--) {
      const int tmp = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = tmp;
    }
  for (int r = 0; r < 4; r++) x[r] = V[r * 4 + ord[3]];
}

/* ---- cv::Mat arithmetic --------------------------------------------------------------------- */

/* y = M x (3 x 3 times 3 x 1); tr: M^T */
static void matvec3(const float* M, int tr, const float* x, float* y) {
  for (int i = 0; i < 3; i++) {
    double acc = 0.0;
    for (int k = 0; k < 3; k++) acc += (double)(tr ? M[3 * k + i] : M[3 * i + k]) * (double)x[k];
    y[i] = (float)acc;
  }
}

static double dot3(const float* a, const float* b) {
  double acc = 0.0;
  for (int k = 0; k < 3; k++) acc += (double)a[k] * (double)b[k];
  return acc;
}

static double norm3(const float* a) { return sqrt(dot3(a, a)); }

/* ---- the stereo parallax (:362, :365) -------------------------------------------------------- */

float np_cos_stereo(float mb, float depth) {
  const float h = mb / 2;
  const double hh = (double)h * (double)h, dd = (double)depth * (double)depth;
  return (float)((dd - hh) / (dd + hh));
}

float np_cos_stereo_libm(float mb, float depth) { return cosf(2 * atan2f(mb / 2, depth)); }

/* Both forms for n depths at once. */
void np_cos_stereo_many(float mb, const float* depth, int n, float* identity, float* libm) {
  for (int i = 0; i < n; i++) {
    identity[i] = np_cos_stereo(mb, depth[i]);
    libm[i] = np_cos_stereo_libm(mb, depth[i]);
  }
}

/* ---- DLT (:376-392); x3D only when the result is 0 ------------------------------------------ */

static void dlt_rows(const float* xn1, const np_kf* K1, const float* xn2, const np_kf* K2, float* A) {
  for (int c = 0; c < 4; c++) {
    const float t1_0 = c < 3 ? K1->Rcw[c] : K1->tcw[0], t1_1 = c < 3 ? K1->Rcw[3 + c] : K1->tcw[1],
                t1_2 = c < 3 ? K1->Rcw[6 + c] : K1->tcw[2];
    const float t2_0 = c < 3 ? K2->Rcw[c] : K2->tcw[0], t2_1 = c < 3 ? K2->Rcw[3 + c] : K2->tcw[1],
                t2_2 = c < 3 ? K2->Rcw[6 + c] : K2->tcw[2];
    A[c] = xn1[0] * t1_2 - t1_0;
    A[4 + c] = xn1[1] * t1_2 - t1_1;
    A[8 + c] = xn2[0] * t2_2 - t2_0;
    A[12 + c] = xn2[1] * t2_2 - t2_1;
  }
}

/* The 4 x 4 matrix of a pair and its null vector in double, for tools and tests. */
void np_dlt(const np_kf* K1, const np_kf* K2, int idx1, int idx2, int sweeps, float* A, double* x) {
  const np_keypoint kp1 = K1->kps[idx1], kp2 = K2->kps[idx2];
  const float xn1[3] = {(kp1.x - K1->cx) * (1.0f / K1->fx), (kp1.y - K1->cy) * (1.0f / K1->fy), 1.0f};
  const float xn2[3] = {(kp2.x - K2->cx) * (1.0f / K2->fx), (kp2.y - K2->cy) * (1.0f / K2->fy), 1.0f};
  dlt_rows(xn1, K1, xn2, K2, A);
  null_vector4(A, sweeps, x);
}

/* KeyFrame::UnprojectStereo (keyframe.cpp:478-492): Twc = [Rcw^T | Ow] */
static int unproject_stereo(const np_kf* K, int i, float* x3D) {
  const float z = K->depth[i];
  if (!(z > 0)) return 0;
  const np_keypoint* raw = K->raw_kps ? K->raw_kps : K->kps;
  const float u = raw[i].x, v = raw[i].y;
  const float invfx = 1.0f / K->fx, invfy = 1.0f / K->fy;
  const float c[3] = {(u - K->cx) * z * invfx, (v - K->cy) * z * invfy, z};
  float r[3];
  matvec3(K->Rcw, 1, c, r);
  for (int k = 0; k < 3; k++) x3D[k] = r[k] + K->Ow[k];
  return 1;
}

/* One pair (:335-489). scale / sigma2: the level tables; scale_factor: KeyFrame::scale_factor.
 * first_obs: 0 = the current keyframe comes first in the new point's observation map, 1 = the
 * neighbour. out is written only for a status > 0. */
int np_pair_one(const np_kf* K1, const np_kf* K2, int idx1, int idx2, const float* scale,
                const float* sigma2, int nlevels, float scale_factor, int first_obs, int libm_cos,
                int sweeps, np_fuse_point* out) {
  if (idx2 < 0 || idx2 >= K2->n) return NP_MALFORMED;
  const np_keypoint kp1 = K1->kps[idx1], kp2 = K2->kps[idx2];
  if (kp1.octave < 0 || kp1.octave >= nlevels || kp2.octave < 0 || kp2.octave >= nlevels)
    return NP_MALFORMED;
  const float ur1 = K1->u_right[idx1], ur2 = K2->u_right[idx2];
  const int st1 = ur1 >= 0, st2 = ur2 >= 0;

  /* :347-355 */
  const float invfx1 = 1.0f / K1->fx, invfy1 = 1.0f / K1->fy;
  const float invfx2 = 1.0f / K2->fx, invfy2 = 1.0f / K2->fy;
  const float xn1[3] = {(kp1.x - K1->cx) * invfx1, (kp1.y - K1->cy) * invfy1, 1.0f};
  const float xn2[3] = {(kp2.x - K2->cx) * invfx2, (kp2.y - K2->cy) * invfy2, 1.0f};
  float ray1[3], ray2[3];
  matvec3(K1->Rcw, 1, xn1, ray1);
  matvec3(K2->Rcw, 1, xn2, ray2);
  const float cosRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));

  /* :357-369 */
  float cosSt = cosRays + 1;
  float cosSt1 = cosSt, cosSt2 = cosSt;
  if (st1)
    cosSt1 = libm_cos ? np_cos_stereo_libm(K1->mb, K1->depth[idx1]) : np_cos_stereo(K1->mb, K1->depth[idx1]);
  else if (st2)
    cosSt2 = libm_cos ? np_cos_stereo_libm(K2->mb, K2->depth[idx2]) : np_cos_stereo(K2->mb, K2->depth[idx2]);
  cosSt = cosSt2 < cosSt1 ? cosSt2 : cosSt1; /* std::min(cosSt1, cosSt2) */

  float x3D[3];
  int source;
  if (cosRays < cosSt && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) { /* :372-374 */
    float A[16];
    double xd[4];
    dlt_rows(xn1, K1, xn2, K2, A);
    null_vector4(A, sweeps, xd);
    const float x[4] = {(float)xd[0], (float)xd[1], (float)xd[2], (float)xd[3]};
    if (x[3] == 0) return NP_W_ZERO;
    const float s = (float)(1.0 / (double)x[3]);
    for (int k = 0; k < 3; k++) x3D[k] = x[k] * s;
    source = NP_DLT;
  } else if (st1 && cosSt1 < cosSt2) {
    if (!unproject_stereo(K1, idx1, x3D)) return NP_NO_DEPTH;
    source = NP_STEREO1;
  } else if (st2 && cosSt2 < cosSt1) {
    if (!unproject_stereo(K2, idx2, x3D)) return NP_NO_DEPTH;
    source = NP_STEREO2;
  } else {
    return NP_LOW_PARALLAX;
  }

  /* :406-414 */
  const float z1 = (float)(dot3(K1->Rcw + 6, x3D) + (double)K1->tcw[2]);
  if (z1 <= 0) return NP_BEHIND1;
  const float z2 = (float)(dot3(K2->Rcw + 6, x3D) + (double)K2->tcw[2]);
  if (z2 <= 0) return NP_BEHIND2;

  /* :417-435 */
  const float sig1 = sigma2[kp1.octave];
  const float x1 = (float)(dot3(K1->Rcw, x3D) + (double)K1->tcw[0]);
  const float y1 = (float)(dot3(K1->Rcw + 3, x3D) + (double)K1->tcw[1]);
  const float u1 = (K1->fx * x1) / z1 + K1->cx;
  const float v1 = (K1->fy * y1) / z1 + K1->cy;
  const float ex1 = u1 - kp1.x, ey1 = v1 - kp1.y;
  if (st1) {
    const float u1r = u1 - (K1->mbf / z1);
    const float er1 = u1r - ur1;
    if ((double)fmaf(er1, er1, fmaf(ex1, ex1, ey1 * ey1)) > 7.8 * (double)sig1)
      return NP_REPROJ1_STEREO;
  } else {
    if ((double)fmaf(ex1, ex1, ey1 * ey1) > 5.991 * (double)sig1) return NP_REPROJ1_MONO;
  }

  /* :438-456; the current keyframe's mbf at :447 */
  const float sig2 = sigma2[kp2.octave];
  const float x2 = (float)(dot3(K2->Rcw, x3D) + (double)K2->tcw[0]);
  const float y2 = (float)(dot3(K2->Rcw + 3, x3D) + (double)K2->tcw[1]);
  const float u2 = (K2->fx * x2) / z2 + K2->cx;
  const float v2 = (K2->fy * y2) / z2 + K2->cy;
  const float ex2 = u2 - kp2.x, ey2 = v2 - kp2.y;
  if (st2) {
    const float u2r = u2 - (K1->mbf / z2);
    const float er2 = u2r - ur2;
    if (fmaf(er2, er2, fmaf(ex2, ex2, ey2 * ey2)) > 7.8f * sig2) return NP_REPROJ2_STEREO;
  } else {
    if ((double)fmaf(ex2, ex2, ey2 * ey2) > 5.991 * (double)sig2) return NP_REPROJ2_MONO;
  }

  /* :459-471 */
  const float n1[3] = {x3D[0] - K1->Ow[0], x3D[1] - K1->Ow[1], x3D[2] - K1->Ow[2]};
  const float n2[3] = {x3D[0] - K2->Ow[0], x3D[1] - K2->Ow[1], x3D[2] - K2->Ow[2]};
  const double nd1 = norm3(n1), nd2 = norm3(n2);
  const float dist1 = (float)nd1, dist2 = (float)nd2;
  if (dist1 == 0 || dist2 == 0) return NP_DIST_ZERO;
  const float ratioDist = dist2 / dist1;
  const float ratioFactor = 1.5f * scale_factor;
  const float ratioOctave = scale[kp1.octave] / scale[kp2.octave];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist / ratioFactor > ratioOctave) return NP_SCALE;

  /* the MapPoint after :474-485 (map_point.cpp:249-354) */
  memset(out, 0, sizeof(*out));
  const float s1 = (float)(1.0 / nd1), s2 = (float)(1.0 / nd2);
  for (int k = 0; k < 3; k++) {
    out->xyz[k] = x3D[k];
    float normal = 0.0f;
    normal = normal + n1[k] * s1;
    normal = normal + n2[k] * s2;
    out->normal[k] = normal * 0.5f; /* normal / n, n = 2 */
  }
  out->max_dist = dist1 * scale[kp1.octave];
  out->min_dist = out->max_dist / scale[nlevels - 1];
  memcpy(out->desc, first_obs ? K2->desc + 32 * (size_t)idx2 : K1->desc + 32 * (size_t)idx1, 32);
  return source;
}

/* One neighbour: every idx1 with match12[idx1] >= 0, ascending. Appends the accepted points to
 * points / news at *n_new, writes status[n1] and sets has_mp1 of the accepted idx1. */
void np_pair(const np_kf* K1, const np_kf* K2, const int32_t* match12, int neighbour,
             const float* scale, const float* sigma2, int nlevels, float scale_factor, int first_obs,
             int libm_cos, int sweeps, np_fuse_point* points, np_new_point* news, int32_t* n_new,
             int8_t* status, uint8_t* has_mp1) {
  for (int i = 0; i < K1->n; i++) {
    status[i] = 0;
    if (match12[i] < 0) continue;
    np_fuse_point p;
    const int st = np_pair_one(K1, K2, i, match12[i], scale, sigma2, nlevels, scale_factor,
                               first_obs, libm_cos, sweeps, &p);
    status[i] = (int8_t)st;
    if (st <= 0) continue;
    points[*n_new] = p;
    const np_new_point q = {neighbour, i, match12[i], st};
    news[*n_new] = q;
    ++*n_new;
    has_mp1[i] = 1;
  }
}
