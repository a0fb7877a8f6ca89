/* pnpsolver_ref.c -- CPU restatement of the RANSAC EPnP solver (include/slamgpu_pnpsolver.h,
 * csrc/pnp_ransac.hip): the contract the device is compared against bit for bit. It follows the
 * reference's PnPsolver (src/solvers/pnp_solver.cpp) function by function; what the reference
 * leaves to OpenCV is stated here (DESIGN.md "RANSAC EPnP solver"):
 *   - every cvSVD / cvInvert(CV_SVD) / cvSolve(CV_SVD) is ONE routine, a cyclic one-sided Jacobi
 *     SVD in FP64 with a fixed sweep count, singular values sorted descending, ties by index;
 *   - every sum over correspondences has one order: partial l sums the points i = l, l + 64, ...
 *     ascending from 0.0, then the 64 partials are added ascending from 0.0;
 *   - gauss_newton zeroes x once; qr_solve leaves x as it was on its zero-column return.
 * Built with the oracle Makefile's CFLAGS (-ffp-contract=off): no fused multiply-add anywhere.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PNP_SWEEPS 15 /* tools/pnp_jacobi_sweeps.py settles after 13, plus two */
#define PNP_LANES 64
#define PNP_MAX_ITS 512

typedef struct {
  float xw[3];
  float u, v;
  int32_t octave;
} pnp_match;

typedef struct {
  float Rcw[9], tcw[3];
  int32_t n_inliers, best;
  int32_t pad[2];
} pnp_hyp;

int pnp_jacobi_sweeps(void) { return PNP_SWEEPS; }

/* ---- the one SVD -------------------------------------------------------------------------- */

/* A (m x n, row-major, stride n) becomes A V with mutually orthogonal columns; V (n x n) is the
 * product of the rotations. A sweep visits the column pairs in round-robin (tournament) order:
 * np = n players, plus a bye when n is odd; in round r = 0 .. np - 2 pair 0 is (np - 1, r) and
 * pair i = 1 .. np / 2 - 1 is ((r + i) mod (np - 1), (r - i) mod (np - 1)); the lower column is p.
 * The pairs of a round share no column, so the device rotates them at once. */
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

/* A = U diag(d) Vt. d[n] descending (ties: lower column first), vt[n][n] rows = right singular
 * vectors, ut[n][m] rows = left singular vectors (column of A V over its norm). m, n <= 12. */
static void svd(const double* A_in, int m, int n, int sweeps, double* d, double* vt, double* ut) {
  double A[144], V[144], s[12];
  int ord[12];
  memcpy(A, A_in, sizeof(double) * (size_t)(m * n));
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

/* Least squares / minimum norm x (n) of A x = b through the SVD: singular values at or below
 * 2 eps sum(d) count as zero. */
static void svd_solve(const double* A, int m, int n, const double* b, int sweeps, double* x) {
  double d[12], vt[144], ut[144], sum = 0.0;
  svd(A, m, n, sweeps, d, vt, ut);
  for (int k = 0; k < n; k++) sum += d[k];
  const double thr = 2.0 * 2.220446049250313e-16 * sum;
  for (int i = 0; i < n; i++) x[i] = 0.0;
  for (int k = 0; k < n; k++) {
    if (!(d[k] > thr)) continue;
    double ub = 0.0;
    for (int r = 0; r < m; r++) ub += ut[k * m + r] * b[r];
    const double w = ub / d[k];
    for (int i = 0; i < n; i++) x[i] += vt[k * n + i] * w;
  }
}

void pnp_svd(const double* A, int m, int n, int sweeps, double* d, double* vt, double* ut) {
  svd(A, m, n, sweeps, d, vt, ut);
}

void pnp_svd_solve(const double* A, int m, int n, const double* b, int sweeps, double* x) {
  svd_solve(A, m, n, b, sweeps, x);
}

/* ---- EPnP --------------------------------------------------------------------------------- */

typedef struct {
  const pnp_match* m;
  const int* sel;  /* the correspondences of this solve */
  int n;
  double fu, fv, uc, vc;
  int sweeps;
  double cws[4][3], ccs[4][3], cc_inv[9];
  /* stages kept for the tests */
  double mtm[144], d[12], ut[144], l_6x10[60], rho[6], betas[4][4], rep_errors[4];
  int chosen;
} epnp;

/* The one order of every sum over correspondences. */
#define ORDERED_SUM(result, n_, i_, expr)                     \
  do {                                                        \
    double part_[PNP_LANES];                                  \
    for (int l_ = 0; l_ < PNP_LANES; l_++) {                  \
      part_[l_] = 0.0;                                        \
      for (int i_ = l_; i_ < (n_); i_ += PNP_LANES) part_[l_] += (expr); \
    }                                                         \
    double tot_ = 0.0;                                        \
    for (int l_ = 0; l_ < PNP_LANES; l_++) tot_ += part_[l_]; \
    (result) = tot_;                                          \
  } while (0)

static double pw(const epnp* E, int i, int j) { return (double)E->m[E->sel[i]].xw[j]; }
static double pu(const epnp* E, int i) { return (double)E->m[E->sel[i]].u; }
static double pv(const epnp* E, int i) { return (double)E->m[E->sel[i]].v; }

static double dot(const double* v1, const double* v2) {
  return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2];
}

static double dist2(const double* p1, const double* p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) +
         (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

static void choose_control_points(epnp* E) {
  const int n = E->n;
  for (int j = 0; j < 3; j++) {
    double s;
    ORDERED_SUM(s, n, i, pw(E, i, j));
    E->cws[0][j] = s / n;
  }
  double pw0tpw0[9], dc[3], uct[9], unused[9];
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) {
      double s;
      ORDERED_SUM(s, n, i, (pw(E, i, a) - E->cws[0][a]) * (pw(E, i, b) - E->cws[0][b]));
      pw0tpw0[3 * a + b] = pw0tpw0[3 * b + a] = s;
    }
  svd(pw0tpw0, 3, 3, E->sweeps, dc, uct, unused);
  for (int i = 1; i < 4; i++) {
    const double k = sqrt(dc[i - 1] / n);
    for (int j = 0; j < 3; j++) E->cws[i][j] = E->cws[0][j] + k * uct[3 * (i - 1) + j];
  }
}

static void compute_cc_inv(epnp* E) {
  double cc[9];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = E->cws[j][i] - E->cws[0][i];
  for (int j = 0; j < 3; j++) {
    double e[3] = {0.0, 0.0, 0.0}, x[3];
    e[j] = 1.0;
    svd_solve(cc, 3, 3, e, E->sweeps, x);
    for (int i = 0; i < 3; i++) E->cc_inv[3 * i + j] = x[i];
  }
}

static void alphas_of(const epnp* E, int i, double* a) {
  const double* ci = E->cc_inv;
  const double p0 = pw(E, i, 0), p1 = pw(E, i, 1), p2 = pw(E, i, 2);
  for (int j = 0; j < 3; j++)
    a[1 + j] = ci[3 * j] * (p0 - E->cws[0][0]) + ci[3 * j + 1] * (p1 - E->cws[0][1]) +
               ci[3 * j + 2] * (p2 - E->cws[0][2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

/* rows 2i and 2i + 1 of M (fill_M) */
static void m_rows(const epnp* E, int i, double* M1, double* M2) {
  double as[4];
  alphas_of(E, i, as);
  const double u = pu(E, i), v = pv(E, i);
  for (int k = 0; k < 4; k++) {
    M1[3 * k] = as[k] * E->fu;
    M1[3 * k + 1] = 0.0;
    M1[3 * k + 2] = as[k] * (E->uc - u);
    M2[3 * k] = 0.0;
    M2[3 * k + 1] = as[k] * E->fv;
    M2[3 * k + 2] = as[k] * (E->vc - v);
  }
}

static void compute_mtm(epnp* E) {
  const int n = E->n;
  double part[PNP_LANES][78];
  for (int l = 0; l < PNP_LANES; l++) {
    for (int e = 0; e < 78; e++) part[l][e] = 0.0;
    for (int i = l; i < n; i += PNP_LANES) {
      double M1[12], M2[12];
      m_rows(E, i, M1, M2);
      int e = 0;
      for (int a = 0; a < 12; a++)
        for (int b = a; b < 12; b++, e++) {
          part[l][e] += M1[a] * M1[b];
          part[l][e] += M2[a] * M2[b];
        }
    }
  }
  int e = 0;
  for (int a = 0; a < 12; a++)
    for (int b = a; b < 12; b++, e++) {
      double tot = 0.0;
      for (int l = 0; l < PNP_LANES; l++) tot += part[l][e];
      E->mtm[12 * a + b] = E->mtm[12 * b + a] = tot;
    }
}

static void compute_L_6x10(const double* ut, double* l_6x10) {
  const double* v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
  double dv[4][6][3];
  for (int i = 0; i < 4; i++) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
      dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
      dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
      b++;
      if (b > 3) {
        a++;
        b = a + 1;
      }
    }
  }
  for (int i = 0; i < 6; i++) {
    double* row = l_6x10 + 10 * i;
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
}

static void compute_rho(const epnp* E, double* rho) {
  rho[0] = dist2(E->cws[0], E->cws[1]);
  rho[1] = dist2(E->cws[0], E->cws[2]);
  rho[2] = dist2(E->cws[0], E->cws[3]);
  rho[3] = dist2(E->cws[1], E->cws[2]);
  rho[4] = dist2(E->cws[1], E->cws[3]);
  rho[5] = dist2(E->cws[2], E->cws[3]);
}

static void find_betas_approx_1(const epnp* E, double* betas) {
  double l[24], b4[4];
  for (int i = 0; i < 6; i++) {
    l[4 * i] = E->l_6x10[10 * i];
    l[4 * i + 1] = E->l_6x10[10 * i + 1];
    l[4 * i + 2] = E->l_6x10[10 * i + 3];
    l[4 * i + 3] = E->l_6x10[10 * i + 6];
  }
  svd_solve(l, 6, 4, E->rho, E->sweeps, b4);
  if (b4[0] < 0) {
    betas[0] = sqrt(-b4[0]);
    betas[1] = -b4[1] / betas[0];
    betas[2] = -b4[2] / betas[0];
    betas[3] = -b4[3] / betas[0];
  } else {
    betas[0] = sqrt(b4[0]);
    betas[1] = b4[1] / betas[0];
    betas[2] = b4[2] / betas[0];
    betas[3] = b4[3] / betas[0];
  }
}

static void find_betas_approx_2(const epnp* E, double* betas) {
  double l[18], b3[3];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 3; j++) l[3 * i + j] = E->l_6x10[10 * i + j];
  svd_solve(l, 6, 3, E->rho, E->sweeps, b3);
  if (b3[0] < 0) {
    betas[0] = sqrt(-b3[0]);
    betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
  } else {
    betas[0] = sqrt(b3[0]);
    betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
  }
  if (b3[1] < 0) betas[0] = -betas[0];
  betas[2] = 0.0;
  betas[3] = 0.0;
}

static void find_betas_approx_3(const epnp* E, double* betas) {
  double l[30], b5[5];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 5; j++) l[5 * i + j] = E->l_6x10[10 * i + j];
  svd_solve(l, 6, 5, E->rho, E->sweeps, b5);
  if (b5[0] < 0) {
    betas[0] = sqrt(-b5[0]);
    betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
  } else {
    betas[0] = sqrt(b5[0]);
    betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) betas[0] = -betas[0];
  betas[2] = b5[3] / betas[0];
  betas[3] = 0.0;
}

/* qr_solve (:813-903) for the 6 x 4 system; returns 1 on the zero-column return. */
static int qr_solve(double* pA, double* pb, double* pX) {
  const int nr = 6, nc = 4;
  double A1[6], A2[6];
  for (int k = 0; k < nc; k++) {
    double eta = fabs(pA[k * nc + k]);
    /* the reference's scan re-reads A[k][k] first, then A[k+1..nr-2][k]: its pointer starts at
     * A[k][k] and the loop runs nr - k - 1 times */
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(pA[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) return 1;
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      pA[i * nc + k] *= inv_eta;
      sum += pA[i * nc + k] * pA[i * nc + k];
    }
    double sigma = sqrt(sum);
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
  return 0;
}

static int g_qr_zero_returns = 0; /* counts the zero-column returns: the tests look for one */
int pnp_qr_zero_returns(void) { return g_qr_zero_returns; }

static void gauss_newton(const epnp* E, double* betas) {
  double a[24], b[6], x[4] = {0.0, 0.0, 0.0, 0.0};
  const double* rho = E->rho;
  for (int k = 0; k < 5; k++) {
    for (int i = 0; i < 6; i++) {
      const double* rowL = E->l_6x10 + i * 10;
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
    g_qr_zero_returns += qr_solve(a, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

static void pcs_of(const epnp* E, int i, int flip, double* pc) {
  double a[4];
  alphas_of(E, i, a);
  for (int j = 0; j < 3; j++) {
    pc[j] = a[0] * E->ccs[0][j] + a[1] * E->ccs[1][j] + a[2] * E->ccs[2][j] + a[3] * E->ccs[3][j];
    if (flip) pc[j] = -pc[j];
  }
}

static double compute_R_and_t(epnp* E, const double* betas, double R[3][3], double t[3]) {
  const int n = E->n;
  /* compute_ccs */
  for (int i = 0; i < 4; i++) E->ccs[i][0] = E->ccs[i][1] = E->ccs[i][2] = 0.0;
  for (int i = 0; i < 4; i++) {
    const double* v = E->ut + 12 * (11 - i);
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) E->ccs[j][k] += betas[i] * v[3 * j + k];
  }
  /* solve_for_sign: pcs[2] of the first correspondence; ccs is not read again */
  double first[3];
  pcs_of(E, 0, 0, first);
  const int flip = first[2] < 0.0;
  /* estimate_R_and_t */
  double pc0[3], pw0[3], abt[9], abt_d[3], abt_vt[9], abt_ut[9];
  for (int j = 0; j < 3; j++) {
    double s;
    ORDERED_SUM(s, n, i, ({ double pc_[3]; pcs_of(E, i, flip, pc_); pc_[j]; }));
    pc0[j] = s / n;
    ORDERED_SUM(s, n, i, pw(E, i, j));
    pw0[j] = s / n;
  }
  for (int j = 0; j < 3; j++)
    for (int c = 0; c < 3; c++) {
      double s;
      ORDERED_SUM(s, n, i,
                  ({ double pc_[3]; pcs_of(E, i, flip, pc_); (pc_[j] - pc0[j]) * (pw(E, i, c) - pw0[c]); }));
      abt[3 * j + c] = s;
    }
  svd(abt, 3, 3, E->sweeps, abt_d, abt_vt, abt_ut);
  /* R[i][j] = dot(abt_u row i, abt_v row j), U and V with the singular vectors as columns */
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      R[i][j] = abt_ut[0 + i] * abt_vt[0 + j] + abt_ut[3 + i] * abt_vt[3 + j] +
                abt_ut[6 + i] * abt_vt[6 + j];
  const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] +
                     R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
                     R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
  if (det < 0) {
    R[2][0] = -R[2][0];
    R[2][1] = -R[2][1];
    R[2][2] = -R[2][2];
  }
  t[0] = pc0[0] - dot(R[0], pw0);
  t[1] = pc0[1] - dot(R[1], pw0);
  t[2] = pc0[2] - dot(R[2], pw0);
  /* reprojection_error */
  double sum2;
  ORDERED_SUM(sum2, n, i, ({
                const double w_[3] = {pw(E, i, 0), pw(E, i, 1), pw(E, i, 2)};
                const double Xc = dot(R[0], w_) + t[0];
                const double Yc = dot(R[1], w_) + t[1];
                const double inv_Zc = 1.0 / (dot(R[2], w_) + t[2]);
                const double ue = E->uc + E->fu * Xc * inv_Zc;
                const double ve = E->vc + E->fv * Yc * inv_Zc;
                const double u = pu(E, i), v = pv(E, i);
                sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
              }));
  return sum2 / n;
}

/* compute_pose (:430-478). With ut_override the eigenvectors are taken as given (the tests pin
 * the stages after the eigen-solve against a numpy model fed the same ut). */
static void compute_pose(epnp* E, const double* ut_override, double R[3][3], double t[3]) {
  choose_control_points(E);
  compute_cc_inv(E);
  compute_mtm(E);
  double unused[144];
  svd(E->mtm, 12, 12, E->sweeps, E->d, E->ut, unused);
  if (ut_override) memcpy(E->ut, ut_override, sizeof(E->ut));
  compute_L_6x10(E->ut, E->l_6x10);
  compute_rho(E, E->rho);
  double Rs[4][3][3], ts[4][3];
  find_betas_approx_1(E, E->betas[1]);
  gauss_newton(E, E->betas[1]);
  E->rep_errors[1] = compute_R_and_t(E, E->betas[1], Rs[1], ts[1]);
  find_betas_approx_2(E, E->betas[2]);
  gauss_newton(E, E->betas[2]);
  E->rep_errors[2] = compute_R_and_t(E, E->betas[2], Rs[2], ts[2]);
  find_betas_approx_3(E, E->betas[3]);
  gauss_newton(E, E->betas[3]);
  E->rep_errors[3] = compute_R_and_t(E, E->betas[3], Rs[3], ts[3]);
  int N = 1;
  if (E->rep_errors[2] < E->rep_errors[1]) N = 2;
  if (E->rep_errors[3] < E->rep_errors[N]) N = 3;
  E->chosen = N;
  memcpy(R, Rs[N], sizeof(Rs[N]));
  memcpy(t, ts[N], sizeof(ts[N]));
}

static void epnp_init(epnp* E, const pnp_match* m, const int* sel, int n, const float* K,
                      int sweeps) {
  memset(E, 0, sizeof(*E));
  E->m = m;
  E->sel = sel;
  E->n = n;
  E->fu = K[0];
  E->fv = K[1];
  E->uc = K[2];
  E->vc = K[3];
  E->sweeps = sweeps;
}

/* One EPnP solve over matches[sel[0 .. n)]. stages (may be NULL): cws[12] mtm[144] d[12] ut[144]
 * l_6x10[60] rho[6] betas[3][4] rep_errors[3] chosen[1] = 394 doubles. */
void pnp_epnp(const pnp_match* m, const int* sel, int n, const float* K, int sweeps,
              const double* ut_override, double* R, double* t, double* stages) {
  epnp E;
  double Rm[3][3];
  epnp_init(&E, m, sel, n, K, sweeps);
  compute_pose(&E, ut_override, Rm, t);
  memcpy(R, Rm, sizeof(Rm));
  if (stages) {
    double* s = stages;
    memcpy(s, E.cws, 12 * 8), s += 12;
    memcpy(s, E.mtm, 144 * 8), s += 144;
    memcpy(s, E.d, 12 * 8), s += 12;
    memcpy(s, E.ut, 144 * 8), s += 144;
    memcpy(s, E.l_6x10, 60 * 8), s += 60;
    memcpy(s, E.rho, 6 * 8), s += 6;
    memcpy(s, E.betas[1], 12 * 8), s += 12;
    memcpy(s, E.rep_errors + 1, 3 * 8), s += 3;
    *s = E.chosen;
  }
}

/* ---- RANSAC ------------------------------------------------------------------------------- */

float pnp_threshold(float sigma2, float th2) { return sigma2 * th2; }

/* The sample of :144-154 for the four draws; 0 when one is out of range. */
int pnp_resolve(int n, const int* randi, int* idx) {
  int pos[4], val[4], size = n;
  for (int i = 0; i < 4; i++) {
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

/* CheckInliers (:261-292) with mRi / mti in double as compute_pose left them. */
void pnp_check_inliers(const pnp_match* m, int n, const double* R, const double* t, const float* K,
                       const float* sigma2, int nlevels, float th2, uint64_t* bits, int words,
                       int* count) {
  const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
  int cnt = 0;
  for (int w = 0; w < words; w++) bits[w] = 0;
  for (int i = 0; i < n; i++) {
    const float x = m[i].xw[0], y = m[i].xw[1], z = m[i].xw[2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float distX = (float)(m[i].u - ue);
    const float distY = (float)(m[i].v - ve);
    const float error2 = distX * distX + distY * distY;
    const int o = m[i].octave;
    if (o >= 0 && o < nlevels && error2 < sigma2[o] * th2) {
      bits[i >> 6] |= (uint64_t)1 << (i & 63);
      cnt++;
    }
  }
  *count = cnt;
}

static void to_hyp(const double* R, const double* t, int n_inliers, int best, pnp_hyp* h) {
  memset(h, 0, sizeof(*h));
  for (int i = 0; i < 9; i++) h->Rcw[i] = (float)R[i];
  for (int i = 0; i < 3; i++) h->tcw[i] = (float)t[i];
  h->n_inliers = n_inliers;
  h->best = best;
}

static int bits_to_sel(const uint64_t* bits, int n, int* sel) {
  int c = 0;
  for (int i = 0; i < n; i++)
    if (bits[i >> 6] >> (i & 63) & 1) sel[c++] = i;
  return c;
}

/* The whole schedule of one job in the device call's layout: hyp[max_its], bits[max_its][words],
 * refined[max_its], refined_bits[max_its][words], events[max_its], *n_events. Rows >= n_its are
 * not written; an invalid job writes *n_events = -1 only. */
void pnp_ransac(const pnp_match* m, int n, const float* K, const float* sigma2, int nlevels,
                float th2, const int* draws, int n_its, int max_its, int min_inliers, int words,
                pnp_hyp* hyp, uint64_t* bits, pnp_hyp* refined, uint64_t* refined_bits,
                int* events, int* n_events) {
  *n_events = -1;
  if (n < 4 || n > words * 64 || n_its < 1 || n_its > max_its || min_inliers < 4) return;
  int idx[4];
  for (int k = 0; k < n_its; k++)
    if (!pnp_resolve(n, draws + 4 * k, idx)) return;
  int* sel = (int*)malloc(sizeof(int) * (size_t)n);
  int best = -1, best_n = 0, ne = 0;
  for (int k = 0; k < n_its; k++) {
    double R[9], t[3];
    int cnt;
    pnp_resolve(n, draws + 4 * k, idx);
    pnp_epnp(m, idx, 4, K, PNP_SWEEPS, NULL, R, t, NULL);
    pnp_check_inliers(m, n, R, t, K, sigma2, nlevels, th2, bits + (size_t)k * words, words, &cnt);
    memset(&refined[k], 0, sizeof(pnp_hyp));
    refined[k].n_inliers = refined[k].best = -1;
    memset(refined_bits + (size_t)k * words, 0, sizeof(uint64_t) * (size_t)words);
    if (cnt >= min_inliers && cnt > best_n) {
      best = k;
      best_n = cnt;
      const int ns = bits_to_sel(bits + (size_t)k * words, n, sel);
      double Rr[9], tr[3];
      int rc;
      pnp_epnp(m, sel, ns, K, PNP_SWEEPS, NULL, Rr, tr, NULL);
      pnp_check_inliers(m, n, Rr, tr, K, sigma2, nlevels, th2, refined_bits + (size_t)k * words,
                        words, &rc);
      to_hyp(Rr, tr, rc, k, &refined[k]);
    }
    to_hyp(R, t, cnt, best, &hyp[k]);
    if (cnt >= min_inliers && refined[best].n_inliers > min_inliers) events[ne++] = k;
  }
  free(sel);
  *n_events = ne;
}

/* ---- the sequential solver: iterate / find / Refine as the reference runs them -------------- */

typedef struct {
  const pnp_match* m;
  int n, nlevels, words;
  float K[4], sigma2[64], th2;
  const int* draws; /* 4 per iteration, n_draw_its iterations available */
  int n_draw_its;
  int min_inliers, max_its; /* the effective mRansacMinInliers, mRansacMaxIts */
  int mnIterations, mnBestInliers;
  uint64_t *inliers_i, *best_inliers, *refined_inliers;
  pnp_hyp best_T, refined_T;
  int mnRefinedInliers;
  int n_refines; /* Refine() calls so far */
} pnp_solver;

pnp_solver* pnp_create(const pnp_match* m, int n, const float* K, const float* sigma2, int nlevels,
                       float th2, const int* draws, int n_draw_its, int min_inliers, int max_its) {
  pnp_solver* S = (pnp_solver*)calloc(1, sizeof(pnp_solver));
  S->m = m;
  S->n = n;
  S->nlevels = nlevels;
  S->words = n > 0 ? (n + 63) / 64 : 1;
  memcpy(S->K, K, sizeof(S->K));
  memcpy(S->sigma2, sigma2, sizeof(float) * (size_t)nlevels);
  S->th2 = th2;
  S->draws = draws;
  S->n_draw_its = n_draw_its;
  S->min_inliers = min_inliers;
  S->max_its = max_its;
  S->inliers_i = (uint64_t*)calloc((size_t)S->words, 8);
  S->best_inliers = (uint64_t*)calloc((size_t)S->words, 8);
  S->refined_inliers = (uint64_t*)calloc((size_t)S->words, 8);
  return S;
}

void pnp_destroy(pnp_solver* S) {
  free(S->inliers_i);
  free(S->best_inliers);
  free(S->refined_inliers);
  free(S);
}

static int refine(pnp_solver* S) {
  int* sel = (int*)malloc(sizeof(int) * (size_t)S->n);
  const int ns = bits_to_sel(S->best_inliers, S->n, sel);
  double R[9], t[3];
  S->n_refines++;
  pnp_epnp(S->m, sel, ns, S->K, PNP_SWEEPS, NULL, R, t, NULL);
  free(sel);
  pnp_check_inliers(S->m, S->n, R, t, S->K, S->sigma2, S->nlevels, S->th2, S->refined_inliers,
                    S->words, &S->mnRefinedInliers);
  if (S->mnRefinedInliers > S->min_inliers) {
    to_hyp(R, t, S->mnRefinedInliers, -1, &S->refined_T);
    return 1;
  }
  return 0;
}

/* iterate (:118-211). Returns 1 with *T / bits / *n_inliers when a pose is returned, 0 for the
 * empty Mat, -2 when the draws ran out. */
int pnp_iterate(pnp_solver* S, int nIterations, int* bNoMore, int* n_inliers, uint64_t* bits,
                pnp_hyp* T) {
  *bNoMore = 0;
  *n_inliers = 0;
  memset(bits, 0, 8 * (size_t)S->words);
  if (S->n < S->min_inliers) {
    *bNoMore = 1;
    return 0;
  }
  int nCurrentIterations = 0;
  while (S->mnIterations < S->max_its || nCurrentIterations < nIterations) {
    if (S->mnIterations >= S->n_draw_its) return -2;
    nCurrentIterations++;
    const int k = S->mnIterations++;
    int idx[4], cnt;
    double R[9], t[3];
    if (!pnp_resolve(S->n, S->draws + 4 * k, idx)) return -2;
    pnp_epnp(S->m, idx, 4, S->K, PNP_SWEEPS, NULL, R, t, NULL);
    pnp_check_inliers(S->m, S->n, R, t, S->K, S->sigma2, S->nlevels, S->th2, S->inliers_i,
                      S->words, &cnt);
    if (cnt >= S->min_inliers) {
      if (cnt > S->mnBestInliers) {
        memcpy(S->best_inliers, S->inliers_i, 8 * (size_t)S->words);
        S->mnBestInliers = cnt;
        to_hyp(R, t, cnt, k, &S->best_T);
      }
      if (refine(S)) {
        *n_inliers = S->mnRefinedInliers;
        memcpy(bits, S->refined_inliers, 8 * (size_t)S->words);
        *T = S->refined_T;
        return 1;
      }
    }
  }
  if (S->mnIterations >= S->max_its) {
    *bNoMore = 1;
    if (S->mnBestInliers >= S->min_inliers) {
      *n_inliers = S->mnBestInliers;
      memcpy(bits, S->best_inliers, 8 * (size_t)S->words);
      *T = S->best_T;
      return 1;
    }
  }
  return 0;
}

int pnp_find(pnp_solver* S, int* n_inliers, uint64_t* bits, pnp_hyp* T) {
  int flag;
  return pnp_iterate(S, S->max_its, &flag, n_inliers, bits, T);
}

int pnp_iterations(const pnp_solver* S) { return S->mnIterations; }
int pnp_refines(const pnp_solver* S) { return S->n_refines; }

/* SetRansacParameters (:87-105): the effective mRansacMinInliers and mRansacMaxIts. */
void pnp_parameters(int N, double probability, int minInliers, int maxIterations, int minSet,
                    float epsilon, int* min_inliers, int* max_its) {
  int nMinInliers = (int)(N * epsilon);
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  if (epsilon < (float)nMinInliers / N) epsilon = (float)nMinInliers / N;
  int nIterations;
  if (nMinInliers == N) {
    nIterations = 1;
  } else {
    const double q = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
    nIterations = (q >= 1.0 && q <= 2147483647.0) ? (int)q : (int)0x80000000;
  }
  *min_inliers = nMinInliers;
  const int lo = nIterations < maxIterations ? nIterations : maxIterations;
  *max_its = lo > 1 ? lo : 1;
}
