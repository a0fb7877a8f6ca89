// jacobi_svd.h -- the one SVD of the RANSAC EPnP solver (pnp_ransac.hip) and the monocular
// Initializer (init_ransac.hip): a cyclic one-sided Jacobi in FP64 (DESIGN.md "Linear algebra
// contract"; tests/pnpsolver_ref.c and tests/initializer_ref.c restate it as jacobi_columns).
// svd_lds runs it on a matrix in LDS with one 64-lane wave, svd_lane on a small square matrix in
// one lane's registers, from the same rotation, pair schedule and column order; each solver passes
// its own sweep count. sim3_ransac.hip's two-sided Jacobi takes its angle from jacobi_angle. What
// else the solvers share is in ransac_device.h.
#pragma once
#include <hip/hip_runtime.h>

namespace slamgpu {

// Lanes per column pair: the up to 6 disjoint pairs of a round fit a wave.
constexpr int kJacobiPairLanes = 10;

// tan, cos and sin of the rotation angle from zeta = cot of twice the angle: the smaller root.
__device__ __forceinline__ void jacobi_angle(double zeta, double& t, double& c, double& s) {
  const double root = __builtin_sqrt(zeta * zeta + 1.0);
  t = zeta >= 0.0 ? 1.0 / (zeta + root) : 1.0 / (zeta - root);
  c = 1.0 / __builtin_sqrt(t * t + 1.0);
  s = t * c;
}

// Squared norms alpha, beta and dot product gamma of columns p and q of A (M x N, row-major).
// False: no rotation, they are orthogonal to 1e-15 of their norms or hold a NaN; else the angle is
// jacobi_angle's for zeta = (beta - alpha) / (2.0 * gamma).
template <int M, int N>
__device__ __forceinline__ bool jacobi_dots(const double* A, int p, int q, double& alpha,
                                            double& beta, double& gamma) {
  alpha = beta = gamma = 0.0;
#pragma unroll
  for (int r = 0; r < M; r++) {
    const double ap = A[r * N + p], aq = A[r * N + q];
    alpha += ap * ap;
    beta += aq * aq;
    gamma += ap * aq;
  }
  return __builtin_fabs(gamma) > 1e-15 * __builtin_sqrt(alpha * beta);
}

// Round-robin order (tests/pnpsolver_ref.c: jacobi_columns): pair g < NP / 2 of round < NP - 1
// over NP (even) columns, p < q. The pairs of a round share no column; q >= N is the bye.
template <int NP>
__device__ __forceinline__ void jacobi_pair(int round, int g, int& p, int& q) {
  const int a = g == 0 ? NP - 1 : (round + g) % (NP - 1);
  const int b = g == 0 ? round : (round - g + NP - 1) % (NP - 1);
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// s[j]: the norm of column j of A (M x N, row-major); ord: the columns by descending norm, ties
// to the lower column.
template <int M, int N>
__device__ __forceinline__ void order_columns(const double* A, double* s, int* ord) {
  for (int j = 0; j < N; j++) {
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < M; r++) sum += A[r * N + j] * A[r * N + j];
    s[j] = __builtin_sqrt(sum);
    ord[j] = j;
  }
  for (int i = 1; i < N; i++)
    for (int j = i; j > 0 && s[ord[j - 1]] < s[ord[j]]; j--) {
      const int tmp = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = tmp;
    }
}

// Lds holds double A[>= M * N] and V[>= N * N].
// S.A (M x N, row-major) becomes A V with mutually orthogonal columns, S.V the rotations' product;
// d[N] the column norms descending (ties: lower column first), ord[k] the column of d[k]. Right
// singular vector k is column ord[k] of S.V, left singular vector k column ord[k] of S.A over d[k].
template <int M, int N, int SWEEPS, typename Lds>
__device__ __noinline__ void svd_lds(Lds& S, int lane, double* d, int* ord) {
  for (int t = lane; t < N * N; t += 64) S.V[t] = (t / N == t % N) ? 1.0 : 0.0;
  __syncthreads();
  // Group g of kJacobiPairLanes lanes takes pair g of the round -- the dot products redundantly
  // on each of its lanes, then the M rows of A and the N rows of V dealt over them.
  constexpr int NP = N + (N & 1);
  const int g = lane / kJacobiPairLanes, gl = lane % kJacobiPairLanes;
#pragma unroll 1
  for (int sw = 0; sw < SWEEPS; sw++)
#pragma unroll 1
    for (int round = 0; round < NP - 1; round++) {
      int p, q;
      jacobi_pair<NP>(round, g, p, q);
      bool rot = false;
      double alpha, beta, gamma, t, c = 1.0, s = 0.0;
      if (g < NP / 2 && q < N) rot = jacobi_dots<M, N>(S.A, p, q, alpha, beta, gamma);
      if (rot) jacobi_angle((beta - alpha) / (2.0 * gamma), t, c, s);
      __syncthreads();  // every group has read its two columns
      if (rot)
        for (int row = gl; row < M + N; row += kJacobiPairLanes) {
          double* x = row < M ? &S.A[row * N] : &S.V[(row - M) * N];
          const double xp = x[p], xq = x[q];
          x[p] = c * xp - s * xq;
          x[q] = s * xp + c * xq;
        }
      __syncthreads();
    }
  double s[N];
  order_columns<M, N>(S.A, s, ord);
  for (int k = 0; k < N; k++) d[k] = s[ord[k]];
}

// The same routine on one lane for a square N x N matrix: A (float, row-major) -> d[N],
// vt[N][N] rows = columns of V, ut[N][N] rows = columns of A V over their norms.
template <int N, int SWEEPS>
__device__ __forceinline__ void svd_lane(const float* A_in, double* d, double* vt, double* ut) {
  double A[N * N], V[N * N], s[N];
  int ord[N];
#pragma unroll
  for (int i = 0; i < N * N; i++) {
    A[i] = (double)A_in[i];
    V[i] = (i / N == i % N) ? 1.0 : 0.0;
  }
  constexpr int NP = N + (N & 1);
#pragma unroll 1
  for (int sw = 0; sw < SWEEPS; sw++)
#pragma unroll
    for (int round = 0; round < NP - 1; round++)
#pragma unroll
      for (int g = 0; g < NP / 2; g++) {
        int p, q;
        jacobi_pair<NP>(round, g, p, q);
        if (q >= N) continue;
        double alpha, beta, gamma, t, c, sn;
        if (!jacobi_dots<N, N>(A, p, q, alpha, beta, gamma)) continue;
        jacobi_angle((beta - alpha) / (2.0 * gamma), t, c, sn);
#pragma unroll
        for (int r = 0; r < N; r++) {
          const double ap = A[r * N + p], aq = A[r * N + q];
          A[r * N + p] = c * ap - sn * aq;
          A[r * N + q] = sn * ap + c * aq;
          const double vp = V[r * N + p], vq = V[r * N + q];
          V[r * N + p] = c * vp - sn * vq;
          V[r * N + q] = sn * vp + c * vq;
        }
      }
  order_columns<N, N>(A, s, ord);
  for (int k = 0; k < N; k++) {
    const int j = ord[k];
    d[k] = s[j];
    for (int r = 0; r < N; r++) {
      vt[k * N + r] = V[r * N + j];
      ut[k * N + r] = A[r * N + j] / s[j];
    }
  }
}

}  // namespace slamgpu
