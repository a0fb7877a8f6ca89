// jacobi_svd.h -- the one SVD of the RANSAC EPnP solver (pnp_ransac.hip) and the monocular
// Initializer (init_ransac.hip): a cyclic one-sided Jacobi in FP64 on a matrix held in LDS, run by
// one 64-lane wave (DESIGN.md "Linear algebra contract"; tests/pnpsolver_ref.c and
// tests/initializer_ref.c restate it as jacobi_columns). Each solver passes its own sweep count.
#pragma once
#include <hip/hip_runtime.h>

namespace slamgpu {

// Lanes per column pair: the up to 6 disjoint pairs of a round fit a wave.
constexpr int kJacobiPairLanes = 10;

// Lds holds double A[>= M * N] and V[>= N * N].
// S.A (M x N, row-major) becomes A V with mutually orthogonal columns, S.V the rotations' product;
// d[N] the column norms descending (ties: lower column first), ord[k] the column of d[k]. Right
// singular vector k is column ord[k] of S.V, left singular vector k column ord[k] of S.A over d[k].
template <int M, int N, int SWEEPS, typename Lds>
__device__ __noinline__ void svd_lds(Lds& S, int lane, double* d, int* ord) {
  for (int t = lane; t < N * N; t += 64) S.V[t] = (t / N == t % N) ? 1.0 : 0.0;
  __syncthreads();
  // Round-robin order (tests/pnpsolver_ref.c: jacobi_columns): the pairs of a round share no
  // column, so group g of kJacobiPairLanes lanes takes pair g -- the dot products redundantly on
  // each of its lanes, then the M rows of A and the N rows of V dealt over them.
  constexpr int NP = N + (N & 1);
  const int g = lane / kJacobiPairLanes, gl = lane % kJacobiPairLanes;
#pragma unroll 1
  for (int sw = 0; sw < SWEEPS; sw++)
#pragma unroll 1
    for (int round = 0; round < NP - 1; round++) {
      const int a = g == 0 ? NP - 1 : (round + g) % (NP - 1);
      const int b = g == 0 ? round : (round - g + NP - 1) % (NP - 1);
      const int p = a < b ? a : b, q = a < b ? b : a;
      bool rot = false;
      double c = 1.0, s = 0.0;
      if (g < NP / 2 && q < N) {  // q >= N: the bye
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < M; r++) {
          const double ap = S.A[r * N + p], aq = S.A[r * N + q];
          alpha += ap * ap;
          beta += aq * aq;
          gamma += ap * aq;
        }
        rot = __builtin_fabs(gamma) > 1e-15 * __builtin_sqrt(alpha * beta);
        if (rot) {
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double root = __builtin_sqrt(zeta * zeta + 1.0);
          const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : 1.0 / (zeta - root);
          c = 1.0 / __builtin_sqrt(t * t + 1.0);
          s = t * c;
        }
      }
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
  for (int j = 0; j < N; j++) {
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < M; r++) sum += S.A[r * N + j] * S.A[r * N + j];
    s[j] = __builtin_sqrt(sum);
    ord[j] = j;
  }
  for (int i = 1; i < N; i++)
    for (int j = i; j > 0 && s[ord[j - 1]] < s[ord[j]]; j--) {
      const int tmp = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = tmp;
    }
  for (int k = 0; k < N; k++) d[k] = s[ord[k]];
}

}  // namespace slamgpu
