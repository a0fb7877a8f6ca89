/* Stand-alone run of tests/pnpsolver_ref.c under the address and undefined-behaviour sanitizers
 * (tests/test_pnpsolver_ref.py builds it with -fsanitize=address,undefined and runs it as a
 * program of its own): the degenerate cases of the GPU tests -- a coplanar, a collinear, a
 * repeated-point and a four-identical-points sample (qr_solve's zero-column return), points at
 * Zc = 0 and behind the camera, octaves outside the table -- then a job at the 4096 cap, an
 * invalid job, and the sequential solver run past its schedule. Prints "ok" and the counts. */
#include <stdio.h>

#include "pnpsolver_ref.c"

static unsigned g_state = 12345u;
static double rnd(void) { /* [0, 1) */
  g_state = g_state * 1664525u + 1013904223u;
  return (g_state >> 8) / 16777216.0;
}

static void make(pnp_match* m, int n, const float* K) {
  for (int i = 0; i < n; i++) {
    const double x = -6 + 12 * rnd(), y = -2 + 4 * rnd(), z = 4 + 16 * rnd();
    m[i].xw[0] = (float)(x - 0.3);
    m[i].xw[1] = (float)(y + 0.2);
    m[i].xw[2] = (float)(z - 0.5);
    m[i].u = (float)(K[0] * x / z + K[2] + (rnd() - 0.5));
    m[i].v = (float)(K[1] * y / z + K[3] + (rnd() - 0.5));
    m[i].octave = (int)(8 * rnd());
    if (rnd() < 0.3) m[i].u += 80.0f;
  }
}

/* the draws that resolve to the sample s, by search */
static int draws_of(int n, const int* s, int* d) {
  int idx[4];
  for (d[0] = 0; d[0] < n; d[0]++)
    for (d[1] = 0; d[1] < n - 1; d[1]++)
      for (d[2] = 0; d[2] < n - 2; d[2]++)
        for (d[3] = 0; d[3] < n - 3; d[3]++)
          if (pnp_resolve(n, d, idx) && idx[0] == s[0] && idx[1] == s[1] && idx[2] == s[2] &&
              idx[3] == s[3])
            return 1;
  return 0;
}

int main(void) {
  const float K[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
  float sigma2[8];
  for (int l = 0; l < 8; l++) sigma2[l] = l ? sigma2[l - 1] * 1.44f : 1.0f;
  enum { N = 20, ITS = 9, BIG = 4096, BIG_ITS = 4 };
  static pnp_match m[BIG];
  make(m, N, K);
  for (int j = 0; j < 3; j++) /* 0..3 coplanar */
    m[3].xw[j] = m[0].xw[j] + 0.4f * (m[1].xw[j] - m[0].xw[j]) + 0.7f * (m[2].xw[j] - m[0].xw[j]);
  for (int i = 5; i < 8; i++) { /* 4..7 collinear */
    m[i].xw[0] = m[4].xw[0] + (i - 4) * 1.0f;
    m[i].xw[1] = m[4].xw[1] + (i - 4) * 0.5f;
    m[i].xw[2] = m[4].xw[2] - (i - 4) * 0.25f;
  }
  for (int j = 0; j < 3; j++) {
    m[9].xw[j] = m[8].xw[j];                               /* repeated */
    m[13].xw[j] = m[14].xw[j] = m[15].xw[j] = m[12].xw[j]; /* rho = 0 */
  }
  m[16].xw[0] = 0.2f, m[16].xw[1] = -0.45f, m[16].xw[2] = 0.5f;  /* Zc = 0 for t = (.3, -.2, .5) */
  m[17].xw[2] = -6.0f;                                           /* behind the camera */
  m[18].octave = -1;
  m[19].octave = 8;
  const int samples[ITS][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {8, 9, 10, 11}, {12, 13, 14, 15},
                               {16, 0, 1, 2}, {17, 10, 11, 2}, {18, 19, 0, 1}, {0, 1, 2, 10},
                               {12, 13, 0, 1}};
  int draws[4 * ITS];
  for (int k = 0; k < ITS; k++)
    if (!draws_of(N, samples[k], draws + 4 * k)) return 1;
  {
    pnp_hyp hyp[ITS], refined[ITS];
    uint64_t bits[ITS], rbits[ITS];
    int events[ITS], ne = 0;
    pnp_ransac(m, N, K, sigma2, 8, 5.991f, draws, ITS, ITS, 4, 1, hyp, bits, refined, rbits, events,
               &ne);
    if (ne < 0 || pnp_qr_zero_returns() < 1) return 2;
    printf("degenerate: %d events, %d zero-column returns\n", ne, pnp_qr_zero_returns());
    pnp_ransac(m, 3, K, sigma2, 8, 5.991f, draws, ITS, ITS, 4, 1, hyp, bits, refined, rbits, events,
               &ne);
    if (ne != -1) return 3;
  }
  {
    make(m, BIG, K);
    static pnp_hyp hyp[BIG_ITS], refined[BIG_ITS];
    static uint64_t bits[BIG_ITS * 64], rbits[BIG_ITS * 64];
    int big_draws[4 * BIG_ITS], events[BIG_ITS], ne = 0;
    for (int i = 0; i < 4 * BIG_ITS; i++) big_draws[i] = (int)(rnd() * (BIG - 3));
    pnp_ransac(m, BIG, K, sigma2, 8, 5.991f, big_draws, BIG_ITS, BIG_ITS, 20, 64, hyp, bits,
               refined, rbits, events, &ne);
    if (ne < 0) return 4;
    printf("cap: %d events, best %d\n", ne, hyp[BIG_ITS - 1].best);
  }
  {
    enum { M = 40, SCHED = 60 };
    make(m, M, K);
    int d[4 * SCHED], mi, its, calls = 0, found = 0;
    for (int i = 0; i < 4 * SCHED; i++) d[i] = (int)(rnd() * (M - i % 4));
    pnp_parameters(M, 0.99, 10, 300, 4, 0.5f, &mi, &its);
    pnp_solver* S = pnp_create(m, M, K, sigma2, 8, 5.991f, d, SCHED, mi, its);
    for (; calls < 20; calls++) {
      int no_more, ni;
      uint64_t bits[1];
      pnp_hyp T;
      const int r = pnp_iterate(S, 5, &no_more, &ni, bits, &T);
      if (r == -2) break; /* the draws ran out: past the schedule, as intended */
      found += r == 1 && !no_more;
      if (no_more && pnp_iterations(S) + 5 > SCHED) break;
    }
    printf("solver: min_inliers %d max_its %d, %d calls, %d poses, %d iterations\n", mi, its, calls,
           found, pnp_iterations(S));
    if (pnp_iterations(S) <= its) return 5;
    pnp_destroy(S);
  }
  printf("ok\n");
  return 0;
}
