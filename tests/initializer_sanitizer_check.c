/* Stand-alone run of tests/initializer_ref.c under the address and undefined-behaviour sanitizers
 * (tests/test_initializer_ref.py builds it with -fsanitize=address,undefined and runs it as a
 * program of its own): a general and a planar pair of frames with holes in matches12 and
 * n1 != n2, all-identical points (NaN everywhere), a job of exactly 8 matches, a job at the
 * 8192 cap and invalid jobs. Prints the counts and "ok". */
#include <stdio.h>

#include "initializer_ref.c"

static unsigned g_state = 12345u;
static double rnd(void) { /* [0, 1) */
  g_state = g_state * 1664525u + 1013904223u;
  return (g_state >> 8) / 16777216.0;
}

static const float K[4] = {600.0f, 598.5f, 642.3f, 357.1f};

/* n matches among n1 >= n and n2 >= n keys; planar: the points lie on a plane. */
static void make(int planar, int n, int n1, int n2, float* k1, float* k2, int32_t* m12) {
  const double c = cos(0.12), s = sin(0.12), t[3] = {-2.4, 0.3, 0.9};
  for (int i = 0; i < n1; i++) {
    k1[2 * i] = (float)(1280 * rnd());
    k1[2 * i + 1] = (float)(720 * rnd());
    m12[i] = -1;
  }
  for (int i = 0; i < n2; i++) {
    k2[2 * i] = (float)(1280 * rnd());
    k2[2 * i + 1] = (float)(720 * rnd());
  }
  for (int i = 0; i < n; i++) {
    const int a = (int)((long)i * n1 / n), b = n2 - 1 - (int)((long)i * n2 / n);
    const double rx = (k1[2 * a] - K[2]) / K[0], ry = (k1[2 * a + 1] - K[3]) / K[1];
    const double z = planar ? 6.0 / (rx + 0.1 * ry + 0.5) : 4 + 16 * rnd();
    const double X[3] = {rx * z, ry * z, z};
    const double Y[3] = {c * X[0] + s * X[2] + t[0], X[1] + t[1], -s * X[0] + c * X[2] + t[2]};
    m12[a] = b;
    if (rnd() < 0.2 || Y[2] < 0.5 || z < 0.5) continue; /* a wrong match: the random key stays */
    k2[2 * b] = (float)(K[0] * Y[0] / Y[2] + K[2] + (rnd() - 0.5));
    k2[2 * b + 1] = (float)(K[1] * Y[1] / Y[2] + K[3] + (rnd() - 0.5));
  }
}

static void draw(int n, int n_its, int* d) {
  for (int k = 0; k < n_its; k++)
    for (int j = 0; j < 8; j++) d[8 * k + j] = (int)(rnd() * (n - j));
}

enum { CAP = INIT_MAX_KEYS, ITS = 64 };
static float k1[2 * CAP], k2[2 * CAP], p3d[8 * CAP * 3];
static int32_t m12[CAP], pairs[2 * CAP];
static int draws[8 * ITS];
static init_hyp hyp[2 * ITS];
static uint64_t bits[2 * ITS * (CAP / 64)], good[8 * (CAP / 64)];

static int run(int n, int n1, int n2, int n_its, int max_n1, int max_its, init_result* res) {
  init_motion motion[8];
  int chosen;
  memset(res, 0, sizeof(*res));
  init_ransac(k1, n1, k2, n2, m12, K, 1.0f, draws, n_its, max_n1, max_its, hyp, bits, res, pairs,
              motion, good, p3d);
  const int ok = init_reconstruct(res, bits, max_n1, max_its, motion, 1.0f, 50, &chosen);
  printf("n %d n1 %d n2 %d its %d: status %d N %d best %d %d model %d motions %d -> %d\n", n, n1,
         n2, n_its, res->status, res->n, res->best[0], res->best[1], res->model, res->n_motions, ok);
  return ok;
}

int main(void) {
  init_result res;
  int failures = 0;
  for (int planar = 0; planar < 2; planar++) {
    make(planar, 300, 341, 325, k1, k2, m12);
    draw(300, ITS, draws);
    run(300, 341, 325, ITS, 341, ITS, &res);
    failures += res.status != 0 || res.n != 300 || res.n_motions == 0;
    run(300, 341, 325, 5, 400, ITS, &res); /* rows wider than the job */
    failures += res.status != 0;
  }
  make(0, 8, 8, 9, k1, k2, m12);
  draw(8, 3, draws);
  run(8, 8, 9, 3, 8, 3, &res);
  failures += res.status != 0 || res.n != 8;
  for (int i = 0; i < 2 * 70; i++) k1[i] = k2[i] = 100.5f; /* all identical */
  for (int i = 0; i < 70; i++) m12[i] = i;
  draw(70, 9, draws);
  failures += run(70, 70, 70, 9, 70, 9, &res) != 0 || res.best[0] != -1 || res.best[1] != -1;
  make(0, CAP, CAP, CAP, k1, k2, m12);
  draw(CAP, 16, draws);
  run(CAP, CAP, CAP, 16, CAP, 16, &res);
  failures += res.status != 0 || res.n != CAP;
  /* invalid jobs: a draw out of range, a match outside frame 2, too few matches, n_its > max_its,
   * n1 > max_n1 */
  draws[8 * 3 + 7] = CAP - 7;
  run(CAP, CAP, CAP, 16, CAP, 16, &res);
  failures += res.status != -1;
  draw(CAP, 16, draws);
  m12[5] = CAP;
  run(CAP, CAP, CAP, 16, CAP, 16, &res);
  failures += res.status != -1;
  for (int i = 0; i < CAP; i++) m12[i] = i < 7 ? i : -1;
  run(7, CAP, CAP, 16, CAP, 16, &res);
  failures += res.status != -1;
  make(0, 100, 100, 100, k1, k2, m12);
  draw(100, 16, draws);
  run(100, 100, 100, 16, 100, 15, &res);
  failures += res.status != -1;
  run(100, 100, 100, 16, 99, 16, &res);
  failures += res.status != -1;
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
