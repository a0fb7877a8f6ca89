/* newpoints_sanitizer_check.c -- tests/newpoints_ref.c plus a main of its own, for the address and
 * undefined-behaviour sanitizers (tests/test_newpoints_ref.py builds and runs it as a program): a
 * regular keyframe pair, a row without matches, x3D(3) == 0, NaN poses, a stereo keypoint without
 * depth, malformed matches and octaves. Prints "ok" last. */
#include <stdio.h>
#include <stdlib.h>

#include "newpoints_ref.c"

#define N 64

static float scale[8], sigma2[8];

typedef struct {
  np_keypoint kps[N];
  float ur[N], depth[N];
  uint8_t desc[N * 32];
  np_kf kf;
} frame;

/* A camera at (cx0, 0, 0), unrotated, seeing points on a slanted plane 8 .. 24 m ahead. */
static void make_frame(frame* f, float cx0, int stereo_every) {
  memset(f, 0, sizeof(*f));
  const float fx = 700.0f, fy = 700.0f, cx = 600.0f, cy = 180.0f, bf = 380.0f;
  for (int i = 0; i < N; i++) {
    const float X = -6.0f + 0.2f * (float)i, Y = -1.0f + 0.03f * (float)i, Z = 8.0f + 0.25f * (float)i;
    f->kps[i].x = fx * (X - cx0) / Z + cx;
    f->kps[i].y = fy * Y / Z + cy;
    f->kps[i].octave = i % 8;
    const int st = stereo_every && i % stereo_every == 0;
    f->ur[i] = st ? f->kps[i].x - bf / Z : -1.0f;
    f->depth[i] = st ? Z : -1.0f;
    for (int b = 0; b < 32; b++) f->desc[32 * i + b] = (uint8_t)(i * 7 + b);
  }
  np_kf* k = &f->kf;
  k->kps = f->kps;
  k->raw_kps = NULL;
  k->u_right = f->ur;
  k->depth = f->depth;
  k->desc = f->desc;
  k->n = N;
  k->Rcw[0] = k->Rcw[4] = k->Rcw[8] = 1.0f;
  k->tcw[0] = -cx0;
  k->Ow[0] = cx0;
  k->fx = fx, k->fy = fy, k->cx = cx, k->cy = cy, k->mbf = bf, k->mb = bf / fx;
}

static void fail(const char* what) {
  printf("failed: %s\n", what);
  exit(1);
}

static int run(const np_kf* a, const np_kf* b, const int32_t* m, int8_t* status, int* counts) {
  np_fuse_point* pts = malloc(sizeof(np_fuse_point) * N);
  np_new_point* news = malloc(sizeof(np_new_point) * N);
  uint8_t* has_mp = calloc(N, 1);
  int32_t n_new = 0;
  np_pair(a, b, m, 0, scale, sigma2, 8, scale[1], 1, 0, NP_SWEEPS, pts, news, &n_new, status,
          has_mp);
  int set = 0;
  for (int i = 0; i < N; i++) {
    set += has_mp[i];
    if (counts) counts[status[i] + 16]++;
  }
  if (set != n_new) fail("has_mp flags != n_new");
  for (int i = 1; i < n_new; i++)
    if (news[i].idx1 <= news[i - 1].idx1) fail("order");
  free(pts);
  free(news);
  free(has_mp);
  return n_new;
}

int main(void) {
  scale[0] = 1.0f;
  for (int i = 1; i < 8; i++) scale[i] = scale[i - 1] * 1.2f;
  for (int i = 0; i < 8; i++) sigma2[i] = scale[i] * scale[i];
  frame* a = malloc(sizeof(frame));
  frame* b = malloc(sizeof(frame));
  int32_t m[N];
  int8_t status[N];
  int counts[32] = {0};

  /* a regular pair, all matched, mono / stereo mixed */
  make_frame(a, 0.0f, 3);
  make_frame(b, 0.8f, 2);
  for (int i = 0; i < N; i++) m[i] = i;
  const int n_reg = run(&a->kf, &b->kf, m, status, counts);
  printf("regular: %d of %d\n", n_reg, N);
  if (n_reg < N / 2) fail("regular pair");

  /* no match at all */
  for (int i = 0; i < N; i++) m[i] = -1;
  if (run(&a->kf, &b->kf, m, status, NULL) != 0) fail("no match: points");
  for (int i = 0; i < N; i++)
    if (status[i] != 0) fail("no match: status");

  /* malformed: matches past n2 and negative octaves */
  for (int i = 0; i < N; i++) m[i] = i % 2 ? N + i : i;
  a->kps[0].octave = -1;
  a->kps[2].octave = 8;
  run(&a->kf, &b->kf, m, status, NULL);
  if (status[1] != NP_MALFORMED || status[0] != NP_MALFORMED || status[2] != NP_MALFORMED)
    fail("malformed");

  /* stereo keypoints without a depth */
  make_frame(a, 0.0f, 1);
  make_frame(b, 0.01f, 0);
  for (int i = 0; i < N; i++) {
    m[i] = i;
    a->depth[i] = i % 2 ? 0.0f : -3.0f;
  }
  run(&a->kf, &b->kf, m, status, NULL);

  /* NaN and infinite poses and cameras (a NaN error passes `>`, as in the reference) */
  make_frame(a, 0.0f, 3);
  make_frame(b, 0.8f, 2);
  a->kf.tcw[1] = NAN;
  run(&a->kf, &b->kf, m, status, NULL);
  make_frame(a, 0.0f, 3);
  b->kf.Rcw[4] = INFINITY;
  b->kf.fx = 0.0f;
  run(&a->kf, &b->kf, m, status, NULL);
  for (int i = 0; i < 9; i++) a->kf.Rcw[i] = NAN, b->kf.Rcw[i] = NAN;
  if (run(&a->kf, &b->kf, m, status, NULL) != 0) fail("NaN rotations");

  /* x3D(3) == 0: rotation blocks with a zero third column */
  make_frame(a, 0.0f, 0);
  make_frame(b, 0.0f, 0);
  memset(a->kf.Rcw, 0, sizeof(a->kf.Rcw));
  memset(b->kf.Rcw, 0, sizeof(b->kf.Rcw));
  a->kf.Rcw[0] = a->kf.Rcw[4] = 1.0f, a->kf.Rcw[7] = 0.5f;
  b->kf.Rcw[0] = b->kf.Rcw[4] = 1.0f, b->kf.Rcw[6] = 0.5f;
  a->kf.tcw[0] = 0.0f, a->kf.tcw[2] = 1.0f;
  b->kf.tcw[0] = 1.0f, b->kf.tcw[2] = 1.0f;
  for (int i = 0; i < N; i++) {
    a->kps[i].x = b->kps[i].x = 600.0f + 140.0f;
    a->kps[i].y = b->kps[i].y = 180.0f + 70.0f;
  }
  run(&a->kf, &b->kf, m, status, NULL);
  for (int i = 0; i < N; i++)
    if (status[i] != NP_W_ZERO) fail("w == 0");

  /* an empty keyframe */
  a->kf.n = 0;
  np_fuse_point p;
  np_new_point q;
  int32_t n_new = 0;
  np_pair(&a->kf, &b->kf, m, 0, scale, sigma2, 8, scale[1], 0, 0, NP_SWEEPS, &p, &q, &n_new, status,
          NULL);
  if (n_new != 0) fail("empty keyframe");
  free(a);
  free(b);
  printf("ok\n");
  return 0;
}
