/* kfdb_sanitizer_check.c -- tests/kfdb_ref.c under -fsanitize=address,undefined as a stand-alone
 * program (tests/test_kfdb_ref.py builds and runs it): empty vectors, a query with no listed
 * keyframe, neighbour / connected / covisible ids out of range, n_covisible = 0, erase of an
 * unlisted keyframe, Clear and re-add. */
#include <stdio.h>

#include "kfdb_ref.c"

#define MAX_KF 8
#define CHECK(c)                                        \
  do {                                                  \
    if (!(c)) {                                         \
      printf("line %d: %s failed\n", __LINE__, #c);     \
      return 1;                                         \
    }                                                   \
  } while (0)

int main(void) {
  kr_db* db = kr_create(MAX_KF, 64);
  int32_t cand[MAX_KF], words[MAX_KF];
  float scores[MAX_KF], ms = -1;
  const uint32_t w8[8] = {1, 2, 3, 5, 8, 13, 21, 34};
  const double v8[8] = {0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125};

  /* empty vectors on both sides of the score */
  CHECK(kr_score(NULL, NULL, 0, NULL, NULL, 0) == 0);
  CHECK(kr_score(w8, v8, 8, NULL, NULL, 0) == 0);
  CHECK(kr_score(w8, v8, 8, w8, v8, 8) == 1.0);

  /* an empty database, an empty query keyframe, n_covisible = 0 */
  kr_set_bow(db, 0, NULL, NULL, 0);
  CHECK(kr_detect_loop(db, 0, NULL, 0, NULL, 0, &ms, cand, words, scores) == 0 && ms == 1.0f);
  CHECK(kr_detect_reloc(db, NULL, NULL, 0, cand, words, scores) == 0);
  kr_add(db, 0); /* a listed keyframe without a word */
  CHECK(kr_detect_reloc(db, w8, v8, 8, cand, NULL, NULL) == 0);

  /* a query with vectors around but no listed keyframe sharing a word */
  kr_set_bow(db, 1, w8, v8, 8);
  kr_set_bow(db, 2, w8, v8, 8);
  CHECK(kr_detect_loop(db, 1, NULL, 0, NULL, 0, &ms, cand, words, scores) == 0);
  CHECK(words[1] == -1 && words[0] == 0);

  /* neighbour, connected and covisible ids out of range */
  const int32_t odd[6] = {-1, MAX_KF, 1000, 2, 1, -2147483647 - 1};
  kr_set_covisible(db, 1, odd, 6);
  kr_set_covisible(db, 2, odd, 6);
  kr_add(db, 1);
  kr_add(db, 2);
  kr_set_bow(db, 3, w8, v8, 4);
  CHECK(kr_detect_loop(db, 3, odd, 3, odd, 6, &ms, cand, words, scores) == 2);
  CHECK(cand[0] == 1 && cand[1] == 2);
  CHECK(ms == 0.5f && words[1] == 4 && words[2] == 4 && scores[2] == 0.5f);
  CHECK(kr_detect_reloc(db, w8, v8, 8, cand, words, scores) == 2 && cand[1] == 2);
  CHECK(kr_detect_loop(db, 3, odd + 3, 2, NULL, 0, &ms, cand, words, scores) == 0 && ms == 1.0f);

  /* erase of an unlisted keyframe, erase, Clear, re-add */
  kr_erase(db, 4);
  kr_erase(db, 1);
  CHECK(kr_detect_reloc(db, w8, v8, 8, cand, words, scores) == 1 && cand[0] == 2);
  kr_clear(db);
  CHECK(kr_detect_reloc(db, w8, v8, 8, cand, words, scores) == 0 && words[2] == -1);
  kr_add(db, 1);
  CHECK(kr_detect_reloc(db, w8, v8, 8, cand, words, scores) == 1 && cand[0] == 1);
  kr_destroy(db);
  printf("kfdb_sanitizer_check ok\n");
  return 0;
}
