/* kfdb_ref.c -- CPU restatement of KeyframeDatabase (src/data/keyframe_database.cpp), of
 * L1Scoring::score (third_party/DBoW2/DBoW2/ScoringObject.cpp:23-68) and of the min_score loop of
 * LoopCloser::DetectLoop (src/core/loop_closer.cpp:214-221), stated literally: one insertion-
 * ordered list per word, add / erase / Clear on those lists, per-keyframe mnLoopQuery / Words /
 * Score and mnRelocQuery / Words / Score, the lower_bound walk of the score. It does not know the
 * ordering key (smallest shared word, add sequence) of include/slamgpu_kfdb.h: it is the
 * independent statement the key is checked against.
 *
 * Declared where the reference has no answer: mLoopScore and mRelocScore start at 0.0f (the
 * reference leaves them uninitialised, keyframe.h:119); a neighbour / connected / covisible id
 * outside [0, max_kf) is skipped (the reference holds pointers); every query gets a fresh non-zero
 * query id (the reference uses KeyFrame::Id() / Frame::Id(), unique per query).
 * Diagnostics after a query: words[k] = -1 for a keyframe that is not listed or is connected,
 * else mnXWords of this query (0 if it shares nothing); scores[k] = mLoopScore if scored by this
 * query else 0 (loop), mRelocScore as it stands (relocalisation). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct node {
  int kf;
  struct node* next;
} node;

typedef struct {
  uint32_t* words;
  double* values;
  int n;
  int covis[10];
  int n_covis;
  int in_lists; /* add() without a later erase() / Clear() */
  long mnLoopQuery, mnRelocQuery;
  int mnLoopWords, mnRelocWords;
  float mLoopScore, mRelocScore;
} keyframe;

typedef struct {
  int max_kf, n_vocab;
  keyframe* kf;
  node** head; /* mvInvertedFile[word]: std::list<KeyFrame*> in push_back order */
  node** tail;
  long next_query;
} kr_db;

kr_db* kr_create(int max_kf, int n_vocab) {
  kr_db* db = calloc(1, sizeof(kr_db));
  db->max_kf = max_kf;
  db->n_vocab = n_vocab;
  db->kf = calloc((size_t)max_kf, sizeof(keyframe));
  db->head = calloc((size_t)n_vocab, sizeof(node*));
  db->tail = calloc((size_t)n_vocab, sizeof(node*));
  db->next_query = 1;
  return db;
}

void kr_clear(kr_db* db) { /* :42-45 */
  for (int w = 0; w < db->n_vocab; w++) {
    node* p = db->head[w];
    while (p) {
      node* q = p->next;
      free(p);
      p = q;
    }
    db->head[w] = db->tail[w] = NULL;
  }
  for (int k = 0; k < db->max_kf; k++) db->kf[k].in_lists = 0;
}

void kr_destroy(kr_db* db) {
  if (!db) return;
  kr_clear(db);
  for (int k = 0; k < db->max_kf; k++) {
    free(db->kf[k].words);
    free(db->kf[k].values);
  }
  free(db->kf);
  free(db->head);
  free(db->tail);
  free(db);
}

void kr_set_bow(kr_db* db, int k, const uint32_t* words, const double* values, int n) {
  keyframe* f = &db->kf[k];
  free(f->words);
  free(f->values);
  f->words = malloc(sizeof(uint32_t) * (size_t)(n > 0 ? n : 1));
  f->values = malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
  if (n > 0) {
    memcpy(f->words, words, sizeof(uint32_t) * (size_t)n);
    memcpy(f->values, values, sizeof(double) * (size_t)n);
  }
  f->n = n;
}

void kr_set_covisible(kr_db* db, int k, const int32_t* ids, int n) {
  db->kf[k].n_covis = n;
  for (int i = 0; i < n; i++) db->kf[k].covis[i] = ids[i];
}

void kr_add(kr_db* db, int k) { /* :10-18 */
  const keyframe* f = &db->kf[k];
  for (int i = 0; i < f->n; i++) {
    const uint32_t w = f->words[i];
    node* p = malloc(sizeof(node));
    p->kf = k;
    p->next = NULL;
    if (db->tail[w]) db->tail[w]->next = p; else db->head[w] = p;
    db->tail[w] = p;
  }
  db->kf[k].in_lists = 1;
}

void kr_erase(kr_db* db, int k) { /* :20-40 */
  const keyframe* f = &db->kf[k];
  for (int i = 0; i < f->n; i++) {
    const uint32_t w = f->words[i];
    node *prev = NULL, *p = db->head[w];
    for (; p; prev = p, p = p->next)
      if (p->kf == k) {
        if (prev) prev->next = p->next; else db->head[w] = p->next;
        if (db->tail[w] == p) db->tail[w] = prev;
        free(p);
        break;
      }
  }
  db->kf[k].in_lists = 0;
}

/* std::map::lower_bound from position `from` on */
static int lower_bound_from(const uint32_t* w, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (w[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

double kr_score(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2,
                int n2) { /* ScoringObject.cpp:23-68 */
  int i1 = 0, i2 = 0;
  double score = 0;
  while (i1 != n1 && i2 != n2) {
    const double vi = v1[i1];
    const double wi = v2[i2];
    if (w1[i1] == w2[i2]) {
      score += fabs(vi - wi) - fabs(vi) - fabs(wi);
      ++i1;
      ++i2;
    } else if (w1[i1] < w2[i2]) {
      i1 = lower_bound_from(w1, n1, w2[i2]);
    } else {
      i2 = lower_bound_from(w2, n2, w1[i1]);
    }
  }
  score = -score / 2.0;
  return score;
}

static int in_range(const kr_db* db, int k) { return k >= 0 && k < db->max_kf; }

/* candidates[max_kf]; words_out / scores_out [max_kf] or NULL. Returns the candidate count. */
int kr_detect_loop(kr_db* db, int q, const int32_t* connected, int n_connected,
                   const int32_t* covisible, int n_covisible, float* min_score_out,
                   int32_t* candidates, int32_t* words_out, float* scores_out) {
  const long qid = db->next_query++;
  const keyframe* pKF = &db->kf[q];
  int n_out = 0;
  /* loop_closer.cpp:214-221 */
  float min_score = 1;
  for (int i = 0; i < n_covisible; i++) {
    if (!in_range(db, covisible[i])) continue;
    const keyframe* c = &db->kf[covisible[i]];
    const float score = (float)kr_score(pKF->words, pKF->values, pKF->n, c->words, c->values, c->n);
    min_score = (score < min_score) ? score : min_score; /* std::min(min_score, score) */
  }
  *min_score_out = min_score;
  const float minScore = min_score;

  uint8_t* is_connected = calloc((size_t)db->max_kf, 1); /* spConnectedKeyFrames */
  for (int i = 0; i < n_connected; i++)
    if (in_range(db, connected[i])) is_connected[connected[i]] = 1;
  int* sharing = malloc(sizeof(int) * (size_t)db->max_kf); /* lKFsSharingWords */
  int n_sharing = 0;
  for (int i = 0; i < pKF->n; i++) /* :58-78 */
    for (node* p = db->head[pKF->words[i]]; p; p = p->next) {
      keyframe* f = &db->kf[p->kf];
      if (f->mnLoopQuery != qid) {
        f->mnLoopWords = 0;
        if (!is_connected[p->kf]) {
          f->mnLoopQuery = qid;
          sharing[n_sharing++] = p->kf;
        }
      }
      ++f->mnLoopWords;
    }
  int minCommonWords = 0;
  int* sam_kf = malloc(sizeof(int) * (size_t)db->max_kf); /* lScoreAndMatch */
  float* sam_score = malloc(sizeof(float) * (size_t)db->max_kf);
  float* acc_score = malloc(sizeof(float) * (size_t)db->max_kf); /* lAccScoreAndMatch */
  int* acc_kf = malloc(sizeof(int) * (size_t)db->max_kf);
  uint8_t* added = calloc((size_t)db->max_kf, 1); /* spAlreadyAddedKF */
  int n_sam = 0;
  if (n_sharing == 0) goto done; /* :81-83 */
  {
    int maxCommonWords = 0; /* :88-98 */
    for (int i = 0; i < n_sharing; i++)
      if (db->kf[sharing[i]].mnLoopWords > maxCommonWords)
        maxCommonWords = db->kf[sharing[i]].mnLoopWords;
    minCommonWords = (int)(maxCommonWords * 0.8f);
  }
  for (int i = 0; i < n_sharing; i++) { /* :102-114 */
    keyframe* f = &db->kf[sharing[i]];
    if (f->mnLoopWords > minCommonWords) {
      f->mLoopScore = (float)kr_score(pKF->words, pKF->values, pKF->n, f->words, f->values, f->n);
      if (f->mLoopScore >= minScore) {
        sam_score[n_sam] = f->mLoopScore;
        sam_kf[n_sam++] = sharing[i];
      }
    }
  }
  if (n_sam == 0) goto done; /* :116-118 */
  {
    float bestAccScore = minScore; /* :121-153 */
    for (int i = 0; i < n_sam; i++) {
      const keyframe* f = &db->kf[sam_kf[i]];
      float bestScore = sam_score[i];
      float accScore = sam_score[i];
      int pBestKF = sam_kf[i];
      for (int j = 0; j < f->n_covis; j++) {
        if (!in_range(db, f->covis[j])) continue;
        const keyframe* f2 = &db->kf[f->covis[j]];
        if (f2->mnLoopQuery == qid && f2->mnLoopWords > minCommonWords) {
          accScore += f2->mLoopScore;
          if (f2->mLoopScore > bestScore) {
            pBestKF = f->covis[j];
            bestScore = f2->mLoopScore;
          }
        }
      }
      acc_score[i] = accScore;
      acc_kf[i] = pBestKF;
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    const float minScoreToRetain = 0.75f * bestAccScore; /* :156-173 */
    for (int i = 0; i < n_sam; i++)
      if (acc_score[i] > minScoreToRetain && !added[acc_kf[i]]) {
        candidates[n_out++] = acc_kf[i];
        added[acc_kf[i]] = 1;
      }
  }
done:
  for (int k = 0; k < db->max_kf; k++) {
    const keyframe* f = &db->kf[k];
    const int shared = f->mnLoopQuery == qid;
    if (words_out) words_out[k] = (!f->in_lists || is_connected[k]) ? -1 : (shared ? f->mnLoopWords : 0);
    if (scores_out)
      scores_out[k] = (n_sharing > 0 && shared && f->mnLoopWords > minCommonWords) ? f->mLoopScore : 0.0f;
  }
  free(is_connected);
  free(sharing);
  free(sam_kf);
  free(sam_score);
  free(acc_score);
  free(acc_kf);
  free(added);
  return n_out;
}

int kr_detect_reloc(kr_db* db, const uint32_t* words, const double* values, int n,
                    int32_t* candidates, int32_t* words_out, float* scores_out) {
  const long qid = db->next_query++;
  int n_out = 0;
  int* sharing = malloc(sizeof(int) * (size_t)db->max_kf);
  int n_sharing = 0;
  for (int i = 0; i < n; i++) /* :186-203 */
    for (node* p = db->head[words[i]]; p; p = p->next) {
      keyframe* f = &db->kf[p->kf];
      if (f->mnRelocQuery != qid) {
        f->mnRelocWords = 0;
        f->mnRelocQuery = qid;
        sharing[n_sharing++] = p->kf;
      }
      ++f->mnRelocWords;
    }
  int* sam_kf = malloc(sizeof(int) * (size_t)db->max_kf);
  float* sam_score = malloc(sizeof(float) * (size_t)db->max_kf);
  float* acc_score = malloc(sizeof(float) * (size_t)db->max_kf);
  int* acc_kf = malloc(sizeof(int) * (size_t)db->max_kf);
  uint8_t* added = calloc((size_t)db->max_kf, 1);
  int n_sam = 0;
  if (n_sharing == 0) goto done; /* :206-208 */
  int minCommonWords;
  {
    int maxCommonWords = 0; /* :212-222 */
    for (int i = 0; i < n_sharing; i++)
      if (db->kf[sharing[i]].mnRelocWords > maxCommonWords)
        maxCommonWords = db->kf[sharing[i]].mnRelocWords;
    minCommonWords = (int)(maxCommonWords * 0.8f);
  }
  for (int i = 0; i < n_sharing; i++) { /* :227-238 */
    keyframe* f = &db->kf[sharing[i]];
    if (f->mnRelocWords > minCommonWords) {
      f->mRelocScore = (float)kr_score(words, values, n, f->words, f->values, f->n);
      sam_score[n_sam] = f->mRelocScore;
      sam_kf[n_sam++] = sharing[i];
    }
  }
  if (n_sam == 0) goto done; /* :240-242 */
  {
    float bestAccScore = 0; /* :244-278 */
    for (int i = 0; i < n_sam; i++) {
      const keyframe* f = &db->kf[sam_kf[i]];
      float bestScore = sam_score[i];
      float accScore = bestScore;
      int pBestKF = sam_kf[i];
      for (int j = 0; j < f->n_covis; j++) {
        if (!in_range(db, f->covis[j])) continue;
        const keyframe* f2 = &db->kf[f->covis[j]];
        if (f2->mnRelocQuery != qid) continue;
        accScore += f2->mRelocScore;
        if (f2->mRelocScore > bestScore) {
          pBestKF = f->covis[j];
          bestScore = f2->mRelocScore;
        }
      }
      acc_score[i] = accScore;
      acc_kf[i] = pBestKF;
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    const float minScoreToRetain = 0.75f * bestAccScore; /* :281-297 */
    for (int i = 0; i < n_sam; i++)
      if (acc_score[i] > minScoreToRetain && !added[acc_kf[i]]) {
        candidates[n_out++] = acc_kf[i];
        added[acc_kf[i]] = 1;
      }
  }
done:
  for (int k = 0; k < db->max_kf; k++) {
    const keyframe* f = &db->kf[k];
    if (words_out) words_out[k] = !f->in_lists ? -1 : (f->mnRelocQuery == qid ? f->mnRelocWords : 0);
    if (scores_out) scores_out[k] = f->mRelocScore;
  }
  free(sharing);
  free(sam_kf);
  free(sam_score);
  free(acc_score);
  free(acc_kf);
  free(added);
  return n_out;
}
