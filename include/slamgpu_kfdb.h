/*
 * slamgpu_kfdb.h -- C ABI of the place-recognition database (libslamgpu.so). Drop-in for (paths
 * relative to the reference repository root):
 *   KeyframeDatabase (src/data/keyframe_database.cpp): add :10-18, erase :20-40, Clear :42-45,
 *     DetectLoopCandidates :48-176 (caller LoopCloser::DetectLoop, src/core/loop_closer.cpp:224,
 *     with the min_score loop of :213-221), DetectRelocalizationCandidates :179-299 (caller
 *     Tracker::Relocalization, tracker.cpp:832).
 * TemplatedVocabulary::score is slamgpu_bow_score in slamgpu_bow.h.
 *
 * There is no inverted file. The reference lists a keyframe in lKFsSharingWords at the first query
 * word (ascending word id) it shares, and inside one word's list in the order of the add() calls
 * (erase() takes an entry out without disturbing the others), so the reference's order is the
 * order of the key (smallest word id shared with the query, add sequence number).
 *
 * A keyframe's slot is its id (KeyFrame::Id(), a dense counter): 0 <= kf_id < max_keyframes.
 * All device tables are allocated by slamgpu_kfdb_create; no later call allocates.
 *
 * Conventions as slamgpu_bow.h: POD types, 0 or a negative SLAMGPU_E* code with the message in
 * slamgpu_kfdb_last_error() (per thread). A call that returns an error has written nothing.
 *
 * Threads. The reference guards the database with a mutex (tracking queries it while loop closing
 * adds and local mapping erases). Here:
 *   - every synchronous call takes a mutex owned by the handle for the whole call, stages through
 *     the calling thread's buffer and stream and returns after synchronising once, at the end;
 *   - the *_device calls take no lock, never allocate, launch on the caller's stream and return
 *     without synchronising. Ordering between them (and against synchronous calls on the same
 *     handle) is the caller's responsibility: one stream, or events. The argument checks of add
 *     ("already listed", "no BoW vector") follow the order of the calls on the host.
 *
 * Assumptions stated: query ids are unique and non-zero, so "mnLoopQuery == pKF->Id()" and
 * "mnRelocQuery == frame.Id()" reduce to "in this query's sharing list". BoW values are finite.
 * mRelocScore, which the reference leaves uninitialised (keyframe.h:119), is 0.0f for a keyframe
 * that no relocalisation query has scored yet; clear() does not reset it (Clear() does not either).
 */
#ifndef SLAMGPU_KFDB_H_
#define SLAMGPU_KFDB_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu_bow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GetBestCovisibilityKeyFrames(10) (keyframe_database.cpp:133, :258). */
#define SLAMGPU_KFDB_MAX_NEIGHBOURS 10
/* Most keyframes one query can put in lScoreAndMatch (the select kernel sorts them in LDS). A
 * query with more leaves *n_candidates = -1; the synchronous forms return SLAMGPU_EDEVICE. */
#define SLAMGPU_KFDB_MAX_SCORED 4096

typedef struct slamgpu_kfdb slamgpu_kfdb;

const char* slamgpu_kfdb_last_error(void);

/* 1 <= max_keyframes, 1 <= max_words <= SLAMGPU_BOW_MAX_FEATURES. */
int slamgpu_kfdb_create(int device, int max_keyframes, int max_words, slamgpu_kfdb** out);
void slamgpu_kfdb_destroy(slamgpu_kfdb* db);

/* What KeyFrame::ComputeBoW leaves: the keyframe's BowVector (ascending word ids). The device
 * form takes a device count pointer, so it can point straight at one set of
 * slamgpu_bow_transform_device outputs; a count above max_words is cut there (the host form
 * returns SLAMGPU_EINVAL). */
int slamgpu_kfdb_set_bow(slamgpu_kfdb* db, int kf_id, const uint32_t* words, const double* values,
                         int n);
int slamgpu_kfdb_set_bow_device(slamgpu_kfdb* db, int kf_id, const uint32_t* d_words,
                                const double* d_values, const int32_t* d_n, void* stream);

/* The keyframe's GetBestCovisibilityKeyFrames(10), in order, n <= 10. The caller refreshes it
 * where UpdateBestCovisibles changes the list. */
int slamgpu_kfdb_set_covisible(slamgpu_kfdb* db, int kf_id, const int32_t* ids, int n);
int slamgpu_kfdb_set_covisible_device(slamgpu_kfdb* db, int kf_id, const int32_t* d_ids, int n,
                                      void* stream);

/* add: the keyframe gets the next add sequence number (host counter, from 1; 0 = not listed).
 * SLAMGPU_EINVAL for a listed keyframe or one without a BoW vector. erase zeroes the number
 * (nothing to do for an unlisted keyframe); add after erase puts the keyframe at the back.
 * clear unlists every keyframe (BoW vectors, neighbour lists and mRelocScore stay). */
int slamgpu_kfdb_add(slamgpu_kfdb* db, int kf_id);
int slamgpu_kfdb_erase(slamgpu_kfdb* db, int kf_id);
int slamgpu_kfdb_clear(slamgpu_kfdb* db);
int slamgpu_kfdb_add_device(slamgpu_kfdb* db, int kf_id, void* stream);
int slamgpu_kfdb_erase_device(slamgpu_kfdb* db, int kf_id, void* stream);
int slamgpu_kfdb_clear_device(slamgpu_kfdb* db, void* stream);

/* Scratch of one detect call on this database (either kind). */
size_t slamgpu_kfdb_detect_scratch_bytes(const slamgpu_kfdb* db);

/* DetectLoopCandidates(pKF = keyframe kf_id, minScore) with minScore as LoopCloser::DetectLoop
 * computes it (loop_closer.cpp:214-221): float, from 1, std::min over `covisible`
 * (GetVectorCovisibleKeyFrames() with bad keyframes already dropped; they need a BoW vector but
 * need not be listed). `connected` = GetConnectedKeyFrames(). Both lists hold at most
 * max_keyframes ids; an id outside [0, max_keyframes) is skipped.
 * Outputs: *min_score, candidates[max_keyframes] in the reference's order, *n_candidates.
 * Optional diagnostics, [max_keyframes] each, either may be NULL: common_words = mnLoopWords
 * (-1 for a keyframe that is not listed or is connected), scores = mLoopScore of the keyframes
 * this query scored and 0 for the others (the loop variant never reads a score of an earlier
 * query, so it keeps none). */
int slamgpu_kfdb_detect_loop_candidates(slamgpu_kfdb* db, int kf_id, const int32_t* connected,
                                        int n_connected, const int32_t* covisible, int n_covisible,
                                        float* min_score, int32_t* candidates, int* n_candidates,
                                        int32_t* common_words, float* scores);
int slamgpu_kfdb_detect_loop_candidates_device(slamgpu_kfdb* db, int kf_id,
                                               const int32_t* d_connected, int n_connected,
                                               const int32_t* d_covisible, int n_covisible,
                                               float* d_min_score, int32_t* d_candidates,
                                               int32_t* d_n_candidates, int32_t* d_common_words,
                                               float* d_scores, void* d_scratch, void* stream);

/* DetectRelocalizationCandidates(frame) for the frame's BowVector (a Frame is no keyframe).
 * scores = mRelocScore of every slot after the query: what this query or an earlier one left
 * (keyframe_database.cpp:264-272 reads the earlier ones), 0.0f if never scored. */
int slamgpu_kfdb_detect_relocalization_candidates(slamgpu_kfdb* db, const uint32_t* words,
                                                  const double* values, int n,
                                                  int32_t* candidates, int* n_candidates,
                                                  int32_t* common_words, float* scores);
int slamgpu_kfdb_detect_relocalization_candidates_device(
    slamgpu_kfdb* db, const uint32_t* d_words, const double* d_values, const int32_t* d_n,
    int32_t* d_candidates, int32_t* d_n_candidates, int32_t* d_common_words, float* d_scores,
    void* d_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_KFDB_H_ */
