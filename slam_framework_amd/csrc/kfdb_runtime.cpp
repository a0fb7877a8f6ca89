// kfdb_runtime.cpp -- host side of include/slamgpu_kfdb.h: the handle (device tables allocated
// once, the add sequence counter and the host's record of which slots hold a BoW vector / are
// listed, the mutex of the synchronous calls), the *_device calls (validate, launch on the
// caller's stream, never allocate) and the synchronous forms, which stage through the calling
// thread's buffer and stream (host_stage.h), run the *_device form there and synchronise once.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/slamgpu_kfdb.h"
#include "host_stage.h"
#include "kfdb_kernels.h"
#include "stage_layout.h"

using namespace slamgpu;

static_assert(SLAMGPU_KFDB_MAX_NEIGHBOURS == kKfdbNeighbours, "neighbour count");
static_assert(SLAMGPU_KFDB_MAX_SCORED == kKfdbMaxScored, "select capacity");
static_assert(SLAMGPU_BOW_MAX_FEATURES == kKfdbMaxQuery, "query capacity");

struct slamgpu_kfdb {
  int device = 0;
  KfdbDev d{};
  uint32_t next_seq = 1;          // add() hands these out
  std::vector<uint8_t> has_bow;   // set_bow was called for the slot
  std::vector<uint8_t> listed;    // add() without a later erase() / clear()
  std::mutex mutex;               // held by every synchronous call
};

namespace {

int check_db(const slamgpu_kfdb* db) {
  return db ? 0 : t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL database");
}
int check_id(const slamgpu_kfdb* db, int kf_id) {
  if (int r = check_db(db)) return r;
  if (kf_id < 0 || kf_id >= db->d.max_kf)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "kf_id %d outside [0, %d)", kf_id, db->d.max_kf);
  return 0;
}

void release(slamgpu_kfdb* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  void* tables[] = {db->d.words, db->d.values, db->d.n_words, db->d.seq,
                    db->d.covis, db->d.n_covis, db->d.reloc_score};
  for (void* p : tables)
    if (p) (void)hipFree(p);
  delete db;
}

// Runs one synchronous call: the handle's mutex, the thread's stage on the database's device.
struct SyncCall {
  std::unique_lock<std::mutex> lock;
  StageLease S;
  explicit SyncCall(slamgpu_kfdb* db) : lock(db->mutex), S(t_kfdb_err) {}
};

int add_checked(slamgpu_kfdb* db, int kf_id) {
  if (int r = check_id(db, kf_id)) return r;
  if (!db->has_bow[kf_id])
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "add: keyframe %d has no BoW vector", kf_id);
  if (db->listed[kf_id])
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "add: keyframe %d is already listed", kf_id);
  return 0;
}

int check_loop_args(const slamgpu_kfdb* db, int kf_id, const void* connected, int n_connected,
                    const void* covisible, int n_covisible, const void* min_score,
                    const void* candidates, const void* n_candidates) {
  if (int r = check_id(db, kf_id)) return r;
  if (n_connected < 0 || n_connected > db->d.max_kf || n_covisible < 0 ||
      n_covisible > db->d.max_kf)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "n_connected %d / n_covisible %d outside [0, %d]",
                           n_connected, n_covisible, db->d.max_kf);
  if ((n_connected > 0 && !connected) || (n_covisible > 0 && !covisible) || !min_score ||
      !candidates || !n_candidates)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL argument");
  return 0;
}

}  // namespace

extern "C" {

const char* slamgpu_kfdb_last_error(void) { return t_kfdb_err.c_str(); }

int slamgpu_kfdb_create(int device, int max_keyframes, int max_words, slamgpu_kfdb** out) {
  if (!out) return t_kfdb_err.fail(SLAMGPU_EINVAL, "out is NULL");
  *out = nullptr;
  if (max_keyframes < 1 || max_words < 1 || max_words > SLAMGPU_BOW_MAX_FEATURES)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "max_keyframes %d < 1 or max_words %d outside [1, %d]",
                           max_keyframes, max_words, SLAMGPU_BOW_MAX_FEATURES);
  slamgpu_kfdb* db = new slamgpu_kfdb();
  db->device = device;
  db->d.max_kf = max_keyframes;
  db->d.max_words = max_words;
  db->has_bow.assign(max_keyframes, 0);
  db->listed.assign(max_keyframes, 0);
  const size_t n = (size_t)max_keyframes, nw = n * (size_t)max_words;
  auto fail = [&](hipError_t e) {
    release(db);
    return t_kfdb_err.fail(SLAMGPU_EHIP, "kfdb_create: %s", hipGetErrorString(e));
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(e);
  struct { void** p; size_t bytes; } tables[] = {
      {(void**)&db->d.words, nw * 4}, {(void**)&db->d.values, nw * 8},
      {(void**)&db->d.n_words, n * 4}, {(void**)&db->d.seq, n * 4},
      {(void**)&db->d.covis, n * kKfdbNeighbours * 4}, {(void**)&db->d.n_covis, n * 4},
      {(void**)&db->d.reloc_score, n * 4}};
  for (auto& t : tables) {
    if ((e = hipMalloc(t.p, t.bytes)) != hipSuccess) return fail(e);
    if ((e = hipMemset(*t.p, 0, t.bytes)) != hipSuccess) return fail(e);
  }
  if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(e);
  *out = db;
  return 0;
}

void slamgpu_kfdb_destroy(slamgpu_kfdb* db) { release(db); }

// ---- set_bow / set_covisible ----------------------------------------------------------------
int slamgpu_kfdb_set_bow_device(slamgpu_kfdb* db, int kf_id, const uint32_t* d_words,
                                const double* d_values, const int32_t* d_n, void* stream) {
  if (int r = check_id(db, kf_id)) return r;
  if (!d_words || !d_values || !d_n) return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  HIPCHECK(t_kfdb_err, launch_kfdb_set_bow(db->d, kf_id, d_words, d_values, d_n,
                                           static_cast<hipStream_t>(stream)));
  db->has_bow[kf_id] = 1;
  return 0;
}

int slamgpu_kfdb_set_bow(slamgpu_kfdb* db, int kf_id, const uint32_t* words, const double* values,
                         int n) {
  if (int r = check_id(db, kf_id)) return r;
  if (n < 0 || n > db->d.max_words)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "set_bow: n %d outside [0, max_words %d]", n,
                           db->d.max_words);
  if (n > 0 && (!words || !values)) return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL buffer");
  for (int i = 1; i < n; i++)
    if (words[i] <= words[i - 1])
      return t_kfdb_err.fail(SLAMGPU_EINVAL, "set_bow: words not strictly ascending at %d", i);
  SyncCall c(db);
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  StageLayout L;
  const KfdbVecLayout l = layout_kfdb_vec(L, n);
  if (int r = c.S.reserve(L.size())) return r;
  const int32_t cnt = n;
  HIPCHECK(t_kfdb_err, c.S.upload(l.words, words, (size_t)n * 4));
  HIPCHECK(t_kfdb_err, c.S.upload(l.values, values, (size_t)n * 8));
  HIPCHECK(t_kfdb_err, c.S.upload(l.n, &cnt, 4));
  if (int r = slamgpu_kfdb_set_bow_device(db, kf_id, c.S.at<uint32_t>(l.words),
                                          c.S.at<double>(l.values), c.S.at<int32_t>(l.n),
                                          c.S.stream()))
    return r;
  HIPCHECK(t_kfdb_err, hipStreamSynchronize(c.S.stream()));
  return 0;
}

int slamgpu_kfdb_set_covisible_device(slamgpu_kfdb* db, int kf_id, const int32_t* d_ids, int n,
                                      void* stream) {
  if (int r = check_id(db, kf_id)) return r;
  if (n < 0 || n > SLAMGPU_KFDB_MAX_NEIGHBOURS)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "set_covisible: n %d outside [0, %d]", n,
                           SLAMGPU_KFDB_MAX_NEIGHBOURS);
  if (n > 0 && !d_ids) return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  HIPCHECK(t_kfdb_err, launch_kfdb_set_covisible(db->d, kf_id, d_ids, n,
                                                 static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_kfdb_set_covisible(slamgpu_kfdb* db, int kf_id, const int32_t* ids, int n) {
  if (int r = check_id(db, kf_id)) return r;
  if (n < 0 || n > SLAMGPU_KFDB_MAX_NEIGHBOURS)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "set_covisible: n %d outside [0, %d]", n,
                           SLAMGPU_KFDB_MAX_NEIGHBOURS);
  if (n > 0 && !ids) return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL buffer");
  SyncCall c(db);
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  StageLayout L;
  const size_t at = L.take<int32_t>(SLAMGPU_KFDB_MAX_NEIGHBOURS);
  if (int r = c.S.reserve(L.size())) return r;
  HIPCHECK(t_kfdb_err, c.S.upload(at, ids, (size_t)n * 4));
  if (int r = slamgpu_kfdb_set_covisible_device(db, kf_id, c.S.at<int32_t>(at), n, c.S.stream()))
    return r;
  HIPCHECK(t_kfdb_err, hipStreamSynchronize(c.S.stream()));
  return 0;
}

// ---- add / erase / clear -------------------------------------------------------------------
int slamgpu_kfdb_add_device(slamgpu_kfdb* db, int kf_id, void* stream) {
  if (int r = add_checked(db, kf_id)) return r;
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  HIPCHECK(t_kfdb_err, launch_kfdb_set_seq(db->d, kf_id, db->next_seq,
                                           static_cast<hipStream_t>(stream)));
  db->next_seq++;
  db->listed[kf_id] = 1;
  return 0;
}

int slamgpu_kfdb_erase_device(slamgpu_kfdb* db, int kf_id, void* stream) {
  if (int r = check_id(db, kf_id)) return r;
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  HIPCHECK(t_kfdb_err, launch_kfdb_set_seq(db->d, kf_id, 0u, static_cast<hipStream_t>(stream)));
  db->listed[kf_id] = 0;
  return 0;
}

int slamgpu_kfdb_clear_device(slamgpu_kfdb* db, void* stream) {
  if (int r = check_db(db)) return r;
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  HIPCHECK(t_kfdb_err, launch_kfdb_set_seq(db->d, -1, 0u, static_cast<hipStream_t>(stream)));
  db->listed.assign(db->listed.size(), 0);
  return 0;
}

#define KFDB_SYNC_UPDATE(check, call)                                  \
  if (int r = (check)) return r;                                       \
  SyncCall c(db);                                                      \
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));                      \
  if (int r = c.S.reserve(0)) return r;                                \
  if (int r = (call)) return r;                                        \
  HIPCHECK(t_kfdb_err, hipStreamSynchronize(c.S.stream()));            \
  return 0

int slamgpu_kfdb_add(slamgpu_kfdb* db, int kf_id) {
  KFDB_SYNC_UPDATE(check_id(db, kf_id), slamgpu_kfdb_add_device(db, kf_id, c.S.stream()));
}
int slamgpu_kfdb_erase(slamgpu_kfdb* db, int kf_id) {
  KFDB_SYNC_UPDATE(check_id(db, kf_id), slamgpu_kfdb_erase_device(db, kf_id, c.S.stream()));
}
int slamgpu_kfdb_clear(slamgpu_kfdb* db) {
  KFDB_SYNC_UPDATE(check_db(db), slamgpu_kfdb_clear_device(db, c.S.stream()));
}

// ---- detect ----------------------------------------------------------------------------------
size_t slamgpu_kfdb_detect_scratch_bytes(const slamgpu_kfdb* db) {
  return db ? kfdb_scratch_bytes(db->d.max_kf) : 0;
}

int slamgpu_kfdb_detect_loop_candidates_device(slamgpu_kfdb* db, int kf_id,
                                               const int32_t* d_connected, int n_connected,
                                               const int32_t* d_covisible, int n_covisible,
                                               float* d_min_score, int32_t* d_candidates,
                                               int32_t* d_n_candidates, int32_t* d_common_words,
                                               float* d_scores, void* d_scratch, void* stream) {
  if (int r = check_loop_args(db, kf_id, d_connected, n_connected, d_covisible, n_covisible,
                              d_min_score, d_candidates, d_n_candidates))
    return r;
  if (!d_scratch) return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL scratch");
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  const KfdbQuery q{kf_id, nullptr, nullptr, nullptr, d_connected, n_connected, d_covisible,
                    n_covisible, d_min_score, d_candidates, d_n_candidates, d_common_words,
                    d_scores};
  HIPCHECK(t_kfdb_err, launch_kfdb_detect(db->d, q, d_scratch, static_cast<hipStream_t>(stream)));
  return 0;
}

int slamgpu_kfdb_detect_relocalization_candidates_device(
    slamgpu_kfdb* db, const uint32_t* d_words, const double* d_values, const int32_t* d_n,
    int32_t* d_candidates, int32_t* d_n_candidates, int32_t* d_common_words, float* d_scores,
    void* d_scratch, void* stream) {
  if (int r = check_db(db)) return r;
  if (!d_words || !d_values || !d_n || !d_candidates || !d_n_candidates || !d_scratch)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL device buffer");
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  const KfdbQuery q{-1, d_words, d_values, d_n, nullptr, 0, nullptr, 0, nullptr, d_candidates,
                    d_n_candidates, d_common_words, d_scores};
  HIPCHECK(t_kfdb_err, launch_kfdb_detect(db->d, q, d_scratch, static_cast<hipStream_t>(stream)));
  return 0;
}

// The outputs of a staged detect call, once the stream is synchronised.
static int finish_detect(SyncCall& c, const slamgpu_kfdb* db, const KfdbDetectLayout& l,
                         float* min_score, int32_t* candidates, int* n_candidates,
                         int32_t* common_words, float* scores) {
  const size_t n = (size_t)db->d.max_kf;
  std::vector<int32_t> cand(n);
  std::vector<int32_t> cw(common_words ? n : 0);
  std::vector<float> sc(scores ? n : 0);
  float ms = 0;
  int32_t nc = 0;
  HIPCHECK(t_kfdb_err, c.S.download(&ms, l.min_score, 4));
  HIPCHECK(t_kfdb_err, c.S.download(&nc, l.n_candidates, 4));
  HIPCHECK(t_kfdb_err, c.S.download(cand.data(), l.candidates, n * 4));
  HIPCHECK(t_kfdb_err, c.S.download(cw.data(), l.common_words, cw.size() * 4));
  HIPCHECK(t_kfdb_err, c.S.download(sc.data(), l.scores, sc.size() * 4));
  HIPCHECK(t_kfdb_err, hipStreamSynchronize(c.S.stream()));
  if (nc < 0)
    return t_kfdb_err.fail(SLAMGPU_EDEVICE, "detect: more than %d scored keyframes in one query",
                           SLAMGPU_KFDB_MAX_SCORED);
  if (min_score) *min_score = ms;
  for (int i = 0; i < nc; i++) candidates[i] = cand[i];
  *n_candidates = nc;
  for (size_t i = 0; i < cw.size(); i++) common_words[i] = cw[i];
  for (size_t i = 0; i < sc.size(); i++) scores[i] = sc[i];
  return 0;
}

int slamgpu_kfdb_detect_loop_candidates(slamgpu_kfdb* db, int kf_id, const int32_t* connected,
                                        int n_connected, const int32_t* covisible, int n_covisible,
                                        float* min_score, int32_t* candidates, int* n_candidates,
                                        int32_t* common_words, float* scores) {
  if (int r = check_loop_args(db, kf_id, connected, n_connected, covisible, n_covisible, min_score,
                              candidates, n_candidates))
    return r;
  SyncCall c(db);
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  StageLayout L;
  const KfdbDetectLayout l = layout_kfdb_detect(L, db->d.max_kf, n_connected, n_covisible,
                                                kfdb_scratch_bytes(db->d.max_kf));
  if (int r = c.S.reserve(L.size())) return r;
  HIPCHECK(t_kfdb_err, c.S.upload(l.connected, connected, (size_t)n_connected * 4));
  HIPCHECK(t_kfdb_err, c.S.upload(l.covisible, covisible, (size_t)n_covisible * 4));
  if (int r = slamgpu_kfdb_detect_loop_candidates_device(
          db, kf_id, c.S.at<int32_t>(l.connected), n_connected, c.S.at<int32_t>(l.covisible),
          n_covisible, c.S.at<float>(l.min_score), c.S.at<int32_t>(l.candidates),
          c.S.at<int32_t>(l.n_candidates), common_words ? c.S.at<int32_t>(l.common_words) : nullptr,
          scores ? c.S.at<float>(l.scores) : nullptr, c.S.at<char>(l.scratch), c.S.stream()))
    return r;
  return finish_detect(c, db, l, min_score, candidates, n_candidates, common_words, scores);
}

int slamgpu_kfdb_detect_relocalization_candidates(slamgpu_kfdb* db, const uint32_t* words,
                                                  const double* values, int n,
                                                  int32_t* candidates, int* n_candidates,
                                                  int32_t* common_words, float* scores) {
  if (int r = check_db(db)) return r;
  if (n < 0 || n > SLAMGPU_BOW_MAX_FEATURES)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "n %d outside [0, %d]", n, SLAMGPU_BOW_MAX_FEATURES);
  if ((n > 0 && (!words || !values)) || !candidates || !n_candidates)
    return t_kfdb_err.fail(SLAMGPU_EINVAL, "NULL argument");
  for (int i = 1; i < n; i++)
    if (words[i] <= words[i - 1])
      return t_kfdb_err.fail(SLAMGPU_EINVAL, "words not strictly ascending at %d", i);
  SyncCall c(db);
  HIPCHECK(t_kfdb_err, hipSetDevice(db->device));
  StageLayout L;
  const KfdbVecLayout v = layout_kfdb_vec(L, n);
  const KfdbDetectLayout l =
      layout_kfdb_detect(L, db->d.max_kf, 0, 0, kfdb_scratch_bytes(db->d.max_kf));
  if (int r = c.S.reserve(L.size())) return r;
  const int32_t cnt = n;
  HIPCHECK(t_kfdb_err, c.S.upload(v.words, words, (size_t)n * 4));
  HIPCHECK(t_kfdb_err, c.S.upload(v.values, values, (size_t)n * 8));
  HIPCHECK(t_kfdb_err, c.S.upload(v.n, &cnt, 4));
  if (int r = slamgpu_kfdb_detect_relocalization_candidates_device(
          db, c.S.at<uint32_t>(v.words), c.S.at<double>(v.values), c.S.at<int32_t>(v.n),
          c.S.at<int32_t>(l.candidates), c.S.at<int32_t>(l.n_candidates),
          common_words ? c.S.at<int32_t>(l.common_words) : nullptr,
          scores ? c.S.at<float>(l.scores) : nullptr, c.S.at<char>(l.scratch), c.S.stream()))
    return r;
  return finish_detect(c, db, l, nullptr, candidates, n_candidates, common_words, scores);
}

}  // extern "C"
