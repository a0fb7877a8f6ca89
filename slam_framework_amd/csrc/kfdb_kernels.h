// kfdb_kernels.h -- device tables, per-query scratch and launchers of the keyframe database
// (include/slamgpu_kfdb.h) and of TemplatedVocabulary::score.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace slamgpu {

constexpr int kKfdbNeighbours = 10;    // == SLAMGPU_KFDB_MAX_NEIGHBOURS
constexpr int kKfdbMaxScored = 4096;   // == SLAMGPU_KFDB_MAX_SCORED
constexpr int kKfdbMaxQuery = 4096;    // == SLAMGPU_BOW_MAX_FEATURES

// The database's tables: slot = keyframe id.
struct KfdbDev {
  uint32_t* words;     // [max_kf][max_words] BowVector word ids, ascending
  double* values;      // [max_kf][max_words]
  int32_t* n_words;    // [max_kf]
  uint32_t* seq;       // [max_kf] add sequence number, 0 = not listed
  int32_t* covis;      // [max_kf][10] GetBestCovisibilityKeyFrames(10), in order
  int32_t* n_covis;    // [max_kf]
  float* reloc_score;  // [max_kf] mRelocScore: persists from one relocalisation query to the next
  int32_t max_kf, max_words;
};

// == slamgpu_bow_vec_view
struct BowVecView {
  const uint32_t* words;
  const double* values;
  const int32_t* n;
};

// One query's scratch, carved from the caller's buffer; every array [max_kf] but ctrl.
struct KfdbScratch {
  int32_t* ctrl;       // [0] = maxCommonWords
  uint8_t* mask;       // connected to the query keyframe (loop)
  int32_t* cnt;        // common words, -1 = not listed or connected
  uint32_t* key_word;  // smallest word id shared with the query
  float* score;        // mLoopScore of this query
  uint32_t* first;     // select: first retained entry naming this keyframe as pBestKF
  float* cov_score;    // loop: score against covisible[i]
};

inline size_t kfdb_pad(size_t b) { return (b + 255) / 256 * 256; }
inline size_t kfdb_scratch_bytes(int max_kf) {
  const size_t n = (size_t)max_kf;
  return 256 + kfdb_pad(n) + 5 * kfdb_pad(4 * n);
}
inline KfdbScratch kfdb_scratch(void* base, int max_kf) {
  char* p = static_cast<char*>(base);
  const size_t n = (size_t)max_kf, a4 = kfdb_pad(4 * n);
  KfdbScratch s;
  s.ctrl = reinterpret_cast<int32_t*>(p);
  s.mask = reinterpret_cast<uint8_t*>(p + 256);
  p += 256 + kfdb_pad(n);
  s.cnt = reinterpret_cast<int32_t*>(p);
  s.key_word = reinterpret_cast<uint32_t*>(p + a4);
  s.score = reinterpret_cast<float*>(p + 2 * a4);
  s.first = reinterpret_cast<uint32_t*>(p + 3 * a4);
  s.cov_score = reinterpret_cast<float*>(p + 4 * a4);
  return s;
}

hipError_t launch_bow_score(const BowVecView* a, const BowVecView* b, int n_pairs, double* out,
                            hipStream_t st);
hipError_t launch_kfdb_set_bow(const KfdbDev& d, int kf, const uint32_t* words,
                               const double* values, const int32_t* n, hipStream_t st);
hipError_t launch_kfdb_set_covisible(const KfdbDev& d, int kf, const int32_t* ids, int n,
                                     hipStream_t st);
// kf >= 0: seq[kf] = value; kf < 0: every slot.
hipError_t launch_kfdb_set_seq(const KfdbDev& d, int kf, uint32_t value, hipStream_t st);

// The query of one detect call. Loop: query_kf >= 0 (its row of the tables), connected /
// covisible id lists, min_score written. Relocalisation: query_kf < 0 and the frame's vector.
struct KfdbQuery {
  int query_kf;
  const uint32_t* words;
  const double* values;
  const int32_t* n;
  const int32_t* connected;
  int n_connected;
  const int32_t* covisible;
  int n_covisible;
  float* min_score;
  int32_t* candidates;
  int32_t* n_candidates;
  int32_t* common_words;  // optional
  float* scores;          // optional
};
hipError_t launch_kfdb_detect(const KfdbDev& d, const KfdbQuery& q, void* scratch, hipStream_t st);

}  // namespace slamgpu
