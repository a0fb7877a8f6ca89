// kfdb.hip -- the keyframe database's queries and TemplatedVocabulary::score on gfx950.
//
// KeyframeDatabase::DetectLoopCandidates / DetectRelocalizationCandidates
// (src/data/keyframe_database.cpp:48-176, :179-299) without an inverted file: the reference's
// lKFsSharingWords is ordered by (smallest word id shared with the query, add sequence number),
// so a query is three data-parallel passes over the keyframe slots.
//
//   kfdb_common   one wave per slot. The query's word ids sit in LDS; each lane binary-searches
//                 one of the keyframe's words. mnLoopWords / mnRelocWords = the popcount of the
//                 ballots, the key word = the first hit, maxCommonWords = an integer atomicMax
//                 (exact, order-free).
//   kfdb_score    one wave per slot plus one per covisible keyframe of the loop query's min_score.
//                 A wave leaves unless its keyframe has words > minCommonWords. L1Scoring::score
//                 (third_party/DBoW2/DBoW2/ScoringObject.cpp:23-68): lanes form the terms of 64
//                 keyframe words at a time, the ballot names the common ones and the FP64 sum takes
//                 them one after another in ascending word order -- no tree, which would change the
//                 double.
//   kfdb_select   one workgroup: min_score, the entries of lScoreAndMatch sorted by the 64-bit key
//                 (bitonic in LDS, slot as payload), one lane per entry over its <= 10 neighbours
//                 in order, bestAccScore by a float max (only compared, so +-0 and order are
//                 free), "first in order wins" by an integer atomicMin per pBestKF, compaction in
//                 order by a workgroup scan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "kfdb_kernels.h"

namespace slamgpu {

namespace {

constexpr int kWaves = 4;  // waves per workgroup of the per-slot kernels

// First index with w[i] >= x (std::lower_bound).
__device__ __forceinline__ int lower_bound_u32(const uint32_t* w, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (w[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// L1Scoring::score(v1, v2) by one wave; every lane returns the double.
__device__ double l1_score_wave(const uint32_t* __restrict__ w1, const double* __restrict__ v1,
                                int n1, const uint32_t* __restrict__ w2,
                                const double* __restrict__ v2, int n2) {
  const int lane = lane_id();
  double score = 0;
  for (int c = 0; c < n2; c += 64) {
    const int i = c + lane;
    bool hit = false;
    double term = 0;
    if (i < n2) {
      const uint32_t w = w2[i];
      const int p = lower_bound_u32(w1, n1, w);
      if (p < n1 && w1[p] == w) {
        hit = true;
        const double vi = v1[p], wi = v2[i];
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);  // ScoringObject.cpp:41
      }
    }
    uint64_t m = __ballot(hit);
    while (m) {  // wave-uniform: ascending word order
      const int b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      score += __shfl(term, b, 64);
    }
  }
  return -score / 2.0;  // :65
}

__global__ __launch_bounds__(64 * kWaves) void bow_score_kernel(const BowVecView* __restrict__ a,
                                                                const BowVecView* __restrict__ b,
                                                                int n_pairs,
                                                                double* __restrict__ out) {
  const int p = blockIdx.x * kWaves + wave_id();
  if (p >= n_pairs) return;
  const BowVecView A = a[p], B = b[p];
  const int n1 = max(*A.n, 0), n2 = max(*B.n, 0);
  const double s = l1_score_wave(A.words, A.values, n1, B.words, B.values, n2);
  if (lane_id() == 0) out[p] = s;
}

// ---- table updates -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kfdb_set_bow_kernel(KfdbDev d, int kf,
                                                           const uint32_t* __restrict__ words,
                                                           const double* __restrict__ values,
                                                           const int32_t* __restrict__ n_ptr) {
  const int n = clamp_count(*n_ptr, d.max_words);
  const size_t row = (size_t)kf * d.max_words;
  for (int i = threadIdx.x; i < n; i += 256) {
    d.words[row + i] = words[i];
    d.values[row + i] = values[i];
  }
  if (threadIdx.x == 0) d.n_words[kf] = n;
}

__global__ __launch_bounds__(64) void kfdb_set_covisible_kernel(KfdbDev d, int kf,
                                                                const int32_t* __restrict__ ids,
                                                                int n) {
  const int t = threadIdx.x;
  if (t < n) d.covis[(size_t)kf * kKfdbNeighbours + t] = ids[t];
  if (t == 0) d.n_covis[kf] = n;
}

__global__ __launch_bounds__(256) void kfdb_set_seq_kernel(KfdbDev d, int kf, uint32_t value) {
  if (kf >= 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) d.seq[kf] = value;
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < d.max_kf) d.seq[i] = value;
}

// ---- queries -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kfdb_mask_kernel(uint8_t* __restrict__ mask,
                                                        const int32_t* __restrict__ ids, int n,
                                                        int max_kf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  if (id >= 0 && id < max_kf) mask[id] = 1;
}

__global__ __launch_bounds__(64 * kWaves) void kfdb_common_kernel(
    KfdbDev d, const uint32_t* __restrict__ qw, const int32_t* __restrict__ qn_ptr, int qn_cap,
    const uint8_t* __restrict__ mask, int32_t* __restrict__ cnt, uint32_t* __restrict__ key_word,
    uint32_t* __restrict__ first, float* __restrict__ score_zero, int32_t* __restrict__ ctrl) {
  __shared__ uint32_t s_q[kKfdbMaxQuery];
  const int qn = clamp_count(*qn_ptr, qn_cap);
  for (int i = threadIdx.x; i < qn; i += 64 * kWaves) s_q[i] = qw[i];
  __syncthreads();
  const int slot = blockIdx.x * kWaves + wave_id(), lane = lane_id();
  if (slot >= d.max_kf) return;
  if (lane == 0) {
    first[slot] = 0xffffffffu;
    if (score_zero) score_zero[slot] = 0.0f;
  }
  if (d.seq[slot] == 0 || (mask && mask[slot])) {
    if (lane == 0) cnt[slot] = -1;
    return;
  }
  const int nk = clamp_count(d.n_words[slot], d.max_words);
  const uint32_t* kw = d.words + (size_t)slot * d.max_words;
  int count = 0;
  uint32_t key = 0xffffffffu;
  for (int c = 0; c < nk; c += 64) {
    const int i = c + lane;
    uint32_t w = 0;
    bool hit = false;
    if (i < nk) {
      w = kw[i];
      const int p = lower_bound_u32(s_q, qn, w);
      hit = p < qn && s_q[p] == w;
    }
    const uint64_t m = __ballot(hit);
    if (m != 0 && count == 0) key = (uint32_t)__shfl((int)w, __ffsll((unsigned long long)m) - 1, 64);
    count += __popcll(m);
  }
  if (lane == 0) {
    cnt[slot] = count;
    key_word[slot] = key;
    if (count > 0) atomicMax(ctrl, count);
  }
}

// minCommonWords (keyframe_database.cpp:98, :222)
__device__ __forceinline__ int min_common_words(int max_common) {
  return static_cast<int>(max_common * 0.8f);
}

__global__ __launch_bounds__(64 * kWaves) void kfdb_score_kernel(
    KfdbDev d, const uint32_t* __restrict__ qw, const double* __restrict__ qv,
    const int32_t* __restrict__ qn_ptr, int qn_cap, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ ctrl, float* __restrict__ score,
    const int32_t* __restrict__ cov_ids, int n_cov, float* __restrict__ cov_score) {
  const int job = blockIdx.x * kWaves + wave_id();
  int slot;
  float* dst;
  if (job < d.max_kf) {
    if (cnt[job] <= min_common_words(ctrl[0])) return;
    slot = job;
    dst = score + job;
  } else {
    const int i = job - d.max_kf;
    if (i >= n_cov) return;
    slot = cov_ids[i];
    if (slot < 0 || slot >= d.max_kf) return;
    dst = cov_score + i;
  }
  const int qn = clamp_count(*qn_ptr, qn_cap);
  const int nk = clamp_count(d.n_words[slot], d.max_words);
  const double s = l1_score_wave(qw, qv, qn, d.words + (size_t)slot * d.max_words,
                                 d.values + (size_t)slot * d.max_words, nk);
  if (lane_id() == 0) *dst = (float)s;  // mLoopScore / mRelocScore are floats
}

constexpr int kSelThreads = 1024;
constexpr int kSelPer = kKfdbMaxScored / kSelThreads;

// Exclusive prefix of one int per thread over the workgroup; *total = the sum.
__device__ int select_scan(int x, int* s_w, int* total) {
  const int lane = lane_id(), wid = wave_id();
  int inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(inc, off, 64);
    if (lane >= off) inc += y;
  }
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kSelThreads / 64; w++) {
    const int s = s_w[w];
    if (w < wid) base += s;
    tot += s;
  }
  *total = tot;
  __syncthreads();  // s_w is reused by the next call
  return base + inc - x;
}

__global__ __launch_bounds__(kSelThreads) void kfdb_select_kernel(
    KfdbDev d, int loop, const int32_t* __restrict__ cnt, const uint32_t* __restrict__ key_word,
    const float* __restrict__ sc, uint32_t* __restrict__ first, const int32_t* __restrict__ ctrl,
    const int32_t* __restrict__ cov_ids, int n_cov, const float* __restrict__ cov_score,
    float* __restrict__ out_min_score, int32_t* __restrict__ out_cand,
    int32_t* __restrict__ out_n, float* __restrict__ out_scores) {
  __shared__ uint64_t s_key[kKfdbMaxScored];
  __shared__ int32_t s_slot[kKfdbMaxScored];
  __shared__ int s_w[kSelThreads / 64];
  __shared__ float s_wmax[kSelThreads / 64];
  __shared__ int s_n;
  __shared__ float s_min;
  const int tid = threadIdx.x;
  if (tid == 0) s_n = 0;

  // min_score (loop_closer.cpp:214-221): std::min in the list's order.
  if (loop) {
    float* s_f = reinterpret_cast<float*>(s_key);
    float ms = 1.0f;
    for (int base = 0; base < n_cov; base += kKfdbMaxScored) {
      const int m = min(n_cov - base, kKfdbMaxScored);
      for (int j = tid; j < m; j += kSelThreads) {
        const int id = cov_ids[base + j];
        const bool ok = id >= 0 && id < d.max_kf;
        s_slot[j] = ok;
        s_f[j] = ok ? cov_score[base + j] : 0.0f;
      }
      __syncthreads();
      if (tid == 0)
        for (int j = 0; j < m; j++)
          if (s_slot[j]) {
            const float x = s_f[j];
            ms = (x < ms) ? x : ms;
          }
      __syncthreads();
    }
    if (tid == 0) {
      s_min = ms;
      *out_min_score = ms;
    }
  } else if (tid == 0) {
    s_min = 0.0f;
  }
  __syncthreads();
  const float min_score = s_min;
  const int min_common = min_common_words(ctrl[0]);

  // lScoreAndMatch (:102-114, :227-238), in any order: the sort below fixes it.
  for (int slot = tid; slot < d.max_kf; slot += kSelThreads) {
    if (out_scores && !loop) out_scores[slot] = sc[slot];
    if (cnt[slot] > min_common && (!loop || sc[slot] >= min_score)) {
      const int p = atomicAdd(&s_n, 1);
      if (p < kKfdbMaxScored) {
        s_key[p] = (uint64_t)key_word[slot] << 32 | d.seq[slot];
        s_slot[p] = slot;
      }
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n == 0 || n > kKfdbMaxScored) {
    if (tid == 0) *out_n = n == 0 ? 0 : -1;
    return;
  }
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += kSelThreads) s_key[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kSelThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t x = s_key[i], y = s_key[ixj];
          if ((x > y) == ((i & k) == 0)) {
            s_key[i] = y;
            s_key[ixj] = x;
            const int32_t t = s_slot[i];
            s_slot[i] = s_slot[ixj];
            s_slot[ixj] = t;
          }
        }
      }
      __syncthreads();
    }

  // accumulate over the stored neighbours (:121-153, :244-278)
  float acc[kSelPer];
  int best[kSelPer];
  float best_acc = min_score;
#pragma unroll
  for (int k = 0; k < kSelPer; k++) {
    const int i = k * kSelThreads + tid;
    acc[k] = 0.0f;
    best[k] = -1;
    if (i < n) {
      const int slot = s_slot[i];
      float bs = sc[slot], a = bs;
      int b = slot;
      const int nn = clamp_count(d.n_covis[slot], kKfdbNeighbours);
      for (int j = 0; j < nn; j++) {
        const int nb = d.covis[(size_t)slot * kKfdbNeighbours + j];
        if (nb < 0 || nb >= d.max_kf) continue;
        const int c = cnt[nb];
        if (loop ? c > min_common : c > 0) {
          const float x = sc[nb];
          a += x;
          if (x > bs) {
            b = nb;
            bs = x;
          }
        }
      }
      acc[k] = a;
      best[k] = b;
      if (a > best_acc) best_acc = a;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) best_acc = fmaxf(best_acc, __shfl_xor(best_acc, off, 64));
  if (lane_id() == 0) s_wmax[wave_id()] = best_acc;
  __syncthreads();
  for (int w = 0; w < kSelThreads / 64; w++) best_acc = fmaxf(best_acc, s_wmax[w]);
  const float retain = 0.75f * best_acc;  // :156, :281

  // first occurrence of a pBestKF wins (:162-173, :286-297)
#pragma unroll
  for (int k = 0; k < kSelPer; k++) {
    const int i = k * kSelThreads + tid;
    if (i < n && acc[k] > retain) atomicMin(&first[best[k]], (uint32_t)i);
  }
  __threadfence();
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int k = 0; k < kSelPer; k++) {
    if (k * kSelThreads >= n) break;  // uniform
    const int i = k * kSelThreads + tid;
    int keep = 0;
    if (i < n && acc[k] > retain)
      keep = __hip_atomic_load(&first[best[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             (uint32_t)i;
    int total = 0;
    const int pos = base + select_scan(keep, s_w, &total);
    if (keep) out_cand[pos] = best[k];
    base += total;
  }
  if (tid == 0) *out_n = base;
}

}  // namespace

hipError_t launch_bow_score(const BowVecView* a, const BowVecView* b, int n_pairs, double* out,
                            hipStream_t st) {
  if (n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(bow_score_kernel, dim3((n_pairs + kWaves - 1) / kWaves), dim3(64 * kWaves), 0,
                     st, a, b, n_pairs, out);
  return hipGetLastError();
}

hipError_t launch_kfdb_set_bow(const KfdbDev& d, int kf, const uint32_t* words,
                               const double* values, const int32_t* n, hipStream_t st) {
  hipLaunchKernelGGL(kfdb_set_bow_kernel, dim3(1), dim3(256), 0, st, d, kf, words, values, n);
  return hipGetLastError();
}

hipError_t launch_kfdb_set_covisible(const KfdbDev& d, int kf, const int32_t* ids, int n,
                                     hipStream_t st) {
  hipLaunchKernelGGL(kfdb_set_covisible_kernel, dim3(1), dim3(64), 0, st, d, kf, ids, n);
  return hipGetLastError();
}

hipError_t launch_kfdb_set_seq(const KfdbDev& d, int kf, uint32_t value, hipStream_t st) {
  const int blocks = kf >= 0 ? 1 : (d.max_kf + 255) / 256;
  hipLaunchKernelGGL(kfdb_set_seq_kernel, dim3(blocks), dim3(256), 0, st, d, kf, value);
  return hipGetLastError();
}

hipError_t launch_kfdb_detect(const KfdbDev& d, const KfdbQuery& q, void* scratch,
                              hipStream_t st) {
  const KfdbScratch s = kfdb_scratch(scratch, d.max_kf);
  const bool loop = q.query_kf >= 0;
  const uint32_t* qw = loop ? d.words + (size_t)q.query_kf * d.max_words : q.words;
  const double* qv = loop ? d.values + (size_t)q.query_kf * d.max_words : q.values;
  const int32_t* qn = loop ? d.n_words + q.query_kf : q.n;
  const int qn_cap = loop ? d.max_words : kKfdbMaxQuery;
  int32_t* cnt = q.common_words ? q.common_words : s.cnt;
  // loop: this query's scores (zeroed by kfdb_common); relocalisation: the persistent ones
  float* sc = loop ? (q.scores ? q.scores : s.score) : d.reloc_score;
  // ctrl and, for the loop query, the connected mask behind it
  hipError_t e = hipMemsetAsync(s.ctrl, 0, loop ? 256 + kfdb_pad((size_t)d.max_kf) : 256, st);
  if (e != hipSuccess) return e;
  if (loop && q.n_connected > 0)
    hipLaunchKernelGGL(kfdb_mask_kernel, dim3((q.n_connected + 255) / 256), dim3(256), 0, st,
                       s.mask, q.connected, q.n_connected, d.max_kf);
  const int slots = (d.max_kf + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(kfdb_common_kernel, dim3(slots), dim3(64 * kWaves), 0, st, d, qw, qn, qn_cap,
                     loop ? s.mask : nullptr, cnt, s.key_word, s.first, loop ? sc : nullptr,
                     s.ctrl);
  const int n_cov = loop ? q.n_covisible : 0;
  const int jobs = (d.max_kf + n_cov + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(kfdb_score_kernel, dim3(jobs), dim3(64 * kWaves), 0, st, d, qw, qv, qn,
                     qn_cap, cnt, s.ctrl, sc, q.covisible, n_cov, s.cov_score);
  hipLaunchKernelGGL(kfdb_select_kernel, dim3(1), dim3(kSelThreads), 0, st, d, loop ? 1 : 0, cnt,
                     s.key_word, sc, s.first, s.ctrl, q.covisible, n_cov, s.cov_score, q.min_score,
                     q.candidates, q.n_candidates, q.scores);
  return hipGetLastError();
}

}  // namespace slamgpu
