// orb_search.hip -- the OrbMatcher searches of a frame's keypoint grid on gfx950, batched over
// frames: tracking, relocalisation and initialisation.
//
//   search_cand     projection + window + Hamming     OrbMatcher::SearchByProjection (both
//   search_resolve  greedy in-order claims            overloads, orb_matcher.cpp:13-103 and
//                                                     :1312-1453) + rotation histogram; and the
//                                                     relocalisation overload (Frame, KeyFrame,
//                                                     sAlreadyFound, th, ORBdist) :1455-1582
//   init_resolve    in-order loop with take-overs     OrbMatcher::SearchForInitialization :264-382
// Every Hamming distance is popcount(a ^ b) over the 256 bits (== DescriptorDistance,
// :1630-1646; orbmatch_device.h, which also holds the other rules shared with the keyframe matchers).
// The projection matchers are greedy in query order (a keypoint taken by an earlier query whose
// map point has observations is skipped, :59-63 / :1389-1393), so candidate search is parallel
// over queries and only a short claim-resolution pass per frame is sequential.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "match_kernels.h"
#include "orbmatch_device.h"
#include "timing.h"

namespace slamgpu {

// ---------------------------------------------------------------------------------------
// Candidate scan of one query by one wave: Frame::GetFeaturesInArea (frame.cpp:348-403) plus the
// matcher's per-candidate filters, keeping the kTopK best candidates by (distance, position in
// GetFeaturesInArea order): the candidate keys of orbmatch_device.h.
struct ScanCtx {
  float x, y, r;         // GetFeaturesInArea(x, y, r, min_level, max_level)
  int min_level, max_level;
  float ur, gate;        // skip if u_right > 0 && fabsf(ur - u_right) > gate
  int max_dist;          // keep candidates with distance <= max_dist
  const uint8_t* desc;   // query descriptor
  float nnratio;         // SearchForInitialization's filter only (see scan_query_k)
};

struct FrameView {
  const KeyPoint* kps;
  const uint8_t* desc;
  const float* u_right;
  const int* cell_start;
  const uint4* cell_items;
  const uint8_t* blocked;
};

// The scan's candidate key, ordered as (distance, cell, index): 32 bits -- dist (<= 256) << 23 |
// cell (< 4096) << 11 | index (< 2048) -- when the frame's keypoint capacity allows, else the 64-bit
// form the resolution pass reads (cand_key).
template <typename K>
__device__ __forceinline__ K scan_key(int dist, int cell, int i) {
  if constexpr (sizeof(K) == 4)
    return (uint32_t)dist << 23 | (uint32_t)cell << 11 | (uint32_t)i;
  else
    return cand_key(dist, cell, i);
}
template <typename K>
__device__ __forceinline__ uint64_t key64(K k) {
  if constexpr (sizeof(K) == 4)
    return k == ~0u ? kNoKey : cand_key(k >> 23, (int)((k >> 11) & 0xfffu), (int)(k & 0x7ffu));
  else
    return k;
}

// G lanes per query (the group of `lane`): 64 for the resolution pass's rescans, 16 for
// search_cand (a window holds a handful of keypoints: four queries per wave keep the lanes busy)
// skip: the group has no query (or its context failed): it scans nothing -- no cell bound is
// derived from its coordinates -- but still takes part in the group's shuffles and the merge
// kInit: SearchForInitialization's per-candidate filter in place of the projection searches'
// three (no slot state, no right coordinate): `claimed` is then the vMatchedDistance table (ints,
// INT_MAX = unmatched; null in search_cand) and a candidate with table[i] <= dist is skipped
// (:306-307). Candidates that can never matter are dropped too: one above TH_LOW never is an
// accepted best, and as a second with (float)dist * nnratio > TH_LOW it passes every best the
// ratio test can see (:321-323), as the seconds behind it and an absent second (INT_MAX) do.
template <typename K, int G = 64, bool kInit = false>
__device__ int scan_query_k(const ScanCtx& c, const Camera& cam, const FrameView& F,
                            const uint32_t* claimed, uint64_t* top, int lane, bool skip = false) {
  const int gl = lane & (G - 1), gb = lane & ~(G - 1);
  int nMinCellX = 0, nMaxCellX = -1, nMinCellY = 0, nMaxCellY = -1;  // empty window
  if (!skip)
    cell_window(c.x, c.y, c.r, cam.min_x, cam.min_y, cam.cell_w, cam.cell_h, &nMinCellX,
                &nMaxCellX, &nMinCellY, &nMaxCellY);
  constexpr K kNone = (K)~(K)0;
  K t[kTopK];
#pragma unroll
  for (int k = 0; k < kTopK; k++) t[k] = kNone;
  int cnt = 0;
  if (window_on_grid(nMinCellX, nMaxCellX, nMinCellY, nMaxCellY)) {
    const bool bCheckLevels = (c.min_level > 0) || (c.max_level >= 0);
    const int ny = nMaxCellY - nMinCellY + 1;
    const int total = (nMaxCellX - nMinCellX + 1) * ny;
    // The window's (cell, keypoint) pairs are spread over the lanes, one keypoint each: a lane
    // per cell would walk its cell's keypoints as one serial chain of dependent loads while the
    // lanes of empty or absent cells idle. Cells 64 at a time: per-lane keypoint counts, their
    // wave prefix sum, then lane k takes pair k (its cell found by a binary search over the
    // prefix sums). The kept candidates are an order-free minimum, so any order gives the same.
    for (int cb = 0; cb < total; cb += G) {
      const int ci = cb + gl;
      int cell = 0, q0 = 0, nq = 0;
      if (ci < total) {
        const int ix = nMinCellX + ci / ny, iy = nMinCellY + ci % ny;
        cell = ix * kGridRows + iy;
        q0 = F.cell_start[cell];
        nq = F.cell_start[cell + 1] - q0;
      }
      const int incl = group_incl_scan<G>(nq);
      const int excl = incl - nq;
      const int npairs = G == 64 ? __builtin_amdgcn_readlane(incl, 63) : __shfl(incl, gb + G - 1, 64);
      // every lane of the group takes part in the shuffles (a shuffle reads 0 from an inactive
      // lane); groups run their own trip counts, their shuffles stay inside the group
      for (int k0 = 0; k0 < npairs; k0 += G) {
        const int k = k0 + gl;
        int lo = 0;  // the group's last lane whose exclusive offset is <= k
#pragma unroll
        for (int step = G / 2; step >= 1; step >>= 1) {
          const int cand = lo + step;
          const int ec = __shfl(excl, gb + (cand & (G - 1)), 64);
          if (cand < G && ec <= k) lo = cand;
        }
        const int p = __shfl(q0, gb + lo, 64) + (k - __shfl(excl, gb + lo, 64));
        const int pcell = __shfl(cell, gb + lo, 64);
        if (k >= npairs) continue;
        const uint4 it = F.cell_items[p];
        const int i = (int)(it.x & 0xffffu), octave = (int)(it.x >> 16);
        if (bCheckLevels) {
          if (octave < c.min_level) continue;
          if (c.max_level >= 0 && octave > c.max_level) continue;
        }
        const float distx = __uint_as_float(it.y) - c.x, disty = __uint_as_float(it.z) - c.y;
        if (!(fabsf(distx) < c.r && fabsf(disty) < c.r)) continue;
        int dist;
        if constexpr (kInit) {
          dist = hamming32(c.desc, F.desc + i * 32);
          if (claimed && (int)claimed[i] <= dist) continue;
          if (dist > kThLow && (float)dist * c.nnratio > (float)kThLow) continue;
        } else {
          // the remaining filters' loads all in flight together (the filters commute)
          const bool blk = F.blocked[i] != 0;
          const float ur = F.u_right[i];
          dist = hamming32(c.desc, F.desc + i * 32);
          if (blk) continue;
          if (claimed && (claimed[i >> 5] >> (i & 31)) & 1u) continue;
          if (ur > 0 && fabsf(c.ur - ur) > c.gate) continue;
          if (dist > c.max_dist) continue;
        }
        const K key = scan_key<K>(dist, pcell, i);
        cnt++;
        if (key < t[kTopK - 1]) {
          t[kTopK - 1] = key;
#pragma unroll
          for (int k2 = kTopK - 1; k2 > 0; k2--)
            if (t[k2] < t[k2 - 1]) {
              const K s2 = t[k2];
              t[k2] = t[k2 - 1];
              t[k2 - 1] = s2;
            }
        }
      }
    }
  }
  // merge the per-lane sorted lists: up to kTopK rounds of wave minimum, ending early once the
  // wave has no candidate left (most queries keep fewer than kTopK)
#pragma unroll
  for (int k = 0; k < kTopK; k++) top[k] = kNoKey;
#pragma unroll
  for (int k = 0; k < kTopK; k++) {
    const K m = group_min_key<G>(t[0]);
    if (G == 64) {
      if (m == kNone) break;  // wave-uniform
    } else if (__ballot(m != kNone) == 0) {
      break;  // no group has a candidate left
    }
    if (m != kNone) {
      if (t[0] == m) {
#pragma unroll
        for (int j = 0; j < kTopK - 1; j++) t[j] = t[j + 1];
        t[kTopK - 1] = kNone;
      }
      top[k] = key64<K>(m);
    }
  }
  return group_sum<G>(cnt);
}

// 32-bit keys whenever the frame's keypoint indices fit 11 bits (kp_cap <= 2048: nfeatures up to
// ~2000 with the per-level slack), the 64-bit form otherwise.
template <int G = 64, bool kInit = false>
__device__ __forceinline__ int scan_query(const ScanCtx& c, const Camera& cam, const FrameView& F,
                                          const uint32_t* claimed, uint64_t* top, int lane,
                                          int kp_cap, bool skip = false) {
  if (kp_cap <= 2048) return scan_query_k<uint32_t, G, kInit>(c, cam, F, claimed, top, lane, skip);
  return scan_query_k<uint64_t, G, kInit>(c, cam, F, claimed, top, lane, skip);
}

// SearchByProjection(CurrentFrame, LastFrame) per-query setup (orb_matcher.cpp:1336-1376).
__device__ bool f2f_ctx(const F2FQuery& q, const F2FPose& P, const Camera& cam,
                        const OrbGeom* g, ScanCtx* c) {
  const float xc = gemm_row(P.Rcw, q.xyz, P.tcw[0]);
  const float yc = gemm_row(P.Rcw + 3, q.xyz, P.tcw[1]);
  const float zc = gemm_row(P.Rcw + 6, q.xyz, P.tcw[2]);
  const float invzc = (float)(1.0 / (double)zc);
  if (invzc < 0) return false;
  const float u = fmaf(cam.fx * xc, invzc, cam.cx);
  const float v = fmaf(cam.fy * yc, invzc, cam.cy);
  if (u < cam.min_x || u > cam.max_x) return false;
  if (v < cam.min_y || v > cam.max_y) return false;
  const int nLastOctave = q.last_octave;
  const float radius = P.th * g->lv[nLastOctave].scale;
  const bool bForward = P.tlc_z > P.baseline && !P.mono;
  const bool bBackward = -P.tlc_z > P.baseline && !P.mono;
  c->x = u;
  c->y = v;
  c->r = radius;
  if (bForward) {
    c->min_level = nLastOctave;
    c->max_level = -1;
  } else if (bBackward) {
    c->min_level = 0;
    c->max_level = nLastOctave;
  } else {
    c->min_level = nLastOctave - 1;
    c->max_level = nLastOctave + 1;
  }
  c->ur = fmaf(-cam.bf, invzc, u);
  c->gate = radius;
  c->max_dist = kThHigh;  // a candidate above kThHigh can never become the accepted match
  c->desc = q.desc;
  return true;
}

// SearchByProjection(F, vpMapPoints, th) per-query setup (orb_matcher.cpp:21-41, 105-111).
__device__ bool mps_ctx(const MpsQuery& q, int th, const OrbGeom* g, ScanCtx* c) {
  if (!q.in_view || q.is_bad) return false;
  float r = ((double)q.view_cos > 0.998) ? 2.5f : 4.0f;
  if (th != 1) r *= (float)th;
  const float rs = r * g->lv[q.level].scale;
  c->x = q.proj_x;
  c->y = q.proj_y;
  c->r = rs;
  c->min_level = q.level - 1;
  c->max_level = q.level;
  c->ur = q.proj_xr;
  c->gate = rs;
  c->max_dist = 256;
  c->desc = q.desc;
  return true;
}

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) per-query setup
// (orb_matcher.cpp:1473-1513; PredictScale map_point.cpp:382-396). No depth gate and no
// right-coordinate gate; the octave window is level-1 .. level+1. Where the reference's
// arithmetic is undefined (a non-finite invzc, u, v, dist3D or max_dist / dist3D, a ratio <= 0:
// float -> int of NaN / inf in GetFeaturesInArea or PredictScale) the query matches nothing.
__device__ bool reloc_ctx(const RelocQuery& q, const RelocPose& P, const Camera& cam,
                          const OrbGeom* g, ScanCtx* c) {
  if (q.skip) return false;
  const float xc = gemm_row(P.Rcw, q.xyz, P.tcw[0]);
  const float yc = gemm_row(P.Rcw + 3, q.xyz, P.tcw[1]);
  const float zc = gemm_row(P.Rcw + 6, q.xyz, P.tcw[2]);
  const float invzc = (float)(1.0 / (double)zc);
  const float u = fmaf(cam.fx * xc, invzc, cam.cx);
  const float v = fmaf(cam.fy * yc, invzc, cam.cy);
  if (!isfinite(invzc) || !isfinite(u) || !isfinite(v)) return false;
  if (u < cam.min_x || u > cam.max_x) return false;
  if (v < cam.min_y || v > cam.max_y) return false;
  const float dist3D = norm3(q.xyz[0] - P.Ow[0], q.xyz[1] - P.Ow[1], q.xyz[2] - P.Ow[2]);
  if (!isfinite(dist3D)) return false;
  if (dist3D < 0.8f * q.min_dist || dist3D > 1.2f * q.max_dist) return false;
  const float ratio = q.max_dist / dist3D;
  if (!isfinite(ratio) || !(ratio > 0.0f)) return false;
  const int level = predict_scale(q.max_dist, dist3D, g->log_scale_factor, g->nlevels);
  c->x = u;
  c->y = v;
  c->r = P.th * g->lv[level].scale;
  c->min_level = level - 1;
  c->max_level = level + 1;
  c->ur = 0.0f;
  c->gate = __builtin_huge_valf();  // no right-coordinate gate
  c->max_dist = P.orb_dist;  // a best above ORBdist never claims
  c->desc = q.desc;
  return true;
}

// SearchForInitialization per-query setup (orb_matcher.cpp:282-287): no projection -- the window
// is GetFeaturesInArea(vbPrevMatched[i1], windowSize, level1, level1) for a level-0 keypoint.
// Where the reference's arithmetic is undefined (a vbPrevMatched entry that is not finite: float
// -> int of NaN / inf in GetFeaturesInArea) the query matches nothing.
__device__ bool init_ctx(const InitQuery& q, float2 prev, const InitSearch& P, ScanCtx* c) {
  const int level1 = q.octave;
  if (level1 > 0) return false;
  if (!isfinite(prev.x) || !isfinite(prev.y)) return false;
  c->x = prev.x;
  c->y = prev.y;
  c->r = (float)P.window_size;
  c->min_level = level1;
  c->max_level = level1;
  c->ur = 0.0f;
  c->gate = __builtin_huge_valf();
  c->max_dist = 256;
  c->desc = q.desc;
  c->nnratio = P.nnratio;
  return true;
}

#ifndef SEARCH_LANES
#define SEARCH_LANES 16
#endif
constexpr int kSearchG = SEARCH_LANES;  // lanes per query in search_cand (16 or 64)

// What differs between the four searches, one record per query type: the per-frame pose record
// (the local-map search has none), the caller's arrays, the lanes per query in search_cand, which
// resolution pass follows it (kInit: init_resolve, and scan_query's SearchForInitialization
// filter), the per-query setup, and the two FrameView fields that are not the same.
template <typename Q>
struct SearchTraits;

// The three SearchByProjection overloads differ in the pose record and the setup only.
struct ProjectionSearch {
  using IO = MatchIO;
  static constexpr int kLanes = kSearchG;
  static constexpr bool kInit = false;
  static __device__ __forceinline__ const float* u_right(const float* ur, int64_t stride, int f) {
    return ur + f * stride;
  }
  static __device__ __forceinline__ const uint8_t* blocked(const IO& io, int f) {
    return io.blocked + f * io.mp_stride;
  }
};
template <>
struct SearchTraits<F2FQuery> : ProjectionSearch {
  using Pose = F2FPose;
  static __device__ __forceinline__ bool ctx(const F2FQuery& q, const Pose* poses, int f, int,
                                             const Camera& cam, const OrbGeom* g, ScanCtx* c) {
    return f2f_ctx(q, poses[f], cam, g, c);
  }
};
template <>
struct SearchTraits<MpsQuery> : ProjectionSearch {
  using Pose = F2FPose;  // none: the launcher passes null
  static __device__ __forceinline__ bool ctx(const MpsQuery& q, const Pose*, int, int th,
                                             const Camera&, const OrbGeom* g, ScanCtx* c) {
    return mps_ctx(q, th, g, c);
  }
};
template <>
struct SearchTraits<RelocQuery> : ProjectionSearch {
  using Pose = RelocPose;
  static __device__ __forceinline__ bool ctx(const RelocQuery& q, const Pose* poses, int f, int,
                                             const Camera& cam, const OrbGeom* g, ScanCtx* c) {
    return reloc_ctx(q, poses[f], cam, g, c);
  }
};
// SearchForInitialization reads neither u_right nor the slot state. Its window (windowSize 100:
// 200 x 200 px, some 300 grid cells and a few hundred keypoints of all levels, against a handful
// in the projection searches) is walked 64 lanes wide: a quarter of the dependent cell / pair
// rounds per query, and its level-0 queries (some 440 to 870 waves) still fill the device.
// No ctx(): its two callers call init_ctx themselves -- behind a wrapper the compiler sinks the
// parameter loads below init_ctx's early returns, and search_cand's machine code changes.
template <>
struct SearchTraits<InitQuery> {
  using Pose = InitSearch;
  using IO = InitIO;
  static constexpr int kLanes = 64;
  static constexpr bool kInit = true;
  static __device__ __forceinline__ const float* u_right(const float*, int64_t, int) {
    return nullptr;
  }
  static __device__ __forceinline__ const uint8_t* blocked(const IO&, int) { return nullptr; }
};

template <typename Q>
__device__ __forceinline__ FrameView frame_view(int f, const FrameKps& cur, const float* u_right,
                                                int64_t ur_stride, const GridWorkspace& gw,
                                                const typename SearchTraits<Q>::IO& io,
                                                int kp_cap) {
  FrameView F;
  F.kps = cur.kps + f * cur.stride;
  F.desc = cur.desc + f * cur.stride * 32;
  F.u_right = SearchTraits<Q>::u_right(u_right, ur_stride, f);
  F.cell_start = gw.cell_start + (int64_t)f * (kGridCells + 1);
  F.cell_items = gw.cell_items + (int64_t)f * kp_cap;
  F.blocked = SearchTraits<Q>::blocked(io, f);
  return F;
}

template <typename Q>
__global__ __launch_bounds__(256) void search_cand_kernel(
    FrameKps cur, const float* __restrict__ u_right, int64_t ur_stride, Camera cam,
    const OrbGeom* __restrict__ g, const Q* __restrict__ queries,
    const typename SearchTraits<Q>::Pose* __restrict__ poses, int th, GridWorkspace gw,
    MatchWorkspace mw, typename SearchTraits<Q>::IO io) {
  using T = SearchTraits<Q>;
  constexpr int kG = T::kLanes;
  int f, bx;
  xcd_image_block(&f, &bx);  // a frame's work-groups share one XCD's L2 (its grid and keypoints)
  // kG lanes per query: 64 / kG queries per wave
  const int lane = threadIdx.x & 63, gl = lane & (kG - 1);
  const int qi = (bx * 4 + wave_id()) * (64 / kG) + lane / kG;
  const int qcount = io.q_count[f];
  if (__builtin_amdgcn_readfirstlane((bx * 4 + wave_id()) * (64 / kG)) >= qcount) return;
  const bool live = qi < qcount;  // the wave's last groups may have no query
  const int q = io.q_start[f] + (live ? qi : 0);
  const FrameView F = frame_view<Q>(f, cur, u_right, ur_stride, gw, io, g->kp_cap);
  ScanCtx c;
  bool ok;
  if constexpr (T::kInit)
    ok = init_ctx(queries[q], make_float2(io.prev_matched[2 * q], io.prev_matched[2 * q + 1]),
                  poses[f], &c) && live;
  else
    ok = T::ctx(queries[q], poses, f, th, cam, g, &c) && live;
  uint64_t top[kTopK];
  // a group without a query scans nothing but takes part in the merge
  const int n = scan_query<kG, T::kInit>(c, cam, F, nullptr, top, lane, g->kp_cap, !ok);
  if (live && gl < kTopK) {
    uint64_t v = top[0];
#pragma unroll
    for (int k = 1; k < kTopK; k++)
      if (gl == k) v = top[k];
    mw.topk[(int64_t)q * kTopK + gl] = ok ? v : kNoKey;
  }
  if (live && gl == 0) mw.ncand[q] = ok ? n : 0;
}

// Sequential, in-query-order claim resolution: one wave per frame. The kernel is a chain of
// latency (a frame's queries in order), so everything it can take off that chain is: the
// keypoint fields it needs are staged with all loads in flight, the next 64 queries' candidates
// are loaded while the current ones resolve, a candidate's "claimed" state is read once per
// round (claims change only when a round commits), and the rotation-histogram bookkeeping of the
// first kResolveLdsQ queries stays in LDS (a frame's later queries, if any, use the workspace).
constexpr int kResolveLdsQ = 4096;
template <typename Q>
__global__ __launch_bounds__(64) void search_resolve_kernel(
    FrameKps cur, const float* __restrict__ u_right, int64_t ur_stride, Camera cam,
    const OrbGeom* __restrict__ g, const Q* __restrict__ queries,
    const typename SearchTraits<Q>::Pose* __restrict__ poses, int th, float nnratio,
    GridWorkspace gw, MatchWorkspace mw, MatchIO io) {
  // kReloc: the relocalisation overload resolves as the frame-to-frame one does (distance gate,
  // rotation histogram), with every query blocking and the caller's ORBdist as the gate -- its
  // kept candidates are all <= ORBdist (reloc_ctx), so any kept candidate is accepted
  constexpr bool kReloc = std::is_same<Q, RelocQuery>::value;
  constexpr bool kF2F = std::is_same<Q, F2FQuery>::value || kReloc;
  constexpr int kAccept = kReloc ? 256 : kThHigh;
  __shared__ uint32_t claimed[128];  // kp_cap <= 4096
  __shared__ int hist[kHisto];
  __shared__ float s_kang[kF2F ? 4096 : 1];
  __shared__ int8_t s_koct[kF2F ? 1 : 4096];
  __shared__ int owner[4096];
  __shared__ int8_t s_bin[kF2F ? kResolveLdsQ : 1];     // rotation bin of query qi (-1 none)
  __shared__ int16_t s_best[kF2F ? kResolveLdsQ : 1];   // its matched keypoint
  const int f = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = cur.n[f * cur.n_stride];
  for (int i = lane; i < 128; i += 64) claimed[i] = 0;
  if (lane < kHisto) hist[lane] = 0;
  const FrameView F = frame_view<Q>(f, cur, u_right, ur_stride, gw, io, g->kp_cap);
  int* mp = io.map_point + f * io.mp_stride;
  uint8_t* blk = io.blocked + f * io.mp_stride;
  bool check_ori = false;
  if constexpr (kF2F) check_ori = poses[f].check_ori != 0;
  const int q0 = io.q_start[f], qn = io.q_count[f];
  int nm = 0;
  // The reference resolves queries strictly in order: a query takes its first candidate (in
  // (distance, GetFeaturesInArea) order) not claimed by an earlier *blocking* query
  // (orb_matcher.cpp:59-63, :1389-1393). Here 64 queries (one per lane) are resolved together
  // to the same result: each lane's choice is iterated to a fixed point against the claims
  // committed so far and the choices of the earlier lanes (owner[] holds the lowest blocking
  // lane per keypoint) -- lane i is final once lanes < i are, and conflicts are rare, so a few
  // rounds suffice. A lane whose kept top-K is exhausted while more candidates exist is rescanned
  // alone, at its place in the order. For non-blocking duplicates the last writer of mp[idx]
  // wins, as in the sequential loop.
  // keypoint fields (F2F: the angle, only with the rotation check; local map: the octave),
  // four loads in flight per lane
  for (int i0 = 0; i0 < n; i0 += 256) {
    float ang[4];
    int oct[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + 64 * u + lane;
      ang[u] = 0.f;
      oct[u] = 0;
      if (i < n) {
        if constexpr (kF2F) {
          if (check_ori) ang[u] = F.kps[i].angle;
        } else {
          oct[u] = F.kps[i].octave;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + 64 * u + lane;
      if (i < n) {
        if constexpr (kF2F) s_kang[i] = ang[u];
        else s_koct[i] = (int8_t)oct[u];
        owner[i] = INT_MAX;
      }
    }
  }
  wave_lds_sync();
  const int need = kF2F ? 1 : 2;
  auto is_claimed = [&](int idx) { return (claimed[idx >> 5] >> (idx & 31)) & 1u; };
  // acceptance of a query's best candidate b1 (a candidate, not kNoKey) given its second b2 (F2F:
  // the distance gate; local map: + the ratio test between candidates of one level, :76-99)
  auto accepts = [&](uint64_t b1, uint64_t b2) {
    bool acc = key_dist(b1) <= kAccept;
    if constexpr (!kF2F) {
      if (acc) {
        const int lv1 = s_koct[key_idx(b1)];
        const int d2 = b2 == kNoKey ? 256 : key_dist(b2);
        const int lv2 = b2 == kNoKey ? -1 : s_koct[key_idx(b2)];
        if (lv1 == lv2 && (float)key_dist(b1) > nnratio * (float)d2) acc = false;
      }
    }
    return acc;
  };
  // one lane's query of a chunk: its kept candidates, candidate count, map point word, angle
  struct QIn {
    uint64_t key[kTopK];
    int nc, mpw;
    float qang;
  };
  auto load_chunk = [&](int c0, QIn& in) {
    const int qi = c0 + lane;
    if (qi < qn) {
      const int q = q0 + qi;
#pragma unroll
      for (int k = 0; k < kTopK; k++) in.key[k] = mw.topk[(int64_t)q * kTopK + k];
      in.nc = mw.ncand[q];
      const Q& qq = queries[q];
      in.qang = 0.f;
      if constexpr (kReloc) {
        in.mpw = (qq.mp_id & 0x7fffffff) | (int)0x80000000u;  // SetMapPoint: every accept blocks
        in.qang = qq.kf_angle;
      } else {
        in.mpw = (qq.mp_id & 0x7fffffff) | (qq.blocks ? (int)0x80000000u : 0);
        if constexpr (kF2F) in.qang = qq.last_angle;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kTopK; k++) in.key[k] = kNoKey;
      in.nc = 0;
      in.mpw = 0;
      in.qang = 0.f;
    }
  };
  auto set_bin = [&](int qi, int bin, int idx) {
    if (qi < kResolveLdsQ) {
      s_bin[qi] = (int8_t)bin;
      s_best[qi] = (int16_t)idx;
    } else {
      mw.rot_bin[q0 + qi] = bin;
      mw.best_idx[q0 + qi] = idx;
    }
  };
  QIn nx;
  load_chunk(0, nx);
  for (int c0 = 0; c0 < qn; c0 += 64) {
    const int qi = c0 + lane;
    const bool valid = qi < qn;
    const QIn in = nx;
    if (c0 + 64 < qn) load_chunk(c0 + 64, nx);  // in flight while this chunk resolves
    const uint64_t* key = in.key;
    const int nc = in.nc, mpw = in.mpw;
    const float qang = in.qang;
    if constexpr (kF2F) {
      if (valid) set_bin(qi, -1, 0);
    }
    const bool qblocks = mpw < 0;
    int start = 0;
    while (start < 64 && c0 + start < qn) {
      const bool act = valid && lane >= start && nc > 0;
      // the kept candidates still unclaimed (claims change only at the commits below)
      uint32_t live = 0;
      if (act) {
#pragma unroll
        for (int k = 0; k < kTopK; k++)
          if (key[k] != kNoKey && !is_claimed(key_idx(key[k]))) live |= 1u << k;
      }
      // -- fixed point of the choices of lanes >= start
      uint64_t b1 = kNoKey, b2 = kNoKey;
      int navail = 0, mine = -1, prev = -2;
      for (int it = 0; it < 64; it++) {
        b1 = kNoKey;
        b2 = kNoKey;
        navail = 0;
#pragma unroll
        for (int k = 0; k < kTopK; k++) {
          if (!((live >> k) & 1u)) continue;
          if (owner[key_idx(key[k])] < lane) continue;
          if (navail == 0) b1 = key[k];
          else if (navail == 1) b2 = key[k];
          navail++;
        }
        // accepted blocking choice -> owner (the lowest such lane wins the keypoint)
        const bool acc = b1 != kNoKey && accepts(b1, b2);
        mine = (act && acc && qblocks) ? key_idx(b1) : -1;
        if (!__ballot(mine != prev)) break;
        if (prev >= 0) owner[prev] = INT_MAX;
        wave_lds_sync();
        if (mine >= 0) atomicMin(&owner[mine], lane);
        wave_lds_sync();
        prev = mine;
      }
      // -- the first lane that needs a rescan ends this round's committed range
      const uint64_t rs = __ballot(act && navail < need && nc > kTopK);
      const int r = rs ? __ffsll((long long)rs) - 1 : 64;
      if (prev >= 0) owner[prev] = INT_MAX;  // committed claims move to claimed[]
      wave_lds_sync();
      auto commit = [&](bool doit, uint64_t c1, uint64_t c2) {
        const bool touched = doit && c1 != kNoKey;
        const bool acc = touched && accepts(c1, c2);
        const int idx = touched ? key_idx(c1) : 0;
        nm += __popcll(__ballot(acc));
        // last writer (highest lane) of each keypoint sets mp / blocked
        if (touched) owner[idx] = 0;
        wave_lds_sync();
        if (acc) atomicMax(&owner[idx], lane + 1);
        wave_lds_sync();
        if (acc && owner[idx] == lane + 1) {
          mp[idx] = mpw & 0x7fffffff;
          blk[idx] = qblocks ? 1 : 0;
        }
        if (acc && qblocks) atomicOr(&claimed[idx >> 5], 1u << (idx & 31));
        if constexpr (kF2F) {
          if (acc && check_ori) {
            const int bin = rot_bin(qang, s_kang[idx]);
            set_bin(qi, bin, idx);
            atomicAdd(&hist[bin], 1);
          }
        }
        wave_lds_sync();
        if (touched) owner[idx] = INT_MAX;
        wave_lds_sync();
      };
      commit(act && lane < r, b1, b2);
      if (r < 64 && c0 + r < qn) {
        // lane r: every kept candidate is taken -> rescan its window with the live claims
        ScanCtx c;
        const bool okc =
            SearchTraits<Q>::ctx(queries[q0 + c0 + r], poses, f, th, cam, g, &c);
        uint64_t top[kTopK];
        if (okc) scan_query(c, cam, F, claimed, top, lane, g->kp_cap);
        const uint64_t t1 = __shfl(okc ? top[0] : kNoKey, 0, 64);
        const uint64_t t2 = __shfl(okc ? top[1] : kNoKey, 0, 64);
        commit(lane == r, t1, t2);
      }
      start = r + 1;
    }
  }
  wave_lds_sync();
  if constexpr (kF2F) {
    if (check_ori) {
      int ind1, ind2, ind3;
      three_maxima(hist, &ind1, &ind2, &ind3);
      // SetMapPoint(rotHist[i][j], nullptr) for every entry of a rejected bin (:1441-1450)
      int removed = 0;
      for (int qi = lane; qi < qn; qi += 64) {
        const bool in_lds = qi < kResolveLdsQ;
        const int bin = in_lds ? (int)s_bin[qi] : mw.rot_bin[q0 + qi];
        if (bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3) {
          const int idx = in_lds ? (int)s_best[qi] : mw.best_idx[q0 + qi];
          mp[idx] = -1;
          blk[idx] = 0;
          removed++;
        }
      }
      nm -= wave_sum(removed);
    }
  }
  if (lane == 0) io.nmatches[f] = nm;
}

// SearchForInitialization's in-order loop (orb_matcher.cpp:280-349) and its tail (:351-379): one
// wave per frame. A match here carries its distance and can be taken over by a later query with
// a strictly smaller one (:306-307, :325-333), so the state per keypoint of F2 is
// vMatchedDistance and vnMatches21, both in LDS (kp_cap <= 4096), and per query the keypoint it
// matched when it was accepted (s_best; queries past kResolveLdsQ use the workspace). 64 queries
// (one per lane) are decided together against the committed tables from their kept candidates: a
// kept candidate i2 is eligible iff vMatchedDistance[i2] > dist, the first two eligible ones in
// (distance, GetFeaturesInArea order) are bestDist / bestDist2. Accepting lanes stamp their
// keypoint with the lowest such lane; the first lane that needs a rescan, or that has a kept
// candidate stamped by a lower lane (its decision may change once that lane commits), ends the
// round: the lanes below it commit -- no two of them share a keypoint, each has the other's in
// its kept list or not at all -- and the round restarts there. A query whose kept list runs out
// before the decision is known is rescanned alone at its place in the order, the live
// vMatchedDistance table as the scan's filter.
// vnMatches12 is not kept while the loop runs: query i1 holds its match at the end iff
// vnMatches21[s_best[i1]] == i1 (a query is accepted once, a take-over rewrites vnMatches21).
// The rotation bins are taken after the loop from s_best, taken-over entries included (:344: the
// entry is never removed), and the removal loop clears only matches that still hold (:366).
__global__ __launch_bounds__(64) void init_resolve_kernel(
    FrameKps cur, Camera cam, const OrbGeom* __restrict__ g, const InitQuery* __restrict__ queries,
    const InitSearch* __restrict__ params, GridWorkspace gw, MatchWorkspace mw, InitIO io) {
  __shared__ int matched_dist[4096];  // vMatchedDistance
  __shared__ int matches21[4096];     // vnMatches21
  __shared__ int stamp[4096];         // lowest lane of the round that accepts the keypoint
  __shared__ int hist[kHisto];
  __shared__ int16_t s_best[kResolveLdsQ];  // keypoint query qi matched at accept time (-1 none)
  __shared__ int8_t s_bin[kResolveLdsQ];    // its rotation bin
  const int f = blockIdx.x;
  const int lane = threadIdx.x;
  const int kp_cap = g->kp_cap;
  const int n = min(cur.n[f * cur.n_stride], 4096);
  for (int i = lane; i < n; i += 64) {
    matched_dist[i] = INT_MAX;
    matches21[i] = -1;
    stamp[i] = INT_MAX;
  }
  if (lane < kHisto) hist[lane] = 0;
  const FrameView F = frame_view<InitQuery>(f, cur, nullptr, 0, gw, io, kp_cap);
  const InitSearch P = params[f];
  const float nnratio = P.nnratio;
  const bool check_ori = P.check_ori != 0;
  const int q0 = io.q_start[f], qn = io.q_count[f];
  auto set_best = [&](int qi, int idx) {
    if (qi < kResolveLdsQ) s_best[qi] = (int16_t)idx;
    else mw.best_idx[q0 + qi] = idx;
  };
  wave_lds_sync();
  auto get_best = [&](int qi) {
    return qi < kResolveLdsQ ? (int)s_best[qi] : mw.best_idx[q0 + qi];
  };
  // :321-323 -- int against float, the product in float, bestDist2 possibly INT_MAX
  auto accepts = [&](int bestDist, int bestDist2) {
    return bestDist <= kThLow && (float)bestDist < (float)bestDist2 * nnratio;
  };
  struct QIn {
    uint64_t key[kTopK];
    int nc;
  };
  auto load_chunk = [&](int c0, QIn& in) {
    const int qi = c0 + lane;
#pragma unroll
    for (int k = 0; k < kTopK; k++)
      in.key[k] = qi < qn ? mw.topk[(int64_t)(q0 + qi) * kTopK + k] : kNoKey;
    in.nc = qi < qn ? mw.ncand[q0 + qi] : 0;
  };
  QIn nx;
  load_chunk(0, nx);
  for (int c0 = 0; c0 < qn; c0 += 64) {
    const int qi = c0 + lane;
    const bool valid = qi < qn;
    const QIn in = nx;
    if (c0 + 64 < qn) load_chunk(c0 + 64, nx);  // in flight while this chunk resolves
    const uint64_t* key = in.key;
    const int nc = in.nc;
    if (valid) set_best(qi, -1);
    int start = 0;
    while (start < 64 && c0 + start < qn) {
      const bool act = valid && lane >= start && nc > 0;
      // -- every lane's decision against the committed tables
      int d1 = INT_MAX, d2 = INT_MAX, i1 = -1, nel = 0, dlast = 0;
      if (act) {
#pragma unroll
        for (int k = 0; k < kTopK; k++) {
          if (key[k] == kNoKey) continue;
          const int d = key_dist(key[k]), idx = key_idx(key[k]);
          dlast = d;
          if (matched_dist[idx] <= d) continue;
          if (nel == 0) {
            d1 = d;
            i1 = idx;
          } else if (nel == 1) {
            d2 = d;
          }
          nel++;
        }
      }
      // the kept list decides unless more candidates exist behind it and it holds no eligible
      // one, or a best within TH_LOW without a second -- and then still decides when the best
      // passes the ratio test against the last kept distance (a second behind the list is no
      // nearer; nnratio >= 0 keeps the product monotonic)
      bool rescan = false;
      if (act && nc > kTopK) {
        if (nel == 0) rescan = true;
        else if (nel == 1 && d1 <= kThLow)
          rescan = !(nnratio >= 0.0f && (float)d1 < (float)dlast * nnratio);
      }
      const bool acc = act && !rescan && nel > 0 && accepts(d1, d2);
      if (acc) atomicMin(&stamp[i1], lane);
      wave_lds_sync();
      bool conflict = false;
      if (act) {
#pragma unroll
        for (int k = 0; k < kTopK; k++)
          if (key[k] != kNoKey && stamp[key_idx(key[k])] < lane) conflict = true;
      }
      const uint64_t stop = __ballot(rescan || conflict);
      const int r = stop ? __ffsll((long long)stop) - 1 : 64;
      const bool r_conflict = r < 64 && ((__ballot(conflict) >> r) & 1ull);
      wave_lds_sync();
      if (acc) stamp[i1] = INT_MAX;
      if (acc && lane < r) {  // :325-333
        matched_dist[i1] = d1;
        matches21[i1] = qi;
        set_best(qi, i1);
      }
      wave_lds_sync();
      if (r < 64 && !r_conflict) {
        // lane r: rescanned alone, the candidates vMatchedDistance excludes left out by the scan
        const int qr = q0 + c0 + r;
        ScanCtx c;
        const bool okc = init_ctx(
            queries[qr], make_float2(io.prev_matched[2 * qr], io.prev_matched[2 * qr + 1]), P, &c);
        uint64_t top[kTopK];
        if (okc)
          scan_query<64, true>(c, cam, F, reinterpret_cast<const uint32_t*>(matched_dist), top,
                               lane, kp_cap);
        const uint64_t t1 = okc ? top[0] : kNoKey, t2 = okc ? top[1] : kNoKey;
        if (lane == r && t1 != kNoKey &&
            accepts(key_dist(t1), t2 == kNoKey ? INT_MAX : key_dist(t2))) {
          const int idx = key_idx(t1);
          matched_dist[idx] = key_dist(t1);
          matches21[idx] = qi;
          set_best(qi, idx);
        }
        wave_lds_sync();
        start = r + 1;
      } else {
        start = r;  // 64, or a lane to decide again against the tables as they are now
      }
    }
  }
  wave_lds_sync();
  // -- rotation histogram (:335-345) of every accepted query, then the tail
  if (check_ori) {
    for (int qi = lane; qi < qn; qi += 64) {
      const int idx = get_best(qi);
      int bin = -1;
      if (idx >= 0) {
        bin = rot_bin(queries[q0 + qi].angle, F.kps[idx].angle);
        atomicAdd(&hist[bin], 1);
      }
      if (qi < kResolveLdsQ) s_bin[qi] = (int8_t)bin;
      else mw.rot_bin[q0 + qi] = bin;
    }
  }
  wave_lds_sync();
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (check_ori) three_maxima(hist, &ind1, &ind2, &ind3);
  int nm = 0;
  for (int qi = lane; qi < qn; qi += 64) {
    const int idx = get_best(qi);
    bool holds = idx >= 0 && matches21[idx] == qi;
    if (holds && check_ori) {
      const int bin = qi < kResolveLdsQ ? (int)s_bin[qi] : mw.rot_bin[q0 + qi];
      if (bin != ind1 && bin != ind2 && bin != ind3) holds = false;  // :359-372
    }
    io.matches12[q0 + qi] = holds ? idx : -1;
    if (holds) {  // :377-379
      const KeyPoint& kp = F.kps[idx];
      io.prev_matched[2 * (q0 + qi)] = kp.x;
      io.prev_matched[2 * (q0 + qi) + 1] = kp.y;
      nm++;
    }
  }
  nm = wave_sum(nm);
  if (lane == 0) io.nmatches[f] = nm;
}

// The candidate search of every frame's queries, then the query type's in-order resolution pass.
template <typename Q>
static void launch_search(const FrameKps& cur, const float* u_right, int64_t ur_stride,
                          const Camera& cam, const OrbGeomDev& g, const Q* queries,
                          const typename SearchTraits<Q>::Pose* poses, int th, float nnratio,
                          int n_frames, int max_q, const GridWorkspace& gw,
                          const MatchWorkspace& mw, const typename SearchTraits<Q>::IO& io,
                          hipStream_t st) {
  using T = SearchTraits<Q>;
  constexpr int kPerBlock = 4 * (64 / T::kLanes);  // queries per work-group of search_cand
  if (max_q > 0)
    SLAMGPU_LAUNCH("search_cand", st, search_cand_kernel<Q>,
                   dim3((max_q + kPerBlock - 1) / kPerBlock, n_frames), dim3(256), 0, st, cur,
                   u_right, ur_stride, cam, g.dev, queries, poses, th, gw, mw, io);
  if constexpr (T::kInit)
    SLAMGPU_LAUNCH("init_resolve", st, init_resolve_kernel, dim3(n_frames), dim3(64), 0, st, cur,
                   cam, g.dev, queries, poses, gw, mw, io);
  else
    SLAMGPU_LAUNCH("search_resolve", st, search_resolve_kernel<Q>, dim3(n_frames), dim3(64), 0,
                   st, cur, u_right, ur_stride, cam, g.dev, queries, poses, th, nnratio, gw, mw,
                   io);
}

void launch_search_init(const FrameKps& cur, const Camera& cam, const OrbGeomDev& g,
                        const InitQuery* queries, const InitSearch* params, int n_frames,
                        int max_q, const GridWorkspace& gw, const MatchWorkspace& mw,
                        const InitIO& io, hipStream_t st) {
  launch_search(cur, nullptr, 0, cam, g, queries, params, 0, 0.0f, n_frames, max_q, gw, mw, io,
                st);
}

void launch_search_frame(const FrameKps& cur, const float* u_right, int64_t ur_stride,
                         const Camera& cam, const OrbGeomDev& g, const F2FQuery* queries,
                         const F2FPose* poses, int n_frames, int max_q, const GridWorkspace& gw,
                         const MatchWorkspace& mw, const MatchIO& io, hipStream_t st) {
  launch_search(cur, u_right, ur_stride, cam, g, queries, poses, 0, 0.0f, n_frames, max_q, gw, mw,
                io, st);
}

void launch_search_mps(const FrameKps& cur, const float* u_right, int64_t ur_stride,
                       const Camera& cam, const OrbGeomDev& g, const MpsQuery* queries,
                       float nnratio, int th, int n_frames, int max_q, const GridWorkspace& gw,
                       const MatchWorkspace& mw, const MatchIO& io, hipStream_t st) {
  launch_search(cur, u_right, ur_stride, cam, g, queries, (const F2FPose*)nullptr, th, nnratio,
                n_frames, max_q, gw, mw, io, st);
}

void launch_search_reloc(const FrameKps& cur, const float* u_right, int64_t ur_stride,
                         const Camera& cam, const OrbGeomDev& g, const RelocQuery* queries,
                         const RelocPose* poses, int n_frames, int max_q, const GridWorkspace& gw,
                         const MatchWorkspace& mw, const MatchIO& io, hipStream_t st) {
  launch_search(cur, u_right, ur_stride, cam, g, queries, poses, 0, 0.0f, n_frames, max_q, gw, mw,
                io, st);
}

}  // namespace slamgpu
