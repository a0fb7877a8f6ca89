// match_kernels.hip -- stereo and projection matching on gfx950, batched over frames.
//
//   stereo_rows     right-keypoint row table          Frame::ComputeStereoMatches :412-433
//   stereo_match    row-band Hamming + 11x11 SAD      :446-562   (one wave per left keypoint)
//   stereo_median   2.1 x median SAD rejection        :564-576   (one workgroup per frame)
//   grid_build      64x48 keypoint grid (CSR)         Frame::AssignFeaturesToGrid :234-248
//   search_cand     projection + window + Hamming     OrbMatcher::SearchByProjection (both
//   search_resolve  greedy in-order claims            overloads, orb_matcher.cpp:13-103 and
//                                                     :1312-1453) + rotation histogram; and the
//                                                     relocalisation overload (Frame, KeyFrame,
//                                                     sAlreadyFound, th, ORBdist) :1455-1582
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
#include "undistort.h"

namespace slamgpu {

// NT-thread exclusive scan of arr[0..n) in place; returns the total. wsum: NT / 64 ints.
template <int CAP, int NT = 256>
__device__ int scan256(int* arr, int n, int* wsum) {
  constexpr int per = (CAP + NT - 1) / NT;
  const int lane = threadIdx.x & 63, wid = wave_id();
  const int base = threadIdx.x * per;
  int loc[per];
  int s = 0;
#pragma unroll
  for (int i = 0; i < per; i++) {
    loc[i] = (base + i < n) ? arr[base + i] : 0;
    s += loc[i];
  }
  int x = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) {
    pre += (w < wid) ? wsum[w] : 0;
    tot += wsum[w];
  }
  pre += x - s;
#pragma unroll
  for (int i = 0; i < per; i++) {
    if (base + i < n) arr[base + i] = pre;
    pre += loc[i];
  }
  __syncthreads();
  return tot;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------------------------------
// Stereo (frame.cpp:406-577). Frame f: left = image 2f, right = image 2f+1.
constexpr int kMaxRows = 2048;

// NT threads per frame: 256 for batches, 1024 for the single-frame call (its one work-group is
// the whole launch: a quarter of the serial LDS-atomic loops per thread).
template <int NT>
__device__ __forceinline__ void stereo_rows_body(int f, const OrbGeom* __restrict__ g,
                                                 const FrameKps& ext, int nrows,
                                                 const StereoWorkspace& ws,
                                                 uint32_t* __restrict__ err) {
  __shared__ int cnt[kMaxRows + 1];
  __shared__ int wsum[NT / 64];
  const int tid = threadIdx.x;
  const int ir = 2 * f + 1;
  const KeyPoint* kr = ext.kps + ir * ext.stride;
  const int nr = ext.n[ir * ext.n_stride];
  int* rs = ws.row_start + (int64_t)f * (nrows + 1);
  uint2* items = ws.row_items + (int64_t)f * ws.row_cap;
  for (int i = tid; i <= nrows; i += NT) cnt[i] = 0;
  __syncthreads();
  // a thread's keypoints are loaded kChunk at a time before their row updates: one load latency
  // per chunk instead of one per keypoint (a single frame runs this as one work-group)
  constexpr int kChunk = 2048 / NT;
  // the row items carry the candidate's octave and x, the matcher's first filter (one load per
  // candidate instead of the item and then its keypoint)
  uint2 kit[kChunk];
  auto row_span = [&](int base, int (&lo)[kChunk], int (&hi)[kChunk]) {
    float ky[kChunk];
    int ko[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; u++) {
      const int i = base + NT * u + tid;
      ky[u] = 0.0f;
      ko[u] = -1;
      if (i < nr) {
        ky[u] = kr[i].y;
        ko[u] = kr[i].octave;
        kit[u] = make_uint2((uint32_t)i | (uint32_t)ko[u] << 16, __float_as_uint(kr[i].x));
      }
    }
#pragma unroll
    for (int u = 0; u < kChunk; u++) {
      lo[u] = 0;
      hi[u] = -1;
      if (ko[u] >= 0) {
        const float r = 2.0f * g->lv[ko[u]].scale;
        lo[u] = max((int)floorf(ky[u] - r), 0);
        hi[u] = min((int)ceilf(ky[u] + r), nrows - 1);
      }
    }
  };
  for (int base = 0; base < nr; base += NT * kChunk) {
    int lo[kChunk], hi[kChunk];
    row_span(base, lo, hi);
#pragma unroll
    for (int u = 0; u < kChunk; u++)
      for (int yi = lo[u]; yi <= hi[u]; ++yi) atomicAdd(&cnt[yi], 1);
  }
  __syncthreads();
  const int total = scan256<kMaxRows + 1, NT>(cnt, nrows, wsum);
  for (int i = tid; i < nrows; i += NT) rs[i] = cnt[i];
  if (tid == 0) {
    rs[nrows] = total;
    if (total > ws.row_cap) atomicOr(err, kErrRowOverflow);
  }
  __syncthreads();
  for (int base = 0; base < nr; base += NT * kChunk) {
    int lo[kChunk], hi[kChunk];
    row_span(base, lo, hi);
#pragma unroll
    for (int u = 0; u < kChunk; u++)
      for (int yi = lo[u]; yi <= hi[u]; ++yi) {
        const int pos = atomicAdd(&cnt[yi], 1);
        if (pos < ws.row_cap) items[pos] = kit[u];
      }
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void stereo_rows_kernel(const OrbGeom* __restrict__ g,
                                                         FrameKps ext, int nrows,
                                                         StereoWorkspace ws,
                                                         uint32_t* __restrict__ err) {
  stereo_rows_body<NT>(blockIdx.x, g, ext, nrows, ws, err);
}

// One left keypoint per G = 16 lanes, four per wave: the Hamming stage is a chain of dependent
// loads per keypoint (row table -> candidates -> descriptors), so several independent chains per
// wave hide the latency at the same occupancy; in the SAD stage the 16 lanes are one DPP row, one
// lane per window row.
template <int G>
__device__ __forceinline__ uint32_t group_min(uint32_t v) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));

// The u16 pair (byte p, byte p + 1) of the byte string e[0], e[1], ... (little-endian dwords),
// p a constant: one v_perm, its high bytes the selector's constant zero (0x0c).
__device__ __forceinline__ uint32_t byte_pair(const uint32_t* e, int p) {
  const int q = p >> 2;
  switch (p & 3) {
    case 0: return __builtin_amdgcn_perm(0u, e[q], 0x0c010c00u);
    case 1: return __builtin_amdgcn_perm(0u, e[q], 0x0c020c01u);
    case 2: return __builtin_amdgcn_perm(0u, e[q], 0x0c030c02u);
    default: return __builtin_amdgcn_perm(e[q + 1], e[q], 0x0c040c03u);
  }
}

template <int G>
__global__ __launch_bounds__(256) void stereo_match_kernel(ImageBatch b,
                                                           const OrbGeom* __restrict__ g,
                                                           FrameKps ext, Camera cam, int nrows,
                                                           StereoWorkspace ws, StereoOut out) {
  static_assert(G == 16, "the SAD stage puts a keypoint's 11 window rows on one 16-lane DPP row");
  constexpr int NPW = 64 / G;  // keypoints per wave
  int f, bx;
  xcd_image_block(&f, &bx);  // a frame's work-groups share one XCD's L2 (its right keypoints)
  const int il = 2 * f, ir = 2 * f + 1;
  const int nl = ext.n[il * ext.n_stride];
  if (bx * 4 * NPW >= nl) return;  // the whole work-group
  const int lane = threadIdx.x & 63, grp = lane / G, hl = lane % G;
  const int iL = (bx * 4 + wave_id()) * NPW + grp;
  const bool valid = iL < nl;
  bool ok = valid;
  KeyPoint kpL{};
  if (ok) kpL = ext.kps[il * ext.stride + iL];
  const int levelL = kpL.octave;
  const float vL = kpL.y, uL = kpL.x;
  const int row = (int)vL;
  ok = ok && row >= 0 && row < nrows;
  const int* rs = ws.row_start + (int64_t)f * (nrows + 1);
  const uint2* items = ws.row_items + (int64_t)f * ws.row_cap;
  int c0 = 0, c1 = 0;
  if (ok) {
    c0 = rs[row];
    c1 = min(rs[row + 1], ws.row_cap);
  }
  ok = ok && c0 < c1;
  const float baseline = cam.bf / cam.fx;  // see DESIGN.md: maxD is UB in the reference (:436)
  const float minZ = baseline, minD = 0, maxD = cam.bf / minZ;
  const float minU = uL - maxD, maxU = uL - minD;
  ok = ok && !(maxU < 0);
  const uint8_t* dL = ext.desc + (il * ext.stride + (ok ? iL : 0)) * 32;
  const uint8_t* dRb = ext.desc + ir * ext.stride * 32;
  uint32_t best = ((uint32_t)kThHigh << 16) | 0xffffu;
  float bestU = 0.0f;  // x of this lane's best candidate
  if (ok) {
    // kCandU candidates per lane at a time, each stage's loads all in flight before the next
    // stage needs them: row items -> (octave, x) -> descriptors -> distances (the loop was a
    // chain of three dependent loads per candidate)
    // 2 and 4 measured equal (0.35 ms/step), 2 holds fewer VGPRs; with the packed row items
    // (two loads per candidate) 2 is still best, as are 16 lanes per keypoint (8 / 32 lanes and
    // 4 candidates: 0.29-0.36 ms against 0.28, profiles/r6d_stereo_lanes_ab.log)
    constexpr int kCandU = 2;
    const uint4* dLq = reinterpret_cast<const uint4*>(dL);
    const uint4 l0 = dLq[0], l1 = dLq[1];
    for (int cb = c0 + hl; cb < c1; cb += G * kCandU) {
      int iR[kCandU];
      float uR[kCandU];
      bool pass[kCandU];
#pragma unroll
      for (int u = 0; u < kCandU; u++) {
        const int c = cb + G * u;
        const uint2 it = c < c1 ? items[c] : make_uint2(0xffffffffu, 0u);
        iR[u] = (int)(it.x & 0xffffu);
        const int oct = (int)(it.x >> 16);
        uR[u] = __uint_as_float(it.y);
        pass[u] = c < c1 && oct >= levelL - 1 && oct <= levelL + 1 && uR[u] >= minU &&
                  uR[u] <= maxU;
      }
      uint4 r0[kCandU], r1[kCandU];
#pragma unroll
      for (int u = 0; u < kCandU; u++)
        if (pass[u]) {
          const uint4* dr = reinterpret_cast<const uint4*>(dRb + iR[u] * 32);
          r0[u] = dr[0];
          r1[u] = dr[1];
        }
#pragma unroll
      for (int u = 0; u < kCandU; u++)
        if (pass[u]) {
          const int dist = __popc(l0.x ^ r0[u].x) + __popc(l0.y ^ r0[u].y) + __popc(l0.z ^ r0[u].z) +
                           __popc(l0.w ^ r0[u].w) + __popc(l1.x ^ r1[u].x) + __popc(l1.y ^ r1[u].y) +
                           __popc(l1.z ^ r1[u].z) + __popc(l1.w ^ r1[u].w);
          const uint32_t key = ((uint32_t)dist << 16) | (uint32_t)iR[u];
          if (dist < kThHigh && key < best) {
            best = key;
            bestU = uR[u];
          }
        }
    }
  }
  const uint32_t mine = best;
  best = group_min<G>(best);
  // the x of the group's best candidate from the lane that found it (keys are unique)
  const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (G * grp);
  const uint64_t hit = __ballot(mine == best) & gmask;
  const float uRbest = __shfl(bestU, hit ? __builtin_ctzll(hit) : lane, 64);
  const int bestDist = (int)(best >> 16);
  const int thOrbDist = (kThHigh + kThLow) / 2;
  ok = ok && bestDist < thOrbDist;
  // sliding-window SAD at the left keypoint's level (:481-531)
  const float uR0 = ok ? uRbest : 0.f;
  const float scaleFactor = g->lv[levelL].inv_scale;
  const float scaleduL = roundf(kpL.x * scaleFactor);
  const float scaledvL = roundf(kpL.y * scaleFactor);
  const float scaleduR0 = roundf(uR0 * scaleFactor);
  const int w = 5, L = 5;
  const LevelGeom& LG = g->lv[levelL];
  const float iniu = scaleduR0 + L - w;
  const float endu = scaleduR0 + L + w + 1;
  ok = ok && !(iniu < 0 || endu >= (float)LG.w);
  const int yc = (int)scaledvL, xcl = (int)scaleduL, xcr = (int)scaleduR0;
  // windows the reference would reject with a cv::Mat ROI assertion are treated as no match
  ok = ok && !(yc - w < 0 || yc + w >= LG.h || xcl - w < 0 || xcl + w >= LG.w || xcr - L - w < 0);
  // Every left keypoint's outputs have one writer: lane 0 of its group here when it has no
  // candidate window, lane 10 after the SAD stage otherwise.
  const int64_t o = (int64_t)f * g->kp_cap + iL;
  if (valid && !ok && hl == 0) {
    out.u_right[o] = -1.0f;
    out.depth[o] = -1.0f;
    ws.sad[o] = -1;
  }
  if (!ok) return;  // whole groups leave: every DPP row below is full
  // SAD of the 11 window offsets (level levelL, window centres (xcl, yc) and (xcr, yc)): lane
  // r = 0..10 of the group owns window row yc - 5 + r and holds it in registers, 16 left bytes
  // from column al = (xcl - 5) & ~3 and 28 right bytes from ar = (xcr - 10) & ~3 (lanes 11..15
  // repeat row 10; their sums are not used). The loads go through buffer descriptors over the
  // frame's two level-0 images and its two pyramids (wave-uniform, whatever levels the wave's four
  // keypoints are on), so the lane offset is 32 bits and a read past the end of an image's last
  // row returns zeros; no pair uses such a byte, nor one past the row's last pixel. Caller images
  // whose base or pitch is no multiple of 4 are read byte by byte.
  const LevelGeom& L0 = g->lv[0];
  const uint8_t* const img_l = batch_image(b, il);
  const uint8_t* const img_r = batch_image(b, ir);
  const bool dw = ((((uintptr_t)img_l | (uintptr_t)img_r) | (uintptr_t)b.in_pitch) & 3) == 0;
  // dword loads may read the dword that holds the row's last pixel, as the pyramid rows allow
  const int bytes0 = __builtin_amdgcn_readfirstlane((L0.h - 1) * b.in_pitch +
                                                    (dw ? (L0.w + 3) & ~3 : L0.w));
  const int bytesp = __builtin_amdgcn_readfirstlane((int)g->pyr_bytes);
  const __amdgpu_buffer_rsrc_t rs_l0 = buf_rsrc(img_l, bytes0), rs_r0 = buf_rsrc(img_r, bytes0);
  const __amdgpu_buffer_rsrc_t rs_lp = buf_rsrc(b.pyr + (int64_t)il * g->pyr_bytes, bytesp);
  const __amdgpu_buffer_rsrc_t rs_rp = buf_rsrc(b.pyr + (int64_t)ir * g->pyr_bytes, bytesp);
  const int al = (xcl - 5) & ~3, ar = (xcr - 10) & ~3;
  const int wy = yc - 5 + min(hl, 10);
  uint32_t lw[4], rw[7];
  auto rows = [&](__amdgpu_buffer_rsrc_t rl, __amdgpu_buffer_rsrc_t rr, int ol, int orr) {
    const u32x4_t l4 = __builtin_amdgcn_raw_buffer_load_b128(rl, ol, 0, 0);
    const u32x4_t r4 = __builtin_amdgcn_raw_buffer_load_b128(rr, orr, 0, 0);
    const u32x3_t r3 = __builtin_amdgcn_raw_buffer_load_b96(rr, orr + 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) lw[i] = l4[i], rw[i] = r4[i];
#pragma unroll
    for (int i = 0; i < 3; i++) rw[4 + i] = r3[i];
  };
  if (levelL != 0) {
    const int ro = (int)LG.offset + wy * LG.pitch;
    rows(rs_lp, rs_rp, ro + al, ro + ar);
  } else if (dw) {
    const int ro = wy * b.in_pitch;
    rows(rs_l0, rs_r0, ro + al, ro + ar);
  } else {
    const int ro = wy * b.in_pitch;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      lw[i] = 0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        lw[i] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs_l0, ro + al + 4 * i + j, 0, 0)
                 << (8 * j);
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
      rw[i] = 0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        rw[i] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs_r0, ro + ar + 4 * i + j, 0, 0)
                 << (8 * j);
    }
  }
  // Once per lane: the left row's 11 bytes from its window's first column (a), the right row's 21
  // bytes from its first offset's first column (e), and from the centre row's lane (5) the dwords
  // that hold the centre pixels cl = a[5] and cr_k = e[k + 5] (offset k's window is e[k..k+10]).
  const uint32_t oL = (uint32_t)(xcl - 5 - al), oR = (uint32_t)(xcr - 10 - ar);
  uint32_t a[3], e[6], ec[6];
#pragma unroll
  for (int i = 0; i < 3; i++) a[i] = __builtin_amdgcn_alignbyte(lw[i + 1], lw[i], oL);
#pragma unroll
  for (int i = 0; i < 6; i++) e[i] = __builtin_amdgcn_alignbyte(rw[i + 1], rw[i], oR);
  const uint32_t ac = __shfl(a[1], 5, G);
#pragma unroll
  for (int i = 0; i < 6; i++) ec[i] = i >= 1 && i <= 3 ? __shfl(e[i], 5, G) : 0u;
  // A task (offset k, window row) sums |(IL - cl) - (IR - cr_k)| over 11 pixels as v_sad_u16 on
  // u16 pairs: (IL + 512) against (IR + 512 + cl - cr_k); every half stays within [257, 1022].
  // The left pairs are built once (v_perm takes the high byte 0x02 = +512 from a constant
  // operand), the right pairs once per byte position (offsets k and k + 2 share all but one), and
  // cl - cr_k + 512 is added per offset. The 12th element of a task is (cl + 512) against (cr_k +
  // 512 + cl - cr_k): equal on both sides, from the same additions as the rest.
  constexpr uint32_t kBias = 0x02020202u;  // a u16 half's high byte: + 512
  constexpr uint32_t kBias2 = 0x02000200u;  // + 512 on both halves
  uint32_t A[6];
#pragma unroll
  for (int j = 0; j < 5; j++)
    A[j] = __builtin_amdgcn_perm(kBias, a[j >> 1], (j & 1) ? 0x04030402u : 0x05010400u);
  A[5] = __builtin_amdgcn_perm(ac, a[2], 0x0c050c02u) + kBias2;          // (a[10], cl) + 512
  const uint32_t C = __builtin_amdgcn_perm(0u, ac, 0x0c010c01u) + kBias2;  // (cl, cl) + 512
  int S[11];
#pragma unroll
  for (int k = 0; k < 11; k++) {
    const int c = k + 5, hc = c & 3, p = k + 10, h = p & 3;  // centre and last byte of offset k
    const uint32_t crr =
        __builtin_amdgcn_perm(0u, ec[c >> 2], 0x0c000c00u | (uint32_t)hc | (uint32_t)hc << 16);
    const uint32_t dd = C - crr;  // (cl + 512 - cr_k) in both halves, each positive: no borrow
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 5; j++)
      acc = __builtin_amdgcn_sad_u16(A[j], byte_pair(e, k + 2 * j) + dd, acc);
    const uint32_t last = __builtin_amdgcn_perm(
        ec[c >> 2], e[p >> 2], 0x0c000c00u | (uint32_t)h | (uint32_t)(4 + hc) << 16);  // (e[p], cr_k)
    S[k] = (int)__builtin_amdgcn_sad_u16(A[5], last + dd, acc);
  }
  // rows summed per offset down the DPP row: lane 10 ends with rows 0..10
#pragma unroll
  for (int k = 0; k < 11; k++) {
    S[k] += __builtin_amdgcn_update_dpp(0, S[k], 0x111, 0xf, 0xf, true);  // row_shr:1
    S[k] += __builtin_amdgcn_update_dpp(0, S[k], 0x112, 0xf, 0xf, true);  // row_shr:2
    S[k] += __builtin_amdgcn_update_dpp(0, S[k], 0x114, 0xf, 0xf, true);  // row_shr:4
    S[k] += __builtin_amdgcn_update_dpp(0, S[k], 0x118, 0xf, 0xf, true);  // row_shr:8
  }
  if (hl != 10) return;
  float vDists[11];
#pragma unroll
  for (int k = 0; k < 11; k++) vDists[k] = (float)S[k];
  int bestSad = 0x7fffffff, bestincR = 0;
#pragma unroll
  for (int k = 0; k < 11; k++) {
    if (vDists[k] < (float)bestSad) {
      bestSad = (int)vDists[k];
      bestincR = k - L;
    }
  }
  float o_ur = -1.0f, o_depth = -1.0f;
  int o_sad = -1;
  if (!(bestincR == -L || bestincR == L)) {
    const float dist1 = vDists[L + bestincR - 1];
    const float dist2 = vDists[L + bestincR];
    const float dist3 = vDists[L + bestincR + 1];
    const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
    if (!(deltaR < -1 || deltaR > 1)) {
      float bestuR = LG.scale * ((float)xcr + (float)bestincR + deltaR);
      float disparity = (uL - bestuR);
      if (disparity >= minD && disparity < maxD) {
        if (disparity <= 0) {
          disparity = 0.01f;
          bestuR = uL - 0.01f;
        }
        o_depth = cam.bf / disparity;
        o_ur = bestuR;
        o_sad = bestSad;
      }
    }
  }
  out.u_right[o] = o_ur;
  out.depth[o] = o_depth;
  ws.sad[o] = o_sad;
}

// Median SAD filter (:564-576): drop matches whose SAD >= 2.1 * median. The median (element
// n / 2 of the ascending sort, :564-566) is found by an MSB-first radix select over the SADs
// (four 8-bit digit histograms) instead of sorting them.
// pack (the single-frame call, frame 0 only): the frame's final u_right / depth also go to the
// packed host-mirror record (frame_pack_kernel's layout), and the device error word to its
// header slot 8 -- no frame_pack launch after this one on the call's critical path.
// NT threads per frame (1024 for the single-frame call). The digit rounds start at the highest
// non-zero byte of the OR of all SADs (SADs are below 121 * 510 < 2^16: two rounds, not four).
template <int NT>
__global__ __launch_bounds__(NT) void stereo_median_kernel(const OrbGeom* __restrict__ g,
                                                           FrameKps ext, StereoWorkspace ws,
                                                           StereoOut out,
                                                           uint8_t* __restrict__ pack,
                                                           const uint32_t* __restrict__ err) {
  constexpr int kCap = 4096;
  __shared__ uint32_t vals[kCap];
  __shared__ int hist[256];
  __shared__ int n_valid, s_digit, s_rank;
  __shared__ uint32_t s_or;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nl = min(ext.n[2 * f * ext.n_stride], kCap);
  const int64_t base = (int64_t)f * g->kp_cap;
  if (tid == 0) {
    n_valid = 0;
    s_or = 0;
  }
  __syncthreads();
  uint32_t vor = 0;
  for (int i0 = 0; i0 < nl; i0 += NT * 4) {  // 4 loads in flight per thread
    int sv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + NT * u + tid;
      sv[u] = i < nl ? ws.sad[base + i] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (sv[u] >= 0) {
        vals[atomicAdd(&n_valid, 1)] = (uint32_t)sv[u];
        vor |= (uint32_t)sv[u];
      }
  }
  vor = wave_or(vor);
  if (lane == 0 && vor) atomicOr(&s_or, vor);
  __syncthreads();
  const int n = n_valid;
  const uint32_t all_or = s_or;
  // n == 0: the reference indexes an empty vector here (UB); we skip the filter
  uint32_t prefix = 0, mask = 0;
  int k = n / 2;  // rank of the median among the values matching prefix under mask
  const int top = all_or >> 24 ? 24 : all_or >> 16 ? 16 : all_or >> 8 ? 8 : 0;
  for (int shift = top; shift >= 0 && n > 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      const uint32_t v = vals[i];
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid < 64) {  // the digit whose cumulative count passes k: lane owns bins 4 lane .. +3
      int h[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        h[j] = hist[4 * lane + j];
        sum += h[j];
      }
      int x = sum;  // inclusive scan over the wave
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
      }
      const int before = x - sum;
      if (before <= k && k < x) {  // exactly one lane
        int acc = before, d = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (d == 0 && acc + h[j] > k) d = j + 1;
          else if (d == 0) acc += h[j];
        s_digit = 4 * lane + d - 1;
        s_rank = k - acc;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)s_digit << shift;
    mask |= 255u << shift;
    k = s_rank;
    __syncthreads();
  }
  const float median = (float)(int)prefix;
  const float thDist = (1.5f * 1.4f) * median;
  const size_t kc = (size_t)g->kp_cap;
  float* const pur = pack && f == 0
                         ? reinterpret_cast<float*>(pack + 16 + 2 * kc * sizeof(KeyPoint) + 2 * kc * 32)
                         : nullptr;
  const int nall = pur ? min(max(ext.n[0], 0), (int)kc) : nl;
  for (int i = tid; i < nall; i += NT) {
    const int s = i < nl ? ws.sad[base + i] : -1;
    if (n > 0 && s >= 0 && !((float)s < thDist)) {
      out.u_right[base + i] = -1.0f;
      out.depth[base + i] = -1.0f;
      ws.sad[base + i] = -1;
      if (pur) pur[i] = pur[kc + i] = -1.0f;
    } else if (pur) {
      pur[i] = out.u_right[base + i];
      pur[kc + i] = out.depth[base + i];
    }
  }
  __syncthreads();  // every error bit this stream's kernels raise is in err by now
  if (pur && tid == 0) reinterpret_cast<uint32_t*>(pack)[2] = *err;
}

// ---------------------------------------------------------------------------------------
// Frame results -> the host mirror's layout (see match_kernels.h), copied as dwords.
// parts: bit 0 -- the counts, both views' keypoints and descriptors, the error word to header
// slot 12; bit 1 -- u_right / depth, the error word to slot 8 (stereo_median_kernel does this part
// itself in the single-frame call). The host ORs the two error slots.
__device__ __forceinline__ void frame_pack_body(const FrameKps& ext,
                                                const float* __restrict__ u_right,
                                                const float* __restrict__ depth,
                                                const uint32_t* __restrict__ err, int kp_cap,
                                                uint8_t* __restrict__ dst, int parts, int gid,
                                                int gsz) {
  const int c0 = ext.n[0], c1 = ext.n[ext.n_stride];
  const int n0 = min(max(c0, 0), kp_cap), n1 = min(max(c1, 0), kp_cap);
  const size_t kc = (size_t)kp_cap;
  if (gid == 0) {
    int* h = reinterpret_cast<int*>(dst);
    if (parts & 1) {
      h[0] = c0;
      h[1] = c1;
      h[3] = (int)*err;
    }
    if (parts & 2) h[2] = (int)*err;
  }
  auto copy = [&](const void* src, size_t dst_off, int words) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + dst_off);
    for (int i = gid; i < words; i += gsz) d[i] = s[i];
  };
  const size_t kps_off = 16, desc_off = kps_off + 2 * kc * sizeof(KeyPoint);
  const size_t ur_off = desc_off + 2 * kc * 32, dp_off = ur_off + kc * sizeof(float);
  if (parts & 1) {
    copy(ext.kps, kps_off, 7 * n0);
    copy(ext.kps + ext.stride, kps_off + kc * sizeof(KeyPoint), 7 * n1);
    copy(ext.desc, desc_off, 8 * n0);
    copy(ext.desc + 32 * ext.stride, desc_off + 32 * kc, 8 * n1);
  }
  if (parts & 2) {
    copy(u_right, ur_off, n0);
    copy(depth, dp_off, n0);
  }
}
__global__ __launch_bounds__(256) void frame_pack_kernel(FrameKps ext,
                                                         const float* __restrict__ u_right,
                                                         const float* __restrict__ depth,
                                                         const uint32_t* __restrict__ err,
                                                         int kp_cap, uint8_t* __restrict__ dst,
                                                         int parts) {
  frame_pack_body(ext, u_right, depth, err, kp_cap, dst, parts,
                  blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

void launch_frame_pack(const FrameKps& ext, const float* u_right, const float* depth,
                       const uint32_t* err, int kp_cap, uint8_t* dst, hipStream_t st, int parts) {
  static_assert(sizeof(KeyPoint) == 28, "keypoint layout");
  SLAMGPU_LAUNCH("frame_pack", st, frame_pack_kernel, dim3(32), dim3(256), 0, st, ext, u_right,
                 depth, err, kp_cap, dst, parts);
}

__global__ void trace_marker_kernel() {}

void launch_trace_marker(int id, hipStream_t st) {
  hipLaunchKernelGGL(trace_marker_kernel, dim3(1, id), dim3(64), 0, st);
}

void launch_stereo(const ImageBatch& b, const OrbGeomDev& gd, const Camera& cam, int n_frames,
                   const StereoWorkspace& ws, const StereoOut& out, hipStream_t st,
                   uint8_t* pack, bool rows_done) {
  const OrbGeom& g = *gd.host;
  FrameKps ext{gd.out.kps, gd.out.desc, gd.out.nkps, g.kp_cap, 1};
  const int nrows = g.lv[0].h;
  if (rows_done) {  // frame_aux_kernel built them
  } else if (n_frames <= 8)
    SLAMGPU_LAUNCH("stereo_rows", st, stereo_rows_kernel<1024>, dim3(n_frames), dim3(1024), 0, st,
                   gd.dev, ext, nrows, ws, gd.ws.err);
  else
    SLAMGPU_LAUNCH("stereo_rows", st, stereo_rows_kernel<256>, dim3(n_frames), dim3(256), 0, st,
                   gd.dev, ext, nrows, ws, gd.ws.err);
  constexpr int kG = 16, kPerBlock = 4 * (64 / kG);
  SLAMGPU_LAUNCH("stereo_match", st, stereo_match_kernel<kG>,
                 dim3((g.kp_cap + kPerBlock - 1) / kPerBlock, n_frames), dim3(256), 0, st, b,
                 gd.dev, ext, cam, nrows, ws, out);
  if (n_frames <= 8)
    SLAMGPU_LAUNCH("stereo_median", st, stereo_median_kernel<1024>, dim3(n_frames), dim3(1024), 0,
                   st, gd.dev, ext, ws, out, pack, gd.ws.err);
  else
    SLAMGPU_LAUNCH("stereo_median", st, stereo_median_kernel<256>, dim3(n_frames), dim3(256), 0,
                   st, gd.dev, ext, ws, out, pack, gd.ws.err);
}

// ---------------------------------------------------------------------------------------
// Grid (AssignFeaturesToGrid + PosInGrid, frame.cpp:234-248, 339-346).
__device__ __forceinline__ int grid_cell(const Camera& cam, float x, float y) {
  int px, py;
  if (!pos_in_grid(x, y, cam.min_x, cam.min_y, cam.cell_w, cam.cell_h, &px, &py)) return -1;
  return px * kGridRows + py;
}

template <int NT>
__device__ __forceinline__ void grid_build_body(int f, const FrameKps& cur, const Camera& cam,
                                                int kp_cap, const GridWorkspace& gw) {
  __shared__ int cnt[kGridCells + 1];
  __shared__ int wsum[NT / 64];
  const int tid = threadIdx.x;
  const KeyPoint* k = cur.kps + f * cur.stride;
  const int n = cur.n[f * cur.n_stride];
  int* cs = gw.cell_start + (int64_t)f * (kGridCells + 1);
  uint4* items = gw.cell_items + (int64_t)f * kp_cap;
  for (int i = tid; i <= kGridCells; i += NT) cnt[i] = 0;
  // cells of a thread's keypoints, kChunk loads in flight at a time; the items carry the fields
  // the projection searches filter on first (one load per candidate instead of two)
  constexpr int kChunk = 2048 / NT;
  float kx[kChunk], ky[kChunk];
  int ko[kChunk];
  auto cells = [&](int base, int (&c)[kChunk]) {
#pragma unroll
    for (int u = 0; u < kChunk; u++) {
      const int i = base + NT * u + tid;
      kx[u] = ky[u] = 0.0f;
      ko[u] = 0;
      if (i < n) {
        kx[u] = k[i].x;
        ky[u] = k[i].y;
        ko[u] = k[i].octave;
      }
    }
#pragma unroll
    for (int u = 0; u < kChunk; u++)
      c[u] = base + NT * u + tid < n ? grid_cell(cam, kx[u], ky[u]) : -1;
  };
  __syncthreads();
  for (int base = 0; base < n; base += NT * kChunk) {
    int c[kChunk];
    cells(base, c);
#pragma unroll
    for (int u = 0; u < kChunk; u++)
      if (c[u] >= 0) atomicAdd(&cnt[c[u]], 1);
  }
  __syncthreads();
  const int total = scan256<kGridCells + 1, NT>(cnt, kGridCells, wsum);
  for (int i = tid; i < kGridCells; i += NT) cs[i] = cnt[i];
  if (tid == 0) cs[kGridCells] = total;
  __syncthreads();
  for (int base = 0; base < n; base += NT * kChunk) {
    int c[kChunk];
    cells(base, c);
#pragma unroll
    for (int u = 0; u < kChunk; u++)
      if (c[u] >= 0)
        items[atomicAdd(&cnt[c[u]], 1)] =
            make_uint4((uint32_t)(base + NT * u + tid) | (uint32_t)ko[u] << 16,
                       __float_as_uint(kx[u]), __float_as_uint(ky[u]), 0u);
  }
}
__global__ __launch_bounds__(256) void grid_build_kernel(FrameKps cur, Camera cam, int kp_cap,
                                                         GridWorkspace gw) {
  grid_build_body<256>(blockIdx.x, cur, cam, kp_cap, gw);
}

void launch_grid(const FrameKps& cur, const Camera& cam, int n_frames, int kp_cap,
                 const GridWorkspace& gw, hipStream_t st) {
  SLAMGPU_LAUNCH("grid_build", st, grid_build_kernel, dim3(n_frames), dim3(256), 0, st, cur, cam,
                 kp_cap, gw);
}

// The single-frame call's three independent steps after the descriptors, as three work-groups
// of one launch (side by side on three CUs): blockIdx.y 0 the stereo row tables, 1 the left
// view's grid, 2 the counts / keypoints / descriptors packed into the host mirror.
__global__ __launch_bounds__(1024) void frame_aux_kernel(const OrbGeom* __restrict__ g,
                                                         FrameKps ext, int nrows,
                                                         StereoWorkspace ws, uint32_t* err,
                                                         FrameKps left, Camera cam, int kp_cap,
                                                         GridWorkspace gw, uint8_t* pack) {
  switch (blockIdx.y) {
    case 0: stereo_rows_body<1024>(0, g, ext, nrows, ws, err); break;
    case 1: grid_build_body<1024>(0, left, cam, kp_cap, gw); break;
    default:
      frame_pack_body(ext, nullptr, nullptr, err, kp_cap, pack, 1, threadIdx.x, 1024);
      break;
  }
}

void launch_frame_aux(const OrbGeomDev& gd, const FrameKps& left, const Camera& cam,
                      const GridWorkspace& gw, const StereoWorkspace& ws, uint8_t* pack,
                      hipStream_t st) {
  const OrbGeom& g = *gd.host;
  FrameKps ext{gd.out.kps, gd.out.desc, gd.out.nkps, g.kp_cap, 1};
  SLAMGPU_LAUNCH("frame_aux", st, frame_aux_kernel, dim3(1, 3), dim3(1024), 0, st, gd.dev, ext,
                 g.lv[0].h, ws, gd.ws.err, left, cam, g.kp_cap, gw, pack);
}

// ---------------------------------------------------------------------------------------
// Frame::UndistortKeyPoints (frame.cpp:614-641): a thread per keypoint of every set, the
// keypoint copied with pt replaced by cv::undistortPoints (undistort.h; IEEE double, no
// contraction, bit-identical to the oracle). dist k1 == 0 copies (:616-619).
__global__ __launch_bounds__(256) void undistort_kernel(FrameKps src, KeyPoint* __restrict__ dst,
                                                        int64_t dst_stride, float fx, float fy,
                                                        float cx, float cy, Distortion dc) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= src.n[f * src.n_stride]) return;
  KeyPoint kp = src.kps[f * src.stride + i];
  if (dc.k[0] != 0.0f) undistort_point(fx, fy, cx, cy, dc, kp.x, kp.y, &kp.x, &kp.y);
  dst[f * dst_stride + i] = kp;
}

void launch_undistort(const FrameKps& src, KeyPoint* dst, int64_t dst_stride, const Camera& cam,
                      const Distortion& dc, int n_sets, int kp_cap, hipStream_t st) {
  SLAMGPU_LAUNCH("undistort", st, undistort_kernel, dim3((kp_cap + 255) / 256, n_sets), dim3(256),
                 0, st, src, dst, dst_stride, cam.fx, cam.fy, cam.cx, cam.cy, dc);
}

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

// The per-frame pose record of a query type (the local-map search has none).
template <typename Q>
struct SearchPose {
  using type = F2FPose;
};
template <>
struct SearchPose<RelocQuery> {
  using type = RelocPose;
};

template <>
struct SearchPose<InitQuery> {
  using type = InitSearch;
};

// The caller's arrays of a query type's search.
template <typename Q>
struct SearchIO {
  using type = MatchIO;
};
template <>
struct SearchIO<InitQuery> {
  using type = InitIO;
};

// The per-query setup of the query type's overload.
template <typename Q>
__device__ __forceinline__ bool make_ctx(const Q& q, const typename SearchPose<Q>::type* poses,
                                         int f, int th, const Camera& cam, const OrbGeom* g,
                                         ScanCtx* c) {
  if constexpr (std::is_same<Q, F2FQuery>::value) return f2f_ctx(q, poses[f], cam, g, c);
  else if constexpr (std::is_same<Q, RelocQuery>::value) return reloc_ctx(q, poses[f], cam, g, c);
  else return mps_ctx(q, th, g, c);
}

// SearchForInitialization reads neither u_right nor the slot state
__device__ __forceinline__ FrameView frame_view(int f, const FrameKps& cur, const float*,
                                                int64_t, const GridWorkspace& gw, const InitIO&,
                                                int kp_cap) {
  FrameView F;
  F.kps = cur.kps + f * cur.stride;
  F.desc = cur.desc + f * cur.stride * 32;
  F.u_right = nullptr;
  F.cell_start = gw.cell_start + (int64_t)f * (kGridCells + 1);
  F.cell_items = gw.cell_items + (int64_t)f * kp_cap;
  F.blocked = nullptr;
  return F;
}

__device__ __forceinline__ FrameView frame_view(int f, const FrameKps& cur, const float* u_right,
                                                int64_t ur_stride, const GridWorkspace& gw,
                                                const MatchIO& io, int kp_cap) {
  FrameView F;
  F.kps = cur.kps + f * cur.stride;
  F.desc = cur.desc + f * cur.stride * 32;
  F.u_right = u_right + f * ur_stride;
  F.cell_start = gw.cell_start + (int64_t)f * (kGridCells + 1);
  F.cell_items = gw.cell_items + (int64_t)f * kp_cap;
  F.blocked = io.blocked + f * io.mp_stride;
  return F;
}

#ifndef SEARCH_LANES
#define SEARCH_LANES 16
#endif
constexpr int kSearchG = SEARCH_LANES;  // lanes per query in search_cand (16 or 64)
// SearchForInitialization's window (windowSize 100: 200 x 200 px, some 300 grid cells and a few
// hundred keypoints of all levels, against a handful in the projection searches) is walked 64
// lanes wide: a quarter of the dependent cell / pair rounds per query, and its level-0 queries
// (some 440 to 870 waves) still fill the device.
template <typename Q>
constexpr int kSearchLanes = std::is_same<Q, InitQuery>::value ? 64 : kSearchG;
template <typename Q>
__global__ __launch_bounds__(256) void search_cand_kernel(
    FrameKps cur, const float* __restrict__ u_right, int64_t ur_stride, Camera cam,
    const OrbGeom* __restrict__ g, const Q* __restrict__ queries,
    const typename SearchPose<Q>::type* __restrict__ poses, int th, GridWorkspace gw,
    MatchWorkspace mw, typename SearchIO<Q>::type io) {
  constexpr bool kInit = std::is_same<Q, InitQuery>::value;
  constexpr int kG = kSearchLanes<Q>;
  int f, bx;
  xcd_image_block(&f, &bx);  // a frame's work-groups share one XCD's L2 (its grid and keypoints)
  // kG lanes per query: 64 / kG queries per wave
  const int lane = threadIdx.x & 63, gl = lane & (kG - 1);
  const int qi = (bx * 4 + wave_id()) * (64 / kG) + lane / kG;
  const int qcount = io.q_count[f];
  if (__builtin_amdgcn_readfirstlane((bx * 4 + wave_id()) * (64 / kG)) >= qcount) return;
  const bool live = qi < qcount;  // the wave's last groups may have no query
  const int q = io.q_start[f] + (live ? qi : 0);
  const FrameView F = frame_view(f, cur, u_right, ur_stride, gw, io, g->kp_cap);
  ScanCtx c;
  bool ok;
  if constexpr (kInit) ok = init_ctx(queries[q], make_float2(io.prev_matched[2 * q], io.prev_matched[2 * q + 1]),
                                   poses[f], &c) && live;
  else ok = make_ctx(queries[q], poses, f, th, cam, g, &c) && live;
  uint64_t top[kTopK];
  // a group without a query scans nothing but takes part in the merge
  const int n = scan_query<kG, kInit>(c, cam, F, nullptr, top, lane, g->kp_cap, !ok);
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
    const typename SearchPose<Q>::type* __restrict__ poses, int th, float nnratio,
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
  const FrameView F = frame_view(f, cur, u_right, ur_stride, gw, io, g->kp_cap);
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
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
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
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (mine >= 0) atomicMin(&owner[mine], lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        prev = mine;
      }
      // -- the first lane that needs a rescan ends this round's committed range
      const uint64_t rs = __ballot(act && navail < need && nc > kTopK);
      const int r = rs ? __ffsll((long long)rs) - 1 : 64;
      if (prev >= 0) owner[prev] = INT_MAX;  // committed claims move to claimed[]
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      auto commit = [&](bool doit, uint64_t c1, uint64_t c2) {
        const bool touched = doit && c1 != kNoKey;
        const bool acc = touched && accepts(c1, c2);
        const int idx = touched ? key_idx(c1) : 0;
        nm += __popcll(__ballot(acc));
        // last writer (highest lane) of each keypoint sets mp / blocked
        if (touched) owner[idx] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (acc) atomicMax(&owner[idx], lane + 1);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
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
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (touched) owner[idx] = INT_MAX;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      };
      commit(act && lane < r, b1, b2);
      if (r < 64 && c0 + r < qn) {
        // lane r: every kept candidate is taken -> rescan its window with the live claims
        ScanCtx c;
        const bool okc = make_ctx(queries[q0 + c0 + r], poses, f, th, cam, g, &c);
        uint64_t top[kTopK];
        if (okc) scan_query(c, cam, F, claimed, top, lane, g->kp_cap);
        const uint64_t t1 = __shfl(okc ? top[0] : kNoKey, 0, 64);
        const uint64_t t2 = __shfl(okc ? top[1] : kNoKey, 0, 64);
        commit(lane == r, t1, t2);
      }
      start = r + 1;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
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
  const FrameView F = frame_view(f, cur, nullptr, 0, gw, io, kp_cap);
  const InitSearch P = params[f];
  const float nnratio = P.nnratio;
  const bool check_ori = P.check_ori != 0;
  const int q0 = io.q_start[f], qn = io.q_count[f];
  auto set_best = [&](int qi, int idx) {
    if (qi < kResolveLdsQ) s_best[qi] = (int16_t)idx;
    else mw.best_idx[q0 + qi] = idx;
  };
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
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
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      bool conflict = false;
      if (act) {
#pragma unroll
        for (int k = 0; k < kTopK; k++)
          if (key[k] != kNoKey && stamp[key_idx(key[k])] < lane) conflict = true;
      }
      const uint64_t stop = __ballot(rescan || conflict);
      const int r = stop ? __ffsll((long long)stop) - 1 : 64;
      const bool r_conflict = r < 64 && ((__ballot(conflict) >> r) & 1ull);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (acc) stamp[i1] = INT_MAX;
      if (acc && lane < r) {  // :325-333
        matched_dist[i1] = d1;
        matches21[i1] = qi;
        set_best(qi, i1);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
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
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        start = r + 1;
      } else {
        start = r;  // 64, or a lane to decide again against the tables as they are now
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
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
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
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

void launch_search_init(const FrameKps& cur, const Camera& cam, const OrbGeomDev& g,
                        const InitQuery* queries, const InitSearch* params, int n_frames,
                        int max_q, const GridWorkspace& gw, const MatchWorkspace& mw,
                        const InitIO& io, hipStream_t st) {
  constexpr int kPerBlock = 4 * (64 / kSearchLanes<InitQuery>);
  if (max_q > 0)
    SLAMGPU_LAUNCH("search_cand", st, search_cand_kernel<InitQuery>,
                   dim3((max_q + kPerBlock - 1) / kPerBlock, n_frames), dim3(256), 0, st, cur,
                   (const float*)nullptr, (int64_t)0, cam, g.dev, queries, params, 0, gw, mw, io);
  SLAMGPU_LAUNCH("init_resolve", st, init_resolve_kernel, dim3(n_frames), dim3(64), 0, st, cur,
                 cam, g.dev, queries, params, gw, mw, io);
}

// The candidate search of every frame's queries, then the in-order claim resolution.
template <typename Q>
static void launch_search(const FrameKps& cur, const float* u_right, int64_t ur_stride,
                          const Camera& cam, const OrbGeomDev& g, const Q* queries,
                          const typename SearchPose<Q>::type* poses, int th, float nnratio,
                          int n_frames, int max_q, const GridWorkspace& gw,
                          const MatchWorkspace& mw, const MatchIO& io, hipStream_t st) {
  constexpr int kPerBlock = 4 * (64 / kSearchG);  // queries per work-group of search_cand
  if (max_q > 0)
    SLAMGPU_LAUNCH("search_cand", st, search_cand_kernel<Q>,
                   dim3((max_q + kPerBlock - 1) / kPerBlock, n_frames), dim3(256), 0, st, cur,
                   u_right, ur_stride, cam, g.dev, queries, poses, th, gw, mw, io);
  SLAMGPU_LAUNCH("search_resolve", st, search_resolve_kernel<Q>, dim3(n_frames), dim3(64), 0, st,
                 cur, u_right, ur_stride, cam, g.dev, queries, poses, th, nnratio, gw, mw, io);
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

// ---------------------------------------------------------------------------------------
// VO map points of the previous frame as queries for frame f (Tracker::UpdateLastFrame's
// visual-odometry points, tracker.cpp:695-753, with every stereo keypoint kept): keypoint i of
// frame f-1 with depth > 0 becomes a point at Frame::UnprojectStereo(i) (frame.cpp:594-607).
// Queries keep last-frame keypoint order (block-wide ordered compaction).
__global__ __launch_bounds__(256) void vo_queries_kernel(FrameKps src, const float* __restrict__ depth,
                                                         int64_t depth_stride, Camera cam,
                                                         const F2FPose* __restrict__ poses,
                                                         int blocks, int kp_cap,
                                                         F2FQuery* __restrict__ queries,
                                                         int* __restrict__ q_start,
                                                         int* __restrict__ q_count) {
  __shared__ int wsum[4];
  __shared__ int base;
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    q_start[f] = f * kp_cap;
    base = 0;
  }
  if (f == 0) {
    if (tid == 0) q_count[0] = 0;
    return;
  }
  const int s = f - 1;
  const KeyPoint* k = src.kps + s * src.stride;
  const uint8_t* d = src.desc + s * src.stride * 32;
  const int n = src.n[s * src.n_stride];
  const float* z = depth + s * depth_stride;
  const F2FPose& P = poses[s];
  // Twc: Rwc = Rcw^T, Ow = -Rcw^T tcw
  float Rwc[9], Ow[3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Rwc[3 * r + c] = P.Rcw[3 * c + r];
  for (int r = 0; r < 3; r++)
    Ow[r] = -(Rwc[3 * r] * P.tcw[0] + Rwc[3 * r + 1] * P.tcw[1] + Rwc[3 * r + 2] * P.tcw[2]);
  const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int i = c0 + tid;
    const bool ok = i < n && z[i] > 0;
    const int lane = tid & 63, wid = tid >> 6;
    const uint64_t m = __ballot(ok);
    if (lane == 0) wsum[wid] = __popcll(m);
    __syncthreads();
    int pre = base;
    for (int w = 0; w < wid; w++) pre += wsum[w];
    pre += lanes_below(m);
    if (ok) {
      const KeyPoint kp = k[i];
      const float zz = z[i];
      const float x = (kp.x - cam.cx) * zz * invfx;
      const float y = (kp.y - cam.cy) * zz * invfy;
      F2FQuery q;
      const float xc[3] = {x, y, zz};
      for (int r = 0; r < 3; r++) q.xyz[r] = gemm_row(Rwc + 3 * r, xc, Ow[r]);
      q.last_angle = kp.angle;
      q.last_octave = kp.octave;
      q.mp_id = i;
      q.blocks = blocks;
      q.pad = 0;
      for (int b = 0; b < 32; b++) q.desc[b] = d[i * 32 + b];
      queries[(int64_t)f * kp_cap + pre] = q;
    }
    __syncthreads();
    if (tid == 0) base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) q_count[f] = base;
}

void launch_vo_queries(const FrameKps& src, const float* depth, int64_t depth_stride,
                       const Camera& cam, const F2FPose* poses, int blocks, int kp_cap,
                       F2FQuery* queries, int* q_start, int* q_count, int n_frames,
                       hipStream_t st) {
  SLAMGPU_LAUNCH("vo_queries", st, vo_queries_kernel, dim3(n_frames), dim3(256), 0, st, src, depth,
                 depth_stride, cam, poses, blocks, kp_cap, queries, q_start, q_count);
}

}  // namespace slamgpu
