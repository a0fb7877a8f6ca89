// stereo_match.hip -- Frame::ComputeStereoMatches (frame.cpp:406-577) on gfx950, batched over
// frames. Frame f: left = image 2f, right = image 2f+1.
//
//   stereo_match    row-band Hamming + 11x11 SAD      :446-562   (one wave per left keypoint)
//   stereo_median   2.1 x median SAD rejection        :564-576   (one workgroup per frame)
// The right-keypoint row table the matcher reads (:412-433) is built by stereo_rows in
// frame_tables.hip. Every Hamming distance is popcount(a ^ b) over the 256 bits
// (== DescriptorDistance, orb_matcher.cpp:1630-1646).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"
#include "timing.h"

namespace slamgpu {

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
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

void launch_stereo(const ImageBatch& b, const OrbGeomDev& gd, const Camera& cam, int n_frames,
                   const StereoWorkspace& ws, const StereoOut& out, hipStream_t st,
                   uint8_t* pack, bool rows_done) {
  const OrbGeom& g = *gd.host;
  FrameKps ext{gd.out.kps, gd.out.desc, gd.out.nkps, g.kp_cap, 1};
  const int nrows = g.lv[0].h;
  if (!rows_done) launch_stereo_rows(gd, ext, nrows, n_frames, ws, st);  // else frame_aux_kernel did
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

}  // namespace slamgpu
