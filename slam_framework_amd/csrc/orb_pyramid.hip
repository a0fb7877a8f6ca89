// orb_pyramid.hip -- the extractor's pyramid stage (orb_extract.hip has the pipeline).
//   pyr_down      level l from level l-1 (resize INTER_LINEAR 8U)        one launch per level
//                 (batches: pyr_ring_kernel; small launches: pyr_band_kernel for levels >= 2;
//                 opt-in pyr_cascade_kernel, one launch for all)
// Reference: src/orb_features/orb_extractor.cpp (citations per kernel).
#include <cstdlib>

#include "device_math.h"
#include "timing.h"
#include "orb_device.h"
#include "orb_stages.h"

namespace slamgpu {

// Level addressing. Level 0 is the caller's image; levels >= 1 live in the pyramid buffer.
__device__ __forceinline__ const uint8_t* level_ptr(const ImageBatch& b, const OrbGeom* g,
                                                    int img, int level, int* pitch) {
  if (level == 0) {
    *pitch = b.in_pitch;
    return batch_image(b, img);
  }
  *pitch = g->lv[level].pitch;
  return b.pyr + (int64_t)img * g->pyr_bytes + g->lv[level].offset;
}

// pyr_down: ComputePyramid (:1051-1075) -> cv::resize(level l-1, level l, INTER_LINEAR).
// HResizeLinear (int = S[sx]*a0 + S[sx+1]*a1, or S[sx]*2048 from xmax on) then VResizeLinear
// ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2.
// A lane owns 4 adjacent output columns and walks a 16-row strip. Each source row is fetched
// once (3 dwords, in prefetched chunks of 4 rows) and its horizontal pass is computed once: the
// 8-byte window starting at sx(x0) (host-checked to hold all 4 columns' pixel pairs) is cut with
// two alignbytes, v_perm turns each column's pixel pair into a u16 pair and v_dot2_u32_u16
// applies (a0, a1). An output row combines the current and previous source rows' results.
#ifndef PYR_CHUNK
#define PYR_CHUNK 2
#endif
constexpr int kPyrStrip = PYR_STRIP;  // output rows per wave
constexpr int kPyrRingStrip = PYR_RING_STRIP;
constexpr int kPyrChunk = PYR_CHUNK;  // source rows fetched per batch
#ifndef PYR_SHORT_STRIP
#define PYR_SHORT_STRIP 4
#endif
constexpr int kPyrShortStrip = PYR_SHORT_STRIP;  // small launches (kPyrShortMaxImages)

// kAligned: the source rows are dword-aligned (every level >= 1 source; level 0 when the caller's
// images and pitch are) -- the instantiation without the byte-gather path needs fewer VGPRs, so
// more waves per SIMD hide the strip's chain of row loads.
// kStrip: output rows per wave -- kPyrStrip for batches; small launches (a single frame) take
// short strips so that more waves share a level and each walks a shorter chain of row loads.
// One wave: output rows [dy0, dy0 + min(kStrip, nlim)) x columns [256 tx, 256 tx + 256) of
// `level`. A strip fetches every source row its rows need, so strips compose in any partition.
// kRing (pyr_ring_kernel): every source row of the strip is first staged in the wave's LDS
// slots (`ring`, D.pyr_slots KiB) by 16-byte buffer-to-LDS loads issued at once -- a strip's
// whole input in flight with no VGPRs held -- and the rows are then read from LDS.
template <bool kAligned, int kStrip, bool kRing = false>
__device__ __forceinline__ void pyr_strip(const ImageBatch& b, const OrbGeom* __restrict__ g,
                                          int level, int img, int tx, int dy0,
                                          const ResizeX* __restrict__ rxt,
                                          const ResizeY* __restrict__ ryt, int nlim = kStrip,
                                          const uint8_t* src_rows = nullptr, int src_row0 = 0,
                                          uint8_t* copy_rows = nullptr, int copy_row0 = 0,
                                          uint8_t* ring = nullptr) {
  const int lane = threadIdx.x & 63;
  const LevelGeom& D = g->lv[level];
  const LevelGeom& S = g->lv[level - 1];
  if (dy0 >= D.h || nlim <= 0) return;
  const int nrows = min(min(kStrip, D.h - dy0), nlim);
  // the strip's row table, one entry per lane (read back with readlane)
  int ry_y0 = 0, ry_y1 = 0, ry_b = 0;
  if (lane < nrows) {
    const ResizeY e = ryt[D.ry_base + dy0 + lane];
    ry_y0 = e.y0;
    ry_y1 = e.y1;
    ry_b = (int)(uint16_t)e.b0 | (int)e.b1 << 16;
  }
  const int sy_lo = __builtin_amdgcn_readlane(ry_y0, 0);
  const int sy_hi = __builtin_amdgcn_readlane(ry_y1, nrows - 1);
  // per-lane column constants
  const int x0 = (tx << 8) + 4 * lane;
  int s0 = 0;
  uint32_t sel[4], A[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int dx = min(x0 + k, D.w - 1);
    const ResizeX e = rxt[D.rx_base + dx];
    if (k == 0) s0 = e.sx;
    const uint32_t bk = (uint32_t)min(e.sx - s0, 6);
    sel[k] = bk | 0x0c00u | (bk + 1) << 16 | 0x0c000000u;  // bytes bk, bk+1 -> u16 lanes
    // coefficients x16 (<= 32768): the dot product yields 16 * r, see the vertical pass
    A[k] = dx < D.xmax ? ((uint32_t)(16 * e.a0) | (uint32_t)(16 * e.a1) << 16) : 32768u;
  }
  const int q0 = s0 >> 2, sh = s0 & 3, qmax = (S.w - 1) >> 2;
  int spitch;
  const uint8_t* src = level_ptr(b, g, img, level - 1, &spitch);
  int srow0 = 0;  // row of src's first row (rows staged elsewhere, e.g. LDS, start later)
  if (src_rows) {
    src = src_rows;
    srow0 = src_row0;
  }
  const bool aligned = kAligned;
  const int qa = min(q0, qmax), qb = min(q0 + 1, qmax), qc = min(q0 + 2, qmax);
  // Source rows in global memory (pyr_down) are read through a buffer descriptor of the source
  // level: the row offset is a scalar, the lane's dword offsets are constants, so a row costs
  // three buffer loads and no address arithmetic (a flat load needs a 64-bit add per lane each).
  spitch = __builtin_amdgcn_readfirstlane(spitch);
  const bool gsrc = src_rows == nullptr;
  const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)uniform_ptr(src), 0, __builtin_amdgcn_readfirstlane(spitch * S.h), 0x00020000);
  const int oa = 4 * qa, ob = 4 * qb, oc = 4 * qc;
  // kRing: the strip's rows [sy_lo, sy_hi], row r in slot r / rpi at (r % rpi) * lpr * 16; each
  // row's bytes from seg0 (lane 0's first dword, rounded down to 16 bytes) on
  const int lpr = kRing ? D.pyr_lpr : 1, rpi = kRing ? D.pyr_rpi : 1;
  const int inv_rpi = kRing ? D.pyr_inv_rpi : 0;
  const int seg0 = kRing ? __builtin_amdgcn_readfirstlane(oa) & ~15 : 0;
  // the lane's first dword in a staged row; it reads that dword and the next two unclamped (a
  // byte past the row's end has zero weight, as behind the clamped reads' repeated dword)
  const int ra = (oa - seg0) >> 2;
  if constexpr (kRing) {
    const int rl = (lane * D.pyr_inv_lpr) >> 16, cl = lane - rl * lpr;  // row in a slot, chunk
    const int nsrc = sy_hi - sy_lo + 1;
    for (int k = 0; k * rpi < nsrc; k++) {
      // lanes past the slot's rows repeat its last row into the slot's unused tail
      const int r = min(k * rpi + min(rl, rpi - 1), nsrc - 1);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          srsrc, (__attribute__((address_space(3))) void*)(ring + 1024 * k), 16,
          (uint32_t)((sy_lo + r) * spitch + seg0 + 16 * cl), 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the rows have landed
    wave_lds_sync();
  }
  auto fetch = [&](int sy, uint32_t (&wv)[3]) {
    const int roff = __builtin_amdgcn_readfirstlane((min(sy, sy_hi) - srow0) * spitch);
    const uint8_t* row = src + roff;  // wave-uniform
    if constexpr (kRing) {
      const int r = min(sy, sy_hi) - sy_lo, slot = (r * inv_rpi) >> 16;  // r < 64: exact
      const uint32_t* rw = reinterpret_cast<const uint32_t*>(
          ring + 1024 * slot + (r - slot * rpi) * lpr * 16);
      const uint32_t* rl_ = rw + (uint32_t)ra;
      wv[0] = rl_[0];
      wv[1] = rl_[1];
      wv[2] = rl_[2];
    } else if (aligned && gsrc) {  // clamped dwords stay inside the row; bytes past sx+1: zero weight
      wv[0] = __builtin_amdgcn_raw_buffer_load_b32(srsrc, oa, roff, 0);
      wv[1] = __builtin_amdgcn_raw_buffer_load_b32(srsrc, ob, roff, 0);
      wv[2] = __builtin_amdgcn_raw_buffer_load_b32(srsrc, oc, roff, 0);
    } else if (aligned) {  // rows staged in LDS by pyr_band_kernel
      const uint32_t* rw = reinterpret_cast<const uint32_t*>(row);
      wv[0] = rw[(uint32_t)qa];
      wv[1] = rw[(uint32_t)qb];
      wv[2] = rw[(uint32_t)qc];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) v |= (uint32_t)row[min(4 * (q0 + i) + j, S.w - 1)] << (8 * j);
        wv[i] = v;
      }
    }
  };
  uint8_t* dst = b.pyr + (int64_t)img * g->pyr_bytes + D.offset;
  const int dpitch = __builtin_amdgcn_readfirstlane(D.pitch), dw = __builtin_amdgcn_readfirstlane(D.w);
  const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)uniform_ptr(dst), 0, __builtin_amdgcn_readfirstlane(dpitch * D.h), 0x00020000);
  uint32_t cur[kPyrChunk][3], nxt[kPyrChunk][3];
#pragma unroll
  for (int j = 0; j < kPyrChunk; j++) fetch(sy_lo + j, cur[j]);
  // hp / hc: the previous / current source row's horizontal results, already in the vertical
  // pass's operand form (r >> 4) << 8 = (16 r) & ~0xff (once per source row, not per output row)
  uint32_t hp[4] = {0, 0, 0, 0}, hc[4] = {0, 0, 0, 0};
  int nd = 0;  // next strip row to emit
  // one output row from source rows (r0, r1): v = ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2)
  // >> 2 (<= 255 for any coefficient rounding), packed by two u16 pairs, one
  // v_pk_lshrrev_b16 each and one v_perm
  auto emit = [&](const uint32_t (&r0)[4], const uint32_t (&r1)[4], uint32_t b0, uint32_t b1) {
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // v_mul_hi_u32_u24 as such: the operands are < 2^24 by construction (the C helper's masks
      // would be re-applied to the carried row, whose known bits the loop phi loses)
      uint32_t m0, m1;
      asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(m0) : "s"(b0), "v"(r0[k]));
      asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(m1) : "s"(b1), "v"(r1[k]));
      t[k] = m0 + m1 + 2u;
    }
    typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
    const u16x2_t two = {2, 2};
    const uint32_t p01 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, t[0] | t[1] << 16) >> two);
    const uint32_t p23 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, t[2] | t[3] << 16) >> two);
    const uint32_t packed = __builtin_amdgcn_perm(p23, p01, 0x06040200u);
    const int doff = __builtin_amdgcn_readfirstlane((dy0 + nd) * dpitch);
    uint8_t* drow = dst + doff;
    if (x0 + 4 <= dw) {  // pitch is a multiple of 64
      __builtin_amdgcn_raw_buffer_store_b32(packed, drsrc, x0, doff, 0);
      if (copy_rows)
        *reinterpret_cast<uint32_t*>(copy_rows + (dy0 + nd - copy_row0) * dpitch + x0) = packed;
    } else {
      for (int k = 0; x0 + k < dw; k++) drow[x0 + k] = (uint8_t)(packed >> (8 * k));
      if (copy_rows) {
        uint8_t* crow = copy_rows + (dy0 + nd - copy_row0) * dpitch;
        for (int k = 0; x0 + k < dw; k++) crow[x0 + k] = (uint8_t)(packed >> (8 * k));
      }
    }
  };
  for (int c0 = sy_lo; c0 <= sy_hi; c0 += kPyrChunk) {
    if (c0 + kPyrChunk <= sy_hi) {
#pragma unroll
      for (int j = 0; j < kPyrChunk; j++) fetch(c0 + kPyrChunk + j, nxt[j]);
    }
#pragma unroll
    for (int j = 0; j < kPyrChunk; j++) {
      const int sy = c0 + j;
      if (sy <= sy_hi) {
        const uint32_t W0 = __builtin_amdgcn_alignbyte(cur[j][1], cur[j][0], sh);
        const uint32_t W1 = __builtin_amdgcn_alignbyte(cur[j][2], cur[j][1], sh);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          hp[k] = hc[k];
          hc[k] = dot2u(__builtin_amdgcn_perm(W1, W0, sel[k]), A[k], 0u) & 0xffff00u;  // 16 r < 2^23
        }
        // emit the strip rows whose lower source row is sy (rows are in y1 order)
        while (nd < nrows && __builtin_amdgcn_readlane(ry_y1, nd) == sy) {
          const uint32_t bb = (uint32_t)__builtin_amdgcn_readlane(ry_b, nd);
          // (b * (r >> 4)) >> 16 == mulhi24(b << 8, (r >> 4) << 8) (all operands < 2^24)
          const uint32_t b0 = (bb & 0xffffu) << 8, b1 = (bb >> 16) << 8;
          if (__builtin_amdgcn_readlane(ry_y0, nd) == sy)  // both source rows are row sy
            emit(hc, hc, b0, b1);
          else
            emit(hp, hc, b0, b1);
          nd++;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kPyrChunk; j++)
#pragma unroll
      for (int e = 0; e < 3; e++) cur[j][e] = nxt[j][e];
  }
}

template <bool kAligned, int kStrip>
__global__ __launch_bounds__(256) void pyr_down_kernel(ImageBatch b, const OrbGeom* __restrict__ g,
                                                       int level,
                                                       const ResizeX* __restrict__ rxt,
                                                       const ResizeY* __restrict__ ryt) {
  int img, bx;
  xcd_image_block(&img, &bx);
  const int tiles_x = (g->lv[level].w + 255) >> 8;
  const int tx = bx % tiles_x, ty = bx / tiles_x;
  pyr_strip<kAligned, kStrip>(b, g, level, img, tx, (ty * 4 + wave_id()) * kStrip, rxt, ryt);
}

// pyr_down with each wave's source rows staged in LDS (pyr_strip kRing): g->pyr_ring_slots KiB
// of dynamic LDS per wave
__global__ __launch_bounds__(256) void pyr_ring_kernel(ImageBatch b, const OrbGeom* __restrict__ g,
                                                       int level,
                                                       const ResizeX* __restrict__ rxt,
                                                       const ResizeY* __restrict__ ryt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ring[];
  int img, bx;
  xcd_image_block(&img, &bx);
  const int tiles_x = (g->lv[level].w + 255) >> 8;
  const int tx = bx % tiles_x, ty = bx / tiles_x;
  uint8_t* ring = s_ring + 1024 * g->pyr_ring_slots * wave_id();
  pyr_strip<true, kPyrRingStrip, true>(b, g, level, img, tx, (ty * 4 + wave_id()) * kPyrRingStrip,
                                       rxt, ryt, kPyrRingStrip, nullptr, 0, nullptr, 0, ring);
}

// Small launches (the single-frame call): levels 2 .. nlevels - 1 in one launch of row bands
// (g->pyr_band, geometry): band s computes its rows of each level -- its share plus the source
// rows its next level needs, so it reads only rows it wrote itself (halo rows are computed by
// two bands with the same bytes) -- its 16 waves spread over the level's (tile, strip) tasks,
// a work-group barrier between levels. One launch instead of nlevels - 2 dependent ones (~5 us
// each on the call's critical path), with the levels' work still spread over many CUs.
// The band's rows of each level also go to LDS (two buffers of g->pyr_band_lds bytes, rows at
// the level's pitch), where the next level reads them: one global round trip (level 1) per band.
constexpr int kPyrBandWaves = 16;
__global__ __launch_bounds__(64 * kPyrBandWaves) void pyr_band_kernel(
    ImageBatch b, const OrbGeom* __restrict__ g, const ResizeX* __restrict__ rxt,
    const ResizeY* __restrict__ ryt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_band[];
  const int band = blockIdx.x, img = blockIdx.y, wid = wave_id();
  const int half = g->pyr_band_lds;
  for (int l = 2; l < g->nlevels; l++) {
    const int r0 = g->pyr_band[band][l][0], r1 = g->pyr_band[band][l][1];
    const int tiles = (g->lv[l].w + 255) >> 8;
    const int chunks = (r1 - r0 + kPyrShortStrip - 1) / kPyrShortStrip;
    uint8_t* out = s_band + (l & 1) * half;
    const uint8_t* in = l > 2 ? s_band + ((l - 1) & 1) * half : nullptr;
    const int in_row0 = l > 2 ? g->pyr_band[band][l - 1][0] : 0;
    for (int t = wid; t < tiles * chunks; t += kPyrBandWaves) {
      const int tx = t % tiles, dy0 = r0 + (t / tiles) * kPyrShortStrip;
      pyr_strip<true, kPyrShortStrip>(b, g, l, img, tx, dy0, rxt, ryt, r1 - dy0, in, in_row0, out,
                                      r0);
    }
    __syncthreads();  // this level's rows (LDS) before the next level reads them
  }
}

// Batches: the whole pyramid of one image in one work-group, streamed top to bottom (a cascade
// of line buffers): every barrier step level 1 consumes the next level-0 row and each level
// l >= 2 the rows level l - 1 emitted in the step before, so all levels advance together and a
// level's rows go from LDS to the next level without a global round trip. One launch instead of
// nlevels - 1 dependent ones; level 0 is read once and every level written once (the section
// 8(d) bytes), and the small levels no longer pay a launch and a strip chain each.
// Lanes: task k of level l owns output columns x0 = 8 (k - casc_task_base[l]) .. x0 + 7 as two
// groups of 4 (the pyr_strip column math: an 8-byte window from the group's first source byte,
// v_perm + v_dot2 per column); it keeps the previous / current source row's horizontal results
// in registers (hp, hc) and emits output row y when its lower source row y1 arrives -- from
// (hp, hc), or (hc, hc) where the row table clamps y0 == y1. Every lane of a level takes the
// same steps; the level's first lane publishes the rows emitted so far (P[t & 1][l]).
// The loader wave streams level-0 rows into kCascR0 LDS slots kCascDepth rows ahead (16-byte
// buffer-to-LDS loads; only it issues vector-memory loads, so its vmcnt counts rows).
__global__ __launch_bounds__(1024) void pyr_cascade_kernel(ImageBatch b, const OrbGeom* __restrict__ g,
                                                           const ResizeX* __restrict__ rxt,
                                                           const ResizeY* __restrict__ ryt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_c[];
  const int img = blockIdx.x, tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int nl = g->nlevels, nw = g->casc_waves, T = g->casc_steps;
  const int H0 = g->lv[0].h;
  const int ry0 = g->lv[1].ry_base, nry = g->lv[nl - 1].ry_base + g->lv[nl - 1].h - ry0;
  uint2* s_ry = reinterpret_cast<uint2*>(s_c + g->casc_ry_off);
  int* s_p = reinterpret_cast<int*>(s_c + g->casc_p_off);
  for (int i = tid; i < nry; i += blockDim.x) {
    const ResizeY e = ryt[ry0 + i];
    s_ry[i] = make_uint2((uint32_t)e.y1 | (uint32_t)(e.y0 == e.y1) << 16,
                         (uint32_t)(uint16_t)e.b0 | (uint32_t)(uint16_t)e.b1 << 16);
  }
  if (tid < 2 * kMaxLevels) s_p[tid] = 0;
  const bool loader = wid == nw;
  // ---- the loader: level-0 row r -> slot r % kCascR0, 16-byte chunks, ipr instructions per row
  const int chunks0 = (g->lv[0].w + 15) >> 4, ipr = (chunks0 + 63) >> 6;
  uint8_t* ring0 = s_c + g->casc_ring_off[0];
  const int stride0 = g->casc_ring_stride[0];
  const int pitch0 = __builtin_amdgcn_readfirstlane(b.in_pitch);
  const __amdgpu_buffer_rsrc_t rsrc0 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)uniform_ptr(batch_image(b, img)), 0, __builtin_amdgcn_readfirstlane(pitch0 * H0),
      0x00020000);
  auto issue = [&](int r) {
    uint8_t* dst = ring0 + (r % kCascR0) * stride0;
    for (int k = 0; k < ipr; k++)
      if (64 * k + lane < chunks0)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rsrc0, (__attribute__((address_space(3))) void*)(dst + 1024 * k), 16,
            (uint32_t)(r * pitch0 + 16 * (64 * k + lane)), 0, 0, 0);
  };
  // wait until row r has landed, rows up to min(r + kCascDepth - 1, H0 - 1) issued
  auto wait_row = [&](int r) {
    if (r + kCascDepth - 1 < H0) {
      if (ipr == 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (kCascDepth - 1));
      else __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * (kCascDepth - 1)));
    } else {
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
  };
  if (loader) {
    for (int r = 0; r < kCascDepth && r < H0; r++) issue(r);
    wait_row(0);
  }
  // ---- a compute lane's level, columns and constants
  const int task = wid * 64 + lane;
  int lvl = 0;
  if (!loader)
    for (int l = 1; l < nl; l++)
      if (task >= g->casc_task_base[l] && task < g->casc_task_base[l + 1]) lvl = l;
  const LevelGeom& D = g->lv[lvl > 0 ? lvl : 1];
  const int x0 = 8 * (task - g->casc_task_base[lvl > 0 ? lvl : 1]);
  const int Hl = D.h, Wl = D.w;
  uint32_t sel[8], A[8];
  int qo[2], sh[2];
#pragma unroll
  for (int gi = 0; gi < 2; gi++) {
    int s0 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = min(x0 + 4 * gi + k, Wl - 1);
      const ResizeX e = rxt[D.rx_base + dx];
      if (k == 0) s0 = e.sx;
      const uint32_t bk = (uint32_t)min(e.sx - s0, 6);
      sel[4 * gi + k] = bk | 0x0c00u | (bk + 1) << 16 | 0x0c000000u;
      A[4 * gi + k] = dx < D.xmax ? ((uint32_t)(16 * e.a0) | (uint32_t)(16 * e.a1) << 16) : 32768u;
    }
    qo[gi] = 4 * (s0 >> 2);
    sh[gi] = s0 & 3;
  }
  // source ring (level lvl - 1) and destination ring (level lvl; none for the last level)
  const int sl = lvl > 0 ? lvl - 1 : 0;
  const uint8_t* sring = s_c + g->casc_ring_off[sl];
  const int sstride = g->casc_ring_stride[sl], smod = sl == 0 ? kCascR0 : kCascSlots;
  const bool to_lds = lvl > 0 && lvl + 1 < nl;
  uint8_t* dring = s_c + g->casc_ring_off[to_lds ? lvl : 0];
  const int dstride = g->casc_ring_stride[to_lds ? lvl : 0];
  uint8_t* dst = b.pyr + (int64_t)img * g->pyr_bytes + D.offset;
  const int dpitch = D.pitch;
  const uint2* rytab = s_ry + (D.ry_base - ry0);
  const bool leader = lvl > 0 && task == g->casc_task_base[lvl];
  const bool full = x0 + 8 <= Wl;
  __syncthreads();  // row tables, counters and level-0 row 0 in LDS
  int ns = 0, nd = 0;
  uint2 cur = rytab[0];
  uint32_t hp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int t = 0; t < T; t++) {
    if (loader) {
      if (t + kCascDepth < H0) issue(t + kCascDepth);
    } else if (lvl > 0) {
      const int avail = lvl == 1 ? min(t + 1, H0) : s_p[((t + 1) & 1) * kMaxLevels + lvl - 1];
      while (ns < avail) {
        const uint8_t* row = sring + (ns & (smod - 1)) * sstride;
#pragma unroll
        for (int gi = 0; gi < 2; gi++) {
          const uint32_t* rw = reinterpret_cast<const uint32_t*>(row + qo[gi]);
          const uint32_t d0 = rw[0], d1 = rw[1], d2 = rw[2];
          const uint32_t W0 = __builtin_amdgcn_alignbyte(d1, d0, sh[gi]);
          const uint32_t W1 = __builtin_amdgcn_alignbyte(d2, d1, sh[gi]);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            hp[4 * gi + k] = hc[4 * gi + k];
            hc[4 * gi + k] =
                dot2u(__builtin_amdgcn_perm(W1, W0, sel[4 * gi + k]), A[4 * gi + k], 0u) & 0xffff00u;
          }
        }
        while (nd < Hl && (int)(cur.x & 0xffffu) == ns) {
          const uint32_t b0 = (cur.y & 0xffffu) << 8, b1 = (cur.y >> 16) << 8;
          if (cur.x >> 16) {  // y0 == y1 (the last rows): both source rows are this one
#pragma unroll
            for (int k = 0; k < 8; k++) hp[k] = hc[k];
          }
          uint32_t pk[2];
#pragma unroll
          for (int gi = 0; gi < 2; gi++) {
            uint32_t tt[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const uint32_t r0 = hp[4 * gi + k];
              uint32_t m0, m1;
              asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(m0) : "v"(b0), "v"(r0));
              asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(m1) : "v"(b1), "v"(hc[4 * gi + k]));
              tt[k] = m0 + m1 + 2u;
            }
            typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
            const u16x2_t two = {2, 2};
            const uint32_t p01 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, tt[0] | tt[1] << 16) >> two);
            const uint32_t p23 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, tt[2] | tt[3] << 16) >> two);
            pk[gi] = __builtin_amdgcn_perm(p23, p01, 0x06040200u);
          }
          if (to_lds)
            *reinterpret_cast<uint2*>(dring + ((uint32_t)nd % kCascSlots) * dstride + x0) =
                make_uint2(pk[0], pk[1]);
          uint8_t* drow = dst + (uint32_t)(nd * dpitch);
          if (full) {
            *reinterpret_cast<uint2*>(drow + x0) = make_uint2(pk[0], pk[1]);
          } else {
            for (int k = 0; x0 + k < Wl; k++) drow[x0 + k] = (uint8_t)(pk[k >> 2] >> (8 * (k & 3)));
          }
          nd++;
          cur = rytab[min(nd, Hl - 1)];
        }
        ns++;
      }
      if (leader) s_p[(t & 1) * kMaxLevels + lvl] = nd;
    }
    if (loader) wait_row(t + 1);
    // a work-group barrier that orders LDS only: __syncthreads() (or an LDS-scope fence, as the
    // loader's buffer-to-LDS loads are LDS writes counted by vmcnt) would make every wave wait
    // for its global stores of the step (vmcnt(0)) -- an HBM write latency per step
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

// ---------------------------------------------------------------------------------------
void launch_pyramid(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st,
                    bool glds) {
  const OrbGeom& g = *gd.host;
  const bool in_aligned = (((uintptr_t)b.in_l | (uintptr_t)b.in_r | (uintptr_t)b.in_stride |
                           (uintptr_t)b.in_pitch) & 3) == 0;
  const bool short_strips = n_images <= kPyrShortMaxImages;
  // batches: the LDS-staged strips (16-byte buffer-to-LDS loads need 16-byte aligned rows)
  const bool ring = glds && !short_strips && g.pyr_ring_slots > 0 && g.pyr_ring_slots <= 8;
  // SLAMGPU_PYR_CASCADE=1: batches take the whole pyramid in one cascade launch where the
  // geometry allows it. Not the default: it is 0.57 ms standalone against the per-level
  // launches' 0.69, but its lanes idle in the steps their level emits nothing (186M VALU
  // wave-instructions against 134M) and it holds every CU for its whole run, so level 0's FAST
  // beside it stretches 0.68 -> 0.98 ms and the step gets slower, 2.45 -> 2.57 ms
  // (profiles/r8c_pyr_cascade_ab.log). Read per launch, so that tests can exercise both paths.
  const char* cenv = std::getenv("SLAMGPU_PYR_CASCADE");
  const bool cascade = cenv && std::atoi(cenv) != 0 && glds && !short_strips && g.casc_waves > 0;
  // small launches: level 1 over the chip, then levels 2+ in one launch of row bands
  const int l_end = cascade ? 1 : (short_strips && g.pyr_bands > 0) ? 2 : g.nlevels;
  for (int l = 1; l < l_end; l++) {
    const int strip = short_strips ? kPyrShortStrip : ring ? kPyrRingStrip : kPyrStrip;
    const int tiles = ((g.lv[l].w + 255) >> 8) * ((g.lv[l].h + 4 * strip - 1) / (4 * strip));
    const dim3 grid(tiles, n_images);
    const bool aligned = l > 1 || in_aligned;
    auto* kfn = short_strips ? (aligned ? pyr_down_kernel<true, kPyrShortStrip>
                                        : pyr_down_kernel<false, kPyrShortStrip>)
                : ring       ? pyr_ring_kernel
                : aligned    ? pyr_down_kernel<true, kPyrStrip>
                             : pyr_down_kernel<false, kPyrStrip>;
    SLAMGPU_LAUNCH("pyr_down", st, kfn, grid, dim3(256),
                   ring ? (size_t)4096 * g.pyr_ring_slots : 0, st, b, gd.dev, l, gd.rx, gd.ry);
  }
  if (cascade) {
    SLAMGPU_LAUNCH("pyr_down", st, pyr_cascade_kernel, dim3(n_images),
                   dim3(64 * (g.casc_waves + 1)), (size_t)g.casc_lds, st, b, gd.dev, gd.rx, gd.ry);
  } else if (l_end < g.nlevels) {
    SLAMGPU_LAUNCH("pyr_down", st, pyr_band_kernel, dim3(g.pyr_bands, n_images),
                   dim3(64 * kPyrBandWaves), 2 * (size_t)g.pyr_band_lds, st, b, gd.dev, gd.rx,
                   gd.ry);
  }
}

bool pyramid_build_matches(const OrbGeom& g) { return g.pyr_ring_strip == kPyrRingStrip; }

}  // namespace slamgpu
