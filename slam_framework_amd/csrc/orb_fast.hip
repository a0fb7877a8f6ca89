// orb_fast.hip -- the extractor's FAST stage (orb_extract.hip has the pipeline).
//   fast_cells    per-cell FAST-9 score, threshold fallback, cell NMS    8 cells per wave
// Reference: src/orb_features/orb_extractor.cpp (citations per kernel).
#include <type_traits>

#include "device_math.h"
#include "timing.h"
#include "orb_stages.h"

namespace slamgpu {

// fast_cells: ComputeKeyPointsOctTree cell loop (:730-770) with cv::FAST(th, nonmax=true).
// For a FAST corner the cornerScore<16> value does not depend on the threshold it was found
// at: score = s - 1 with s = max over the 16 contiguous 9-arcs of min |I_ring - I_center|
// (same sign along the arc), and p is a corner at threshold t iff s > t. So one s-map per cell
// serves both passes: NMS at iniTh, and again at minTh if nothing survived (:753-757).
// NMS is strict '>' against the 8 neighbours' scores at that t, zero outside the detect area
// (cell-local, as cv::FAST sees only the cell view). Survivors are written in row-major order.
#ifndef FAST_CELL_WAVES
#define FAST_CELL_WAVES 1
#endif
constexpr int kCellWaves = FAST_CELL_WAVES;  // waves per work-group

// ---- byte-parallel comparisons (r5). v_lerp_u8 adds two bytes and a rounding bit per byte and
// halves, with no carry between bytes: lerp(x, ~y, r) = floor((x - y + 255 + r) / 2) encodes
// x - y in [-255, 255] as a byte, and a second lerp against a constant C sets bit 7 of a byte
// exactly when that byte is >= 256 - C. So "x - y >= t + 1" is bit 7 of two lerps for four
// pixels at once (t + r even makes the halving exact: r = t & 1, K = 128 + (t + r) / 2):
//   bright_a  (a - v >= t + 1) = bit 7 of lerp(lerp(a, ~v, r), 256 - K, 0)
//   !dark_a   (v - a <= t)     = bit 7 of lerp(lerp(~v, a, 1 - r), K, 0)
// (lerp(~v, a, 1 - r) = 255 - lerp(v, ~a, r), so the dark test needs no ~a.)
__device__ __forceinline__ uint32_t lerp_u8(uint32_t a, uint32_t b, uint32_t r) {
  return __builtin_amdgcn_lerp(a, b, r);
}

struct FastTh {        // one pass's threshold constants (wave-uniform)
  int th;              // clamped to [0, 255] as cv::FAST does
  uint32_t r, rn;      // rounding bytes r and 1 - r
  uint32_t cb, cd;     // second-level constants 256 - K and K
};
__device__ __forceinline__ FastTh fast_th(int th) {
  FastTh f;
  f.th = min(max(th, 0), 255);
  const int r = f.th & 1, K = 128 + ((f.th + r) >> 1);  // K = 256 at t = 255: no corner
  f.r = (uint32_t)r * 0x01010101u;
  f.rn = (uint32_t)(r ^ 1) * 0x01010101u;
  f.cb = (uint32_t)(256 - K) * 0x01010101u;
  f.cd = (uint32_t)min(K, 255) * 0x01010101u;
  return f;
}

// The FAST pre-test of 4 pixels (one tile dword c, its row neighbours cm / cp and the dwords 3
// rows below / above): a pixel can be a corner only if both opposite ring pairs (0, 8) and
// (4, 12) hold a pixel darker than v - t (or both a pixel brighter than v + t) -- every 9-arc of
// the ring contains one pixel of each pair. Bit 7 of each byte = that pixel survives.
__device__ __forceinline__ uint32_t fast_pretest4(uint32_t c, uint32_t cm, uint32_t cp,
                                                  uint32_t p0, uint32_t p8, const FastTh& f) {
  const uint32_t a4 = __builtin_amdgcn_alignbyte(cp, c, 3);   // (x + 3, y)
  const uint32_t a12 = __builtin_amdgcn_alignbyte(c, cm, 1);  // (x - 3, y)
  const uint32_t nv = ~c;
  auto B = [&](uint32_t a) { return lerp_u8(lerp_u8(a, nv, f.r), f.cb, 0u); };
  auto G = [&](uint32_t a) { return lerp_u8(lerp_u8(nv, a, f.rn), f.cd, 0u); };
  const uint32_t bright = (B(p0) | B(p8)) & (B(a4) | B(a12));
  const uint32_t ndark = (G(p0) & G(p8)) | (G(a4) & G(a12));
  return bright | ~ndark;  // bit 7 of each byte (other bits: don't care)
}

// Exact FAST-9 strength s of one pixel (see above) on the 16 ring differences as f16 pairs
// x = (v - p, p - v): as f16 bit patterns the bytes v and p are the denormals v 2^-24 and
// p 2^-24, so one v_pk_add_f16 (negation per half, the byte broadcast by op_sel_hi) forms both
// differences exactly, and v_pk_minimum3 / v_pk_maximum3 evaluate the min-over-9-arcs /
// max-over-arcs network three operands at a time (16 + 16 + 8 instructions for both signs).
// A non-negative result's bit pattern is the integer s; a negative one (sign bit) means s < 0.
__device__ __forceinline__ uint32_t pk_minimum3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ uint32_t pk_maximum3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
template <int ts>
__device__ __forceinline__ int fast_score(const uint8_t* w) {  // w: top-left of the 7x7 window
  constexpr int offs[16] = {3 + 6 * ts, 4 + 6 * ts, 5 + 5 * ts, 6 + 4 * ts, 6 + 3 * ts, 6 + 2 * ts,
                            5 + ts,     4,          3,          2,          1 + ts,     2 * ts,
                            3 * ts,     4 * ts,     1 + 5 * ts, 2 + 6 * ts};
  const uint32_t v = w[3 + 3 * ts];
  uint32_t x[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t p = w[offs[k]];
    asm("v_pk_add_f16 %0, %1, %2 op_sel_hi:[0,0] neg_lo:[1,0] neg_hi:[0,1]"
        : "=v"(x[k]) : "v"(p), "v"(v));
  }
  uint32_t m3[16], m9[16];
#pragma unroll
  for (int k = 0; k < 16; k++) m3[k] = pk_minimum3(x[k], x[(k + 1) & 15], x[(k + 2) & 15]);
#pragma unroll
  for (int k = 0; k < 16; k++) m9[k] = pk_minimum3(m3[k], m3[(k + 3) & 15], m3[(k + 6) & 15]);
  const uint32_t u0 = pk_maximum3(pk_maximum3(m9[0], m9[1], m9[2]), pk_maximum3(m9[3], m9[4], m9[5]),
                                  pk_maximum3(m9[6], m9[7], m9[8]));
  const uint32_t u1 = pk_maximum3(pk_maximum3(m9[9], m9[10], m9[11]),
                                  pk_maximum3(m9[12], m9[13], m9[14]), m9[15]);
  const uint32_t best = pk_maximum3(u0, u1, u1);
  return max(max((int)(int16_t)(best & 0xffffu), (int)(int16_t)(best >> 16)), 0);
}

// A wave runs kCellsPerWave consecutive cells of one image.
constexpr int kCellsPerWave = FAST_CELLS_PER_WAVE;  // orb_geometry.h (4: 0.687 ms, 8: 0.670)
static_assert(kCellsPerWave == kCellGroup, "a wave's cells are one key group (orb_geometry.h)");

// ceil(4096 / n) for n = 1..32 (the pre-test's lane -> (row, dword) split by a multiply)
__constant__ int16_t c_inv4096[33] = {
    0,   4096, 2048, 1366, 1024, 820, 683, 586, 512, 456, 410, 373, 342, 316, 293, 274, 256,
    241, 228,  216,  205,  196,  187, 179, 171, 164, 158, 152, 147, 142, 137, 133, 128};

struct CellView {
  int level, ini_x, ini_y, vw, vh, pitch, ax, off, nd;
  const uint8_t* base;
  bool aligned;
};

template <int kAlign = 4>
__device__ __forceinline__ CellView cell_view(const ImageBatch& b, const OrbGeom* g, int img,
                                              int in_pitch, const uint4& d) {
  CellView v;
  v.level = (int)(int16_t)(d.x & 0xffff);
  v.ini_x = (int)(int16_t)(d.x >> 16);
  v.ini_y = (int)(int16_t)(d.y & 0xffff);
  v.vw = (int)(int16_t)(d.y >> 16);
  v.vh = (int)(int16_t)(d.z & 0xffff);
  const LevelGeom& L = g->lv[v.level];
  v.pitch = v.level == 0 ? in_pitch : L.pitch;
  v.base = v.level == 0 ? batch_image(b, img) : b.pyr + (int64_t)img * g->pyr_bytes + L.offset;
  v.ax = v.ini_x & -kAlign;
  v.off = v.ini_x - v.ax;
  v.nd = (v.vw + v.off + 3) >> 2;  // dwords per tile row (<= 18)
  v.aligned = (((uintptr_t)v.base | (uintptr_t)v.pitch) & 3) == 0;
  return v;
}

__device__ __forceinline__ uint4 readlane4(const uint4& x, int j) {
  return make_uint4(__builtin_amdgcn_readlane(x.x, j), __builtin_amdgcn_readlane(x.y, j),
                    __builtin_amdgcn_readlane(x.z, j), __builtin_amdgcn_readlane(x.w, j));
}

// GLDS: every cell view of the launch is 16-byte aligned (pyramid levels, and a caller image
// with 16-byte base/pitch/stride): tiles go HBM -> LDS by global_load_lds_dwordx4 (no VGPRs, one
// instruction per 1 KiB = 1024/TS tile rows). Otherwise dword loads staged through registers
// (4-byte aligned) or a byte copy.
template <int TS, bool GLDS>
__global__ __launch_bounds__(64 * kCellWaves, 1) void fast_cells_kernel(ImageBatch b,
                                                         const OrbGeom* __restrict__ g,
                                                         const CellDesc* __restrict__ cells,
                                                         uint32_t* __restrict__ cell_keys,
                                                         int* __restrict__ cell_count,
                                                         uint32_t* __restrict__ err,
                                                         int cell_lo, int cell_hi) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_fast[];
  const int wid = wave_id(), lane = threadIdx.x & 63;
  constexpr int kTileStride = TS, kScoreStride = TS;  // == g->fast_tile_stride
  constexpr int kLpr = TS / 4, kRps = 64 / kLpr;        // tile copy: lanes per row, rows per step
  constexpr int kTileSteps = (70 + kRps - 1) / kRps;    // cell views are <= 70 rows
  constexpr int kGLpr = TS / 16, kGRows = 64 / kGLpr;   // glds: lanes per row, rows per instr.
  constexpr int kGSteps = (70 + kGRows - 1) / kGRows;
  constexpr int kAlign = GLDS ? 16 : 4;
  int img, bx;
  xcd_image_block(&img, &bx);
  const int ncells = g->cells_per_image;  // per-image stride; this launch runs [cell_lo, cell_hi)
  const int c0 = cell_lo + (bx * kCellWaves + wid) * kCellsPerWave;
  if (c0 >= cell_hi) return;
  const int nc = min(kCellsPerWave, cell_hi - c0);
  const uint4 my_desc = lane < nc ? reinterpret_cast<const uint4*>(cells)[c0 + lane]
                                  : make_uint4(0, 0, 0, 0);
  const int in_pitch = __builtin_amdgcn_readfirstlane(b.in_pitch);
  // configuration scalars read once (the stores below would otherwise make the compiler reload
  // them inside the NMS loop, each behind a scalar-load wait)
  const int cell_cap = __builtin_amdgcn_readfirstlane(g->cell_cap);
  const FastTh th_ini = fast_th(__builtin_amdgcn_readfirstlane(g->ini_th));
  const FastTh th_min = fast_th(__builtin_amdgcn_readfirstlane(g->min_th));
  const int tile_bytes = (kTileStride * g->fast_tile_rows + 15) & ~15;
  uint8_t* tile0 = s_fast + wid * g->fast_lds_per_wave;
  uint8_t* sc = tile0 + tile_bytes;
  const int tile_rows = __builtin_amdgcn_readfirstlane(g->fast_tile_rows);
  uint16_t* cand =
      reinterpret_cast<uint16_t*>(sc + ((kScoreStride * g->fast_score_rows + 15) & ~15));
  {  // the score map starts zero; each FAST pass leaves it zero again
    const int zb = (kScoreStride * g->fast_score_rows + 15) & ~15;
    for (int o = 4 * lane; o < zb; o += 256) *reinterpret_cast<uint32_t*>(sc + o) = 0u;
  }

  // ---- tile prefetch: aligned dwords covering [ini_x & ~3, ini_x + vw) x [ini_y, ini_y + vh)
  // into registers, lane = (row within a step, dword): each element is a scalar row base plus a
  // per-lane offset. Tile column c = image column ax + c.
  const int plr = lane / kLpr, pld = lane % kLpr;
  uint32_t tv[GLDS ? 1 : kTileSteps];
  int tn = 0;
  auto prefetch = [&](const CellView& v) {
    tn = v.aligned ? (v.vh + kRps - 1) / kRps : 0;  // wave-uniform
    const uint8_t* src = v.base + (int64_t)v.ini_y * v.pitch + v.ax;
    const int goff = __umul24(plr, v.pitch) + 4 * pld;
    const bool dok = pld < v.nd;
#pragma unroll
    for (int k = 0; k < kTileSteps; k++)
      if (k < tn && dok && k * kRps + plr < v.vh)
        tv[k] = *reinterpret_cast<const uint32_t*>(src + (int64_t)(k * kRps) * v.pitch + goff);
  };
  // glds: tile row r of the view = image row ini_y + min(r, vh - 1) (rows past the view repeat
  // its last row; they are never read), 16-byte chunk lane % kGLpr of [ax, ax + TS). The view
  // ends >= 16 rows above the level's last row, so the TS-byte row reads stay in the image.
  // The row offsets are 32-bit lane offsets from one scalar base (saddr form).
  const int glr = lane / kGLpr, glc = 16 * (lane % kGLpr);
  auto issue = [&](const CellView& v, uint8_t* buf) {
    const uint8_t* src = v.base + (int64_t)v.ini_y * v.pitch + v.ax;  // wave-uniform
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(src);  // 32-bit lane offsets, no 64-bit adds
    const int n = (v.vh + kGRows - 1) / kGRows;
#pragma unroll
    for (int k = 0; k < kGSteps; k++)
      if (k < n && k * kGRows + glr < tile_rows)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(buf + 1024 * k), 16,
            (uint32_t)(min(k * kGRows + glr, v.vh - 1) * v.pitch + glc), 0, 0, 0);
  };
  CellView nxt = cell_view<kAlign>(b, g, img, in_pitch, readlane4(my_desc, 0));
  if constexpr (!GLDS) {
    if (nxt.vh > 0) prefetch(nxt);
  }

  // the group's keys, contiguous from its first cell's slot (kCellGroup == kCellsPerWave and
  // c0 is group-aligned: launch boundaries are level boundaries, padded to kCellGroup)
  uint32_t* const grp_keys = cell_keys + ((int64_t)img * ncells + c0) * cell_cap;
  int gfill = 0;
  for (int ci = 0; ci < nc; ci++) {
    const CellView v = nxt;
    const int64_t slot = (int64_t)img * ncells + c0 + ci;
    uint8_t* tile = tile0;
    if constexpr (GLDS) {
      // one tile buffer: this cell's rows are loaded now (the previous cell's tile reads have
      // all returned), other waves hide the latency
      if (ci + 1 < nc) nxt = cell_view<kAlign>(b, g, img, in_pitch, readlane4(my_desc, ci + 1));
      if (v.vh == 0) {  // empty cell (:737, :745)
        if (lane == 0) cell_count[slot] = 0;
        continue;
      }
      wave_lds_sync();
      issue(v, tile0);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      wave_lds_sync();
    } else {
    if (v.vh == 0) {  // empty cell (:737, :745)
      if (lane == 0) cell_count[slot] = 0;
      if (ci + 1 < nc) {
        nxt = cell_view<kAlign>(b, g, img, in_pitch, readlane4(my_desc, ci + 1));
        if (nxt.vh > 0) prefetch(nxt);
      }
      continue;
    }
    wave_lds_sync();  // previous cell's LDS reads are done
    if (v.aligned) {
      const bool dok = pld < v.nd;
#pragma unroll
      for (int k = 0; k < kTileSteps; k++)
        if (k < tn && dok && k * kRps + plr < v.vh)
          *reinterpret_cast<uint32_t*>(tile + (k * kRps + plr) * TS + 4 * pld) = tv[k];
    } else {  // caller image with an odd pitch/base: byte copy
      for (int r = 0; r < v.vh; r++)
        for (int x = lane; x < v.vw + v.off; x += 64)
          tile[r * kTileStride + x] = v.base[(int64_t)(v.ini_y + r) * v.pitch + v.ax + x];
    }
    if (ci + 1 < nc) {  // next cell's loads fly while this one is processed
      nxt = cell_view<kAlign>(b, g, img, in_pitch, readlane4(my_desc, ci + 1));
      if (nxt.vh > 0) prefetch(nxt);
    }
    wave_lds_sync();
    }
    const int off = v.off;
    const int dh = v.vh - 6, dw = v.vw - 6;  // detect area [3, vh-3) x [3, vw-3)
    // ---- score map: rows -1 .. dh of the detect area, zeroed before each pass's scores (a zero
    // frame around the detect area lets the NMS read 3x3 neighbourhoods without bounds checks);
    // sc1 = row 0. Until then the pass keeps its prefilter records in the same bytes.
    uint8_t* sc1 = sc + kScoreStride;
    uint32_t* const recs = reinterpret_cast<uint32_t*>(sc);
    // ---- one FAST pass at threshold th: pre-test every detect pixel (4 pixels, one tile dword,
    // per lane), exact score of the survivors into the score map, NMS at th, survivors out in
    // row-major order.
    // Detect pixel (rr, col): tile row rr + 3, tile column col in [off + 3, off + 3 + dw).
    // Lane -> (row lr of a step, dword Q): rows_per rows of nq dwords per step.
    const int q_lo = (off + 3) >> 2, q_hi = (off + 2 + dw) >> 2;
    const int nq = q_hi - q_lo + 1;
    const int inv_nq = c_inv4096[nq];  // lane / nq = (lane * inv_nq) >> 12 (exact for lane < 64)
    const int rows_per = (64 * inv_nq) >> 12;
    const int lr = (lane * inv_nq) >> 12, Q = q_lo + (lane - lr * nq);
    const int blo = max(0, off + 3 - 4 * Q), bhi = min(4, off + 3 + dw - 4 * Q);
    const uint32_t vmask = lr < rows_per
        ? (uint32_t)(0x80808080ull >> (32 - 8 * bhi)) & (uint32_t)(0x80808080ull << (8 * blo))
        : 0u;
    const uint8_t* trow = tile + (lr + 3) * kTileStride + 4 * Q;  // this lane's dword, step 0
    uint32_t* out = grp_keys + gfill;  // this cell's survivors follow the group's earlier cells
    auto fast_pass = [&](const FastTh& f) -> int {
      if (f.th >= 255) return 0;  // FAST at 255: no pixel differs by more
      // pre-test: a lane with any surviving pixel appends one record -- its survivor flags (bit
      // 7 of each byte) | lane | step << 8 -- so records come out in row-major order
      int nrec = 0;
      auto step = [&](int it, int r0, auto tail_case) {
        constexpr bool kTail = decltype(tail_case)::value;
        const uint8_t* row = trow + r0 * kTileStride;
        auto rd = [&](int o) { return *reinterpret_cast<const uint32_t*>(row + o); };
        uint32_t m = fast_pretest4(rd(0), rd(-4), rd(4), rd(3 * kTileStride),
                                   rd(-3 * kTileStride), f) & vmask;
        if (kTail && r0 + lr >= dh) m = 0;
        const uint64_t act = __ballot(m != 0);
        if (m) recs[nrec + lanes_below(act)] = m | (uint32_t)lane | (uint32_t)it << 8;
        nrec += __popcll(act);
      };
      int it = 0, r0 = 0;
      for (; r0 + rows_per <= dh; r0 += rows_per, it++) step(it, r0, std::false_type{});
      if (r0 < dh) step(it, r0, std::true_type{});
      wave_lds_sync();
      // records -> one candidate per surviving pixel, row-major (exclusive prefix of the
      // per-record counts via 3 ballots)
      int ncand = 0;
      for (int i0 = 0; i0 < nrec; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t rec = i < nrec ? recs[i] : 0u;
        const uint32_t fl = rec & 0x80808080u;
        const int cnt = __popc(fl);
        const uint64_t b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
        int pos = ncand + lanes_below(b0) + 2 * lanes_below(b1) + 4 * lanes_below(b2);
        const int ln = (int)(rec & 63u), rit = (int)((rec >> 8) & 127u);
        const int lr2 = (ln * inv_nq) >> 12;
        const uint32_t pix0 =
            (uint32_t)((rit * rows_per + lr2) * kScoreStride + 4 * (q_lo + ln - lr2 * nq));
#pragma unroll
        for (int bb = 0; bb < 4; bb++)
          if (fl & (0x80u << (8 * bb))) cand[pos++] = (uint16_t)(pix0 + bb);
        ncand += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
      }
      wave_lds_sync();
      // the map is zero but for the records just read (it is zeroed once per wave and every
      // pass clears what it wrote): clear them
      for (int i = lane; i < nrec; i += 64) recs[i] = 0u;
      wave_lds_sync();
      // exact FAST score of the survivors (window top-left: tile (r, cc - 3) = tile + pix - 3)
      for (int i = lane; i < ncand; i += 64) {
        const int pix = cand[i];
        sc1[pix] = (uint8_t)fast_score<TS>(tile + pix - 3);
      }
      wave_lds_sync();
      // NMS at th: cv::FAST keeps p iff s - 1 > ns for all 8 neighbours, ns = (q > th ? q - 1 :
      // 0), zero outside the detect area. With Q = max of the 8 neighbours' s that is
      //   s > th  &&  s >= 2  &&  Q < max(s, th + 1),
      // and a neighbour this pass did not score has s <= th < s_p (the pre-test is necessary),
      // so it cannot change the test.
      const int th = f.th;
      int count = 0;
      for (int i0 = 0; i0 < ncand; i0 += 64) {
        const int i = i0 + lane;
        bool keep = false;
        int sv = 0, r = 0, cc = 0;
        if (i < ncand) {
          const int pix = cand[i];
          r = pix / kScoreStride;
          cc = pix - r * kScoreStride;
          const uint8_t* nb = sc1 + pix - kScoreStride - 1;  // (r - 1, cc - 1)
          const int al = (int)((uintptr_t)nb & 3);
          const uint32_t* nw = reinterpret_cast<const uint32_t*>(nb - al);
          constexpr int kW = kScoreStride / 4;
          const uint32_t rA = __builtin_amdgcn_alignbyte(nw[1], nw[0], al);
          const uint32_t rB = __builtin_amdgcn_alignbyte(nw[kW + 1], nw[kW], al);
          const uint32_t rC = __builtin_amdgcn_alignbyte(nw[2 * kW + 1], nw[2 * kW], al);
          sv = (rB >> 8) & 255;
          const int q = max(max(max3((int)(rA & 255), (int)((rA >> 8) & 255), (int)((rA >> 16) & 255)),
                                max((int)(rB & 255), (int)((rB >> 16) & 255))),
                            max3((int)(rC & 255), (int)((rC >> 8) & 255), (int)((rC >> 16) & 255)));
          keep = sv > th && sv >= 2 && q < max(sv, th + 1);
        }
        const uint64_t mk = __ballot(keep);
        if (keep) {
          const int pos = count + lanes_below(mk);
          if (pos < cell_cap) out[pos] = pack_key(v.ax + cc - kMinBorder, v.ini_y + 3 + r - kMinBorder, sv - 1);
        }
        count += __popcll(mk);
      }
      wave_lds_sync();
      for (int i = lane; i < ncand; i += 64) sc1[cand[i]] = 0;  // the map back to zero
      return count;
    };
    // FAST at iniTh; the reference re-runs the whole cell at minTh when the iniTh output (after
    // NMS) is empty (:753-757)
    int count = fast_pass(th_ini);
    if (count == 0) {
      wave_lds_sync();
      count = fast_pass(th_min);
    }
    if (count > cell_cap) {
      if (lane == 0) atomicOr(err, kErrCellOverflow);
      count = cell_cap;
    }
    if (lane == 0) cell_count[slot] = count;
    gfill += count;
  }
}

template <int TS, bool GLDS>
static void launch_fast(const ImageBatch& b, const OrbGeomDev& gd, int n_images, int lo, int hi,
                        hipStream_t st) {
  const int per_group = kCellWaves * kCellsPerWave;
  SLAMGPU_LAUNCH("fast_cells", st, (fast_cells_kernel<TS, GLDS>),
                 dim3((hi - lo + per_group - 1) / per_group, n_images), dim3(64 * kCellWaves),
                 (size_t)kCellWaves * gd.host->fast_lds_per_wave, st, b, gd.dev, gd.cells,
                 gd.ws.cell_keys, gd.ws.cell_count, gd.ws.err, lo, hi);
}

void launch_fast_cells(const ImageBatch& b, const OrbGeomDev& gd, int n_images, int lo, int hi,
                       hipStream_t st, bool glds) {
  auto* fn = gd.host->fast_tile_stride == 64
                 ? (glds ? launch_fast<64, true> : launch_fast<64, false>)
                 : (glds ? launch_fast<128, true> : launch_fast<128, false>);
  fn(b, gd, n_images, lo, hi, st);
}

bool fast_build_matches(const OrbGeom& g) { return g.cell_group == kCellsPerWave; }

}  // namespace slamgpu
