// orb_orient_desc.hip -- the extractor's last stage (orb_extract.hip has the pipeline).
//   orient_desc   IC_Angle + 7x7-blurred rBRIEF (the blur's row sums on the matrix cores, the
//                 vertical taps at the samples), in ORBextractor::Compute order
//                                                                        16 keypoints per wave
// Reference: src/orb_features/orb_extractor.cpp (citations per kernel).
#include <type_traits>
#include <utility>

#include "device_math.h"
#include "timing.h"
#include "orb_device.h"
#include "orb_stages.h"

namespace slamgpu {

__constant__ __attribute__((aligned(16))) int8_t c_pattern[1024] = {
#include "orb_pattern.inc"
};

__device__ __forceinline__ int reflect101(int i, int n) {  // cv::BORDER_REFLECT_101, |overshoot| < n
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// ---------------------------------------------------------------------------------------
// compile-time loops (lane selects and writelane lanes as immediates)
template <class F, int... J>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, J...>) {
  (f(std::integral_constant<int, J>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

constexpr int kKpPerWave = 16;        // batches: keypoints per wave (two halves of 8)
constexpr int kKpPerWaveSmall = 4;    // launches up to kOdSmallMaxImages images
constexpr int kOdSmallMaxImages = 16;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Sum of the 16 per-lane values v[] over the wave; value i ends up in lanes 4i..4i+3.
__device__ __forceinline__ int reduce_scatter16(int (&v)[16], int lane) {
  int w[8], x[4], y[2];
#pragma unroll
  for (int k = 0; k < 8; k++) {  // lanes 32-63 keep index k+8
    auto p = __builtin_amdgcn_permlane32_swap(v[k], v[k + 8], false, false);
    w[k] = (int)p[0] + (int)p[1];
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {  // odd rows keep index +4
    auto p = __builtin_amdgcn_permlane16_swap(w[k], w[k + 4], false, false);
    x[k] = (int)p[0] + (int)p[1];
  }
  const bool up8 = lane & 8, up4 = lane & 4;
#pragma unroll
  for (int k = 0; k < 2; k++) {  // row_mirror: partner lane ^ 15
    const int send = up8 ? x[k] : x[k + 2];
    y[k] = (up8 ? x[k + 2] : x[k]) + __builtin_amdgcn_mov_dpp(send, 0x140, 0xf, 0xf, false);
  }
  const int send = up4 ? y[0] : y[1];  // row_half_mirror: partner lane ^ 7
  int z = (up4 ? y[1] : y[0]) + __builtin_amdgcn_mov_dpp(send, 0x141, 0xf, 0xf, false);
  z += __builtin_amdgcn_mov_dpp(z, 0x4e, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
  z += __builtin_amdgcn_mov_dpp(z, 0xb1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
  return z;
}

// ---------------------------------------------------------------------------------------
// orient_desc: computeOrientation/IC_Angle (:413-420, :18-45) on the unblurred level, then
// computeOrbDescriptor (:49-88) on the level blurred by cv::GaussianBlur(7x7, sigma 2) (:1029-1030),
// with the blur folded in: no blurred pyramid is written or read back. The blur is separable
// with exact integer sums: a pixel is round(sum_i k_i R_i / 2^16), R_i = the row
// sums sum_j k_j I(y+i-3, x+j-3) <= 255 * 257 (u16).
// Per keypoint the row sums of its window (rows y-21..y+21, the columns the rotated samples can
// reach) come from the matrix cores: a banded int8 GEMM per 16 x 16 tile of the window
// (v_mfma_i32_16x16x64_i8: A = the window's bytes - 128 as int8, B = the 7 taps, accumulator
// initialised to 128 * 257, so the i32 result IS the u16 row sum), 3 x 3 tiles per keypoint. The
// A rows are mapped so that a lane's 12 accumulator elements are 12 consecutive window rows of one
// column; it packs them as u16 pairs (one v_perm per pair) and stores them with three
// ds_write_b64 into the wave's transposed u16 table. A sample's 7 vertical taps are then 4
// dwords of its column (two ds_read2_b32, a v_alignbit each for an odd first row) and four
// v_dot2_u32_u16. It rounds with the column's rule (half to even inside the SSE span
// x < W - W%4, half up in the scalar tail); inside the span a test compares the two biased
// sums' high halves directly.
// Border keypoints (the window leaves the image: reflect-101 rows and columns) gather the A bytes
// into the same staging slots; the GEMM and the table are the same.
// Variants measured in round 6 (profiles/r7*): an overlapping-pair table
// (dwords R[e] | R[e+1] << 16, no v_alignbit but twice the bytes stored: 0.87 vs 0.82 ms), A
// operands loaded straight from global memory (16 rows per quarter-wave), 8 keypoints per wave.
// Round 3-5 variants are in git history and DESIGN.md sections 9-11.
// The table per wave: kWCols columns (window column c = image column x - 18 - s + c, s the window
// origin's misalignment) x kUs u16 (rows 0..47, 43 used; 52 u16 = 26 dwords per column, so the 16
// lanes of a ds_write_b64 group hit 16 distinct bank pairs).
constexpr int kWCols = 40, kUs = 52;
constexpr int kWN = kWCols * kUs / 2;  // dwords
// The window staging area per wave: 48 rows x 64 bytes from the dword-aligned origin, filled by
// buffer-to-LDS loads in row order (four lanes per row: each load instruction's quarter-waves
// fetch four rows as whole lines) and read back in the MFMA's A layout (16 rows per quarter-wave,
// which as direct loads made every quarter-wave touch 16 lines). Within a row the four 16-byte
// chunks sit in the order chunk ^ swz(row), a table found by search that makes the A reads
// (ds_read_b128, 16-lane groups) bank-conflict free for the three tile rows.
constexpr int kWinRows = 48, kWinBytes = kWinRows * 64;
__device__ __forceinline__ int win_swz(int r) {
  const uint32_t t = r < 16 ? 0x330dbacdu : r < 32 ? 0x3a652155u : 0x159bb6u;
  return (int)((t >> (2 * (r & 15))) & 3u);
}

// KPW (<= kKpPerWave) keypoints per wave: 8 for batches, 4 for small launches (more waves in
// flight for the single-frame call)
template <int KPW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void orient_desc_kernel(
    ImageBatch b, const OrbGeom* __restrict__ g, const uint32_t* __restrict__ oct_keys,
    const int* __restrict__ oct_count, KeyPoint* __restrict__ kps, uint8_t* __restrict__ desc,
    int* __restrict__ nkps) {
  __shared__ __attribute__((aligned(16))) uint32_t s_w[4][kWN + 4];  // + a 16-byte front pad
  __shared__ __attribute__((aligned(16))) uint8_t s_win[4][kWinBytes];
  int img, bx;
  xcd_image_block(&img, &bx);
  const int lane = threadIdx.x & 63, wid = wave_id();
  int lcount[kMaxLevels];
  int total = 0;
  for (int l = 0; l < g->nlevels; l++) {
    lcount[l] = oct_count[img * g->nlevels + l];
    total += lcount[l];
  }
  if (bx == 0 && threadIdx.x == 0) nkps[img] = total;
  const int k0 = (bx * 4 + wid) * KPW;
  if (k0 >= total) return;
  const int nk = min(KPW, total - k0);
  int my_level = 0, my_key = 0;
  if (lane < nk) {
    int t = k0 + lane, l = 0;
    while (t >= lcount[l]) {
      t -= lcount[l];
      l++;
    }
    my_level = l;
    my_key = (int)oct_keys[(int64_t)img * g->out_per_image + g->lv[l].out_base + t];
  }
  // IC_Angle lane roles: two slots of 16 patch rows, four lanes per row. Lane (row r, k) loads 12
  // bytes at 8 k from the row's dword-aligned start (x - 15) & ~3 -- one 16-row x 36-byte block
  // per load instruction, so the patch's rows are fetched as whole lines (a 2-lanes-per-row map
  // with 5 dword loads touched every row 5 times: the texture data path, not the VALU, bound the
  // kernel) -- and realigns them into its two patch dwords 2 k, 2 k + 1 (columns 8 k .. 8 k + 7 of
  // x - 15 .. x + 15) with v_alignbyte; wt / one: the circle's u + 20 weights and 0/1 masks.
  const int ick = lane & 3;
  const int icv[2] = {(lane >> 2) - 15, (lane >> 2) + 1};
  uint32_t wt[2][2], one[2][2];
  {
    const uint4* t = reinterpret_cast<const uint4*>(g->od_ic[lane]);
    const uint4 w = t[0], o = t[1];
    wt[0][0] = w.x; wt[0][1] = w.y; wt[1][0] = w.z; wt[1][1] = w.w;
    one[0][0] = o.x; one[0][1] = o.y; one[1][0] = o.z; one[1][1] = o.w;
  }
  const int in_pitch = __builtin_amdgcn_readfirstlane(b.in_pitch);
  // every keypoint's window geometry computed once, lane j for keypoint j (vector loads of its
  // level's geometry), then read back per keypoint by v_readlane: the per-keypoint scalar chain
  // (level table loads, 64-bit pointer arithmetic, the window tests) was ~60 SALU instructions
  // per keypoint on the wave's issue stream. gv_k: x | y << 12 | level << 24 | aligned << 28 |
  // fastp << 31 (aligned: level base and pitch dword-aligned; fastp: aligned and the whole
  // 43 x 46 window inside the level)
  uint32_t gv_org_lo, gv_org_hi, gv_pitch, gv_wh, gv_k;
  {
    const LevelGeom& L = g->lv[my_level];
    const int kx = key_x((uint32_t)my_key) + kMinBorder, ky = key_y((uint32_t)my_key) + kMinBorder;
    const int w = L.w, h = L.h;
    const int pitch = my_level == 0 ? in_pitch : L.pitch;
    const uint8_t* im = my_level == 0 ? batch_image(b, img)
                                      : b.pyr + (int64_t)img * g->pyr_bytes + L.offset;
    const bool al = ((((uintptr_t)im | (uintptr_t)pitch) & 3) == 0);
    const bool fastp = al && kx >= 21 && kx <= w - 31 && ky >= 21 && ky + 21 < h;
    const uintptr_t org = (uintptr_t)(im + (int64_t)(ky - 21) * pitch + ((kx - 21) & ~3));
    gv_org_lo = (uint32_t)org;
    gv_org_hi = (uint32_t)(org >> 32);
    gv_pitch = (uint32_t)pitch;
    gv_wh = (uint32_t)w | (uint32_t)h << 16;
    gv_k = (uint32_t)kx | (uint32_t)ky << 12 | (uint32_t)my_level << 24 | (al ? 1u << 28 : 0u) |
           (fastp ? 1u << 31 : 0u);
  }
  // Phases 1-2: the IC_Angle patches (raw level, registers), kPh12Split keypoints at a time,
  // then their moments. The patch base is the window origin + 6 rows + ((x - 15) & ~3) -
  // ((x - 21) & ~3) (4 or 8) bytes: no level lookup per keypoint.
  typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
  constexpr int kPh12Split = 4;
  constexpr int KIC = KPW > 8 ? 16 : 8;  // keypoints whose angles the wave computes
  int mom[2];
#pragma unroll
  for (int g8 = 0; g8 < KIC / 8; g8++) {  // eight keypoints' moments, then their reduction
  int mv[16];
#pragma unroll
  for (int j0 = 8 * g8; j0 < 8 * g8 + 8; j0 += kPh12Split) {
    u32x3 raw[kPh12Split][2];
    int ash[kPh12Split];
#pragma unroll
    for (int jj = 0; jj < kPh12Split; jj++) {
      const int j = min(j0 + jj, nk - 1);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane(gv_k, j);
      const int x = (int)(k & 0xfffu);
      const int pitch = __builtin_amdgcn_readlane(gv_pitch, j);
      const uintptr_t org = (uintptr_t)(uint32_t)__builtin_amdgcn_readlane(gv_org_lo, j) |
                            (uintptr_t)(uint32_t)__builtin_amdgcn_readlane(gv_org_hi, j) << 32;
      const uint8_t* rbase = reinterpret_cast<const uint8_t*>(org) + 6 * pitch +
                             (((x - 15) & ~3) - ((x - 21) & ~3));
      ash[jj] = (x - 15) & 3;
      if ((k >> 28) & 1u) {
        // buffer loads off the patch's (wave-uniform) base: no 64-bit address per lane; row 31
        // (the second slot's last four lanes) lies past the 31-row range and reads zeros
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)uniform_ptr(rbase), 0, 30 * pitch + 36, 0x00020000);
#pragma unroll
        for (int q = 0; q < 2; q++)
          raw[jj][q] = __builtin_amdgcn_raw_buffer_load_b96(
              rs, __umul24((uint32_t)(16 * q + (lane >> 2)), (uint32_t)pitch) + 8u * ick, 0, 0);
      } else {
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const int r = 16 * q + (lane >> 2);
          uint32_t w3[3] = {0, 0, 0};
          if (r < 31) {
            const uint8_t* rp = rbase + (int64_t)r * pitch + 8 * ick;
#pragma unroll
            for (int kk = 0; kk < 12; kk++) w3[kk >> 2] |= (uint32_t)rp[kk] << (8 * (kk & 3));
          }
          raw[jj][q] = (u32x3){w3[0], w3[1], w3[2]};
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < kPh12Split; jj++) {
      const int j = j0 + jj;
      const int a = ash[jj];
      int m10 = 0, m01 = 0;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const uint32_t e0 = __builtin_amdgcn_alignbyte(raw[jj][q].y, raw[jj][q].x, a);
        const uint32_t e1 = __builtin_amdgcn_alignbyte(raw[jj][q].z, raw[jj][q].y, a);
        const uint32_t s = __builtin_amdgcn_udot4(e1, one[q][1], __builtin_amdgcn_udot4(e0, one[q][0], 0u, false), false);
        const uint32_t t = __builtin_amdgcn_udot4(e1, wt[q][1], __builtin_amdgcn_udot4(e0, wt[q][0], 0u, false), false);
        m10 += (int)t - 20 * (int)s;
        m01 += icv[q] * (int)s;
      }
      mv[2 * (j & 7)] = m10;
      mv[2 * (j & 7) + 1] = m01;
    }
    __asm__ volatile("" ::: "memory");
  }
  mom[g8] = reduce_scatter16(mv, lane);  // keypoint j: m10 at lanes 8 j.., m01 at 8 j + 4..
  }
  // the moments reduced over the wave: keypoint j's at lane 8 (j & 7) + 4 (j >> 3) (a DPP row
  // shift merges the second group of 8 into the lanes the first leaves free)
  int m10v, m01v;
  {
    const int mom0 = mom[0];
    m10v = mom0;
    m01v = __builtin_amdgcn_mov_dpp(mom0, 0x104, 0xf, 0xf, false);  // row_shl:4
    if constexpr (KIC > 8) {
      const int mom1 = mom[1];
      const int m10h = __builtin_amdgcn_mov_dpp(mom1, 0x114, 0xf, 0xf, false);  // row_shr:4
      const bool up = lane & 4;
      m10v = up ? m10h : m10v;
      m01v = up ? mom1 : m01v;
    }
  }
  auto angle_lane = [](int j) { return 8 * (j & 7) + 4 * (j >> 3); };
  const float angle = cv_fast_atan2((float)m01v, (float)m10v);
  const float factorPI = (float)(3.14159265358979323846 / 180.0);
  float sa, ca;
  glibc_sincosf(angle * factorPI, &sa, &ca);
  // Phase 3: per keypoint, the pair table (LDS) then the 512 blurred samples
  // the lane's 4 tests (8 points) as int8 (x0, y0, x1, y1) words: 4 VGPRs instead of 32
  // as float pairs (x, y): 16 VGPRs; the packed products broadcast x or y by op_sel
  f32x2 pf[8];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint32_t pw = reinterpret_cast<const uint32_t*>(c_pattern)[r * 64 + lane];
#pragma unroll
    for (int e = 0; e < 2; e++)
      pf[2 * r + e] = (f32x2){(float)(int)(int8_t)(pw >> (16 * e)),
                              (float)(int)(int8_t)(pw >> (16 * e + 8))};
  }
  const uint32_t q0 = g->gauss[0], q1 = g->gauss[1], q2 = g->gauss[2], q3 = g->gauss[3];
  const uint32_t K01 = q0 | q1 << 16, K23 = q2 | q3 << 16, K21 = q2 | q1 << 16, K0 = q0;
  // magic + 18: a rounded sample coordinate comes out as its window index (round(x) + 18; 18 is
  // even, so round-half-even is unchanged)
  const f32x2 magic = {12582930.0f, 12582930.0f};
  uint32_t dlo = 0, dhi = 0;
  // MFMA lane roles (v_mfma_i32_16x16x64_i8): lane l holds row / column l & 15 of A / B and 16
  // bytes of K (lane group g = l >> 4), C[4 g + i][l & 15] in element i (tools/mfma_i8_probe.hip
  // checks the 16x16x32 form's map; only "A and B bytes b of lane group g share one K index" is
  // relied on here, and the parity tests pin it). A lane's 16 K bytes are window bytes 16 g ..
  // 16 g + 15 of its row (from the dword-aligned origin xa = (x - 21) & ~3): one 16-byte load, the
  // row's four lanes one 64-byte block. Output column 16 tj + n is the row sum of bytes
  // 16 tj + n .. + 6, so B is the band shifted by 16 tj: one operand per tile column.
  typedef int v4i __attribute__((ext_vector_type(4)));
  const int mf_n = lane & 15, mf_g = lane >> 4;
  v4i bm[3];
#pragma unroll
  for (int tj = 0; tj < 3; tj++) {
    const uint4 t = reinterpret_cast<const uint4*>(g->od_band[tj])[lane];
    bm[tj] = (v4i){(int)t.x, (int)t.y, (int)t.z, (int)t.w};
  }
  // A rows: tile row ti's row m is window row 12 (m >> 2) + 4 ti + (m & 3), so lane (n, g) ends up
  // with window rows 12 g .. 12 g + 11 of column n. Rows past 42 repeat row 42 (they only feed the
  // table's zero-weight pad): the loads stay inside the window's 43 rows.
  uint32_t arow[3];
#pragma unroll
  for (int ti = 0; ti < 3; ti++)
    arow[ti] = (uint32_t)min(12 * (mf_n >> 2) + 4 * ti + (mf_n & 3), 42);
  struct RsGeo {
    const uint8_t* org;  // window origin (xa, y - 21)
    int pitch, w, h, kx, ky, level;
    bool fastp;          // the whole window is inside the level: buffer loads, no reflection
  };
  auto rs_geo = [&](int j) {
    RsGeo G;
    const int jj = min(j, nk - 1);
    const uintptr_t org = (uintptr_t)(uint32_t)__builtin_amdgcn_readlane(gv_org_lo, jj) |
                          (uintptr_t)(uint32_t)__builtin_amdgcn_readlane(gv_org_hi, jj) << 32;
    G.org = reinterpret_cast<const uint8_t*>(org);
    G.pitch = __builtin_amdgcn_readlane(gv_pitch, jj);
    const uint32_t wh = (uint32_t)__builtin_amdgcn_readlane(gv_wh, jj);
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane(gv_k, jj);
    G.w = (int)(wh & 0xffffu);
    G.h = (int)(wh >> 16);
    G.kx = (int)(k & 0xfffu);
    G.ky = (int)((k >> 12) & 0xfffu);
    G.level = (int)((k >> 24) & 0xfu);
    G.fastp = (k >> 31) != 0;
    return G;
  };
  // The window of a keypoint into the wave's staging area: slot 64 i + lane (16 bytes) holds row
  // 16 i + (lane >> 2) (rows past 42 repeat row 42), chunk (lane & 3) ^ swz(row). Fast path: three
  // buffer-to-LDS loads off the (wave-uniform) window origin xa = (x - 21) & ~3. The table's 40
  // columns are the row sums of window bytes 0 .. 45 (columns x - 21 .. x + 24 at most), so chunk 3
  // (bytes 48 .. 63, up to column x + 42 <= w + 11) only feeds output columns 42 and up, which
  // nothing reads. In rows 0 .. 41 that over-read ends inside the level's next row (w >= 46 > 11,
  // and row 42 <= h - 1 exists); on row 42, which fastp lets be the level's last row, it would
  // leave the image -- past the caller's buffer with pitch == cols -- so row 42's chunk-3 slots load
  // chunk 2 again. Every fast-path load then lies inside [org, level + (h - 1) * pitch + w):
  // row 42 ends at column xa + 47 <= x + 26 <= w - 5. Border windows (reflect-101 rows and
  // columns) gather bytes into the same slots.
  uint8_t* win = &s_win[wid][0];
  uint32_t dma_row[3], dma_off[3], a_lds[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int r = 16 * i + (lane >> 2);
    dma_row[i] = (uint32_t)min(r, 42);
    const uint32_t chunk = (uint32_t)((lane & 3) ^ win_swz(r));
    dma_off[i] = 16u * (r >= 42 && chunk == 3u ? 2u : chunk);
    // the A read of tile row i: row arow[i], chunk g
    a_lds[i] = 16u * (4u * arow[i] + (uint32_t)(mf_g ^ win_swz((int)arow[i])));
  }
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  auto win_fill = [&](const RsGeo& G) {
    if (G.fastp) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)uniform_ptr(G.org), 0, 43 * G.pitch, 0x00020000);
#pragma unroll
      for (int i = 0; i < 3; i++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(win + 1024 * i), 16,
            __umul24(dma_row[i], (uint32_t)G.pitch) + dma_off[i], 0, 0, 0);
    } else {
      // a dword whose 4 columns are inside the level is one aligned load; only the dwords that
      // straddle or leave an edge gather bytes (divergent, few lanes)
      const int xa = (G.kx - 21) & ~3;
      const uint8_t* im = G.level == 0 ? batch_image(b, img)
                                       : b.pyr + (int64_t)img * g->pyr_bytes + g->lv[G.level].offset;
      const bool al = (((uintptr_t)im | (uintptr_t)G.pitch) & 3) == 0;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const uint8_t* row =
            im + (int64_t)reflect101(G.ky - 21 + (int)dma_row[i], G.h) * G.pitch;
        uint32_t wv[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const int c = xa + (int)dma_off[i] + 4 * d;
          if (al && c >= 0 && c + 3 < G.w) {
            wv[d] = *reinterpret_cast<const uint32_t*>(row + c);
          } else {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) v |= (uint32_t)row[reflect101(c + k, G.w)] << (8 * k);
            wv[d] = v;
          }
        }
        reinterpret_cast<uint4*>(win + 1024 * i)[lane] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
      }
    }
  };
  typedef __attribute__((address_space(3))) const uint32_t lds_u32;
  uint32_t* tw = &s_w[wid][4];
  // the lane's first table dword of tile column 0: column n, row 12 g
  uint32_t* tw_lane = tw + mf_n * (kUs / 2) + 6 * mf_g;  // u16 row 12 g of column n
  // Software pipeline over the wave's keypoints: iteration j issues keypoint j's MFMAs, stores
  // keypoint j's table, issues the next keypoint's window loads, finishes keypoint j - 1's tests
  // from the table reads it issued last iteration (their latency covered by this iteration's
  // MFMAs and stores), then issues keypoint j's sample reads. The table is single-buffered: a
  // wave's LDS operations execute in order, so j's stores cannot overtake j - 1's reads.
  // byte address of u16 (c, r) = tw + 2 kUs c + 2 r, c = cx + 18 + s, r = cy + 18:
  // umul24(X, 2 kUs) + 2 Y + 2 kUs s - 2 kUs 0x400000 - 2 M
  const uint32_t rt_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint32_t*)tw -
                          2u * (uint32_t)kUs * 0x400000u - 2u * 0x4B400000u;
  constexpr uint32_t kColBytes = 2u * kUs;
  uint32_t wr[8][4];         // the pending keypoint's sample reads
  uint32_t wsh[8];           // ... and their realignment shifts (u16 table)
  bool tail_p = false;       // ... whether its window reaches the row's scalar tail
  uint32_t xt_p = 0;         // ... and that tail's first column bits
  f32x2 ab_p = {0.f, 0.f}, nab_p = {0.f, 0.f};  // ... and its rotation (the tail case recomputes X)
  // the lane's 8 samples of keypoint j: addresses, then all 16 reads in flight
  auto issue_reads = [&](int alane, const RsGeo& G) {
    const uint32_t sft = (uint32_t)((G.kx - 21) & 3);
    const float cj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ca), alane));
    const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sa), alane));
    const f32x2 ab = {sj, cj}, nab = {cj, -sj};
    // A sample (cx, cy) reads column c = cx + 18 + s, u16 rows cy + 18 .. cy + 24: four aligned
    // dwords from the one holding the first, realigned (v_alignbit by 16 for an odd first row)
    // into the pairs (R0, R1), (R2, R3), (R4, R5), (R6, R7) for v_dot2 -- R7 meets K0's zero high
    // half. The byte address comes straight from the rounded coordinates' float bits
    // X = M + 18 + cx, Y = M + 18 + cy (M = 0x4B400000, low 24 bits 0x400000): see rt_lds.
    const uint32_t rt_base = rt_lds + kColBytes * sft;
    // stage by stage over the 8 samples: a dependent packed-f32 / VALU pair needs a wait state,
    // a sample-at-a-time chain issued one s_nop per step
    // sp = fma({px, px}, ab, {py, py} * nab) + magic, x and y broadcast from the pair
    f32x2 sp[8];
#pragma unroll
    for (int k = 0; k < 8; k++)
      asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(sp[k]) : "v"(pf[k]), "s"(nab));
#pragma unroll
    for (int k = 0; k < 8; k++)
      asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]"
          : "+v"(sp[k]) : "v"(pf[k]), "s"(ab));
#pragma unroll
    for (int k = 0; k < 8; k++) sp[k] = sp[k] + magic;
    uint32_t ta[8];
#pragma unroll
    for (int k = 0; k < 8; k++)  // X * 2 kUs + rt_base in one v_mad_u32_u24 (X's low 24 bits)
      asm("v_mad_u32_u24 %0, %1, %2, %3"
          : "=v"(ta[k]) : "v"(__float_as_uint(sp[k].y)), "v"(kColBytes), "s"(rt_base));
#pragma unroll
    for (int k = 0; k < 8; k++) {
      // 4 aligned dwords from the dword holding row cy: u16 rows cy .. cy + 7 (+ one before
      // when cy is odd); the realignment shift (16 for odd cy) rides along in wsh
      const uint32_t a = (__float_as_uint(sp[k].x) << 1) + ta[k];
      const lds_u32* rw = (const lds_u32*)(uintptr_t)(a & ~3u);
      wr[k][0] = rw[0];
      wr[k][1] = rw[1];
      wr[k][2] = rw[2];
      wr[k][3] = rw[3];
      wsh[k] = __float_as_uint(sp[k].x) << 4;
    }
    // kTail: the window reaches the scalar tail of the row (x >= W - W % 4, rounded half up
    // instead of half to even) -- a wave-uniform case
    const int xvec = G.w - (G.w & 3);
    tail_p = G.kx + 18 >= xvec;
    xt_p = (uint32_t)(xvec - G.kx + 18) + 0x4B400000u;  // X >= this: tail
    ab_p = ab;
    nab_p = nab;
  };
  // keypoint j's 256 tests from the pending reads: descriptor dwords of lanes 4 j .. 4 j + 3
  auto finish = [&](auto jc) {  // the keypoint's index within its half
    constexpr int j = decltype(jc)::value;
    auto run = [&](auto tail_case) {
      constexpr bool kTail = decltype(tail_case)::value;
      // the 8 samples' sums level by level: consecutive v_dot2 are independent (a dependent one
      // needs wait states)
#pragma unroll
      for (int k = 0; k < 8; k++) {  // (R0, R1), (R2, R3), (R4, R5), (R6, R7 | 0)
        wr[k][0] = __builtin_amdgcn_alignbit(wr[k][1], wr[k][0], wsh[k]);
        wr[k][1] = __builtin_amdgcn_alignbit(wr[k][2], wr[k][1], wsh[k]);
        wr[k][2] = __builtin_amdgcn_alignbit(wr[k][3], wr[k][2], wsh[k]);
        wr[k][3] = __builtin_amdgcn_alignbit(0u, wr[k][3], wsh[k]);
      }
      uint32_t smv[8];
#pragma unroll
      for (int k = 0; k < 8; k++) smv[k] = dot2u(wr[k][3], K0, 0u);
#pragma unroll
      for (int k = 0; k < 8; k++) smv[k] = dot2u(wr[k][2], K21, smv[k]);
#pragma unroll
      for (int k = 0; k < 8; k++) smv[k] = dot2u(wr[k][1], K23, smv[k]);
#pragma unroll
      for (int k = 0; k < 8; k++) smv[k] = dot2u(wr[k][0], K01, smv[k]);
      uint64_t words[4];
      static_for<4>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        if constexpr (!kTail) {
          // rounded half to even: o = (s + 0x7fff + bit 16 of s) >> 16, saturated to 255; the
          // test min(o_a, 255) < min(o_b, 255) is (a >> 16) < (b >> 16) && a < 255 << 16 on the
          // biased sums -- compared on their high halves (SDWA) with no shift or clamp
          const uint32_t a = smv[2 * r] + 0x7fffu + ((smv[2 * r] >> 16) & 1u);
          const uint32_t b = smv[2 * r + 1] + 0x7fffu + ((smv[2 * r + 1] >> 16) & 1u);
          words[r] = __ballot((a >> 16) < (b >> 16)) & __ballot(a < 0xff0000u);
          return;
        }
        uint32_t v[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int k = 2 * r + e;
          const uint32_t sm = smv[k];
          uint32_t o;
          if (kTail) {
            f32x2 pq, sp;  // the sample's column bits again (rare case: no VGPRs held for it)
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]"
                : "=v"(pq) : "v"(pf[k]), "s"(nab_p));
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]"
                : "=v"(sp) : "v"(pf[k]), "s"(ab_p), "v"(pq));
            sp = sp + magic;
            const bool tail = __float_as_uint(sp.y) >= xt_p;
            o = (sm + (tail ? 0x8000u : 0x7fffu + ((sm >> 16) & 1u))) >> 16;
          } else {
            o = (sm + 0x7fffu + ((sm >> 16) & 1u)) >> 16;
          }
          v[e] = o > 255u ? 255u : o;
        }
        words[r] = __ballot(v[0] < v[1]);
      });
      // descriptor dword pairs of lanes 4 j .. 4 j + 3 (v_writelane: no per-lane select; the
      // lane selects are inline constants, j and r being compile-time). A v_writelane that reads
      // an SGPR a VALU compare has just written needs wait states (measured: without them bit
      // 7 of ~12 % of the descriptor bytes came out wrong), so the four ballots come first and
      // one s_nop covers them all.
      uint32_t lo = dlo, hi = dhi;  // (local copies: the asm operands of a nested lambda)
      asm volatile("s_nop 4\n\t"
                   "v_writelane_b32 %0, %2, %10\n\tv_writelane_b32 %1, %3, %10\n\t"
                   "v_writelane_b32 %0, %4, %11\n\tv_writelane_b32 %1, %5, %11\n\t"
                   "v_writelane_b32 %0, %6, %12\n\tv_writelane_b32 %1, %7, %12\n\t"
                   "v_writelane_b32 %0, %8, %13\n\tv_writelane_b32 %1, %9, %13"
                   : "+v"(lo), "+v"(hi)
                   : "s"((uint32_t)words[0]), "s"((uint32_t)(words[0] >> 32)),
                     "s"((uint32_t)words[1]), "s"((uint32_t)(words[1] >> 32)),
                     "s"((uint32_t)words[2]), "s"((uint32_t)(words[2] >> 32)),
                     "s"((uint32_t)words[3]), "s"((uint32_t)(words[3] >> 32)),
                     "i"(4 * j), "i"(4 * j + 1), "i"(4 * j + 2), "i"(4 * j + 3));
      dlo = lo;
      dhi = hi;
    };
    if (tail_p) run(std::true_type{});
    else run(std::false_type{});
  };
  RsGeo gn = rs_geo(0);
  win_fill(gn);
  // halves of KH keypoints: the keypoint loop unrolled within a half (its writelane lanes are
  // constants), the halves rolled; each half stores its keypoints' descriptors
  constexpr int KH = KPW < 8 ? KPW : 8;
  const int64_t o = (int64_t)img * g->kp_cap + k0;
#pragma unroll 1
  for (int h = 0; h < KPW / KH; h++) {
    if (KH * h >= nk) break;
    static_for<KH>([&](auto jc) {
    constexpr int jj = decltype(jc)::value;
    const int j = KH * h + jj;
    const RsGeo G = gn;
    // the window has landed (buffer-to-LDS loads count in vmcnt; border windows were stored by
    // this wave's own ds_writes, which its LDS reads follow in order): the A operands
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    wave_lds_sync();
    u32x4 axn[3];
#pragma unroll
    for (int ti = 0; ti < 3; ti++) axn[ti] = *reinterpret_cast<const u32x4*>(win + a_lds[ti]);
    // keypoint j - 1's tests (their table reads were issued last iteration; this VALU covers the
    // A reads' latency, and the sample reads' registers are free again before the MFMA results
    // need theirs)
    if constexpr (jj > 0) finish(std::integral_constant<int, jj - 1>{});
    // the row sums: 9 MFMAs (A bytes - 128 as int8: x ^ 0x80)
    v4i acc[3][3];
    {
      const v4i cinit = {128 * 257, 128 * 257, 128 * 257, 128 * 257};
#pragma unroll
      for (int ti = 0; ti < 3; ti++) {
        const u32x4 x = axn[ti] ^ 0x80808080u;
        const v4i av = {(int)x.x, (int)x.y, (int)x.z, (int)x.w};
#pragma unroll
        for (int tj = 0; tj < 3; tj++)
          acc[ti][tj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bm[tj], cinit, 0, 0, 0);
      }
    }
    if (j + 1 < nk) {
      // the next keypoint's window: its loads overwrite the staging area this keypoint's A reads
      // came from, so they wait for those (the MFMAs above consumed them); none is issued past
      // the wave's last keypoint (no buffer-to-LDS load outlives the wave)
      gn = rs_geo(j + 1);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      win_fill(gn);
    }
    // the u16 table: lane (n, g) writes rows 12 g .. 12 g + 11 of column 16 tj + n as three
    // 8-byte stores (rows past 43 land in the column's spare rows); columns past 39 are outside
    // the table (tile column 2, n >= 8)
    auto st64 = [&](int tj) {
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const uint32_t lo = __builtin_amdgcn_perm((uint32_t)acc[q][tj][1], (uint32_t)acc[q][tj][0], 0x05040100u);
        const uint32_t hi = __builtin_amdgcn_perm((uint32_t)acc[q][tj][3], (uint32_t)acc[q][tj][2], 0x05040100u);
        reinterpret_cast<uint2*>(tw_lane + 16 * tj * (kUs / 2))[q] = make_uint2(lo, hi);
      }
    };
    st64(0);
    st64(1);
    if (mf_n < 8) st64(2);
    __asm__ volatile("" ::: "memory");
    issue_reads(angle_lane(j), G);
    __asm__ volatile("" ::: "memory");
    });
    finish(std::integral_constant<int, KH - 1>{});
    if (lane < 4 * min(KH, nk - KH * h))
      reinterpret_cast<uint64_t*>(desc + (o + KH * h) * 32)[lane] = ((uint64_t)dhi << 32) | dlo;
  }
  const float my_angle = __shfl(angle, angle_lane(lane), 64);
  if (lane < nk) {
    const LevelGeom& L = g->lv[my_level];
    KeyPoint kp;
    kp.x = (float)(key_x((uint32_t)my_key) + kMinBorder);
    kp.y = (float)(key_y((uint32_t)my_key) + kMinBorder);
    if (my_level != 0) {
      kp.x *= L.scale;
      kp.y *= L.scale;
    }
    kp.size = L.patch_size;
    kp.angle = my_angle;
    kp.response = (float)key_score((uint32_t)my_key);
    kp.octave = my_level;
    kp.class_id = -1;
    kps[o + lane] = kp;
  }
}

template <int KPW>
static void launch_od(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st) {
  SLAMGPU_LAUNCH("orient_desc", st, orient_desc_kernel<KPW>,
                 dim3((gd.host->kp_cap + 4 * KPW - 1) / (4 * KPW), n_images), dim3(256), 0, st, b,
                 gd.dev, gd.ws.oct_keys, gd.ws.oct_count, gd.out.kps, gd.out.desc, gd.out.nkps);
}

void launch_orient_desc(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st) {
  if (n_images <= kOdSmallMaxImages)
    launch_od<kKpPerWaveSmall>(b, gd, n_images, st);
  else
    launch_od<kKpPerWave>(b, gd, n_images, st);
}

}  // namespace slamgpu
