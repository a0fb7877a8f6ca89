// frame_tables.hip -- the per-frame tables and records around the matchers on gfx950, batched
// over frames.
//
//   stereo_rows     right-keypoint row table          Frame::ComputeStereoMatches :412-433
//   grid_build      64x48 keypoint grid (CSR)         Frame::AssignFeaturesToGrid :234-248
//   frame_pack      a frame's results in the host mirror's layout (match_kernels.h)
//   frame_aux       the single-frame call's stereo_rows, grid_build and frame_pack as one launch
//   undistort       Frame::UndistortKeyPoints         :614-641
//   vo_queries      the previous frame's stereo keypoints as frame-to-frame queries
//   trace_marker    an empty kernel: a mark in a profiler's kernel trace
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"
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

void launch_stereo_rows(const OrbGeomDev& gd, const FrameKps& ext, int nrows, int n_frames,
                        const StereoWorkspace& ws, hipStream_t st) {
  if (n_frames <= 8)
    SLAMGPU_LAUNCH("stereo_rows", st, stereo_rows_kernel<1024>, dim3(n_frames), dim3(1024), 0, st,
                   gd.dev, ext, nrows, ws, gd.ws.err);
  else
    SLAMGPU_LAUNCH("stereo_rows", st, stereo_rows_kernel<256>, dim3(n_frames), dim3(256), 0, st,
                   gd.dev, ext, nrows, ws, gd.ws.err);
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
