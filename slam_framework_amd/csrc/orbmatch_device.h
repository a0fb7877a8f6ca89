// orbmatch_device.h -- the rules of OrbMatcher (src/orb_features/orb_matcher.cpp) that every
// matcher kernel restates, once: orb_search.hip (frame matchers), kfmatch.hip (LocalMapper),
// loopmatch.hip (LoopCloser) and bow_kernels.hip (SearchByBoW) all call these. Device code only
// (no host staging). Every expression keeps the reference's order, width and fmaf placement (the
// library builds with -ffp-contract=off; results are compared bit for bit with the oracles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slamgpu_kfmatch.h"
#include "device_math.h"

namespace slamgpu {

// OrbMatcher::TH_LOW / TH_HIGH / HISTO_LENGTH (orb_matcher.cpp:5-7)
constexpr int kThLow = 50, kThHigh = 100, kHisto = 30;
// Frame::grid_cols / grid_rows (frame.h:104-105); KeyFrame's grid is the same
constexpr int kGridCols = 64, kGridRows = 48;

// ---- DescriptorDistance (:1630-1646): popcount(a ^ b) over the 256 bits ------------------------
struct Desc {
  uint4 a, b;
};

__device__ __forceinline__ Desc load_desc(const uint8_t* d) {
  const uint4* p = reinterpret_cast<const uint4*>(d);
  return Desc{p[0], p[1]};
}

__device__ __forceinline__ int hamming(const Desc& p, const Desc& q) {
  return __popc(p.a.x ^ q.a.x) + __popc(p.a.y ^ q.a.y) + __popc(p.a.z ^ q.a.z) +
         __popc(p.a.w ^ q.a.w) + __popc(p.b.x ^ q.b.x) + __popc(p.b.y ^ q.b.y) +
         __popc(p.b.z ^ q.b.z) + __popc(p.b.w ^ q.b.w);
}
__device__ __forceinline__ int hamming(const Desc& p, const uint8_t* d) {
  return hamming(p, load_desc(d));
}
__device__ __forceinline__ int hamming32(const uint8_t* a, const uint8_t* b) {
  return hamming(load_desc(a), b);
}

// ---- OpenCV arithmetic -------------------------------------------------------------------------
// OpenCV's small float gemm row d = A * b + c (matmul.cpp, len 3; Rcw * X + tcw): float dot, then
// (float)((double) + (double)).
__device__ __forceinline__ float gemm_row(const float* R, const float* x, float c) {
  const float dot = R[0] * x[0] + R[1] * x[1] + R[2] * x[2];
  return (float)((double)dot + (double)c);
}

// cv::norm of a 3-vector: a double sum of squares, its sqrt rounded to float.
__device__ __forceinline__ float norm3(float a, float b, float c) {
  double s = 0.0;
  s += (double)a * (double)a;
  s += (double)b * (double)b;
  s += (double)c * (double)c;
  return (float)sqrt(s);
}

// MapPoint::PredictScale (map_point.cpp:366-396): ceil(log(max_dist / dist) / log_scale_factor)
// with glibc's logf, clamped to the pyramid.
__device__ __forceinline__ int predict_scale(float max_dist, float dist3D, float log_scale_factor,
                                             int nlevels) {
  const int lvl = (int)ceilf(glibc_logf(max_dist / dist3D) / log_scale_factor);
  return lvl < 0 ? 0 : (lvl >= nlevels ? nlevels - 1 : lvl);
}

// ---- rotation histogram ------------------------------------------------------------------------
// Bin of a match's rotation angle_a - angle_b (:212-217 and its repeats in every matcher).
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b) {
  float rot = angle_a - angle_b;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (1.0f / kHisto));
  if (bin == kHisto) bin = 0;
  return bin;
}

// ComputeThreeMaxima (:1584-1625) of the bin counts hist[0 .. kHisto): the bins the matches of
// which are kept (-1: none).
__device__ __forceinline__ void three_maxima(const int* hist, int* i1, int* i2, int* i3) {
  int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
  for (int i = 0; i < kHisto; i++) {
    const int s = hist[i];
    if (s > max1) {
      max3 = max2; max2 = max1; max1 = s;
      ind3 = ind2; ind2 = ind1; ind1 = i;
    } else if (s > max2) {
      max3 = max2; max2 = s;
      ind3 = ind2; ind2 = i;
    } else if (s > max3) {
      max3 = s;
      ind3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    ind3 = -1;
  }
  *i1 = ind1;
  *i2 = ind2;
  *i3 = ind3;
}

// The end of a workgroup-per-pair matcher of W waves (SearchForTriangulation, SearchByBoW): wave
// w accepted acc matches, match i's rotation bin is s_bin[i] (-1: none) and s_hist counts the
// bins. Thread 0 takes the three maxima; with check_ori every match of another bin is withdrawn
// (out[i] = -1; :241-259, :774-787). Returns, in thread 0, the matches that remain. All threads call it.
// s_hist is the kernel's LDS array of kRotWords<W> ints: the kHisto bins, then this function's
// 2 W + 3 words (one array: separate ones, or LDS declared here, are padded more).
template <int W>
constexpr int kRotWords = kHisto + 2 * W + 3;
template <int W>
__device__ __forceinline__ int rot_filter_count(int acc, int check_ori, int* s_hist,
                                                const int8_t* s_bin, int n, int32_t* out) {
  int* const s_w = s_hist + kHisto;
  int* const s_acc = s_w, * const s_rem = s_w + W, * const s_ind = s_w + 2 * W;
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  if (lane == 0) s_acc[wid] = acc;
  __syncthreads();
  if (tid == 0) three_maxima(s_hist, &s_ind[0], &s_ind[1], &s_ind[2]);
  __syncthreads();
  int removed = 0;
  if (check_ori) {
    const int i1 = s_ind[0], i2 = s_ind[1], i3 = s_ind[2];
    for (int i = tid; i < n; i += 64 * W) {
      const int bin = s_bin[i];
      if (bin >= 0 && bin != i1 && bin != i2 && bin != i3) {
        out[i] = -1;
        removed++;
      }
    }
  }
  removed = wave_sum(removed);
  if (lane == 0) s_rem[wid] = removed;
  __syncthreads();
  int nm = 0;
  if (tid == 0)
    for (int w = 0; w < W; w++) nm += s_acc[w] - s_rem[w];
  return nm;
}

// ---- the grid: PosInGrid and GetFeaturesInArea -------------------------------------------------
// float -> int of a cell coordinate with its argument held in range first: a float-to-int
// conversion out of int's range (or of NaN) is undefined, and keypoints and th are the caller's
// in the keyframe matchers, so no coordinate reaches one
__device__ __forceinline__ float cell_clamp(float v) { return fminf(fmaxf(v, -1e6f), 1e6f); }
__device__ __forceinline__ int cell_floor(float v) { return (int)floorf(cell_clamp(v)); }
__device__ __forceinline__ int cell_ceil(float v) { return (int)ceilf(cell_clamp(v)); }

// Frame::PosInGrid (frame.cpp:339-346) before its conversion to int: one cell coordinate
// AssignFeaturesToGrid gives a keypoint, a whole number held as a float (or not finite). A scan
// that tests it against a window as a float needs no clamp (fuse_kernel, per keypoint).
__device__ __forceinline__ float cell_coord(float x, float min_x, float cell_w) {
  return roundf((x - min_x) / cell_w);
}

// PosInGrid: the keypoint's cell; false when that is outside the 64 x 48 grid (the keypoint is in
// no cell).
__device__ __forceinline__ bool pos_in_grid(float x, float y, float min_x, float min_y,
                                            float cell_w, float cell_h, int* px, int* py) {
  *px = (int)cell_clamp(cell_coord(x, min_x, cell_w));
  *py = (int)cell_clamp(cell_coord(y, min_y, cell_h));
  return !(*px < 0 || *px >= kGridCols || *py < 0 || *py >= kGridRows);
}

// Frame / KeyFrame::GetFeaturesInArea (frame.cpp:348-403, keyframe.cpp:442-476): the cell window
// of a search square of half side r around (u, v); false when the window misses the grid
// (window_on_grid: cx0 = 0, cx1 = -1 is an empty window).
__device__ __forceinline__ bool window_on_grid(int cx0, int cx1, int cy0, int cy1) {
  return !(cx1 < 0 || cx0 >= kGridCols || cy1 < 0 || cy0 >= kGridRows);
}
__device__ __forceinline__ bool cell_window(float u, float v, float r, float min_x, float min_y,
                                            float cell_w, float cell_h, int* cx0, int* cx1,
                                            int* cy0, int* cy1) {
  *cx0 = max(0, cell_floor((u - min_x - r) / cell_w));
  *cx1 = min(kGridCols - 1, cell_ceil((u - min_x + r) / cell_w));
  *cy0 = max(0, cell_floor((v - min_y - r) / cell_h));
  *cy1 = min(kGridRows - 1, cell_ceil((v - min_y + r) / cell_h));
  return window_on_grid(*cx0, *cx1, *cy0, *cy1);
}

// A candidate ordered as (distance, cell, keypoint index). GetFeaturesInArea visits the cells
// x-major then y and each cell by keypoint index, so with cell = ix * 48 + iy the minimum key is
// the first strict-'<' winner of the reference's sequential loop.
constexpr uint64_t kNoKey = ~0ull;
__device__ __forceinline__ uint64_t cand_key(uint32_t dist, int cell, int idx) {
  return (uint64_t)dist << 32 | (uint64_t)cell << 12 | (uint32_t)idx;
}
__device__ __forceinline__ int key_idx(uint64_t k) { return (int)(k & 0xfff); }
__device__ __forceinline__ int key_dist(uint64_t k) { return (int)(k >> 32); }

// ---- Fuse's gate chain -------------------------------------------------------------------------
struct Proj {
  float u, v, r, invz;
  int lvl, cx0, cx1, cy0, cy1;
};

// The camera-frame point to the image: positive depth, projection, IsInImage.
__device__ __forceinline__ bool proj_uv(float xc, float yc, float zc, const slamgpu_camera& cam,
                                        const slamgpu_kf_grid& g, Proj* o) {
  if (zc < 0.0f) return false;
  const float invz = 1.0f / zc;
  const float x = xc * invz, y = yc * invz;
  o->invz = invz;
  o->u = fmaf(cam.fx, x, cam.cx);
  o->v = fmaf(cam.fy, y, cam.cy);
  return o->u >= g.min_x && o->u < g.max_x && o->v >= g.min_y && o->v < g.max_y;
}

// Get{Min,Max}DistanceInvariance (map_point.cpp:356-364) around the distance the method measures.
__device__ __forceinline__ bool in_range(const slamgpu_fuse_point& P, float dist3D) {
  const float maxD = 1.2f * P.max_dist, minD = 0.8f * P.min_dist;
  return !(dist3D < minD || dist3D > maxD);
}

// PredictScale, the search radius and its cell window.
__device__ __forceinline__ bool proj_window(const slamgpu_fuse_point& P, float dist3D, float th,
                                            const slamgpu_levels& lv, const slamgpu_kf_grid& g,
                                            Proj* o) {
  o->lvl = predict_scale(P.max_dist, dist3D, lv.log_scale_factor, lv.nlevels);
  o->r = th * lv.scale[o->lvl];
  return cell_window(o->u, o->v, o->r, g.min_x, g.min_y, g.cell_w, g.cell_h, &o->cx0, &o->cx1,
                     &o->cy0, &o->cy1);
}

// The gates of Fuse(pKF, vpMapPoints) :828-878, Fuse(pKF, Scw, ...) :988-1028 and
// SearchByProjection(pKF, Scw, ...) :415-454: depth, projection, IsInImage, distance range,
// viewing angle, PredictScale, window.
__device__ __forceinline__ bool project_scw(const slamgpu_kf& K, const slamgpu_fuse_point& P,
                                            float th, const slamgpu_camera& cam,
                                            const slamgpu_levels& lv, const slamgpu_kf_grid& g,
                                            Proj* o) {
  const float xc = gemm_row(K.Rcw, P.xyz, K.tcw[0]);
  const float yc = gemm_row(K.Rcw + 3, P.xyz, K.tcw[1]);
  const float zc = gemm_row(K.Rcw + 6, P.xyz, K.tcw[2]);
  if (!proj_uv(xc, yc, zc, cam, g, o)) return false;
  const float po0 = P.xyz[0] - K.Ow[0], po1 = P.xyz[1] - K.Ow[1], po2 = P.xyz[2] - K.Ow[2];
  const float dist3D = norm3(po0, po1, po2);
  if (!in_range(P, dist3D)) return false;
  double dot = 0.0;
  dot += (double)po0 * (double)P.normal[0];
  dot += (double)po1 * (double)P.normal[1];
  dot += (double)po2 * (double)P.normal[2];
  if (dot < 0.5 * (double)dist3D) return false;
  return proj_window(P, dist3D, th, lv, g, o);
}

}  // namespace slamgpu
