// orb_octree.hip -- the extractor's keypoint distribution stage (orb_extract.hip has the pipeline).
//   octree        DistributeOctTree, exact list / pointer-order semantics one work-group per
//                 image, a wave per level (small launches: a work-group per level); levels that
//                 do not fit LDS are redone in global memory (octree_kernel)
// Reference: src/orb_features/orb_extractor.cpp (citations per kernel).
#include <algorithm>
#include <cstdlib>

#include "device_math.h"
#include "timing.h"
#include "orb_stages.h"

namespace slamgpu {

// octree: DistributeOctTree (:480-704), one 256-thread workgroup per (image, level).
// The std::list is kept as an array in list order and rebuilt every pass; node keys are
// contiguous index ranges that DivideNode splits by a stable 4-way partition (ballot ranks)
// into the other half of a ping-pong key buffer. Creation sequence numbers stand in for the
// heap addresses the reference sorts by (:625); see SURVEY.md Appendix B.1.
//   outer pass (:528-613): every node with > 1 key is divided, children are pushed to the front
//     in list order (n1..n4), so the new list is [children in reverse push order] + [nodes
//     with one key, in order];
//   inner loop (:615-676): the vPrev nodes are divided in descending (size, seq) order and the
//     loop stops once the list reaches N -- done speculatively in parallel, then cut with a
//     prefix sum; processed nodes leave the list and their children go to the front.
constexpr int kOctThreads = 256;
constexpr int kOctWaves = kOctThreads / 64;
constexpr int kOctCap = 2048;  // max list length / inner-loop set size held in LDS

struct OctShared {
  uint64_t sortk[kOctCap];
  int a[kOctCap];
  int b[kOctCap];
  int c[kOctCap];
  int wsum[16];  // per-wave totals (up to 16 waves)
  int bucket[64 + 1];
  int m, seq_next, mode, nexp, finish, ktotal, total;
};

// Block-wide exclusive scan of v (one value per thread of kThr); returns prefix, *total the sum.
template <int kThr>
__device__ __forceinline__ int block_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wid = wave_id();
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kThr / 64; w++) {
    const int s = wsum[w];
    pre += (w < wid) ? s : 0;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return pre + x - v;
}

// Exclusive scan of arr[0..n) in place (n <= kOctCap) by kThr threads; returns the total.
template <int kThr>
__device__ int block_scan_array(int* arr, int n, int* wsum) {
  constexpr int per = kOctCap / kThr;
  const int base = threadIdx.x * per;
  int loc[per];
  int s = 0;
#pragma unroll
  for (int i = 0; i < per; i++) {
    loc[i] = (base + i < n) ? arr[base + i] : 0;
    s += loc[i];
  }
  int total;
  int pre = block_scan<kThr>(s, wsum, &total);
#pragma unroll
  for (int i = 0; i < per; i++) {
    if (base + i < n) arr[base + i] = pre;
    pre += loc[i];
  }
  __syncthreads();
  return total;
}

// DivideNode (:422-478) of `nd` by one wave: stable partition of its keys into n1..n4.
__device__ void divide_wave(const OctNode& nd, uint32_t* const keys[2], OctNode ch[4],
                            int lane) {
  const int hx = (nd.x1 - nd.x0 + 1) >> 1;  // ceil((float)(UR.x-UL.x)/2)
  const int hy = (nd.y1 - nd.y0 + 1) >> 1;  // ceil((float)(BR.y-UL.y)/2)
  const int xm = nd.x0 + hx, ym = nd.y0 + hy;
  const uint32_t* src = keys[nd.buf] + nd.kbeg;
  uint32_t* dst = keys[nd.buf ^ 1] + nd.kbeg;
  int cnt[4] = {0, 0, 0, 0};
  for (int s = 0; s < nd.n; s += 64) {
    const int i = s + lane;
    int q = -1;
    if (i < nd.n) {
      const uint32_t k = src[i];
      q = (key_x(k) >= xm ? 1 : 0) + (key_y(k) >= ym ? 2 : 0);
    }
#pragma unroll
    for (int qq = 0; qq < 4; qq++) cnt[qq] += __popcll(__ballot(q == qq));
  }
  int start[4];
  start[0] = 0;
  start[1] = cnt[0];
  start[2] = cnt[0] + cnt[1];
  start[3] = start[2] + cnt[2];
  int run[4] = {start[0], start[1], start[2], start[3]};
  for (int s = 0; s < nd.n; s += 64) {
    const int i = s + lane;
    int q = -1;
    uint32_t k = 0;
    if (i < nd.n) {
      k = src[i];
      q = (key_x(k) >= xm ? 1 : 0) + (key_y(k) >= ym ? 2 : 0);
    }
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
      const uint64_t m = __ballot(q == qq);
      if (q == qq) dst[run[qq] + lanes_below(m)] = k;
      run[qq] += __popcll(m);
    }
  }
  const int16_t xs[3] = {(int16_t)nd.x0, (int16_t)xm, (int16_t)nd.x1};
  const int16_t ys[3] = {(int16_t)nd.y0, (int16_t)ym, (int16_t)nd.y1};
#pragma unroll
  for (int qq = 0; qq < 4; qq++) {
    const int qx = qq & 1, qy = qq >> 1;
    ch[qq].x0 = xs[qx];
    ch[qq].x1 = xs[qx + 1];
    ch[qq].y0 = ys[qy];
    ch[qq].y1 = ys[qy + 1];
    ch[qq].kbeg = nd.kbeg + start[qq];
    ch[qq].n = cnt[qq];
    ch[qq].seq = 0;
    ch[qq].buf = nd.buf ^ 1;
  }
}

// The global-memory DistributeOctTree of one (level, image) by a 256-thread work-group, for the
// levels the LDS kernels cannot hold (their oct_count entry is -1). S: LDS scratch.
template <int kThr>
__device__ __forceinline__ void octree_global(
    OctShared& S, int level, int img, const OrbGeom* __restrict__ g,
    const uint32_t* __restrict__ cell_keys, const int* __restrict__ cell_count,
    uint32_t* __restrict__ key_scratch, OctNode* __restrict__ node_scratch,
    uint32_t* __restrict__ oct_keys, int* __restrict__ oct_count, uint32_t* __restrict__ err) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const LevelGeom& L = g->lv[level];
  const int N = L.budget;
  const int ncell = L.ncols * L.nrows;
  const int64_t cbase = (int64_t)img * g->cells_per_image + L.cell_base;
  uint32_t* const keys[2] = {key_scratch + img * g->keys_per_image + L.key_base,
                             key_scratch + img * g->keys_per_image + L.key_base + L.key_cap};
  OctNode* const lists[2] = {node_scratch + img * g->nodes_per_image + L.node_base,
                             node_scratch + img * g->nodes_per_image + L.node_base +
                                 2 * L.node_cap};
  OctNode* const child = node_scratch + img * g->nodes_per_image + L.node_base + 4 * L.node_cap;
  int* const outc = oct_count + img * g->nlevels + level;
  uint32_t* const outk = oct_keys + (int64_t)img * g->out_per_image + L.out_base;
  if (*outc != -1) return;  // done by octree_img_kernel

  // ---- 1. gather FAST candidates in cell row-major order into keys[0]
  for (int c0 = 0; c0 < ncell; c0 += kOctCap) {
    const int n = min(kOctCap, ncell - c0);
    for (int i = tid; i < n; i += kThr) S.a[i] = cell_count[cbase + c0 + i];
    __syncthreads();
    if (tid == 0) S.total = 0;
    const int tot = block_scan_array<kThr>(S.a, n, S.wsum);
    const int base = (c0 == 0) ? 0 : S.ktotal;
    for (int i = wid; i < n; i += (kThr / 64)) {
      const int cnt = cell_count[cbase + c0 + i];
      const int off = base + S.a[i];
      const int gi = i & ~(kCellGroup - 1);  // the cell's key group (c0 is group-aligned)
      const uint32_t* src = cell_keys + (cbase + c0 + gi) * g->cell_cap + (S.a[i] - S.a[gi]);
      for (int k = lane; k < cnt; k += 64)
        if (off + k < L.key_cap) keys[0][off + k] = src[k];
    }
    __syncthreads();
    if (tid == 0) S.ktotal = base + tot;
    __syncthreads();
  }
  int K = S.ktotal;
  if (K > L.key_cap) {
    if (tid == 0) atomicOr(err, kErrKeyOverflow);
    K = L.key_cap;
  }
  if (K == 0) {
    if (tid == 0) *outc = 0;
    return;
  }
  // ---- 2. initial nodes (:484-526): bucket (int)(x / hX), stable, by wave 0
  const int nIni = L.n_ini;
  const float hX = L.hx;
  if (wid == 0) {
    for (int q0 = 0; q0 < nIni; q0 += 64) {
      const int qn = min(64, nIni - q0);
      int cnt = 0;
      for (int s = 0; s < K; s += 64) {
        const int i = s + lane;
        int q = -1;
        if (i < K) q = (int)((float)key_x(keys[0][i]) / hX) - q0;
        for (int qq = 0; qq < qn; qq++) {
          const int pc = __popcll(__ballot(q == qq));
          if (lane == qq) cnt += pc;
        }
      }
      if (lane < qn) S.a[q0 + lane] = cnt;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int q = 0; q < nIni; q++) {
      const int c = S.a[q];
      S.b[q] = run;
      run += c;
    }
  }
  __syncthreads();
  if (wid == 0) {
    for (int q0 = 0; q0 < nIni; q0 += 64) {
      const int qn = min(64, nIni - q0);
      int run = (lane < qn) ? S.b[q0 + lane] : 0;
      for (int s = 0; s < K; s += 64) {
        const int i = s + lane;
        int q = -1;
        uint32_t k = 0;
        if (i < K) {
          k = keys[0][i];
          q = (int)((float)key_x(k) / hX) - q0;
        }
        for (int qq = 0; qq < qn; qq++) {
          const uint64_t m = __ballot(q == qq);
          const int r = __shfl(run, qq, 64);
          if (q == qq) keys[1][r + lanes_below(m)] = k;
          if (lane == qq) run += __popcll(m);
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int i = 0; i < nIni; i++) {
      const int c = S.a[i];
      if (c == 0) continue;  // empty initial nodes are erased (:513-526)
      OctNode nd;
      nd.x0 = (int16_t)(int)(hX * (float)i);
      nd.x1 = (int16_t)(int)(hX * (float)(i + 1));
      nd.y0 = 0;
      nd.y1 = (int16_t)(L.max_by - kMinBorder);
      nd.kbeg = S.b[i];
      nd.n = c;
      nd.seq = i;
      nd.buf = 1;
      lists[0][m++] = nd;
    }
    S.m = m;
    S.seq_next = nIni;
    S.mode = 0;
    S.finish = 0;
    S.nexp = 0;
  }
  __syncthreads();
  int cur = 0;
  // ---- 3. passes
  while (true) {
    const int m = S.m;
    OctNode* const Lc = lists[cur];
    OctNode* const Ln = lists[cur ^ 1];
    if (S.mode == 0) {
      // outer pass: divide every node with > 1 key, in list order
      for (int j = wid; j < m; j += (kThr / 64)) {
        const OctNode nd = Lc[j];
        int t = 0, e = 0;
        if (nd.n > 1) {
          OctNode ch[4];
          divide_wave(nd, keys, ch, lane);
          if (lane == 0)
            for (int q = 0; q < 4; q++) {
              child[4 * j + q] = ch[q];
              t += ch[q].n > 0;
              e += ch[q].n > 1;
            }
        }
        if (lane == 0) {
          S.a[j] = t;               // children pushed
          S.b[j] = (nd.n == 1);     // survives in place
          S.c[j] = e;               // expandable children
        }
      }
      __syncthreads();
      const int T = block_scan_array<kThr>(S.a, m, S.wsum);
      const int U = block_scan_array<kThr>(S.b, m, S.wsum);
      const int E = block_scan_array<kThr>(S.c, m, S.wsum);
      const int newm = T + U;
      const int seq0 = S.seq_next;
      const bool ovf = newm > min(2 * L.node_cap, kOctCap) || E > kOctCap;
      if (!ovf) {
        for (int j = tid; j < m; j += kThr) {
          const OctNode nd = Lc[j];
          if (nd.n > 1) {
            int gpos = S.a[j], epos = S.c[j];
            for (int q = 0; q < 4; q++) {
              OctNode ch = child[4 * j + q];
              if (ch.n == 0) continue;
              ch.seq = seq0 + gpos;
              const int pos = T - 1 - gpos;
              Ln[pos] = ch;
              if (ch.n > 1) S.sortk[epos++] = (uint64_t)pos;  // vSize in push order
              gpos++;
            }
          } else {
            Ln[T + S.b[j]] = nd;
          }
        }
      }
      __syncthreads();
      if (tid == 0) {
        if (ovf) {
          atomicOr(err, kErrNodeOverflow);
          S.finish = 1;
        } else {
          S.m = newm;
          S.seq_next = seq0 + T;
          S.nexp = E;
          if (newm >= N || newm == m) S.finish = 1;
          else if (newm + E * 3 > N) S.mode = 1;
        }
      }
      if (!ovf) cur ^= 1;
      __syncthreads();
      if (S.finish) break;
    } else {
      // inner loop iteration: vPrev = S.sortk[0..V) (list positions, push order)
      const int V = S.nexp;
      int P2 = 1;
      while (P2 < V) P2 <<= 1;
      for (int i = tid; i < P2; i += kThr) {
        uint64_t key = 0;  // pads sort to the end (descending)
        if (i < V) {
          const int pos = (int)S.sortk[i];
          const OctNode& nd = Lc[pos];
          key = ((uint64_t)nd.n << 44) | ((uint64_t)(uint32_t)nd.seq << 12) | (uint64_t)pos;
        }
        S.sortk[i] = key;
      }
      __syncthreads();
      // bitonic sort, descending by (n, seq): reference processes sort() ascending from the end
      for (int k = 2; k <= P2; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
          for (int i = tid; i < P2; i += kThr) {
            const int ixj = i ^ jj;
            if (ixj > i) {
              const uint64_t x = S.sortk[i], y = S.sortk[ixj];
              const bool desc = (i & k) == 0;
              if (desc ? (x < y) : (x > y)) {
                S.sortk[i] = y;
                S.sortk[ixj] = x;
              }
            }
          }
          __syncthreads();
        }
      }
      // speculative division of every vPrev node in processing order
      for (int j = wid; j < V; j += (kThr / 64)) {
        const int pos = (int)(S.sortk[j] & 0xfff);
        const OctNode nd = Lc[pos];
        OctNode ch[4];
        divide_wave(nd, keys, ch, lane);
        if (lane == 0) {
          int t = 0, e = 0;
          for (int q = 0; q < 4; q++) {
            child[4 * j + q] = ch[q];
            t += ch[q].n > 0;
            e += ch[q].n > 1;
          }
          S.a[j] = t;
          S.c[j] = e;
          S.b[j] = t - 1;
        }
      }
      __syncthreads();
      // cut: first j with m + sum_{i<=j}(t_i - 1) >= N
      for (int i = tid; i < V; i += kThr) S.b[i] = S.a[i] - 1;
      __syncthreads();
      block_scan_array<kThr>(S.b, V, S.wsum);  // exclusive prefix of (t - 1)
      if (tid == 0) S.total = V - 1;
      __syncthreads();
      for (int j = tid; j < V; j += kThr)
        if (m + S.b[j] + (S.a[j] - 1) >= N) atomicMin(&S.total, j);
      __syncthreads();
      const int J = S.total;  // last processed index
      const int nproc = J + 1;
      for (int i = tid; i < V; i += kThr)
        if (i >= nproc) {
          S.a[i] = 0;
          S.c[i] = 0;
        }
      __syncthreads();
      const int T = block_scan_array<kThr>(S.a, V, S.wsum);  // push-order child positions
      const int E = block_scan_array<kThr>(S.c, V, S.wsum);
      // survivors: old list minus processed nodes
      for (int i = tid; i < m; i += kThr) S.b[i] = 1;
      __syncthreads();
      for (int j = tid; j < nproc; j += kThr) S.b[(int)(S.sortk[j] & 0xfff)] = 0;
      __syncthreads();
      const int U = block_scan_array<kThr>(S.b, m, S.wsum);
      // block_scan_array overwrote the flags with prefixes; recover flags from processed set
      const int newm = T + U;
      const int seq0 = S.seq_next;
      const bool ovf = newm > min(2 * L.node_cap, kOctCap) || E > kOctCap;
      __shared__ uint8_t processed[kOctCap];
      for (int i = tid; i < m; i += kThr) processed[i] = 0;
      __syncthreads();
      for (int j = tid; j < nproc; j += kThr) processed[(int)(S.sortk[j] & 0xfff)] = 1;
      __syncthreads();
      // new vSize goes to a temporary (S.c keeps E prefixes): reuse child area tail? keep in LDS
      __shared__ int vnext[kOctCap];
      if (!ovf) {
        for (int j = tid; j < nproc; j += kThr) {
          int gpos = S.a[j], epos = S.c[j];
          for (int q = 0; q < 4; q++) {
            OctNode ch = child[4 * j + q];
            if (ch.n == 0) continue;
            ch.seq = seq0 + gpos;
            const int pos = T - 1 - gpos;
            Ln[pos] = ch;
            if (ch.n > 1) vnext[epos++] = pos;
            gpos++;
          }
        }
        for (int i = tid; i < m; i += kThr)
          if (!processed[i]) Ln[T + S.b[i]] = Lc[i];
      }
      __syncthreads();
      for (int i = tid; i < E; i += kThr) S.sortk[i] = (uint64_t)vnext[i];
      __syncthreads();
      if (tid == 0) {
        if (ovf) {
          atomicOr(err, kErrNodeOverflow);
          S.finish = 1;
        } else {
          S.m = newm;
          S.seq_next = seq0 + T;
          S.nexp = E;
          if (newm >= N || newm == m) S.finish = 1;
        }
      }
      if (!ovf) cur ^= 1;
      __syncthreads();
      if (S.finish) break;
    }
  }
  // ---- 4. retain the best key of each node (:682-701): strict '>' keeps the first maximum
  const int m = S.m;
  const OctNode* Lf = lists[cur];
  const int mout = min(m, L.out_cap);
  for (int j = tid; j < mout; j += kThr) {
    const OctNode nd = Lf[j];
    const uint32_t* ks = keys[nd.buf] + nd.kbeg;
    uint32_t best = ks[0];
    for (int k = 1; k < nd.n; k++) {
      const uint32_t kk = ks[k];
      if (key_score(kk) > key_score(best)) best = kk;
    }
    outk[j] = best;
  }
  if (tid == 0) {
    if (m > L.out_cap) atomicOr(err, kErrNodeOverflow);
    *outc = mout;
  }
}

// The fallback after octree_img_kernel: a grid of G <= kOctFbMaxGroups work-groups redoes the
// (image, level) entries octree_img left at -1; group b owns the entries e = b (mod G), reads
// their results at once (one load per thread) and redoes its -1 entries one after another.
// However many levels overflow -- all of them in a batch of busy textures -- they spread over
// the whole grid (at most total / G per group), and no group reads an entry another group
// writes. A batch whose levels all fit costs each group one load per thread.
constexpr int kOctFbMaxGroups = 256;
__global__ __launch_bounds__(kOctThreads) void octree_kernel(
    const OrbGeom* __restrict__ g, int n_images, const uint32_t* __restrict__ cell_keys,
    const int* __restrict__ cell_count, uint32_t* __restrict__ key_scratch,
    OctNode* __restrict__ node_scratch, uint32_t* __restrict__ oct_keys,
    int* __restrict__ oct_count, uint32_t* __restrict__ err) {
  __shared__ OctShared S;
  __shared__ int s_todo[kOctThreads];
  __shared__ int s_wcnt[kOctWaves];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, nlev = g->nlevels;
  const int total = n_images * nlev;  // entry e = img * nlevels + level (oct_count's layout)
  const int G = gridDim.x;
  for (int j0 = 0; (int)blockIdx.x + j0 * G < total; j0 += kOctThreads) {
    const int e = (int)blockIdx.x + (j0 + tid) * G;
    const bool redo = e < total && oct_count[e] == -1;
    const uint64_t m = __ballot(redo);
    if (lane == 0) s_wcnt[wid] = __popcll(m);
    __syncthreads();
    int off = 0, nt = 0;
    for (int w = 0; w < kOctWaves; w++) {
      if (w < wid) off += s_wcnt[w];
      nt += s_wcnt[w];
    }
    if (redo) s_todo[off + lanes_below(m)] = e;
    __syncthreads();
    for (int i = 0; i < nt; i++) {  // octree_global re-initialises everything it uses in S
      const int ei = s_todo[i];
      octree_global<kOctThreads>(S, ei % nlev, ei / nlev, g, cell_keys, cell_count, key_scratch,
                                 node_scratch, oct_keys, oct_count, err);
      __syncthreads();
    }
    __syncthreads();  // s_wcnt / s_todo read by every thread before the next sweep writes them
  }
}

// ---------------------------------------------------------------------------------------
// octree_img: the same DistributeOctTree for all levels of one image in one work-group, one wave
// per level, entirely in LDS and wave-synchronous (one work-group barrier, to allocate the key
// ranges). Per level: keys (one range, partitioned in place), two node lists and the
// count / prefix arrays of a pass (orb_geometry.cpp lays them out). A pass is
//   count children per node -> wave scans -> divide in place + put children at their final
//   list positions,
// so no child array exists. Dividing a node: a lane per node for n <= 32, the wave through
// registers for n <= 1024, the wave through global scratch above that.
// Creation order (the stand-in for the reference's pointer order, :625) only breaks ties inside
// vPrev, whose nodes were all created in the same pass -- in push order, i.e. ascending list
// position -- so nodes carry no sequence number. Levels whose keys do not fit set
// oct_count = -1 and octree_kernel (global memory) redoes them.
#ifndef OCT_LANE_KEYS
#define OCT_LANE_KEYS 64
#endif
constexpr int kOctLaneKeys = OCT_LANE_KEYS;  // <= 255 (8-bit packed quadrant counts)
constexpr int kOctDivRegs = 16;

struct OctNodeS {
  int16_t x0, x1, y0, y1;
  uint32_t kn;  // kbeg | n << 16 (level-relative key range)
};
static_assert(sizeof(OctNodeS) == 12, "compact node");
__device__ __forceinline__ int node_kbeg(const OctNodeS& d) { return (int)(d.kn & 0xffffu); }
__device__ __forceinline__ int node_n(const OctNodeS& d) { return (int)(d.kn >> 16); }

// lane l's node (l wave-uniform): three readlanes instead of an LDS round trip
__device__ __forceinline__ OctNodeS readlane_node(const OctNodeS& nd, int l) {
  uint32_t w[3];
  __builtin_memcpy(w, &nd, sizeof(w));
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = (uint32_t)__builtin_amdgcn_readlane((int)w[i], l);
  OctNodeS o;
  __builtin_memcpy(&o, w, sizeof(w));
  return o;
}

__device__ __forceinline__ int quadrant(uint32_t k, int xm, int ym) {
  return (key_x(k) >= xm ? 1 : 0) + (key_y(k) >= ym ? 2 : 0);
}
__device__ __forceinline__ int node_xm(const OctNodeS& d) { return d.x0 + ((d.x1 - d.x0 + 1) >> 1); }
__device__ __forceinline__ int node_ym(const OctNodeS& d) { return d.y0 + ((d.y1 - d.y0 + 1) >> 1); }

// exclusive prefix sum over the wave (DPP: row shifts, then row broadcasts); *total = sum
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
  int x = v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  *total = __builtin_amdgcn_readlane(x, 63);
  (void)lane;
  return x - v;
}

// in-place exclusive scan of a[0..n) (int16) by one wave; returns the total
__device__ __forceinline__ int wave_scan_array(int16_t* a, int n, int lane) {
  int carry = 0;
  for (int c = 0; c < n; c += 64) {
    const int i = c + lane;
    const int v = i < n ? a[i] : 0;
    int tot;
    const int ex = wave_excl_scan(v, lane, &tot);
    if (i < n) a[i] = (int16_t)(carry + ex);
    carry += tot;
  }
  return carry;
}

// n <= kOctLaneKeys, one lane: 4 packed 8-bit quadrant counts; partitions in place if part
__device__ __forceinline__ uint32_t lane_divide(const OctNodeS& nd, uint32_t* keys, bool part) {
  const int xm = node_xm(nd), ym = node_ym(nd), kb = node_kbeg(nd), n = node_n(nd);
  uint32_t kr[kOctLaneKeys];
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < kOctLaneKeys; r++)
    if (r < n) {
      kr[r] = keys[kb + r];
      c += 1u << (8 * quadrant(kr[r], xm, ym));
    }
  if (part) {
    uint32_t run = (c << 8) + (c << 16) + (c << 24);  // byte q: keys in quadrants below q
#pragma unroll
    for (int r = 0; r < kOctLaneKeys; r++)
      if (r < n) {
        const int q = quadrant(kr[r], xm, ym);
        keys[kb + ((run >> (8 * q)) & 255)] = kr[r];
        run += 1u << (8 * q);
      }
  }
  return c;
}

// one wave: quadrant counts of a node (uniform)
__device__ __forceinline__ void wave_count(const OctNodeS& nd, const uint32_t* keys, int lane,
                                           int cnt[4]) {
  const int xm = node_xm(nd), ym = node_ym(nd), kb = node_kbeg(nd), n = node_n(nd);
#pragma unroll
  for (int q = 0; q < 4; q++) cnt[q] = 0;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int q = s0 + lane < n ? quadrant(keys[kb + s0 + lane], xm, ym) : -1;
#pragma unroll
    for (int qq = 0; qq < 4; qq++) cnt[qq] += __popcll(__ballot(q == qq));
  }
}

// one wave: stable in-place partition of a node's keys; returns the counts (uniform)
__device__ void wave_partition(const OctNodeS& nd, uint32_t* keys, uint32_t* gscratch, int lane,
                               int cnt[4]) {
  const int xm = node_xm(nd), ym = node_ym(nd), kb = node_kbeg(nd), n = node_n(nd);
  if (n <= 64 * kOctDivRegs) {  // through registers: one read of the keys, counted, then placed
    const int R = (n + 63) >> 6;
    uint32_t kr[kOctDivRegs];
    int qr[kOctDivRegs];
#pragma unroll
    for (int r = 0; r < kOctDivRegs; r++) {
      qr[r] = -1;
      if (r < R && 64 * r + lane < n) {
        kr[r] = keys[kb + 64 * r + lane];
        qr[r] = quadrant(kr[r], xm, ym);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) cnt[q] = 0;
#pragma unroll
    for (int r = 0; r < kOctDivRegs; r++)
      if (r < R) {
#pragma unroll
        for (int q = 0; q < 4; q++) cnt[q] += __popcll(__ballot(qr[r] == q));
      }
    int run[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
#pragma unroll
    for (int r = 0; r < kOctDivRegs; r++)
      if (r < R) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint64_t m = __ballot(qr[r] == q);
          if (qr[r] == q) keys[kb + run[q] + lanes_below(m)] = kr[r];
          run[q] += __popcll(m);
        }
      }
  } else {  // through this level's global scratch (first passes of very dense levels only)
    wave_count(nd, keys, lane, cnt);
    int run[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
    for (int i = lane; i < n; i += 64) gscratch[kb + i] = keys[kb + i];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int i = s0 + lane;
      uint32_t k = 0;
      int q = -1;
      if (i < n) {
        k = gscratch[kb + i];
        q = quadrant(k, xm, ym);
      }
#pragma unroll
      for (int qq = 0; qq < 4; qq++) {
        const uint64_t m = __ballot(q == qq);
        if (q == qq) keys[kb + run[qq] + lanes_below(m)] = k;
        run[qq] += __popcll(m);
      }
    }
  }
}

__global__ __launch_bounds__(64 * kMaxLevels) void octree_img_kernel(
    const OrbGeom* __restrict__ g, const uint32_t* __restrict__ cell_keys,
    const int* __restrict__ cell_count, uint32_t* __restrict__ key_scratch,
    uint32_t* __restrict__ oct_keys, int* __restrict__ oct_count, uint32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_oct[];
  __shared__ int s_K[kMaxLevels];
  const int img = blockIdx.x, lane = threadIdx.x & 63, level = wave_id();
  const int nlev = g->nlevels;
  const bool active = level < nlev;
  const LevelGeom& L = g->lv[active ? level : 0];
  const int ncell = L.ncols * L.nrows;
  const int64_t cbase = (int64_t)img * g->cells_per_image + L.cell_base;
  // ---- 1. candidate counts -> this level's key range (levels that do not fit fall back)
  int K = 0;
  if (active) {
    for (int c = lane; c < ncell; c += 64) K += cell_count[cbase + c];
    K = wave_sum(K);
    if (lane == 0) s_K[level] = K;
  }
  __syncthreads();
  if (!active) return;
  int* const outc = oct_count + img * nlev + level;
  uint32_t* const outk = oct_keys + (int64_t)img * g->out_per_image + L.out_base;
  const int nIni = L.n_ini;
  int koff = 0;
  bool fits = true;
  for (int l = 0; l <= level; l++) {
    const bool f = koff + s_K[l] <= g->oct_kcap;
    if (l == level) fits = f;
    else if (f) koff += s_K[l];
  }
  if (!fits || nIni > 16) {
    if (lane == 0) *outc = -1;  // octree_kernel redoes this level
    return;
  }
  if (K == 0) {
    if (lane == 0) *outc = 0;
    return;
  }
  uint32_t* const keys = reinterpret_cast<uint32_t*>(s_oct) + koff;
  uint32_t* const gscratch = key_scratch + img * g->keys_per_image + L.key_base;
  const int NC = L.oct_nc;
  OctNodeS* const lists = reinterpret_cast<OctNodeS*>(s_oct + L.oct_list_off);
  uint32_t* const sortk = reinterpret_cast<uint32_t*>(s_oct + L.oct_work_off);
  int16_t* const pt = reinterpret_cast<int16_t*>(sortk + NC);
  int16_t* const pe = pt + NC;
  int16_t* const pu = pe + NC;
  int16_t* const vnext = pu + NC;
  uint8_t* const processed = reinterpret_cast<uint8_t*>(vnext + NC);

  // ---- 2. gather in cell row-major order, stably bucketed into the initial nodes
  // (:484-526, bucket (int)(x / hX)). Fast path (<= 512 cells, K <= 3072): all cell counts
  // up front, keys stored in cell order with independent loads (a key slot finds its cell by a
  // binary search over the lanes' prefixes), then one in-place stable partition through
  // registers. Otherwise two sweeps over global memory (count, then place).
  const float hX = L.hx;
  constexpr int kGatherChunks = 8, kGatherRegs = 48;
  // key groups of the fast path's <= 64 * kGatherChunks cells (64 with the default kCellGroup 8,
  // 128 with -DFAST_CELLS_PER_WAVE=4): the search below starts at kMaxGroups / 2, so it reaches
  // every group index < kMaxGroups. gp[] borrows the level's sort scratch (NC >= ncell + 1 u32,
  // checked at run time; ng <= ncell), which the static bound below keeps a group table inside.
  constexpr int kMaxGroups = 64 * kGatherChunks / kCellGroup;
  static_assert(kMaxGroups >= 2 && (kMaxGroups & (kMaxGroups - 1)) == 0,
                "the gather's binary search halves its step from kMaxGroups / 2 down to 1");
  static_assert(kMaxGroups <= 64 * kGatherChunks,
                "gp[] (one int per key group) must fit the ncell + 1 <= NC sort keys it borrows");
  int bcnt = 0;  // lane b < nIni: keys in bucket b
  if (ncell <= 64 * kGatherChunks && K <= 64 * kGatherRegs && ncell + 1 <= NC) {
    // key-group prefixes in LDS (the level's sort scratch, free until the passes): a group's
    // keys are contiguous from its first slot, so a key slot needs only its group -- the
    // largest g with gp[g] <= s (empty groups repeat the next prefix and are skipped) -- found by
    // a branch-free binary search over the <= kMaxGroups groups whose probes for all the wave's
    // slots are issued together, step by step, then every key load at once
    int* const gp = reinterpret_cast<int*>(sortk);
    int ccnt[kGatherChunks];
#pragma unroll
    for (int ch = 0; ch < kGatherChunks; ch++) {
      const int c = 64 * ch + lane;
      ccnt[ch] = c < ncell ? cell_count[cbase + c] : 0;
    }
    int carry = 0;
#pragma unroll
    for (int ch = 0; ch < kGatherChunks; ch++) {
      if (64 * ch < ncell) {
        int ctot;
        const int cex = wave_excl_scan(ccnt[ch], lane, &ctot);
        const int c = 64 * ch + lane;
        if (c < ncell && (c & (kCellGroup - 1)) == 0) gp[c / kCellGroup] = carry + cex;
        carry += ctot;
      }
    }
    wave_lds_sync();
    const int R = (K + 63) >> 6;
    const int ng = (ncell + kCellGroup - 1) / kCellGroup;  // <= kMaxGroups
    uint32_t kr[kGatherRegs];
    int br[kGatherRegs];  // the slot's group during the search, its bucket after
#pragma unroll
    for (int r = 0; r < kGatherRegs; r++) br[r] = 0;
#pragma unroll
    for (int step = kMaxGroups / 2; step >= 1; step >>= 1) {
#pragma unroll
      for (int r = 0; r < kGatherRegs; r++) {
        if (r < R) {
          const int cand = br[r] + step;
          if (cand < ng && gp[cand] <= 64 * r + lane) br[r] = cand;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kGatherRegs; r++) {
      const int s = 64 * r + lane;
      if (r < R && s < K)
        kr[r] = cell_keys[(cbase + kCellGroup * br[r]) * g->cell_cap + (s - gp[br[r]])];
      br[r] = -1;
    }
#pragma unroll
    for (int r = 0; r < kGatherRegs; r++) {
      if (r < R && 64 * r + lane < K) {
        br[r] = (int)((float)key_x(kr[r]) / hX);
        if (br[r] >= nIni) br[r] = -1;
      }
    }
#pragma unroll
    for (int r = 0; r < kGatherRegs; r++)
      if (r < R)
        for (int bb = 0; bb < nIni; bb++) {
          const int pc = __popcll(__ballot(br[r] == bb));
          if (lane == bb) bcnt += pc;
        }
    int tot;
    int brun = wave_excl_scan(lane < nIni ? bcnt : 0, lane, &tot);
#pragma unroll
    for (int r = 0; r < kGatherRegs; r++)
      if (r < R)
        for (int bb = 0; bb < nIni; bb++) {
          const uint64_t mm = __ballot(br[r] == bb);
          const int at = __builtin_amdgcn_readlane(brun, bb);  // bb is wave-uniform
          if (br[r] == bb) keys[at + lanes_below(mm)] = kr[r];
          if (lane == bb) brun += __popcll(mm);
        }
  } else {
    for (int sweep = 0; sweep < 2; sweep++) {
      int brun = 0;  // lane b: next free slot of bucket b (sweep 2)
      if (sweep == 1) {
        int tot;
        brun = wave_excl_scan(lane < nIni ? bcnt : 0, lane, &tot);
      }
      for (int c0 = 0; c0 < ncell; c0 += 64) {
        const int cnt = c0 + lane < ncell ? cell_count[cbase + c0 + lane] : 0;
        int ctot;
        const int cex = wave_excl_scan(cnt, lane, &ctot);
        for (int r0 = 0; r0 < ctot; r0 += 64) {
          const int r = r0 + lane;
          // binary search on all lanes (shuffles read every lane's prefix)
          int lo = 0;
#pragma unroll
          for (int step = 32; step >= 1; step >>= 1) {
            const int cand = lo + step;
            const int pv = __shfl(cex, cand & 63, 64);
            if (cand < 64 && pv <= r) lo = cand;
          }
          const int gs = lo & ~(kCellGroup - 1);  // key group of cell lo (c0 is group-aligned)
          const int base = __shfl(cex, gs, 64);
          int b = -1;
          uint32_t k = 0;
          if (r < ctot) {
            k = cell_keys[(cbase + c0 + gs) * g->cell_cap + (r - base)];
            b = (int)((float)key_x(k) / hX);
            if (b >= nIni) b = -1;
          }
          for (int bb = 0; bb < nIni; bb++) {
            const uint64_t m = __ballot(b == bb);
            if (sweep == 1) {
              const int at = __builtin_amdgcn_readlane(brun, bb);  // bb is wave-uniform
              if (b == bb) keys[at + lanes_below(m)] = k;
              if (lane == bb) brun += __popcll(m);
            } else if (lane == bb) {
              bcnt += __popcll(m);
            }
          }
        }
      }
    }
  }
  // initial nodes: non-empty buckets in order (empty ones are erased, :513-526)
  int m = 0;
  {
    int tot;
    const int bbase = wave_excl_scan(lane < nIni ? bcnt : 0, lane, &tot);
    const bool has = lane < nIni && bcnt > 0;
    const uint64_t hm = __ballot(has);
    if (has) {
      OctNodeS nd;
      nd.x0 = (int16_t)(int)(hX * (float)lane);
      nd.x1 = (int16_t)(int)(hX * (float)(lane + 1));
      nd.y0 = 0;
      nd.y1 = (int16_t)(L.max_by - kMinBorder);
      nd.kn = (uint32_t)bbase | (uint32_t)bcnt << 16;
      lists[lanes_below(hm)] = nd;
    }
    m = __popcll(hm);
  }
  // ---- 3. passes
  const int N = L.budget;
  int cur = 0, nexp = 0;
  bool outer = true;
  while (true) {
    const OctNodeS* Lc = lists + cur * NC;
    OctNodeS* Ln = lists + (cur ^ 1) * NC;
    const int V = outer ? m : nexp;
    if (!outer) {  // vPrev: positions in push order -> descending (n, creation order)
      int P2 = 64;
      while (P2 < V) P2 <<= 1;
      for (int i = lane; i < P2; i += 64) {
        uint32_t key = 0;  // pads sort to the end
        if (i < V) {
          const int pos = (int)sortk[i];
          key = (uint32_t)node_n(Lc[pos]) << 12 | (uint32_t)(4095 - pos);
        }
        sortk[i] = key;
      }
      for (int k = 2; k <= P2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
          wave_lds_sync();
          for (int i = lane; i < P2; i += 64) {
            const int ixj = i ^ jj;
            if (ixj > i) {
              const uint32_t x = sortk[i], y = sortk[ixj];
              const bool desc = (i & k) == 0;
              if (desc ? (x < y) : (x > y)) {
                sortk[i] = y;
                sortk[ixj] = x;
              }
            }
          }
        }
      wave_lds_sync();
    }
    auto nidx = [&](int j) { return outer ? j : 4095 - (int)(sortk[j] & 0xfffu); };
    // -- count children: t (non-empty), e (> 1 key); pu = survivor flag (outer) or t - 1
    for (int j0 = 0; j0 < V; j0 += 64) {
      const int j = j0 + lane;
      const bool valid = j < V;
      OctNodeS nd{};
      if (valid) nd = Lc[nidx(j)];
      const int n = node_n(nd);
      int t = 0, e = 0;
      if (valid && n > 1 && n <= kOctLaneKeys) {
        const uint32_t c = lane_divide(nd, keys, false);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int cq = (c >> (8 * q)) & 255;
          t += cq > 0;
          e += cq > 1;
        }
      }
      uint64_t bigm = __ballot(valid && n > kOctLaneKeys);
      while (bigm) {
        const int bl = __builtin_ctzll(bigm);
        bigm &= bigm - 1;
        const OctNodeS nb = readlane_node(nd, bl);
        int cnt[4];
        wave_count(nb, keys, lane, cnt);
        if (lane == bl) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            t += cnt[q] > 0;
            e += cnt[q] > 1;
          }
        }
      }
      if (valid) {
        pt[j] = (int16_t)t;
        pe[j] = (int16_t)e;
        pu[j] = (int16_t)(outer ? (n == 1) : t - 1);
      }
    }
    int nproc = V;
    if (!outer) {
      // processing stops once the list reaches N: first j with m + sum_{i<=j}(t_i - 1) >= N
      int carry = 0;
      nproc = V;
      for (int j0 = 0; j0 < V; j0 += 64) {
        const int j = j0 + lane;
        const int v = j < V ? pu[j] : 0;
        int tot;
        const int incl = carry + wave_excl_scan(v, lane, &tot) + v;
        const uint64_t hit = __ballot(j < V && m + incl >= N);
        if (hit) {
          nproc = j0 + __builtin_ctzll(hit) + 1;
          break;
        }
        carry += tot;
      }
      for (int i = lane; i < m; i += 64) processed[i] = 0;
      wave_lds_sync();
      for (int j = lane; j < nproc; j += 64) processed[nidx(j)] = 1;
      wave_lds_sync();
      for (int i = lane; i < m; i += 64) pu[i] = (int16_t)(processed[i] ? 0 : 1);
    }
    wave_lds_sync();
    const int T = wave_scan_array(pt, nproc, lane);  // push-order child positions
    const int E = wave_scan_array(pe, nproc, lane);
    const int U = wave_scan_array(pu, m, lane);      // survivors keep their order
    const int newm = T + U;
    if (newm > NC || E > NC) {
      if (lane == 0) atomicOr(err, kErrNodeOverflow);
      break;
    }
    wave_lds_sync();
    // -- divide in place and place children: push order gpos -> list position T-1-gpos
    auto place = [&](int j, const OctNodeS& nd, uint32_t c4) {
      int gpos = pt[j], epos = pe[j];
      const int xm = node_xm(nd), ym = node_ym(nd);
      const int16_t xs[3] = {nd.x0, (int16_t)xm, nd.x1};
      const int16_t ys[3] = {nd.y0, (int16_t)ym, nd.y1};
      int start = node_kbeg(nd);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int cq = (int)((c4 >> (8 * q)) & 255u);
        if (cq > 0) {
          OctNodeS ch;
          ch.x0 = xs[q & 1];
          ch.x1 = xs[(q & 1) + 1];
          ch.y0 = ys[q >> 1];
          ch.y1 = ys[(q >> 1) + 1];
          ch.kn = (uint32_t)start | (uint32_t)cq << 16;
          const int pos = T - 1 - gpos;
          Ln[pos] = ch;
          if (cq > 1) vnext[epos++] = (int16_t)pos;
          gpos++;
        }
        start += cq;
      }
    };
    for (int j0 = 0; j0 < nproc; j0 += 64) {
      const int j = j0 + lane;
      const bool valid = j < nproc;
      OctNodeS nd{};
      if (valid) nd = Lc[nidx(j)];
      const int n = node_n(nd);
      if (valid && n > 1 && n <= kOctLaneKeys) place(j, nd, lane_divide(nd, keys, true));
      uint64_t bigm = __ballot(valid && n > kOctLaneKeys);
      while (bigm) {
        const int bl = __builtin_ctzll(bigm);
        bigm &= bigm - 1;
        const OctNodeS nb = readlane_node(nd, bl);
        const int gpos0 = pt[j0 + bl], epos0 = pe[j0 + bl];  // read before the partition's stores
        int cnt[4];
        wave_partition(nb, keys, gscratch, lane, cnt);
        if (lane == 0) {
          // counts can exceed 255 here: place() takes 8-bit counts, so place big ones inline
          int gpos = gpos0, epos = epos0;
          const int xm = node_xm(nb), ym = node_ym(nb);
          const int16_t xs[3] = {nb.x0, (int16_t)xm, nb.x1};
          const int16_t ys[3] = {nb.y0, (int16_t)ym, nb.y1};
          int start = node_kbeg(nb);
          for (int q = 0; q < 4; q++) {
            if (cnt[q] > 0) {
              OctNodeS ch;
              ch.x0 = xs[q & 1];
              ch.x1 = xs[(q & 1) + 1];
              ch.y0 = ys[q >> 1];
              ch.y1 = ys[(q >> 1) + 1];
              ch.kn = (uint32_t)start | (uint32_t)cnt[q] << 16;
              const int pos = T - 1 - gpos;
              Ln[pos] = ch;
              if (cnt[q] > 1) vnext[epos++] = (int16_t)pos;
              gpos++;
            }
            start += cnt[q];
          }
        }
      }
    }
    for (int i = lane; i < m; i += 64) {
      const OctNodeS nd = Lc[i];
      if (outer ? node_n(nd) == 1 : !processed[i]) Ln[T + pu[i]] = nd;
    }
    wave_lds_sync();
    for (int i = lane; i < E; i += 64) sortk[i] = (uint32_t)vnext[i];
    const int mprev = m;
    m = newm;
    nexp = E;
    cur ^= 1;
    if (newm >= N || newm == mprev) break;
    if (outer && newm + E * 3 > N) outer = false;
  }
  // ---- 4. retain the best key of each node (:682-701): strict '>' keeps the first maximum
  wave_lds_sync();
  const OctNodeS* Lf = lists + cur * NC;
  const int mout = min(m, L.out_cap);
  for (int j = lane; j < mout; j += 64) {
    const OctNodeS nd = Lf[j];
    const int kb = node_kbeg(nd), n = node_n(nd);
    uint32_t best = keys[kb];
    for (int k = 1; k < n; k++) {
      const uint32_t kk = keys[kb + k];
      if (key_score(kk) > key_score(best)) best = kk;
    }
    outk[j] = best;
  }
  if (lane == 0) {
    if (m > L.out_cap) atomicOr(err, kErrNodeOverflow);
    *outc = mout;
  }
}

// ---------------------------------------------------------------------------------------
// The same DistributeOctTree (:480-704) with one work-group of kOctLvlWaves waves per (level,
// image): the latency variant. One wave per level (octree_img_kernel) puts the level-0 wave on
// the critical path of a single frame (0.17 ms of a 0.46 ms frame call: gather 44 us, passes
// 120 us, profiles/r3f_lat_octprof.log); here the gather's loads, the vPrev sort, the per-node
// divides and the big nodes' partitions are spread over the waves. Same list semantics and
// output bytes; a level that does not fit its LDS falls back to octree_kernel as before.
constexpr int kOctLvlWaves = 8, kOctLvlThreads = 64 * kOctLvlWaves;
constexpr int kOctKpt = 16;  // key positions per thread of the passes: levels up to 8192 keys
#ifndef OCT_LVL_MAX_IMAGES
#define OCT_LVL_MAX_IMAGES 16
#endif
constexpr int kOctLvlMaxImages = OCT_LVL_MAX_IMAGES;

__device__ __forceinline__ int lvl_block_sum(int v, int* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[wave_id()] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int k = 0; k < kOctLvlWaves; k++) t += red[k];
  __syncthreads();
  return t;
}

// exclusive scan of a[0..n) in place by the whole work-group
__device__ void lvl_block_scan(int* a, int n, int* red) {
  const int lane = threadIdx.x & 63, w = wave_id();
  int carry = 0;
  for (int c = 0; c < n; c += kOctLvlThreads) {
    const int i = c + (int)threadIdx.x;
    const int v = i < n ? a[i] : 0;
    int wt;
    const int ex = wave_excl_scan(v, lane, &wt);
    if (lane == 0) red[w] = wt;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kOctLvlWaves; k++) {
      pre += k < w ? red[k] : 0;
      tot += red[k];
    }
    if (i < n) a[i] = carry + pre + ex;
    carry += tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kOctLvlThreads) void octree_lvl_kernel(
    const OrbGeom* __restrict__ g, const uint32_t* __restrict__ cell_keys,
    const int* __restrict__ cell_count, uint32_t* __restrict__ key_scratch,
    OctNode* __restrict__ node_scratch, uint32_t* __restrict__ oct_keys,
    int* __restrict__ oct_count, uint32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lvl[];
  __shared__ int s_red[kOctLvlWaves];
  __shared__ int s_bc[kOctLvlWaves][16];  // per-wave bucket counts of one placement round
  __shared__ int s_brun[16];              // next free slot of each initial bucket
  __shared__ int s_bcnt[16];              // keys per initial bucket
  __shared__ int s_u[4];                  // T, E, U of a pass; nproc
  __shared__ int s_scan[kOctLvlWaves][2];  // per-wave totals of the key scan
  const int level = blockIdx.x, img = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int nlev = g->nlevels;
  const LevelGeom& L = g->lv[level];
  const int ncell = L.ncols * L.nrows;
  const int64_t cbase = (int64_t)img * g->cells_per_image + L.cell_base;
  int* const outc = oct_count + img * nlev + level;
  auto otick = [](int) {};
  uint32_t* const outk = oct_keys + (int64_t)img * g->out_per_image + L.out_base;
  // ---- 1. candidate count; a level that does not fit is done here by the global-memory
  // algorithm (octree_global, its scratch on this work-group's LDS; the host checked it fits),
  // so the small launches need no octree_kernel launch after this one
  int K = 0;
  for (int c = tid; c < ncell; c += kOctLvlThreads) K += cell_count[cbase + c];
  K = lvl_block_sum(K, s_red);
  const int nIni = L.n_ini;
  const int NC = L.oct_nc;
  if (K > g->oct2_kcap || K > kOctKpt * kOctLvlThreads || nIni > 16 ||
      ncell + 1 > g->oct2_ccap || NC > g->oct2_nc) {
    if (tid == 0) *outc = -1;
    __syncthreads();
    octree_global<kOctLvlThreads>(*reinterpret_cast<OctShared*>(s_lvl), level, img, g, cell_keys,
                                  cell_count, key_scratch, node_scratch, oct_keys, oct_count, err);
    return;
  }
  if (K == 0) {
    if (tid == 0) *outc = 0;
    return;
  }
  uint32_t* const keys = reinterpret_cast<uint32_t*>(s_lvl);
  uint32_t* const tmp = reinterpret_cast<uint32_t*>(s_lvl + g->oct2_tmp_off);
  int* const cpre = reinterpret_cast<int*>(s_lvl + g->oct2_cpre_off);
  OctNodeS* const lists = reinterpret_cast<OctNodeS*>(s_lvl + g->oct2_list_off);
  uint32_t* const sortk = reinterpret_cast<uint32_t*>(s_lvl + g->oct2_work_off);
  int16_t* const pt = reinterpret_cast<int16_t*>(sortk + NC);
  int16_t* const pe = pt + NC;
  int16_t* const pu = pe + NC;
  int16_t* const vnext = pu + NC;
  uint8_t* const processed = reinterpret_cast<uint8_t*>(vnext + NC);
  uint8_t* const cand = processed + NC;  // the inner passes' candidates (vPrev), by list index
  uint2* const nst = reinterpret_cast<uint2*>(
      (reinterpret_cast<uintptr_t>(cand + NC) + 15) & ~static_cast<uintptr_t>(15));
  uint2* const nen = nst + NC;                         // prefix at / past a node's keys
  int16_t* const cb = reinterpret_cast<int16_t*>(nen + NC);  // first child's push index, or -1

  // ---- 2. gather in cell row-major order (a key slot finds its cell by binary search over the
  // cell prefix), then a stable placement into the initial nodes' buckets (:484-526)
  for (int c = tid; c < ncell; c += kOctLvlThreads) cpre[c] = cell_count[cbase + c];
  if (tid < 16) s_bcnt[tid] = 0;
  __syncthreads();
  lvl_block_scan(cpre, ncell, s_red);
  const float hX = L.hx;
  auto bucket = [&](uint32_t k) {
    const int b = (int)((float)key_x(k) / hX);
    return b >= nIni ? -1 : b;
  };
  constexpr int kGatherUnroll = 4;
  for (int s0 = 0; s0 < K; s0 += kGatherUnroll * kOctLvlThreads) {
    uint32_t kr[kGatherUnroll];
    int sr[kGatherUnroll];
#pragma unroll
    for (int r = 0; r < kGatherUnroll; r++) {
      const int s = s0 + r * kOctLvlThreads + tid;
      sr[r] = s;
      if (s < K) {
        int lo = 0, hi = ncell;  // largest c with cpre[c] <= s: the non-empty cell holding s
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (cpre[mid] <= s) lo = mid;
          else hi = mid;
        }
        const int gs = lo & ~(kCellGroup - 1);  // key group of cell lo: contiguous from gs
        kr[r] = cell_keys[(cbase + gs) * g->cell_cap + (s - cpre[gs])];
      }
    }
#pragma unroll
    for (int r = 0; r < kGatherUnroll; r++)
      if (sr[r] < K) {
        tmp[sr[r]] = kr[r];
        const int b = bucket(kr[r]);
        if (b >= 0) atomicAdd(&s_bcnt[b], 1);
      }
  }
  __syncthreads();
  if (w == 0) {
    int tot;
    const int bb = wave_excl_scan(lane < nIni ? s_bcnt[lane] : 0, lane, &tot);
    if (lane < 16) s_brun[lane] = bb;
  }
  __syncthreads();
  // stable placement, kOctLvlThreads slots per round in slot order
  for (int s0 = 0; s0 < K; s0 += kOctLvlThreads) {
    const int s = s0 + tid;
    uint32_t k = 0;
    int b = -1;
    if (s < K) {
      k = tmp[s];
      b = bucket(k);
    }
    int rank = 0;
    for (int bb = 0; bb < nIni; bb++) {
      const uint64_t m = __ballot(b == bb);
      if (b == bb) rank = lanes_below(m);
      if (lane == bb) s_bc[w][bb] = __popcll(m);
    }
    __syncthreads();
    if (b >= 0) {
      int pos = s_brun[b] + rank;
      for (int k2 = 0; k2 < w; k2++) pos += s_bc[k2][b];
      keys[pos] = k;
    }
    __syncthreads();
    if (tid < nIni) {
      int add = 0;
#pragma unroll
      for (int k2 = 0; k2 < kOctLvlWaves; k2++) add += s_bc[k2][tid];
      s_brun[tid] += add;
    }
    __syncthreads();
  }
  // initial nodes: non-empty buckets in order (empty ones are erased, :513-526)
  if (w == 0) {
    const int bcnt = lane < nIni ? s_bcnt[lane] : 0;
    int tot;
    const int bbase = wave_excl_scan(bcnt, lane, &tot);
    const bool has = lane < nIni && bcnt > 0;
    const uint64_t hm = __ballot(has);
    if (has) {
      OctNodeS nd;
      nd.x0 = (int16_t)(int)(hX * (float)lane);
      nd.x1 = (int16_t)(int)(hX * (float)(lane + 1));
      nd.y0 = 0;
      nd.y1 = (int16_t)(L.max_by - kMinBorder);
      nd.kn = (uint32_t)bbase | (uint32_t)bcnt << 16;
      lists[lanes_below(hm)] = nd;
    }
    if (lane == 0) s_u[0] = __popcll(hm);
  }
  __syncthreads();
  int m = s_u[0];
  __syncthreads();

  // ---- 3. passes: the list semantics of octree_img_kernel, divided key-parallel. Thread t owns
  // the key positions [t * kpt, (t + 1) * kpt) for the whole level: their keys, the node covering
  // each position and the position's exclusive prefix of quadrant one-hots (four 16-bit counters
  // in two words) stay in registers. A pass: one block scan of the one-hots over the candidate
  // nodes' keys -> every node's quadrant counts are the prefix difference across its segment
  // (recorded by the segment's first and last owners) -> the node list's counts, scans and
  // children as before -> each key moves to kbeg + (keys of lower quadrants) + (its rank in its
  // quadrant = its prefix minus the segment's), each position learns its new covering node.
  // No serial per-node loops over keys, and the same stable partition.
  otick(0);
  const int N = L.budget;
  int cur = 0, nexp = 0;
  bool outer = true;
  int Kn = 0;  // keys in the initial nodes (keys past the last bucket are dropped)
  for (int i = 0; i < m; i++) Kn += node_n(lists[i]);
  const int kpt = (Kn + kOctLvlThreads - 1) / kOctLvlThreads;  // <= kOctKpt (checked above)
  const int kb0 = tid * kpt;
  uint32_t kr[kOctKpt];
  int nd[kOctKpt];
  uint32_t plo[kOctKpt], phi[kOctKpt];
  uint64_t qbits = 0;  // 2 bits per position: its key's quadrant in this pass
#pragma unroll
  for (int i = 0; i < kOctKpt; i++) {
    nd[i] = 0;
    if (i < kpt && kb0 + i < Kn) {
      const int k = kb0 + i;
      kr[i] = keys[k];
      int c = 0;  // initial nodes are in key order: the last one starting at or before k
      for (int q = 1; q < m; q++) c += node_kbeg(lists[q]) <= k;
      nd[i] = c;
    }
  }
  while (true) {
    const OctNodeS* Lc = lists + cur * NC;
    OctNodeS* Ln = lists + (cur ^ 1) * NC;
    const int V = outer ? m : nexp;
    if (!outer) {  // vPrev: positions in push order -> descending (n, creation order)
      int P2 = 64;
      while (P2 < V) P2 <<= 1;
      for (int i = tid; i < P2; i += kOctLvlThreads) {
        uint32_t key = 0;  // pads sort to the end
        if (i < V) {
          const int pos = (int)sortk[i];
          key = (uint32_t)node_n(Lc[pos]) << 12 | (uint32_t)(4095 - pos);
        }
        sortk[i] = key;
      }
      for (int i = tid; i < m; i += kOctLvlThreads) cand[i] = 0;
      __syncthreads();
      for (int i = tid; i < V; i += kOctLvlThreads) cand[4095 - (int)(sortk[i] & 0xfffu)] = 1;
      __syncthreads();
      if (V <= 2 * kOctLvlThreads) {
        // rank sort (the keys are distinct): an element's place is the number of larger keys,
        // counted over the whole set with broadcast reads -- two barriers instead of the
        // bitonic network's log^2 steps
        uint32_t mine[2];
        int rk[2] = {0, 0};
#pragma unroll
        for (int r = 0; r < 2; r++) {
          const int i = tid + r * kOctLvlThreads;
          mine[r] = i < V ? sortk[i] : 0u;
        }
        const uint4* s4 = reinterpret_cast<const uint4*>(sortk);
        for (int j4 = 0; j4 < P2 / 4; j4++) {  // pads (0) count for nobody
          const uint4 o = s4[j4];
#pragma unroll
          for (int r = 0; r < 2; r++)
            rk[r] += (int)(o.x > mine[r]) + (int)(o.y > mine[r]) + (int)(o.z > mine[r]) +
                     (int)(o.w > mine[r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; r++)
          if (tid + r * kOctLvlThreads < V) sortk[rk[r]] = mine[r];
        __syncthreads();
      } else {
        for (int k = 2; k <= P2; k <<= 1)
          for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P2; i += kOctLvlThreads) {
              const int ixj = i ^ jj;
              if (ixj > i) {
                const uint32_t x = sortk[i], y = sortk[ixj];
                const bool desc = (i & k) == 0;
                if (desc ? (x < y) : (x > y)) {
                  sortk[i] = y;
                  sortk[ixj] = x;
                }
              }
            }
            __syncthreads();
          }
      }
    }
    otick(1);
    auto nidx = [&](int j) { return outer ? j : 4095 - (int)(sortk[j] & 0xfffu); };
    auto is_cand = [&](int i, const OctNodeS& nn) { return outer ? node_n(nn) > 1 : cand[i] != 0; };
    // -- the key scan: quadrant one-hots of the candidates' keys, exclusive prefix per position
    uint32_t slo = 0, shi = 0;
    qbits = 0;
#pragma unroll
    for (int i = 0; i < kOctKpt; i++) {
      if (i < kpt) {
        uint32_t olo = 0, ohi = 0;
        if (kb0 + i < Kn) {
          const OctNodeS nn = Lc[nd[i]];
          if (is_cand(nd[i], nn)) {
            const uint32_t q = (uint32_t)quadrant(kr[i], node_xm(nn), node_ym(nn));
            qbits |= (uint64_t)q << (2 * i);
            const uint32_t oh = 1u << (16 * (q & 1));
            olo = q < 2 ? oh : 0u;
            ohi = q < 2 ? 0u : oh;
          }
        }
        plo[i] = slo;
        phi[i] = shi;
        slo += olo;
        shi += ohi;
      }
    }
    {
      int tl, th;
      const int el = wave_excl_scan((int)slo, lane, &tl);
      const int eh = wave_excl_scan((int)shi, lane, &th);
      if (lane == 0) {
        s_scan[w][0] = tl;
        s_scan[w][1] = th;
      }
      __syncthreads();
      uint32_t blo = (uint32_t)el, bhi = (uint32_t)eh;
      for (int k = 0; k < w; k++) {
        blo += (uint32_t)s_scan[k][0];
        bhi += (uint32_t)s_scan[k][1];
      }
#pragma unroll
      for (int i = 0; i < kOctKpt; i++) {
        if (i < kpt) {
          plo[i] += blo;
          phi[i] += bhi;
        }
      }
    }
    // segment boundaries: the prefix at a candidate node's first key and past its last
#pragma unroll
    for (int i = 0; i < kOctKpt; i++) {
      if (i < kpt && kb0 + i < Kn) {
        const int k = kb0 + i;
        const OctNodeS nn = Lc[nd[i]];
        if (is_cand(nd[i], nn)) {
          if (k == node_kbeg(nn)) nst[nd[i]] = make_uint2(plo[i], phi[i]);
          if (k == node_kbeg(nn) + node_n(nn) - 1) {
            const uint32_t q = (uint32_t)(qbits >> (2 * i)) & 3u;
            const uint32_t oh = 1u << (16 * (q & 1));
            nen[nd[i]] = make_uint2(plo[i] + (q < 2 ? oh : 0u), phi[i] + (q < 2 ? 0u : oh));
          }
        }
      }
    }
    __syncthreads();
    auto counts = [&](int i, int c[4]) {
      const uint2 a0 = nst[i], a1 = nen[i];
      const uint32_t dl = a1.x - a0.x, dh = a1.y - a0.y;
      c[0] = (int)(dl & 0xffffu);
      c[1] = (int)(dl >> 16);
      c[2] = (int)(dh & 0xffffu);
      c[3] = (int)(dh >> 16);
    };
    // -- count children: t (non-empty), e (> 1 key); pu = survivor flag (outer) or t - 1
    for (int j = tid; j < V; j += kOctLvlThreads) {
      const int i = nidx(j);
      const OctNodeS nn = Lc[i];
      const int n = node_n(nn);
      int t = 0, e = 0;
      if (n > 1) {
        int c[4];
        counts(i, c);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          t += c[q] > 0;
          e += c[q] > 1;
        }
      }
      pt[j] = (int16_t)t;
      pe[j] = (int16_t)e;
      pu[j] = (int16_t)(outer ? (n == 1) : t - 1);
    }
    for (int i = tid; i < m; i += kOctLvlThreads) cb[i] = -1;
    __syncthreads();
    otick(2);
    int nproc = V;
    if (!outer) {
      // processing stops once the list reaches N: first j with m + sum_{i<=j}(t_i - 1) >= N
      if (w == 0) {
        int carry = 0, np = V;
        for (int j0 = 0; j0 < V; j0 += 64) {
          const int j = j0 + lane;
          const int v = j < V ? pu[j] : 0;
          int tot;
          const int incl = carry + wave_excl_scan(v, lane, &tot) + v;
          const uint64_t hit = __ballot(j < V && m + incl >= N);
          if (hit) {
            np = j0 + __builtin_ctzll(hit) + 1;
            break;
          }
          carry += tot;
        }
        if (lane == 0) s_u[3] = np;
      }
      for (int i = tid; i < m; i += kOctLvlThreads) processed[i] = 0;
      __syncthreads();
      nproc = s_u[3];
      for (int j = tid; j < nproc; j += kOctLvlThreads) processed[nidx(j)] = 1;
      __syncthreads();
      for (int i = tid; i < m; i += kOctLvlThreads) pu[i] = (int16_t)(processed[i] ? 0 : 1);
      __syncthreads();
    }
    // push-order child positions, survivors' order: one array per wave
    if (w == 0) {
      const int t = wave_scan_array(pt, nproc, lane);
      if (lane == 0) s_u[0] = t;
    } else if (w == 1) {
      const int t = wave_scan_array(pe, nproc, lane);
      if (lane == 0) s_u[1] = t;
    } else if (w == 2) {
      const int t = wave_scan_array(pu, m, lane);
      if (lane == 0) s_u[2] = t;
    }
    __syncthreads();
    otick(3);
    const int T = s_u[0], E = s_u[1], U = s_u[2];
    const int newm = T + U;
    if (newm > NC || E > NC) {
      if (tid == 0) atomicOr(err, kErrNodeOverflow);
      break;
    }
    // -- children at their final list positions: push order gpos -> list position T-1-gpos
    for (int j = tid; j < nproc; j += kOctLvlThreads) {
      const int i = nidx(j);
      const OctNodeS nn = Lc[i];
      if (node_n(nn) <= 1) continue;
      int c[4];
      counts(i, c);
      int gpos = pt[j], epos = pe[j];
      cb[i] = (int16_t)gpos;
      const int xm = node_xm(nn), ym = node_ym(nn);
      const int16_t xs[3] = {nn.x0, (int16_t)xm, nn.x1};
      const int16_t ys[3] = {nn.y0, (int16_t)ym, nn.y1};
      int start = node_kbeg(nn);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (c[q] > 0) {
          OctNodeS ch;
          ch.x0 = xs[q & 1];
          ch.x1 = xs[(q & 1) + 1];
          ch.y0 = ys[q >> 1];
          ch.y1 = ys[(q >> 1) + 1];
          ch.kn = (uint32_t)start | (uint32_t)c[q] << 16;
          const int pos = T - 1 - gpos;
          Ln[pos] = ch;
          if (c[q] > 1) vnext[epos++] = (int16_t)pos;
          gpos++;
        }
        start += c[q];
      }
    }
    otick(4);
    for (int i = tid; i < m; i += kOctLvlThreads) {
      const OctNodeS nn = Lc[i];
      if (outer ? node_n(nn) == 1 : !processed[i]) Ln[T + pu[i]] = nn;
    }
    __syncthreads();
    // -- keys to their quadrant's range; each position's covering node in the new list
#pragma unroll
    for (int i = 0; i < kOctKpt; i++) {
      if (i < kpt && kb0 + i < Kn) {
        const int k = kb0 + i;
        const int o = nd[i];
        const int base = cb[o];
        if (base >= 0) {
          const OctNodeS nn = Lc[o];
          int c[4];
          counts(o, c);
          const uint2 s0 = nst[o];
          const uint32_t q = (uint32_t)(qbits >> (2 * i)) & 3u;
          const uint32_t dl = plo[i] - s0.x, dh = phi[i] - s0.y;
          const int rank = (int)(((q < 2 ? dl : dh) >> (16 * (q & 1))) & 0xffffu);
          int off = 0;
#pragma unroll
          for (int qq = 0; qq < 4; qq++) off += (uint32_t)qq < q ? c[qq] : 0;
          const int kb = node_kbeg(nn);
          keys[kb + off + rank] = kr[i];
          // the child whose range holds position k: ranges in quadrant order from kb
          const int r = k - kb;
          int cum = 0, nz = 0, child = 0;
#pragma unroll
          for (int qq = 0; qq < 4; qq++) {
            if (c[qq] > 0 && r >= cum) child = nz;
            nz += c[qq] > 0;
            cum += c[qq];
          }
          nd[i] = T - 1 - (base + child);
        } else {
          nd[i] = T + pu[o];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kOctKpt; i++)
      if (i < kpt && kb0 + i < Kn) kr[i] = keys[kb0 + i];
    for (int i = tid; i < E; i += kOctLvlThreads) sortk[i] = (uint32_t)vnext[i];
    __syncthreads();
    otick(5);
    const int mprev = m;
    m = newm;
    nexp = E;
    cur ^= 1;
    if (newm >= N || newm == mprev) break;
    if (outer && newm + E * 3 > N) outer = false;
  }
  // ---- 4. retain the best key of each node (:682-701): strict '>' keeps the first maximum
  __syncthreads();
  const OctNodeS* Lf = lists + cur * NC;
  const int mout = min(m, L.out_cap);
  for (int j = tid; j < mout; j += kOctLvlThreads) {
    const OctNodeS nd = Lf[j];
    const int kb = node_kbeg(nd), n = node_n(nd);
    uint32_t best = keys[kb];
    for (int k = 1; k < n; k++) {
      const uint32_t kk = keys[kb + k];
      if (key_score(kk) > key_score(best)) best = kk;
    }
    outk[j] = best;
  }
  if (tid == 0) {
    if (m > L.out_cap) atomicOr(err, kErrNodeOverflow);
    *outc = mout;
  }
}

// ---------------------------------------------------------------------------------------
// Which octree kernel a launch of n_images uses: the per-level work-groups for small batches
// (the single-frame call's critical path), one work-group per image otherwise.
// SLAMGPU_OCT_LVL=0 / 1 forces one of them (A/B and tests).
static bool octree_per_level(int n_images) {
  static const int mode = [] {
    const char* e = std::getenv("SLAMGPU_OCT_LVL");
    return e ? std::atoi(e) : -1;
  }();
  if (mode >= 0) return mode != 0;
  return n_images <= kOctLvlMaxImages;
}

void launch_octree(const OrbGeomDev& gd, int n_images, hipStream_t st) {
  const OrbGeom& g = *gd.host;
  // the per-level kernel redoes its oversized levels itself (its LDS sized for the global
  // algorithm's scratch too): no octree_kernel launch after it -- the single-frame call's chain
  // is one dependent launch shorter; after the per-image kernel octree_kernel does them
  if (g.oct_kcap == 0 || octree_per_level(n_images)) {
    SLAMGPU_LAUNCH("octree", st, octree_lvl_kernel, dim3(g.nlevels, n_images),
                   dim3(kOctLvlThreads), std::max((size_t)g.oct2_lds_bytes, sizeof(OctShared)),
                   st, gd.dev, gd.ws.cell_keys, gd.ws.cell_count, gd.ws.key_scratch,
                   gd.ws.node_scratch, gd.ws.oct_keys, gd.ws.oct_count, gd.ws.err);
    return;
  }
  SLAMGPU_LAUNCH("octree", st, octree_img_kernel, dim3(n_images), dim3(64 * g.nlevels),
                 (size_t)g.oct_lds_bytes, st, gd.dev, gd.ws.cell_keys, gd.ws.cell_count,
                 gd.ws.key_scratch, gd.ws.oct_keys, gd.ws.oct_count, gd.ws.err);
  const int groups = std::min(g.nlevels * n_images, kOctFbMaxGroups);
  SLAMGPU_LAUNCH("octree_global", st, octree_kernel, dim3(groups), dim3(kOctThreads), 0, st,
                 gd.dev, n_images, gd.ws.cell_keys, gd.ws.cell_count, gd.ws.key_scratch,
                 gd.ws.node_scratch, gd.ws.oct_keys, gd.ws.oct_count, gd.ws.err);
}

hipError_t octree_lds_limits(int device, int* img_bytes, int* lvl_bytes) {
  int max_lds = 0;
  hipError_t e = hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
  if (e != hipSuccess) return e;
  hipFuncAttributes a{};
  if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&octree_img_kernel))) != hipSuccess)
    return e;
  *img_bytes = max_lds - (int)a.sharedSizeBytes;
  if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&octree_lvl_kernel))) != hipSuccess)
    return e;
  // the per-level kernel's dynamic LDS is at least the global algorithm's OctShared
  *lvl_bytes = max_lds - (int)a.sharedSizeBytes;
  if (*lvl_bytes < (int)sizeof(OctShared)) *lvl_bytes = 0;
  return hipSuccess;
}

}  // namespace slamgpu
