// ba_coop.hip -- one bundle-adjustment problem spread over a cooperative grid.
//
// Optimizer::LocalBundleAdjustment (optimizer.cpp:413-716) as the LocalMapper calls it -- one
// problem at a time, on the mapping thread's critical path -- and Optimizer::BundleAdjustment
// (the global BA, optimizer.cpp:33-207), with g2o's BlockSolver_6_3 + Levenberg-Marquardt
// arithmetic (the same statements as the one-work-group kernel in ba_kernels.hip) but:
//   * no cap on the optimised window: the reduced camera system S (6K x 6K) is dense in HBM and
//     only its structurally non-zero 6x6 blocks are listed, found per phase by a radix sort of the
//     (block, point-pair) keys every point contributes (hipcub, stable: each block's pairs stay in
//     point order, so every sum has a fixed order and the solver is deterministic);
//   * one problem over G work-groups (32 by default, all resident at once), synchronised by a
//     grid barrier at each data dependency. Per LM iteration: the linearisation (a thread per
//     point over its edges: errors, Hll, bl, the 6x3 Hpl blocks; a wave per (keyframe, chunk):
//     partial Hpp, bp) -> barrier; per LM trial: the S blocks (a wave per block over its point
//     pairs, the point's (Hll + lambda I)^-1 formed on the fly) and the reduced rhs -> barrier ->
//     work-group 0 factors S (6x6-blocked LDLT, in LDS when 6K <= 144) and updates the keyframes
//     -> barrier -> a thread per point back-substitutes, updates and re-evaluates its edges ->
//     barrier. Three grid barriers per trial, one per iteration.
// Every LM decision (rho, lambda, the stop flag) is computed from the same per-work-group
// partials in the same order by every work-group, so the control flow is grid-uniform.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>

#include "ba_coop.h"
#include "ba_device.h"
#include "ba_ldlt.h"
#include "timing.h"

namespace slamgpu {
namespace {

using namespace ba;

constexpr int kT = kCoopThreads, kW = kT / 64;
constexpr int kMaxGrid = 256;  // work-groups of a cooperative launch (<= one per CU)
constexpr uint32_t kPadKey = 0xFFFFFFFFu;
constexpr int kChunk = 64;  // S-block pairs per assembly task (one per lane)
constexpr int kCP = 42;     // per-chunk partials: 36 of the 6x6 block + 6 of the reduced rhs

struct CoopShared {
  double S[kCoopLdsN * (kCoopLdsN + 1) / 2];  // packed lower L of the factorisation
  double rhs[kCoopLdsN];
  double dg[kCoopLdsN];
  double idg[kCoopLdsN];  // 1 / dg, formed once per pivot by the diagonal factorisation
  double V[kCoopLdsN * 6];
  double red[kW];
  double gpart[4][kMaxGrid];  // per-work-group partials staged for the grid totals
  double tot[4];
  int iscan[kT];
  int itot;
  float isig[SLAMGPU_MAX_LEVELS];
  int ok;
  double pacc[8];  // SLAMGPU_BA_PROFILE: work-group 0's per-phase wall time (LDS, not registers)
  uint64_t pt0;
};

__device__ __forceinline__ double& ptf(const CoopWs& w, int p, int f) {
  return w.pt[(size_t)f * w.n_pt + p];
}
__device__ __forceinline__ double* kfr(const CoopWs& w, int k) { return w.kf + (size_t)k * 64; }

__device__ __forceinline__ void decode_key(uint32_t key, int& kh, int& kl) {
  int h = (int)((sqrt(8.0 * (double)key + 1.0) - 1.0) * 0.5);
  while (tri(h + 1) <= (int)key) h++;
  while (tri(h) > (int)key) h--;
  kh = h;
  kl = (int)key - tri(h);
}

// ---- grid barrier --------------------------------------------------------------------------
// Arrival counter + generation word in device memory. Every wave drains its own stores
// (vmcnt(0)) before the work-group barrier; then ONE lane per work-group releases at device scope
// (one write-back of its XCD's L2), arrives with a relaxed add, polls the generation word with
// relaxed (L1-bypassing) loads, and acquires once for the whole CU (one L1 invalidate, waited
// for) before the second work-group barrier -- the one-fence-per-work-group form, instead of a
// release + acquire from every wave. Work-group 0 can carry a poll of the caller's stop flag
// (system scope: host-mapped memory) into CTL_POLL, which every work-group reads after the
// barrier -- so all of them take the same decision. A waiter gives up only when nothing moves:
// its count of sleeps restarts whenever the arrival counter or work-group 0's heartbeat
// (CTL_BEAT, bumped per block column while it factors S alone) changes, so a long factorisation
// never times out; ~2^22 sleeps (~2 s) without either raise CTL_ERR with the arrivals seen
// (CTL_ARRIVED of CTL_GRID: work-groups that never became resident). Later barriers do not wait
// once it is set.
__device__ void grid_sync(const CoopWs& w, const int32_t* stop_flag, bool poll) {
  vm_drain();  // this wave's stores have reached L2
  __syncthreads();
  if (threadIdx.x == 0) {
    if (poll && blockIdx.x == 0) {
      const int32_t v =
          stop_flag ? __hip_atomic_load(stop_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
      __hip_atomic_store(&w.ctl[CTL_POLL], v != 0 ? 1 : 0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    vm_drain();  // the write-back (and the CTL_POLL store) complete before the arrival
    if (__hip_atomic_load(&w.ctl[CTL_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      const uint32_t g = __hip_atomic_load(&w.bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      vm_drain();  // the generation is read before this work-group can complete the barrier
      const uint32_t a =
          __hip_atomic_fetch_add(&w.bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a == gridDim.x - 1) {
        __hip_atomic_store(&w.bar[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        vm_drain();  // the reset lands before anyone can arrive at the next barrier
        __hip_atomic_store(&w.bar[1], g + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        uint32_t spins = 0, polls = 0, seen_a = a + 1u;
        int32_t seen_beat = __hip_atomic_load(&w.ctl[CTL_BEAT], __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(&w.bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) {
          if (polls < 256) __builtin_amdgcn_s_sleep(1);  // short waits: poll fast
          else __builtin_amdgcn_s_sleep(16);             // then back off (~1k cycles)
          polls++;
          if ((++spins & 1023u) == 0) {  // progress check
            const uint32_t na =
                __hip_atomic_load(&w.bar[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int32_t nb =
                __hip_atomic_load(&w.ctl[CTL_BEAT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (na != seen_a || nb != seen_beat) {
              seen_a = na;
              seen_beat = nb;
              spins = 0;
            } else if (spins > (1u << 22)) {
              __hip_atomic_store(&w.ctl[CTL_ARRIVED], (int32_t)na, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(&w.ctl[CTL_GRID], (int32_t)gridDim.x, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(&w.ctl[CTL_ERR], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // invalidates this CU's L1
    vm_drain();  // ... and waits for it before the other waves are released
  }
  __syncthreads();
}

__device__ __forceinline__ int ctl_load(const CoopWs& w, int i) {
  return __hip_atomic_load(&w.ctl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Work-group sum (wave butterflies, then the waves in order by thread 0) -> part[wg][slot].
__device__ void wg_part(CoopShared& sh, const CoopWs& w, double v, int slot, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sh.red[0];
    for (int k = 1; k < kW; k++) s = is_max ? fmax(s, sh.red[k]) : s + sh.red[k];
    w.part[(size_t)blockIdx.x * 8 + slot] = s;
  }
  __syncthreads();
}
// Grid totals of partial slots slot0 .. slot0 + ns - 1 (ns <= 4), each summed (or max-ed) in
// work-group order, identical in every work-group: the partials are loaded in parallel into LDS,
// then thread 0 reduces them. Results in sh.tot[0 .. ns). Contains barriers.
__device__ void grid_totals(CoopShared& sh, const CoopWs& w, int slot0, int ns, bool is_max) {
  const int G = gridDim.x;
  for (int t = threadIdx.x; t < G * ns; t += kT) {
    const int g = t / ns, k = t - g * ns;
    sh.gpart[k][g] = w.part[(size_t)g * 8 + slot0 + k];
  }
  __syncthreads();
  if (threadIdx.x < ns) {
    const int k = threadIdx.x;
    double v = sh.gpart[k][0];
    for (int g = 1; g < G; g++) v = is_max ? fmax(v, sh.gpart[k][g]) : v + sh.gpart[k][g];
    sh.tot[k] = v;
  }
  __syncthreads();
}

// Write-through (sc1) store / L1-bypassing (sc1) load of a hand-off partial: the reduction
// partials below go from the waves that produce them to the last arriver without any fence.
__device__ __forceinline__ void st_wt(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wt(const double* p) {
  return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wave that has just stored its partial of a reduction with `total` contributors (st_wt):
// drains the stores and counts itself in at `counter` (relaxed add); returns true (wave-uniform)
// in the wave that arrived last, which then reads every partial with ld_wt and resets the counter.
__device__ __forceinline__ bool last_arriver(int32_t* counter, int total) {
  vm_drain();
  int a = 0;
  if ((threadIdx.x & 63) == 0)
    a = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a = __builtin_amdgcn_readfirstlane(a);
  if (a != total - 1) return false;
  if ((threadIdx.x & 63) == 0)
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// ---- setup and structure kernels -------------------------------------------------------------
__global__ __launch_bounds__(256) void coop_setup_kernel(CoopProblem pb, CoopWs w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < pb.n_kf) {  // Converter::toSE3Quat
    const float* T = pb.kf_Tcw + (size_t)i * 16;
    double R[9];
    SE3 E;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[3 * r + c] = T[4 * r + c];
      E.t[r] = T[4 * r + 3];
    }
    E.r = se3::quat_from_R(R);
    se3::normalize_rotation(E.r);
    store_T(kfr(w, i), E);
  }
  if (i < pb.n_pts) {
    for (int c = 0; c < 3; c++) {
      ptf(w, i, PX + c) = pb.points[(size_t)i * 3 + c];
      ptf(w, i, PXL + c) = 0.0;
    }
    for (int ge = pb.pstart[i]; ge < pb.pstart[i + 1]; ge++) w.opoint[ge] = i;
  }
  if (i < pb.n_obs) {
    w.act[i] = 1;
    w.chi2[i] = 0.0;
  }
  if (i < 6 * pb.K) w.xp[i] = 0.0;
  if (i < 8) w.ctl[i] = 0;
  if (i < 2) w.bar[i] = 0u;
  if (w.prof && i < 16) w.prof[i] = 0.0;
}

// Per point: its active edges to optimised keyframes, sorted by keyframe, and its pair count.
__global__ __launch_bounds__(256) void coop_sort_kernel(CoopProblem pb, CoopWs w) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > pb.n_pts) return;
  if (p == pb.n_pts) {
    w.npairs[p] = 0;
    return;
  }
  const int s = pb.pstart[p], e1 = pb.pstart[p + 1];
  int m = 0;
  for (int e = s; e < e1; e++) {
    if (!w.act[e]) continue;
    const int f = w.free_of_kf[pb.obs[e].keyframe];
    if (f < 0) continue;
    int i = m;
    while (i > 0) {
      const int prev = w.psorted[s + i - 1];
      if (w.free_of_kf[pb.obs[prev].keyframe] < f) break;
      w.psorted[s + i] = prev;
      i--;
    }
    w.psorted[s + i] = e;
    m++;
  }
  w.npairs[p] = m * (m + 1) / 2;
}

__global__ __launch_bounds__(256) void coop_emit_kernel(CoopProblem pb, CoopWs w) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= pb.n_pts) return;
  const int s = pb.pstart[p];
  const int np = w.npairs[p];
  int m = 0;
  while ((m + 1) * (m + 2) / 2 <= np) m++;
  const int base = w.poff[p];
  for (int i = 0; i < m; i++) {
    const int ei = w.psorted[s + i], fi = w.free_of_kf[pb.obs[ei].keyframe];
    for (int j = 0; j <= i; j++) {
      const int ej = w.psorted[s + j], fj = w.free_of_kf[pb.obs[ej].keyframe];
      const int o = base + i * (i + 1) / 2 + j;
      w.keys[0][o] = (uint32_t)(tri(fi) + fj);
      w.vals[0][o] = i == j ? make_int2(ei, p) : make_int2(ei, ej);
    }
  }
}

__global__ __launch_bounds__(256) void coop_runs_kernel(CoopWs w) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= *w.n_runs) return;
  const uint32_t key = w.run_key[r];
  if (key == kPadKey) {
    w.run_nch[r] = 0;
    return;
  }
  int kh, kl;
  decode_key(key, kh, kl);
  if (kh == kl) w.diag_run[kh] = r;
  w.run_nch[r] = (w.run_cnt[r] + kChunk - 1) / kChunk;
}

// chunk -> run map (chunks of a run are consecutive, in pair order) and the chunk total.
__global__ __launch_bounds__(256) void coop_chunks_kernel(CoopWs w) {
  const int r = blockIdx.x * 256 + threadIdx.x, nr = *w.n_runs;
  if (r >= nr) return;
  const int c0 = w.run_ch0[r], nc = w.run_nch[r];
  for (int k = 0; k < nc; k++) w.chunk_run[c0 + k] = r;
  if (r == nr - 1) *w.n_chunks = c0 + nc;
}

// ---- the cooperative LM kernel ----------------------------------------------------------------
__device__ __forceinline__ double huber_rho(double c2, double d, double& wgt) {
  const double d2 = d * d;
  if (c2 > d2) {
    const double sq = sqrt(c2);
    wgt = d / sq;
    return 2 * sq * d - d2;
  }
  wgt = 1.0;
  return c2;
}

// Linearisation, part 1: a thread per point over its active edges (edge order): chi2 stored per
// edge, Hll and bl summed, the Hpl block of every edge to an optimised keyframe.
__device__ void lin_points(const CoopWs& w, const CoopProblem& pb, const PoseParams& P,
                           const float* isig, const CoopPhase& ph, double& chi, double& maxd) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int GT = gridDim.x * kT;
  for (int p = blockIdx.x * kT + threadIdx.x; p < pb.n_pts; p += GT) {
    const double X[3] = {ptf(w, p, PX), ptf(w, p, PX + 1), ptf(w, p, PX + 2)};
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int nact = 0;
    for (int ge = pb.pstart[p]; ge < pb.pstart[p + 1]; ge++) {
      if (!w.act[ge]) continue;
      nact++;
      const slamgpu_ba_obs o = pb.obs[ge];
      const double* kr = kfr(w, o.keyframe);
      ObsEval v;
      const double c2 = eval_obs(o, P, isig, kr, X, v);
      w.chi2[ge] = c2;
      double wgt = 1.0;
      chi += ph.robust ? huber_rho(c2, v.stereo ? ph.delta_stereo : ph.delta_mono, wgt) : c2;
      double Jl[3][3], Jp[3][6];
      obs_jacobians(v, P, kr, Jl, Jp);
      const double W = wgt * v.info;
      const double or0 = -(v.info * v.e[0]) * wgt, or1 = -(v.info * v.e[1]) * wgt,
                   or2 = -(v.info * v.e[2]) * wgt;
      for (int i = 0; i < 3; i++) {
        H[6 + i] += Jl[0][i] * or0 + Jl[1][i] * or1 + Jl[2][i] * or2;
        for (int j = i; j < 3; j++)
          H[s3(i, j)] += (Jl[0][i] * W) * Jl[0][j] + (Jl[1][i] * W) * Jl[1][j] +
                         (Jl[2][i] * W) * Jl[2][j];
      }
      if (w.free_of_kf[o.keyframe] >= 0) {
        double* hp = w.hpl + (size_t)ge * 18;
        for (int i = 0; i < 6; i++)
          for (int j = 0; j < 3; j++)
            hp[3 * i + j] = (Jp[0][i] * W) * Jl[0][j] + (Jp[1][i] * W) * Jl[1][j] +
                            (Jp[2][i] * W) * Jl[2][j];
      }
    }
    for (int i = 0; i < 6; i++) ptf(w, p, PH + i) = H[i];
    for (int i = 0; i < 3; i++) ptf(w, p, PB + i) = H[6 + i];
    if (nact) maxd = fmax(maxd, fmax(fabs(H[0]), fmax(fabs(H[3]), fabs(H[5]))));
  }
}

// Linearisation, part 2: a wave per (optimised keyframe, chunk of its edge list) -> partial
// Hpp (packed upper) and bp.
__device__ void lin_keyframes(const CoopWs& w, const CoopProblem& pb, const PoseParams& P,
                              const float* isig, const CoopPhase& ph) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kW, tasks = pb.K * w.nch;
  for (int t = blockIdx.x * kW + (threadIdx.x >> 6); t < tasks; t += nw) {
    const int f = t / w.nch, c = t - f * w.nch;
    const int r = w.diag_run[f];
    const int cnt = r >= 0 ? w.run_cnt[r] : 0, off = r >= 0 ? w.run_off[r] : 0;
    const int h0 = (int)((long long)cnt * c / w.nch), h1 = (int)((long long)cnt * (c + 1) / w.nch);
    const double* kr = kfr(w, w.kf_of_free[f]);
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = 0.0;
    for (int h = h0 + lane; h < h1; h += 64) {
      const int2 ep = w.vals[1][off + h];
      const double X[3] = {ptf(w, ep.y, PX), ptf(w, ep.y, PX + 1), ptf(w, ep.y, PX + 2)};
      ObsEval v;
      const double c2 = eval_obs(pb.obs[ep.x], P, isig, kr, X, v);
      double wgt = 1.0;
      if (ph.robust) (void)huber_rho(c2, v.stereo ? ph.delta_stereo : ph.delta_mono, wgt);
      double Jl[3][3], Jp[3][6];
      obs_jacobians(v, P, kr, Jl, Jp);
      const double W = wgt * v.info;
      const double or0 = -(v.info * v.e[0]) * wgt, or1 = -(v.info * v.e[1]) * wgt,
                   or2 = -(v.info * v.e[2]) * wgt;
      int hh = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
        acc[21 + a] += Jp[0][a] * or0 + Jp[1][a] * or1 + Jp[2][a] * or2;
        const double wa0 = Jp[0][a] * W, wa1 = Jp[1][a] * W, wa2 = Jp[2][a] * W;
#pragma unroll
        for (int cc = a; cc < 6; cc++, hh++)
          acc[hh] += wa0 * Jp[0][cc] + wa1 * Jp[1][cc] + wa2 * Jp[2][cc];
      }
    }
    const double s = wave_reduce_scatter32(acc);
    if ((lane & 1) == 0 && (lane >> 1) < 27) st_wt(&w.hpp_part[((size_t)f * w.nch + c) * 27 + (lane >> 1)], s);
    if (last_arriver(&w.kf_arrive[f], w.nch) && lane < 27) {  // Hpp / bp totals, chunk order
      const double* pp = w.hpp_part + (size_t)f * w.nch * 27 + lane;
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = k < w.nch ? ld_wt(pp + (size_t)k * 27) : 0.0;
      double t = v[0];
#pragma unroll
      for (int k = 1; k < 8; k++) t = k < w.nch ? t + v[k] : t;
      w.hpp_tot[(size_t)f * 27 + lane] = t;
    }
  }
}

// An optimised keyframe with active edges in the current phase (a vertex of g2o's system).
__device__ __forceinline__ bool kf_active(const CoopWs& w, int f) {
  const int r = w.diag_run[f];
  return r >= 0 && w.run_cnt[r] > 0;
}

__device__ __forceinline__ void dinv_point(const CoopWs& w, int p, double lambda, double Di[6]) {
  double D[6];
  for (int i = 0; i < 6; i++) D[i] = ptf(w, p, PH + i);
  D[0] += lambda;
  D[3] += lambda;
  D[5] += lambda;
  inverse3_sym(D, Di);
}

// S-block partial sums: a wave per chunk of kChunk pairs of one block (one pair per lane, in
// point order), sum Hpl_eh Dinv_p Hpl_el^T and, on a diagonal block, sum Hpl_e Dinv_p bl_p; the
// point's Dinv = (Hll + lambda I)^-1 formed on the fly. Work-group 0 adds a block's chunk
// partials in chunk order when it builds S (build_S), so every sum has a fixed order.
__device__ void assemble(const CoopWs& w, int K, double lambda, int n_chunks) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kW;
  for (int ch = blockIdx.x * kW + (threadIdx.x >> 6); ch < n_chunks; ch += nw) {
    const int r = w.chunk_run[ch];
    int kh, kl;
    decode_key(w.run_key[r], kh, kl);
    const bool diag = kh == kl;
    const int h = (ch - w.run_ch0[r]) * kChunk + lane;
    // one pair per lane: B = Hpl_eh Dinv_p, then the block rows in two halves (rows 0-2 with
    // the rhs terms, rows 3-5), each reduced across the wave by a 32-value reduce-scatter
    double B[18], hp[18], db[3] = {0, 0, 0};
    const bool valid = h < w.run_cnt[r];
    int eh = 0, el = 0, p = 0;
    if (valid) {
      const int2 ep = w.vals[1][w.run_off[r] + h];
      eh = ep.x;
      el = diag ? ep.x : ep.y;
      p = diag ? ep.y : w.opoint[ep.x];
    }
    {
      double Di[6] = {0, 0, 0, 0, 0, 0};
      if (valid) dinv_point(w, p, lambda, Di);
      const double* hh = w.hpl + (size_t)eh * 18;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const double h0 = valid ? hh[3 * i] : 0.0, h1 = valid ? hh[3 * i + 1] : 0.0,
                     h2 = valid ? hh[3 * i + 2] : 0.0;
        B[3 * i] = h0 * Di[0] + h1 * Di[1] + h2 * Di[2];
        B[3 * i + 1] = h0 * Di[1] + h1 * Di[3] + h2 * Di[4];
        B[3 * i + 2] = h0 * Di[2] + h1 * Di[4] + h2 * Di[5];
      }
      if (diag && valid) {  // Hpl_e Dinv_p bl_p = B bl_p
        const double b0 = ptf(w, p, PB), b1 = ptf(w, p, PB + 1), b2 = ptf(w, p, PB + 2);
        db[0] = b0;
        db[1] = b1;
        db[2] = b2;
      }
      const double* hpl = w.hpl + (size_t)el * 18;
#pragma unroll
      for (int i = 0; i < 18; i++) hp[i] = valid ? hpl[i] : 0.0;
    }
    double* out = w.chunk_part + (size_t)ch * kCP;
    const int id = lane >> 1;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      double acc[32];
#pragma unroll
      for (int i = 0; i < 32; i++) acc[i] = 0.0;
#pragma unroll
      for (int rr = 0; rr < 3; rr++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
          const int ro = 3 * half + rr;
          acc[6 * rr + c] = B[3 * ro] * hp[3 * c] + B[3 * ro + 1] * hp[3 * c + 1] +
                            B[3 * ro + 2] * hp[3 * c + 2];
        }
      if (half == 0 && diag) {
#pragma unroll
        for (int i = 0; i < 6; i++) acc[18 + i] = B[3 * i] * db[0] + B[3 * i + 1] * db[1] + B[3 * i + 2] * db[2];
      }
      const double sv = wave_reduce_scatter32(acc);
      // partial layout: [0, 36) the block row-major, [36, 42) the rhs terms
      if ((lane & 1) == 0) {
        if (id < 18) st_wt(&out[18 * half + id], sv);
        else if (half == 0 && id < 24) st_wt(&out[36 + id - 18], sv);
      }
    }
    // the run's last chunk to finish sums the run's chunk partials in chunk order and writes
    // S(kh, kl) = [kh == kl](Hpp + lambda I) - sum, bs = bp - sum into the dense S / bs
    const int nch = w.run_nch[r];
    if (!last_arriver(&w.run_arrive[r], nch) || lane >= kCP) continue;
    if (!diag && lane >= 36) continue;
    const int rr = lane / 6, c = lane % 6;
    if (lane < 36 && diag && c > rr) continue;
    const double* pp = w.chunk_part + (size_t)w.run_ch0[r] * kCP + lane;
    double sv = 0.0;
    int k = 0;
    for (; k + 4 <= nch; k += 4) {  // four loads in flight per step
      const double a0 = ld_wt(pp + (size_t)k * kCP), a1 = ld_wt(pp + (size_t)(k + 1) * kCP);
      const double a2 = ld_wt(pp + (size_t)(k + 2) * kCP), a3 = ld_wt(pp + (size_t)(k + 3) * kCP);
      sv = (((sv + a0) + a1) + a2) + a3;
    }
    for (; k < nch; k++) sv += ld_wt(pp + (size_t)k * kCP);
    if (lane < 36) {
      double base = 0.0;
      if (diag) base = w.hpp_tot[(size_t)kh * 27 + hidx(c, rr)] + (rr == c ? lambda : 0.0);
      w.S[w.prow[6 * kh + rr] + 6 * kl + c] = base - sv;
    } else {
      w.bs[6 * kh + lane - 36] = w.hpp_tot[(size_t)kh * 27 + 21 + lane - 36] - sv;
    }
  }
}

// Work-group 0: S (packed lower, at Lp) and the reduced rhs from the dense S / bs the runs'
// last chunks wrote (8 loads in flight per thread); the rows of an optimised keyframe left
// without active edges (not in g2o's system) become I with rhs 0.
template <typename PtrT>
__device__ __forceinline__ void build_S(const CoopWs& w, int K, double lambda, PtrT Lp, PtrT rhs) {
  const int tid = threadIdx.x, n = 6 * K, nl = n * (n + 1) / 2;
  for (int q0 = tid; q0 < nl; q0 += 8 * kT) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int q = q0 + u * kT;
      int i = 0, j = 0;
      if (q < nl) {
        i = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while (tri(i + 1) <= q) i++;
        while (tri(i) > q) i--;
        j = q - tri(i);
      }
      v[u] = q < nl && j >= 6 * w.pfirst[i / 6] ? w.S[w.prow[i] + j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (q0 + u * kT < nl) Lp[q0 + u * kT] = v[u];
  }
  for (int i = tid; i < n; i += kT) rhs[i] = w.bs[i];
  __syncthreads();
  for (int t = tid; t < 6 * K; t += kT) {
    const int f = t / 6, i = t - 6 * f;
    if (kf_active(w, f)) continue;
    Lp[sidx(6 * f + i, 6 * f + i)] = 1.0;
    rhs[6 * f + i] = 0.0;
  }
  __syncthreads();
}

// Work-group 0, 6K > kCoopLdsN: the profile S copied to the factor storage (the same layout),
// the reduced rhs, and I / 0 for the rows of optimised keyframes left without active edges.
__device__ void build_S_profile(const CoopWs& w, int K, double* Lp, double* rhs) {
  const int tid = threadIdx.x, n = 6 * K;
  const size_t nnz = (size_t)w.pnnz;
  size_t q = (size_t)tid * 2;
  for (; q + 2 * kT * 3 + 1 < nnz; q += 2 * kT * 4) {  // 4 x 16 B in flight per thread
    double2 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const double2*>(w.S + q + 2 * kT * u);
#pragma unroll
    for (int u = 0; u < 4; u++) *reinterpret_cast<double2*>(Lp + q + 2 * kT * u) = v[u];
  }
  for (; q < nnz; q += 2 * kT) {
    Lp[q] = w.S[q];
    if (q + 1 < nnz) Lp[q + 1] = w.S[q + 1];
  }
  for (int i = tid; i < n; i += kT) rhs[i] = w.bs[i];
  __syncthreads();
  for (int t = tid; t < 6 * K; t += kT) {
    const int f = t / 6;
    if (kf_active(w, f)) continue;
    Lp[w.prow[t] + t] = 1.0;
    rhs[t] = 0.0;
  }
  __syncthreads();
}

__device__ __forceinline__ double rl64(double x, int l) {  // v_readlane of a double
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, (uint64_t)hi << 32 | lo);
}

// LDLT of S (6x6 block columns, right-looking, forward solve fused) by work-group 0. L is packed
// lower at Lp (LDS, or the global scratch for 6K > kCoopLdsN), row i at offset tri(i). Per block
// column J: wave 0 factors the 6x6 diagonal block (lanes 0-5 hold its rows; one reciprocal per
// pivot, multipliers exchanged by v_readlane), a thread per row
// below forms V = A_iJ L_JJ^-T and L_iJ = V D_J^-1 and updates the rhs, then a wave per group of
// 4 trailing rows (lanes over the columns k <= i) subtracts L_iJ V_kJ^T. Then z = D^-1 y and the
// backward solve L^T x = z, a 6x6 block at a time. Sets sh.ok (0 on an exact zero pivot, as
// Eigen's SimplicialLDLT fails); on success writes the solution to w.xp (a failed solve keeps the
// previous step, which g2o applies anyway: optimization_algorithm_levenberg.cpp:107-109).
template <typename PtrT>
__device__ __forceinline__ void factor_solve(CoopShared& sh, const CoopWs& w, int K, PtrT Lp,
                                             PtrT rhs, PtrT dg, PtrT idg, PtrT V) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, n = 6 * K;
  if (tid == 0) sh.ok = 1;
  // diagnostic build: thread 0's split of the factorisation into prof[8..13] (tick(k): prof[8 + k])
  const bool fp = FS_PROF && w.prof && tid == 0;
  PhaseTimer fs(fp ? w.prof + 8 : nullptr);
  if (fp) w.prof[13] += 1.0;
  const DenseRows rows;
  // the diagonal block J by one lane (lane 0 of wave 0): its 21 entries and 6 rhs values in
  // registers, no cross-lane traffic on the pivot chain
  auto diag_factor = [&](int J) {
    if (lane == 0 && !factor_diag_block(Lp, rows, rhs, dg, idg, 6 * J)) sh.ok = 0;
  };
  __syncthreads();
  if (wid == 0) diag_factor(0);
  __syncthreads();
  // Look-ahead: while waves 1.. apply column J's trailing update to the rows below block J + 1,
  // wave 0 updates block J + 1 itself and factors it, so the next column's panel can start right
  // after one barrier (two barriers per block column instead of three, and the diagonal chain
  // off the critical path).
  for (int J = 0; J < K; J++) {
    const int j0 = 6 * J;
    if (!sh.ok) return;
    {  // panel rows below the diagonal block
      double Ljj[15], rdg[6], yj[6];
      load_strict_lower(Lp, rows, j0, Ljj);
#pragma unroll
      for (int c = 0; c < 6; c++) {
        rdg[c] = idg[j0 + c];
        yj[c] = rhs[j0 + c];
      }
      for (int i = j0 + 6 + tid; i < n; i += kT) {
        const int ro = rows.off(i) + j0;
        double a[6], v[6], l[6];
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] = Lp[ro + c];
        double r = rhs[i];
        panel_row(a, Ljj, rdg, yj, v, l, r);
#pragma unroll
        for (int c = 0; c < 6; c++) {
          V[(size_t)i * 6 + c] = v[c];
          Lp[ro + c] = l[c];
        }
        rhs[i] = r;
      }
    }
    fs.tick(0);
    __syncthreads();
    fs.tick(1);
    if (wid == 0) {
      if (J + 1 < K) {  // block J + 1's lower triangle (21 entries, a lane each), then factor it
        if (lane < 21) {
          int r, c;
          tri_rc(lane, r, c);
          const int i = j0 + 6 + r, k = j0 + 6 + c;
          const int ro = tri(i);
          double s = Lp[ro + k];
#pragma unroll
          for (int m = 0; m < 6; m++) s -= Lp[ro + j0 + m] * V[(size_t)k * 6 + m];
          Lp[ro + k] = s;
        }
        wave_sync();
        diag_factor(J + 1);
      }
    } else {
      // trailing update of the rows below block J + 1: a wave per group of 4 rows, lanes over
      // the columns k <= i; the rows' independent chains interleave and V_k is read once per group
      constexpr int kTW = kW - 1;
      for (int i = j0 + 12 + (wid - 1); i < n; i += 4 * kTW) {
        int ro[4], ic[4];
        double l[4][6];
#pragma unroll
        for (int a = 0; a < 4; a++) {  // rows past n alias row n - 1: loads stay unconditional
          ic[a] = min(i + a * kTW, n - 1);
          ro[a] = tri(ic[a]);
#pragma unroll
          for (int c = 0; c < 6; c++) l[a][c] = Lp[ro[a] + j0 + c];
        }
        const int imax = min(i + 3 * kTW, n - 1);
        for (int k = j0 + 6 + lane; k <= imax; k += 64) {
          double v[6];
#pragma unroll
          for (int c = 0; c < 6; c++) v[c] = V[(size_t)k * 6 + c];
          double s[4];
#pragma unroll
          for (int a = 0; a < 4; a++) s[a] = Lp[ro[a] + min(k, ic[a])];
#pragma unroll
          for (int a = 0; a < 4; a++) {
#pragma unroll
            for (int c = 0; c < 6; c++) s[a] -= l[a][c] * v[c];
            if (k <= i + a * kTW && i + a * kTW < n) Lp[ro[a] + k] = s[a];
          }
        }
      }
    }
    fs.tick(2);
    if (tid == 0)  // heartbeat for the work-groups waiting at the next grid barrier
      __hip_atomic_fetch_add(&w.ctl[CTL_BEAT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    fs.tick(3);
  }
  if (wid == 0) {  // z = D^-1 y; L^T x = z from the last 6x6 block up
    for (int i = lane; i < n; i += 64) rhs[i] /= dg[i];
    for (int J = K - 1; J >= 0; J--) {
      const int j0 = 6 * J;
      wave_sync();
      // within the block, by lane 0 in registers (x_c final when c is reached, descending);
      // the 6 values then go to every lane by v_readlane
      double x[6] = {0, 0, 0, 0, 0, 0};
      if (lane == 0) {
        double Lb[15];
        load_strict_lower(Lp, rows, j0, Lb);
#pragma unroll
        for (int r = 0; r < 6; r++) x[r] = rhs[j0 + r];
        block_back6(Lb, x);
#pragma unroll
        for (int r = 0; r < 6; r++) rhs[j0 + r] = x[r];
      }
#pragma unroll
      for (int c = 0; c < 6; c++) x[c] = rl64(x[c], 0);
      for (int i = lane; i < j0; i += 64) {  // earlier rows: z_i -= sum_c L(j0 + c, i) x_c
        double sx = rhs[i];
#pragma unroll
        for (int c = 0; c < 6; c++) sx -= Lp[tri(j0 + c) + i] * x[c];
        rhs[i] = sx;
      }
    }
    wave_sync();
    for (int i = lane; i < n; i += 64) w.xp[i] = rhs[i];
  }
  __syncthreads();
  fs.tick(4);
}

// z = D^-1 y; L^T x = z from the last 6x6 block up: lane 0 solves the block (x to LDS), then the
// whole work-group applies it to the block's envelope (wave 0 alone: 10 ms per solve at 1500
// keyframes, profiles/r3n_gba_factor_split.log); the solution to w.xp.
__device__ void profile_back_solve(CoopShared& sh, const CoopWs& w, int K, double* Lp,
                                   double* rhs, const double* dg) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int tid = threadIdx.x, n = 6 * K;
  const int64_t* prow = w.prow;
  const int32_t* pfirst = w.pfirst;
  const ProfileRows rows{prow};
  double* const xs = sh.rhs;  // 6 doubles (sh.rhs is unused on the profile path)
  // z in LDS when it fits (the unused dense factor storage): the block steps then hand off
  // through LDS only, and the next block's L values are loaded while this block is solved
  if (n <= (int)(sizeof(sh.S) / sizeof(double))) {
    double* const z = sh.S;
    for (int i = tid; i < n; i += kT) z[i] = rhs[i] / dg[i];
    double Lb[15], Lr[6];  // thread 0: block J's strict lower L; every thread: its first row
    auto fetch = [&](int J) {
      const int j0 = 6 * J;
      if (tid == 0) load_strict_lower(Lp, rows, j0, Lb);
      const int i = 6 * pfirst[J] + tid;
      if (i < j0)
#pragma unroll
        for (int c = 0; c < 6; c++) Lr[c] = Lp[prow[j0 + c] + i];
    };
    if (K > 0) fetch(K - 1);
    __syncthreads();
    for (int J = K - 1; J >= 0; J--) {
      const int j0 = 6 * J;
      double Lbc[15], Lrc[6];
#pragma unroll
      for (int q = 0; q < 15; q++) Lbc[q] = Lb[q];
#pragma unroll
      for (int c = 0; c < 6; c++) Lrc[c] = Lr[c];
      if (J > 0) fetch(J - 1);  // in flight under this block's solve and update
      if (tid == 0) {
        double x[6];
#pragma unroll
        for (int r = 0; r < 6; r++) x[r] = z[j0 + r];
        block_back6(Lbc, x);
#pragma unroll
        for (int r = 0; r < 6; r++) {
          z[j0 + r] = x[r];
          xs[r] = x[r];
        }
      }
      lds_sync();
      double x[6];
#pragma unroll
      for (int c = 0; c < 6; c++) x[c] = xs[c];
      const int i0 = 6 * pfirst[J];
      if (i0 + tid < j0) {
        double sx = z[i0 + tid];
#pragma unroll
        for (int c = 0; c < 6; c++) sx -= Lrc[c] * x[c];
        z[i0 + tid] = sx;
      }
      if (i0 + kT < j0) {
        int64_t rb[6];
#pragma unroll
        for (int c = 0; c < 6; c++) rb[c] = prow[j0 + c];
        for (int i = i0 + kT + tid; i < j0; i += kT) {
          double sx = z[i];
#pragma unroll
          for (int c = 0; c < 6; c++) sx -= Lp[rb[c] + i] * x[c];
          z[i] = sx;
        }
      }
      lds_sync();
    }
    for (int i = tid; i < n; i += kT) w.xp[i] = z[i];
    __syncthreads();
    return;
  }
  for (int i = tid; i < n; i += kT) rhs[i] /= dg[i];
  __syncthreads();
  for (int J = K - 1; J >= 0; J--) {
    const int j0 = 6 * J;
    if (tid == 0) {
      double Lb[15], x[6];
      load_strict_lower(Lp, rows, j0, Lb);
#pragma unroll
      for (int r = 0; r < 6; r++) x[r] = rhs[j0 + r];
      block_back6(Lb, x);
#pragma unroll
      for (int r = 0; r < 6; r++) {
        rhs[j0 + r] = x[r];
        xs[r] = x[r];
      }
    }
    __syncthreads();
    double x[6];
    int64_t rb[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      x[c] = xs[c];
      rb[c] = prow[j0 + c];
    }
    for (int i = 6 * pfirst[J] + tid; i < j0; i += kT) {
      double sx = rhs[i];
#pragma unroll
      for (int c = 0; c < 6; c++) sx -= Lp[rb[c] + i] * x[c];
      rhs[i] = sx;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += kT) w.xp[i] = rhs[i];
  __syncthreads();
}

// The same LDLT for 6K > kCoopLdsN on the block-profile storage (w.prow / w.pfirst): row i holds
// columns 6 pfirst[i / 6] .. i, and every fill-in stays inside that envelope, so block column J
// only touches the active block rows A_J = {I > J : pfirst[I] <= J} -- a band of a few dozen
// keyframes along the trajectory, plus the rows loop closures reach back from. A_J is kept in
// LDS (unordered: every element is updated by one lane per column, so the results do not depend
// on the order) and A_{J+1} is collected while column J's trailing update runs. Otherwise as
// factor_solve: thread-per-row panel with the forward solve fused, wave 0 updating and factoring
// the next diagonal block while the other waves apply the trailing update (A_J x A_J below it),
// two work-group barriers per block column; then D^-1 and the blocked backward solve by wave 0.
__device__ void factor_solve_profile(CoopShared& sh, const CoopWs& w, int K, double* Lp,
                                     double* rhs, double* dg, double* idg, double* V) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, n = 6 * K;
  const int64_t* prow = w.prow;
  const int32_t* pfirst = w.pfirst;
  // A_J lists in the (unused here) LDS factor storage: two buffers of K entries + 2 counters
  int* const lists = reinterpret_cast<int*>(sh.S);
  int* const cnt = lists + 2 * K;
  if (tid == 0) {
    sh.ok = 1;
    cnt[0] = 0;
  }
  // diagnostic build: thread 0's split of the factorisation into prof[8..13], active block rows
  // per column: sum in prof[14], max in prof[15]
  const bool fp = FS_PROF && w.prof && tid == 0;
  PhaseTimer fs(fp ? w.prof + 8 : nullptr);
  if (fp) w.prof[13] += 1.0;
  const ProfileRows rows{prow};
  auto diag_factor = [&](int J) {  // by lane 0 of wave 0, as in factor_solve
    if (lane == 0 && !factor_diag_block(Lp, rows, rhs, dg, idg, 6 * J)) sh.ok = 0;
  };
  __syncthreads();
  for (int I = 1 + tid; I < K; I += kT)  // A_0
    if (pfirst[I] <= 0) lists[atomicAdd(&cnt[0], 1)] = I;
  if (wid == 0) diag_factor(0);
  __syncthreads();
  for (int J = 0; J < K; J++) {
    const int j0 = 6 * J;
    if (!sh.ok) return;
    const int* act = lists + (J & 1) * K;
    int* nxt = lists + ((J + 1) & 1) * K;
    const int na = cnt[J & 1], nr = 6 * na;
    if (fp) {
      w.prof[14] += (double)na;
      w.prof[15] = fmax(w.prof[15], (double)na);
    }
    {  // panel rows of the active blocks (forward solve fused)
      double Ljj[15], rdg[6], yj[6];
      load_strict_lower(Lp, rows, j0, Ljj);
#pragma unroll
      for (int c = 0; c < 6; c++) {
        rdg[c] = idg[j0 + c];
        yj[c] = rhs[j0 + c];
      }
      for (int t = tid; t < nr; t += kT) {
        const int i = 6 * act[t / 6] + t % 6;
        const int64_t ro = rows.off(i) + j0;
        double a[6], v[6], l[6];
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] = Lp[ro + c];
        double r = rhs[i];
        panel_row(a, Ljj, rdg, yj, v, l, r);
#pragma unroll
        for (int c = 0; c < 6; c++) {
          V[(size_t)i * 6 + c] = v[c];
          Lp[ro + c] = l[c];
        }
        rhs[i] = r;
      }
    }
    fs.tick(0);
    if (tid == 0) cnt[(J + 1) & 1] = 0;
    __syncthreads();
    fs.tick(1);
    const bool next_active = J + 1 < K && pfirst[J + 1] <= J;
    if (wid == 0) {
      if (J + 1 < K) {  // block J + 1: its update by column J (when it is active), then its LDLT
        if (next_active && lane < 21) {
          int r, c;
          tri_rc(lane, r, c);
          const int i = j0 + 6 + r, k = j0 + 6 + c;
          const int64_t ro = prow[i];
          double sv = Lp[ro + k];
#pragma unroll
          for (int m = 0; m < 6; m++) sv -= Lp[ro + j0 + m] * V[(size_t)k * 6 + m];
          Lp[ro + k] = sv;
        }
        wave_sync();
        diag_factor(J + 1);
      }
    } else {
      // trailing update A(i, k) -= L(i, J) V(k)^T over the active rows i outside block J + 1 and
      // the active columns k <= i: a wave per group of 4 rows, lanes over the columns
      constexpr int kTW = kW - 1;
      for (int t0 = wid - 1; t0 < nr; t0 += 4 * kTW) {
        int ic[4];
        int64_t ro[4];
        double l[4][6];
        bool live[4];
#pragma unroll
        for (int a = 0; a < 4; a++) {
          const int t = t0 + a * kTW;
          const int tt = t < nr ? t : nr - 1;
          ic[a] = 6 * act[tt / 6] + tt % 6;
          live[a] = t < nr && ic[a] >= j0 + 12;  // block J + 1 is wave 0's
          ro[a] = prow[ic[a]];
#pragma unroll
          for (int c = 0; c < 6; c++) l[a][c] = Lp[ro[a] + j0 + c];
        }
        if (!(live[0] || live[1] || live[2] || live[3])) continue;
        for (int m = lane; m < nr; m += 64) {
          const int k = 6 * act[m / 6] + m % 6;
          double v[6];
#pragma unroll
          for (int c = 0; c < 6; c++) v[c] = V[(size_t)k * 6 + c];
#pragma unroll
          for (int a = 0; a < 4; a++) {
            if (!live[a] || k > ic[a]) continue;
            double sv = Lp[ro[a] + k];
#pragma unroll
            for (int c = 0; c < 6; c++) sv -= l[a][c] * v[c];
            Lp[ro[a] + k] = sv;
          }
        }
      }
    }
    fs.tick(2);
    for (int I = J + 2 + tid; I < K; I += kT)  // A_{J+1}
      if (pfirst[I] <= J + 1) nxt[atomicAdd(&cnt[(J + 1) & 1], 1)] = I;
    if (tid == 0)  // heartbeat for the work-groups waiting at the next grid barrier
      __hip_atomic_fetch_add(&w.ctl[CTL_BEAT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    fs.tick(3);
  }
  profile_back_solve(sh, w, K, Lp, rhs, dg);
  fs.tick(4);
}

// ---- the profile LDLT over the whole grid (6K > kCoopLdsN) ---------------------------------
// Block row I of S (its rows of L and rhs) belongs to work-group I % G for the whole
// factorisation: its panel rows and trailing updates are computed there, so L never crosses
// work-groups and needs no L2 write-back. Per block column J one hand-off does, write-through
// (st_wt / ld_wt, as the reduction partials): every work-group forms the panel rows of its own
// active blocks (V = A_iJ L_JJ^-T, L_iJ = V D_J^-1, rhs updated), publishes V and raises its own
// panel flag (one 128-byte line per work-group: no contended counter) to J + 1; then it stages
// every active V row in LDS and updates its own rows. The diagonal blocks need no hand-off: every
// work-group keeps a replica of each active block's diagonal block and rhs slice in LDS (slots
// from a free ring, filled from S when the block enters the active set) and applies column J's
// update to all of them from the staged V rows -- the same operands and operation order as the
// owner's trailing update and panel, so the replicas equal the owner's values bit for bit -- and
// then factors block J + 1 itself (one lane); the owner also writes that factor to the profile
// for the backward solve. Every element sees the same operations in the same order as in
// factor_solve_profile -- both call ba_ldlt.h's diag_ldlt and panel_row -- so the two give
// identical results (tests/test_gba_gpu.py compares them bit for bit). V is double-buffered by
// column parity: a work-group runs at most one column ahead of the slowest (it cannot pass column
// J + 1's panel flags before every work-group has finished column J). Active block rows per
// column <= prof_na_cap(K) (their V rows and replicas fit the LDS; host-computed na_max, else
// work-group 0 factors alone).

// Wave 0: spin until every work-group's flag (pflag[32 g], one 128-byte line each) reaches target.
// False once the grid has given up (CTL_ERR), or when no flag moved for ~2^22 sleeps (raised here).
__device__ bool wait_flags(const CoopWs& w, const int32_t* pflag, int32_t target) {
  const int lane = threadIdx.x & 63, G = gridDim.x;
  uint32_t spins = 0, polls = 0;
  int seen = -1;
  for (;;) {
    int sum = 0, cnt = 0;  // this lane's flags: their sum (progress) and how many reached target
    bool all = true;
    for (int g0 = 0; g0 < G; g0 += 64) {
      const int g = g0 + lane;
      const int32_t v = g < G ? __hip_atomic_load(const_cast<int32_t*>(pflag) + 32 * g,
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : target;
      all = all && __all(v >= target);
      if (g < G) {
        sum += v;
        cnt += v >= target ? 1 : 0;
      }
    }
    if (all) return true;
    // progress = any flag of the grid moved: the sum over the whole wave, not one lane's part
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      sum += __shfl_xor(sum, m);
      cnt += __shfl_xor(cnt, m);
    }
    if (sum != seen) {
      seen = sum;
      spins = 0;
    }
    if (polls < 256) __builtin_amdgcn_s_sleep(1);
    else __builtin_amdgcn_s_sleep(8);
    polls++;
    if ((++spins & 255u) == 0 && ctl_load(w, CTL_ERR)) return false;
    if (spins > (1u << 22)) {
      if (lane == 0) {  // what the host reports: the work-groups whose flag had got there
        __hip_atomic_store(&w.ctl[CTL_ARRIVED], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.ctl[CTL_GRID], G, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.ctl[CTL_ERR], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return false;
    }
  }
}

// factor_profile_grid's LDS in sh.S: ints -- two A_J lists [2][K], 8 counters, the own blocks'
// list positions [K], pfirst [K], each block's replica slot [K], the free-slot ring [cap] -- then
// doubles (16-byte aligned): block J's factor (32), the active V rows [36 cap], the own L_iJ rows
// [36 cap], the replicas [27 cap] (diagonal block lower 21 + rhs 6).
constexpr int kRep = 27;
__device__ __forceinline__ int prof_ints_dw(int K, int cap) {
  return (4 * (5 * K + 8 + cap + 6 * cap) + 15) / 16 * 2;  // + own rows' prow (low words)
}
__device__ __forceinline__ int prof_na_cap(int K) {
  const int total = (int)(sizeof(CoopShared::S) / 8);
  int cap = (total - 32 - (5 * K + 8) / 2 - 2) * 2 / (2 * (72 + kRep) + 7);
  while (cap > 0 && prof_ints_dw(K, cap) + 32 + (72 + kRep) * cap > total) cap--;
  return cap > 0 ? cap : 0;
}

// Every work-group. Returns false (work-group-uniform, the same in every work-group) on a zero
// pivot or when the grid gave up; the panel flags must be 0 on entry (zeroed before the grid
// barrier that precedes it).
__device__ bool factor_profile_grid(CoopShared& sh, const CoopWs& w, int K, double* Lp,
                                    double* rhs, double* dg, double* idg, double* Vg0,
                                    double* Vg1, int32_t* pflag) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  const int tid = threadIdx.x, wid = tid >> 6;
  const int G = gridDim.x, wg = blockIdx.x;
  const int64_t* prow = w.prow;
  const int32_t* pfirst = w.pfirst;
  const ProfileRows rows{prow};
  const int cap = prof_na_cap(K);
  int* const lists = reinterpret_cast<int*>(sh.S);
  int* const cnt = lists + 2 * K;  // [0], [1]: list sizes; [2]: own count; [3]: flags seen;
                                   // [4]: free-ring pops; [5]: free-ring pushes; [6]: entering
  int* const own = cnt + 8;        // [K] (the blocks entering A_{J+1} after the own ones)
  int* const spf = own + K;        // [K] pfirst
  int* const slot_of = spf + K;    // [K]
  int* const ring = slot_of + K;   // [cap]
  int* const sro = ring + cap;     // [6 cap] prow of the own active rows (32-bit: pnnz < 2^31)
  double* const pd = sh.S + prof_ints_dw(K, cap);  // L_JJ 15, D_J^-1 6, y_J 6, ok
  double* const sV = pd + 32;                      // [36 cap] active V rows, list order
  double* const sL = sV + 36 * (size_t)cap;        // [36 cap] own L_iJ rows
  double* const rep = sL + 36 * (size_t)cap;       // [kRep cap] replicas
  double* const nx = sh.V;  // block J + 1's initial diagonal block when it was never active
  // block I's diagonal block and rhs slice before any update: from S and the reduced rhs (never
  // written during the factorisation -- the profile copy is: its owner may already be a column
  // ahead), with build_S_profile's I / 0 for a keyframe left without active edges
  // entry e of that image (e < 21: lower (r, c) of the diagonal block; 21 + r: rhs row r), one
  // lane per entry (a whole block per lane would hold 27 loads in flight in this register-bound
  // kernel)
  auto initial = [&](int I, int e) -> double {
    const int i0 = 6 * I;
    const bool act_kf = kf_active(w, I);
    if (e >= 21) return act_kf ? w.bs[i0 + e - 21] : 0.0;
    int r, c;
    tri_rc(e, r, c);
    return (!act_kf && c == r) ? 1.0 : w.S[prow[i0 + r] + i0 + c];
  };
  // a block entering the active set takes a free slot (filled by initial())
  auto take_slot = [&](int I) { slot_of[I] = ring[atomicAdd(&cnt[4], 1) % cap]; };
  // thread 0: factor block J from its (updated) diagonal block and rhs slice at src (LDS: 21 + 6)
  // into pd; its owner also writes the factor to the profile. One call site (register pressure:
  // this kernel holds every phase of the solver)
  auto factor_block = [&](int J, const double* src) {
    double A[21], y[6], rdg[6];
#pragma unroll
    for (int e = 0; e < 21; e++) A[e] = src[e];
#pragma unroll
    for (int r = 0; r < 6; r++) y[r] = src[21 + r];
    const bool good = diag_ldlt(A, y, rdg);
    double Ljj[15];
    load_strict_lower(A, DenseRows{}, 0, Ljj);  // the packed block is a dense factor of 6 rows
#pragma unroll
    for (int q = 0; q < 15; q++) pd[q] = Ljj[q];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      pd[15 + c] = rdg[c];
      pd[21 + c] = y[c];
    }
    pd[27] = good ? 1.0 : 0.0;
    if (J % G == wg) {
      // factor_diag_block's store, written out: as a shared helper it cost the 1500-keyframe
      // global BA 0.6 % (the same instructions here, another register allocation elsewhere)
      const int j0 = 6 * J;
#pragma unroll
      for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int k = 0; k < r; k++) Lp[prow[j0 + r] + j0 + k] = A[r * (r + 1) / 2 + k];
        dg[j0 + r] = A[r * (r + 3) / 2];
        idg[j0 + r] = rdg[r];
        rhs[j0 + r] = y[r];
      }
    }
  };
  if (tid == 0) {
    cnt[0] = 0;
    cnt[4] = 0;
    cnt[5] = cap;
  }
  for (int I = tid; I < K; I += kT) spf[I] = pfirst[I];
  for (int q = tid; q < cap; q += kT) ring[q] = q;
  __syncthreads();
  for (int I = 1 + tid; I < K; I += kT)  // A_0
    if (spf[I] <= 0) {
      lists[atomicAdd(&cnt[0], 1)] = I;
      take_slot(I);
    }
  __syncthreads();
  for (int q = tid; q < kRep * cnt[0]; q += kT) {
    const int I = lists[q / kRep], e = q % kRep;
    rep[(size_t)slot_of[I] * kRep + e] = initial(I, e);
  }
  if (tid < kRep && K > 0) nx[tid] = initial(0, tid);  // block 0: no update before column 0
  __syncthreads();
  bool ok = true;
  // diagnostic build: thread 0 of work-group 0 splits each column into prof[8..12], summed here
  // and written once at the end
  const bool gp = FS_PROF && w.prof && wg == 0 && tid == 0;
  double gacc[5] = {0, 0, 0, 0, 0};
  PhaseTimer gt(gp ? gacc : nullptr);
  for (int J = 0; J < K; J++) {
    const int j0 = 6 * J;
    const int* act = lists + (J & 1) * K;
    int* nxt = lists + ((J + 1) & 1) * K;
    const int na = cnt[J & 1], nr = 6 * na;
    double* const Vp = (J & 1) ? Vg1 : Vg0;
    if (tid == 0) {
      // block J: its replica (it was active in A_{J-1}), or its initial values staged in nx;
      // then its slot goes back to the ring
      const bool was_active = J > 0 && spf[J] < J;
      factor_block(J, was_active ? rep + (size_t)slot_of[J] * kRep : nx);
      if (was_active) {
        ring[cnt[5] % cap] = slot_of[J];
        cnt[5]++;
      }
      cnt[2] = 0;
      cnt[6] = 0;
      cnt[(J + 1) & 1] = 0;  // A_{J+1}'s size (A_{J-1} is no longer read)
    }
    __syncthreads();
    if (pd[27] == 0.0) {  // zero pivot: every work-group stops at this column
      ok = false;
      break;
    }
    for (int t = tid; t < na; t += kT)  // own active blocks (any order)
      if (act[t] % G == wg) own[atomicAdd(&cnt[2], 1)] = t;
    __syncthreads();
    const int nro = 6 * cnt[2];
    gt.tick(0);
    // ---- panel rows of the own active blocks (forward solve fused); V published, L_iJ kept
    {
      double Ljj[15], rdg[6], yj[6];
#pragma unroll
      for (int q = 0; q < 15; q++) Ljj[q] = pd[q];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        rdg[c] = pd[15 + c];
        yj[c] = pd[21 + c];
      }
      for (int t = tid; t < nro; t += kT) {
        const int i = 6 * act[own[t / 6]] + t % 6;
        const int64_t pr = rows.off(i);
        sro[t] = (int)pr;
        const int64_t ro = pr + j0;
        double a[6], v[6], l[6];
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] = Lp[ro + c];
        double r = rhs[i];
        panel_row(a, Ljj, rdg, yj, v, l, r);
#pragma unroll
        for (int c = 0; c < 6; c++) {
          st_wt(Vp + (size_t)i * 6 + c, v[c]);
          Lp[ro + c] = l[c];
          sL[t * 6 + c] = l[c];
        }
        rhs[i] = r;
      }
    }
    vm_drain();  // this thread's V hand-off and L / rhs stores have landed
    __syncthreads();
    if (tid == 0)  // this work-group's panel of column J is out (its own 128-byte line)
      __hip_atomic_store(&pflag[32 * wg], J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // while the other panels arrive: the blocks entering A_{J+1} take slots and their initial
    // diagonal blocks (own[] past the own blocks lists them), and block J + 1's when it was never
    // active
    if (wid > 0) {  // each wave fills the blocks its lanes found, one entry per lane
      const int lane = tid & 63;
      for (int I0 = J + 2 + (wid - 1) * 64; I0 < K; I0 += kT - 64) {
        const int I = I0 + lane;
        uint64_t found = __ballot(I < K && spf[I] == J + 1);
        while (found) {
          const int b = __ffsll((long long)found) - 1;
          found &= found - 1;
          const int Ib = __builtin_amdgcn_readlane(I, b);
          if (lane == b) {
            own[cnt[2] + atomicAdd(&cnt[6], 1)] = Ib;
            take_slot(Ib);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          if (lane < kRep) rep[(size_t)slot_of[Ib] * kRep + lane] = initial(Ib, lane);
        }
      }
      if (wid == 1 && J + 1 < K && spf[J + 1] > J && lane < kRep) nx[lane] = initial(J + 1, lane);
    }
    gt.tick(1);
    // ---- every panel of column J: the active V rows to LDS
    if (wid == 0) {
      const bool got = wait_flags(w, pflag, J + 1);
      if (tid == 0) cnt[3] = got ? 1 : 0;
    }
    __syncthreads();
    if (!cnt[3]) {
      ok = false;
      break;
    }
    gt.tick(2);
    for (int q = tid; q < 36 * na; q += kT) {
      const int t = q / 6, c = q - 6 * t;
      sV[q] = ld_wt(Vp + (size_t)(6 * act[t / 6] + t % 6) * 6 + c);
    }
    __syncthreads();
    // ---- trailing update of the own rows, and column J's update of every replica
    for (int p = tid; p < nro * nr; p += kT) {
      const int a = p / nr, m = p - a * nr;
      const int i = 6 * act[own[a / 6]] + a % 6;
      const int k = 6 * act[m / 6] + m % 6;
      if (k > i) continue;
      const int64_t ro = sro[a];
      double sv = Lp[ro + k];
#pragma unroll
      for (int c = 0; c < 6; c++) sv -= sL[a * 6 + c] * sV[m * 6 + c];
      Lp[ro + k] = sv;
    }
    {
      double rdg[6], yj[6];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        rdg[c] = pd[15 + c];
        yj[c] = pd[21 + c];
      }
      for (int q = tid; q < kRep * na; q += kT) {
        const int t = q / kRep, e = q - kRep * t;
        double* R = rep + (size_t)slot_of[act[t]] * kRep;
        if (e < 21) {  // diagonal entry (r, c): -= L(row r) V(row c)^T
          int r, c;
          tri_rc(e, r, c);
          const double* vr = sV + (6 * t + r) * 6;
          const double* vc = sV + (6 * t + c) * 6;
          double sv = R[e];
#pragma unroll
          for (int m = 0; m < 6; m++) sv -= (vr[m] * rdg[m]) * vc[m];
          R[e] = sv;
        } else {  // rhs row r: -= L(row r) y_J
          const double* vr = sV + (6 * t + e - 21) * 6;
          double sv = R[e];
#pragma unroll
          for (int m = 0; m < 6; m++) {
            const double l = vr[m] * rdg[m];
            sv -= l * yj[m];
          }
          R[e] = sv;
        }
      }
    }
    __syncthreads();
    gt.tick(3);
    // ---- A_{J+1} = A_J without block J + 1, and the entering blocks (block J + 1 is factored at
    // the start of the next column)
    if (J + 1 < K) {
      const int no = cnt[2], ne = cnt[6];
      for (int t = tid; t < na + ne; t += kT) {
        const int I = t < na ? act[t] : own[no + t - na];
        if (I != J + 1) nxt[atomicAdd(&cnt[(J + 1) & 1], 1)] = I;
      }
    }
    __syncthreads();
    gt.tick(4);
  }
  if (gp) {
    for (int k = 0; k < 5; k++) w.prof[8 + k] += gacc[k];
    w.prof[13] -= 1.0;  // negative: the grid factorisation's split
  }
  vm_drain();
  __syncthreads();
  return ok;
}

// optimizer.cpp:632-665 between the two optimize() calls: chi2 > threshold or depth <= 0 ->
// level 1 (edge-parallel over the grid).
__device__ void mark_outliers(const CoopWs& w, const CoopProblem& pb, const PoseParams& P,
                              const float* isig) {
  for (int ge = blockIdx.x * kT + threadIdx.x; ge < pb.n_obs; ge += gridDim.x * kT) {
    const int p = w.opoint[ge];
    const double X[3] = {ptf(w, p, PX), ptf(w, p, PX + 1), ptf(w, p, PX + 2)};
    const slamgpu_ba_obs o = pb.obs[ge];
    ObsEval v;
    eval_obs(o, P, isig, kfr(w, o.keyframe), X, v);
    if (w.chi2[ge] > (o.ur >= 0 ? 7.815 : 5.991) || !(v.z > 0.0)) w.act[ge] = 0;
  }
}

// The next phase's S-block pair lists: each run's pairs filtered to the active edges in place,
// in order (a wave per run, ballot prefix counts), so the block structure needs no new sort.
__device__ void compact_runs(const CoopWs& w, int n_runs, int n) {
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * kW + (threadIdx.x >> 6); r < n_runs; r += gridDim.x * kW) {
    const uint32_t key = w.run_key[r];
    if (key == kPadKey) continue;
    int kh, kl;
    decode_key(key, kh, kl);
    const bool diag = kh == kl;
    const int off = w.run_off[r], cnt = w.run_cnt[r];
    int kept = 0;
    for (int h0 = 0; h0 < cnt; h0 += 64) {
      const int h = h0 + lane;
      int2 ep = make_int2(0, 0);
      bool keep = false;
      if (h < cnt) {
        ep = w.vals[1][off + h];
        keep = w.act[ep.x] && (diag || w.act[ep.y]);
      }
      const uint64_t bal = __ballot(keep);
      if (keep) w.vals[1][off + kept + lanes_below(bal)] = ep;  // in place: never past h
      kept += __popcll(bal);
    }
    if (lane == 0) {
      w.run_cnt[r] = kept;
      w.run_nch[r] = (kept + kChunk - 1) / kChunk;
    }
    if (kept == 0 && cnt > 0 && lane < 36 && (!diag || lane % 6 <= lane / 6))
      w.S[w.prow[6 * kh + lane / 6] + 6 * kl + lane % 6] = 0.0;  // the block left the system
  }
}

// Work-group 0: chunk offsets (exclusive scan of run_nch over the runs: a contiguous segment per
// thread, then the segment sums in order) and the chunk -> run map; returns the chunk count.
__device__ int rebuild_chunks(CoopShared& sh, const CoopWs& w, int n_runs) {
  const int tid = threadIdx.x, seg = (n_runs + kT - 1) / kT;
  const int r0 = min(tid * seg, n_runs), r1 = min(r0 + seg, n_runs);
  int sum = 0;
  for (int r = r0; r < r1; r++) sum += w.run_nch[r];
  sh.iscan[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int t = 0; t < kT; t++) {
      const int v = sh.iscan[t];
      sh.iscan[t] = acc;
      acc += v;
    }
    sh.itot = acc;
  }
  __syncthreads();
  int c = sh.iscan[tid];
  for (int r = r0; r < r1; r++) {
    const int nc = w.run_nch[r];
    w.run_ch0[r] = c;
    for (int k = 0; k < nc; k++) w.chunk_run[c + k] = r;
    c += nc;
  }
  const int total = sh.itot;
  __syncthreads();
  return total;
}

__device__ void restore_estimates(const CoopWs& w, const CoopProblem& pb) {
  const int GT = gridDim.x * kT;
  for (int p = blockIdx.x * kT + threadIdx.x; p < pb.n_pts; p += GT)
    for (int i = 0; i < 3; i++) ptf(w, p, PX + i) = ptf(w, p, PXB + i);
  for (int f = blockIdx.x * kT + threadIdx.x; f < pb.K; f += GT) {
    if (!kf_active(w, f)) continue;
    double* kr = kfr(w, w.kf_of_free[f]);
    SE3 T;
    T.r.x = kr[KBQ];
    T.r.y = kr[KBQ + 1];
    T.r.z = kr[KBQ + 2];
    T.r.w = kr[KBQ + 3];
    for (int i = 0; i < 3; i++) T.t[i] = kr[KBT + i];
    store_T(kr, T);
  }
}

__global__ __launch_bounds__(kT) void ba_coop_kernel(PoseParams P, CoopProblem pb, CoopWs w,
                                                     CoopSchedule sch, const int32_t* stop_flag) {
#pragma clang fp contract(fast)  // tolerance-compared FP64 path
  __shared__ CoopShared sh;
  const int tid = threadIdx.x, wg = blockIdx.x, GT = gridDim.x * kT;
  if (ctl_load(w, CTL_STOPPED) || ctl_load(w, CTL_ERR)) return;  // written by earlier kernels
  if (tid < SLAMGPU_MAX_LEVELS) sh.isig[tid] = P.inv_sigma2[tid];
  const int K = pb.K, n = 6 * K;
  const int n_runs = *w.n_runs;
  int n_chunks = *w.n_chunks;
  // factor storage: LDS (explicit address space, so every access is a ds_ op) or the global
  // scratch for systems past kCoopLdsN
  typedef __attribute__((address_space(3))) double* LdsPtr;
  const bool in_lds = n <= kCoopLdsN;
  double* const Gp = w.fac;
  double* const Gv = Gp + (size_t)w.pnnz;
  double* const Gd = Gv + (size_t)6 * n;
  double* const Gr = Gd + n;
  double* const Gi = Gr + n;
  double* const Gv2 = Gi + n;            // the grid factorisation's second V buffer
  // the grid factorisation's panel flags, 128 bytes apart (after 64 spare doubles)
  int32_t* const Gflag = reinterpret_cast<int32_t*>(Gv2 + (size_t)6 * n + 64);
  // the profile LDLT over the whole grid when the active V rows fit the LDS (host: na_max)
  const bool grid_factor = !in_lds && w.mwg && gridDim.x > 1 && w.na_max <= prof_na_cap(K);
  // optional per-phase wall clock of work-group 0 (phase_clock: 100 MHz)
  if (tid < 8) sh.pacc[tid] = 0.0;
  if (tid == 0) sh.pt0 = phase_clock();
  auto tick = [&](int slot) {  // thread 0 of work-group 0 only: no registers held across phases
    if (w.prof && wg == 0 && tid == 0) {
      const uint64_t t = phase_clock();
      sh.pacc[slot] += 0.01 * (double)(t - sh.pt0);
      sh.pt0 = t;
    }
  };
  int lm_total = 0;
  bool stopped = false;
  for (int phs = 0; phs < sch.n_phases; phs++) {
  const CoopPhase ph = sch.ph[phs];
  if (phs > 0) {
    grid_sync(w, stop_flag, true);  // optimizer.cpp:625-627: do_more
    if (ctl_load(w, CTL_POLL)) {
      stopped = true;
      break;
    }
    if (sch.outlier_pass) {  // level-1 outliers, then the next phase's block pair lists
      mark_outliers(w, pb, P, sh.isig);
      grid_sync(w, stop_flag, false);
      compact_runs(w, n_runs, n);
      grid_sync(w, stop_flag, false);
      if (wg == 0) {
        const int nc = rebuild_chunks(sh, w, n_runs);
        if (tid == 0) *w.n_chunks = nc;
      }
      grid_sync(w, stop_flag, false);
      n_chunks = *w.n_chunks;
    }
  }
  grid_sync(w, stop_flag, true);  // the first iteration's terminate() poll
  tick(7);
  bool stop = ctl_load(w, CTL_POLL) != 0;
  double lambda = 0.0;
  int ni = 2, nbad = 0;
  for (int it = 0; it < ph.iterations; it++) {
    if (stop) {  // optimize(): i < iterations && !terminate()
      stopped = true;
      break;
    }
    // ---- linearise: computeActiveErrors + activeRobustChi2 + buildSystem ----
    double chi = 0.0, maxd = 0.0;
    lin_points(w, pb, P, sh.isig, ph, chi, maxd);
    lin_keyframes(w, pb, P, sh.isig, ph);
    wg_part(sh, w, chi, 0, false);
    wg_part(sh, w, maxd, 1, true);
    tick(0);
    grid_sync(w, stop_flag, false);
    tick(1);
    grid_totals(sh, w, 0, 1, false);
    double currentChi = sh.tot[0];
    const double iniChi = currentChi;
    if (it == 0) {  // computeLambdaInit over the active vertices
      double m = 0.0;
      for (int t = tid; t < 6 * K; t += kT) {
        const int f = t / 6, i = t - 6 * f;
        const int dgi[6] = {0, 6, 11, 15, 18, 20};
        if (kf_active(w, f)) m = fmax(m, fabs(w.hpp_tot[(size_t)f * 27 + dgi[i]]));
      }
      m = wave_max(m);
      if ((tid & 63) == 0) sh.red[tid >> 6] = m;
      grid_totals(sh, w, 1, 1, true);  // (its barriers also publish sh.red)
      m = sh.tot[0];
      for (int k = 0; k < kW; k++) m = fmax(m, sh.red[k]);
      __syncthreads();
      lambda = 1e-5 * m;
      ni = 2;
      nbad = 0;
    }
    double rho = 0.0;
    int qmax = 0;
    bool rejected = false;
    do {
      // ---- S, reduced rhs (and the pop of a rejected trial's estimates) ----
      assemble(w, K, lambda, n_chunks);
      if (rejected) restore_estimates(w, pb);
      tick(2);
      grid_sync(w, stop_flag, false);
      tick(1);
      // ---- work-group 0: factor + solve, keyframe update (backup first) ----
      if (grid_factor) {  // the profile LDLT over every work-group, then work-group 0 solves
        if (wg == 0) {
          build_S_profile(w, K, Gp, Gr);
          for (int g = tid; g < (int)gridDim.x; g += kT)
            __hip_atomic_store(&Gflag[32 * g], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        tick(5);
        grid_sync(w, stop_flag, false);
        const bool fok = factor_profile_grid(sh, w, K, Gp, Gr, Gd, Gi, Gv, Gv2, Gflag);
        grid_sync(w, stop_flag, false);
        if (wg == 0) {
          if (tid == 0) sh.ok = fok ? 1 : 0;
          if (fok) profile_back_solve(sh, w, K, Gp, Gr, Gd);
          __syncthreads();
        }
      }
      if (wg == 0) {
        if (in_lds) {
          build_S(w, K, lambda, (LdsPtr)sh.S, (LdsPtr)sh.rhs);
          tick(5);
          factor_solve(sh, w, K, (LdsPtr)sh.S, (LdsPtr)sh.rhs, (LdsPtr)sh.dg, (LdsPtr)sh.idg,
                       (LdsPtr)sh.V);
        } else if (!grid_factor) {
          build_S_profile(w, K, Gp, Gr);
          tick(5);
          factor_solve_profile(sh, w, K, Gp, Gr, Gd, Gi, Gv);
        }
        tick(6);
        double sc = 0.0;
        for (int f = tid; f < K; f += kT) {
          if (!kf_active(w, f)) continue;
          double* kr = kfr(w, w.kf_of_free[f]);
          double x[6];
          for (int i = 0; i < 6; i++) {
            x[i] = w.xp[6 * f + i];
            sc += x[i] * (lambda * x[i] + w.hpp_tot[(size_t)f * 27 + 21 + i]);
          }
          SE3 T;
          load_T(kr, T);
          for (int i = 0; i < 4; i++) kr[KBQ + i] = kr[KQ + i];
          for (int i = 0; i < 3; i++) kr[KBT + i] = kr[KT + i];
          store_T(kr, se3::se3_left_update(x, T));
        }
        wg_part(sh, w, sc, 4, false);  // work-group 0's slot 4: the keyframe share of `scale`
        if (tid == 0) w.ctl[CTL_OK] = sh.ok;
      }
      tick(3);
      grid_sync(w, stop_flag, false);
      tick(1);
      const bool ok = ctl_load(w, CTL_OK) != 0;
      // ---- points: back-substitution, update (backup first), errors of their edges ----
      double scale = 0.0, temp = 0.0;
      for (int p = wg * kT + tid; p < pb.n_pts; p += GT) {
        double c[3] = {ptf(w, p, PB), ptf(w, p, PB + 1), ptf(w, p, PB + 2)};
        int nact = 0;
        const int s = pb.pstart[p], e1 = pb.pstart[p + 1];
        for (int ge = s; ge < e1; ge++) {
          if (!w.act[ge]) continue;
          nact++;
          const int f = w.free_of_kf[pb.obs[ge].keyframe];
          if (!ok || f < 0) continue;
          const double* hp = w.hpl + (size_t)ge * 18;
          for (int i = 0; i < 6; i++) {
            const double x = w.xp[6 * f + i];
            c[0] -= hp[3 * i] * x;
            c[1] -= hp[3 * i + 1] * x;
            c[2] -= hp[3 * i + 2] * x;
          }
        }
        if (ok) {
          double Di[6];
          dinv_point(w, p, lambda, Di);
          ptf(w, p, PXL) = Di[0] * c[0] + Di[1] * c[1] + Di[2] * c[2];
          ptf(w, p, PXL + 1) = Di[1] * c[0] + Di[3] * c[1] + Di[4] * c[2];
          ptf(w, p, PXL + 2) = Di[2] * c[0] + Di[4] * c[1] + Di[5] * c[2];
        }
        double X[3];
        for (int i = 0; i < 3; i++) {
          X[i] = ptf(w, p, PX + i);
          ptf(w, p, PXB + i) = X[i];
        }
        if (nact) {  // oplus on the active vertices only
          for (int i = 0; i < 3; i++) {
            const double x = ptf(w, p, PXL + i);
            X[i] += x;
            ptf(w, p, PX + i) = X[i];
            scale += x * (lambda * x + ptf(w, p, PB + i));
          }
        }
        for (int ge = s; ge < e1; ge++) {
          if (!w.act[ge]) continue;
          const slamgpu_ba_obs o = pb.obs[ge];
          ObsEval v;
          const double c2 = eval_obs(o, P, sh.isig, kfr(w, o.keyframe), X, v);
          w.chi2[ge] = c2;
          double wgt;
          temp += ph.robust ? huber_rho(c2, v.stereo ? ph.delta_stereo : ph.delta_mono, wgt) : c2;
        }
      }
      wg_part(sh, w, temp, 2, false);
      wg_part(sh, w, scale, 3, false);
      tick(4);
      grid_sync(w, stop_flag, true);  // carries the trial loop's terminate() poll
      tick(1);
      stop = ctl_load(w, CTL_POLL) != 0;
      grid_totals(sh, w, 2, 2, false);
      const double tempChi = ok ? sh.tot[0] : DBL_MAX;
      double sc = sh.tot[1] + w.part[4];
      sc += 1e-3;
      rho = (currentChi - tempChi) / sc;
      if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - pow(2 * rho - 1, 3.0);
        alpha = fmin(alpha, 2. / 3.);
        lambda *= fmax(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
        rejected = false;
      } else {
        lambda *= ni;
        ni *= 2;
        rejected = true;  // pop: restored with the next assembly, or below
      }
      qmax++;
    } while (rho < 0 && qmax < 10 && !stop);
    if (rejected) {
      restore_estimates(w, pb);
      grid_sync(w, stop_flag, false);
    }
    lm_total++;
    if (qmax == 10 || rho == 0) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nbad++;
    else nbad = 0;
    if (nbad >= 3) break;
  }
  if (stopped) break;
  }  // phases
  if (w.prof && wg == 0 && tid == 0)
    for (int i = 0; i < 8; i++) w.prof[i] += sh.pacc[i];
  if (wg == 0 && tid == 0) {
    w.ctl[CTL_LM] += lm_total;
    if (stopped) w.ctl[CTL_STOPPED] = 1;
  }
}

// ---- after the schedule ----------------------------------------------------------------------
// optimizer.cpp:672-700 erase list (LocalBA), :702-716 / :170-206 write-back.
__global__ __launch_bounds__(256) void coop_finish_kernel(PoseParams P, CoopProblem pb, CoopWs w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (pb.ctl_out && i < 8) pb.ctl_out[i] = w.ctl[i];  // next to the outputs: one readback
  if (w.ctl[CTL_ERR]) return;
  if (pb.erase && i < pb.n_obs) {
    float isig[SLAMGPU_MAX_LEVELS];
    for (int l = 0; l < P.nlevels; l++) isig[l] = P.inv_sigma2[l];
    const int p = w.opoint[i];
    const double X[3] = {ptf(w, p, PX), ptf(w, p, PX + 1), ptf(w, p, PX + 2)};
    const slamgpu_ba_obs o = pb.obs[i];
    ObsEval v;
    eval_obs(o, P, isig, kfr(w, o.keyframe), X, v);
    pb.erase[i] = (w.chi2[i] > (o.ur >= 0 ? 7.815 : 5.991) || !(v.z > 0.0)) ? 1 : 0;
  }
  if (i < pb.n_pts)
    for (int c = 0; c < 3; c++) pb.points[(size_t)i * 3 + c] = (float)ptf(w, i, PX + c);
  if (i < pb.n_kf && pb.kf_mode[i] != SLAMGPU_KF_FIXED) {
    const double* kr = kfr(w, i);
    float* T = pb.kf_Tcw + (size_t)i * 16;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T[4 * r + c] = (float)kr[KR + 3 * r + c];
      T[4 * r + 3] = (float)kr[KT + r];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
  }
}

size_t cub_bytes_needed(int pairs_cap, int end_bit) {
  size_t a = 0, b = 0, c = 0, d = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (int2*)nullptr, (int2*)nullptr, pairs_cap, 0, end_bit);
  (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (int32_t*)nullptr, (int32_t*)nullptr, pairs_cap);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, (int32_t*)nullptr, (int32_t*)nullptr,
                                         pairs_cap);
  return std::max(std::max(a, b), std::max(c, d));
}

int key_bits(int K) {
  const long long maxkey = (long long)K * (K + 1) / 2;  // pad key (2^bits - 1) > every real key
  int b = 1;
  while (((1ll << b) - 1) <= maxkey) b++;
  return b;
}

}  // namespace

CoopWs coop_layout(void* base, int n_kf, int n_pts, int n_obs, int K, int pairs_cap, int G,
                   int64_t pnnz, size_t* bytes) {
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  size_t off = 0;
  char* b = static_cast<char*>(base);
  auto take = [&](size_t n) {
    char* p = b ? b + off : nullptr;
    off += al(n);
    return p;
  };
  const int n = 6 * K;
  const int pc = pairs_cap > 0 ? pairs_cap : 1;
  CoopWs w{};
  w.chi2 = reinterpret_cast<double*>(take(8 * (size_t)n_obs));
  w.hpl = reinterpret_cast<double*>(take(8 * 18 * (size_t)n_obs));
  w.act = reinterpret_cast<uint8_t*>(take((size_t)n_obs));
  w.opoint = reinterpret_cast<int32_t*>(take(4 * (size_t)n_obs));
  w.psorted = reinterpret_cast<int32_t*>(take(4 * (size_t)n_obs));
  w.pt = reinterpret_cast<double*>(take(8 * 27 * (size_t)n_pts));
  w.n_pt = n_pts;
  w.kf = reinterpret_cast<double*>(take(8 * 64 * (size_t)n_kf));
  w.free_of_kf = reinterpret_cast<int32_t*>(take(4 * (size_t)n_kf));
  w.kf_of_free = reinterpret_cast<int32_t*>(take(4 * (size_t)K + 4));
  w.npairs = reinterpret_cast<int32_t*>(take(4 * ((size_t)n_pts + 1)));
  w.poff = reinterpret_cast<int32_t*>(take(4 * ((size_t)n_pts + 1)));
  for (int i = 0; i < 2; i++) {
    w.keys[i] = reinterpret_cast<uint32_t*>(take(4 * (size_t)pc));
    w.vals[i] = reinterpret_cast<int2*>(take(8 * (size_t)pc));
  }
  w.run_key = reinterpret_cast<uint32_t*>(take(4 * (size_t)pc));
  w.run_cnt = reinterpret_cast<int32_t*>(take(4 * (size_t)pc));
  w.run_off = reinterpret_cast<int32_t*>(take(4 * (size_t)pc));
  w.n_runs = reinterpret_cast<int32_t*>(take(4));
  w.diag_run = reinterpret_cast<int32_t*>(take(4 * (size_t)K + 4));
  w.run_nch = reinterpret_cast<int32_t*>(take(4 * (size_t)pc));
  w.run_ch0 = reinterpret_cast<int32_t*>(take(4 * (size_t)pc));
  w.n_chunks = reinterpret_cast<int32_t*>(take(4));
  const size_t chunk_cap = std::min<size_t>((size_t)pc, (size_t)K * (K + 1) / 2 + pc / kChunk + 1);
  w.chunk_run = reinterpret_cast<int32_t*>(take(4 * chunk_cap));
  w.chunk_part = reinterpret_cast<double*>(take(8 * kCP * chunk_cap));
  w.nch = std::max(1, std::min(8, (G * kW) / std::max(K, 1)));
  w.hpp_part = reinterpret_cast<double*>(take(8 * 27 * (size_t)K * w.nch + 8));
  w.hpp_tot = reinterpret_cast<double*>(take(8 * 27 * (size_t)K + 8));
  w.kf_arrive = reinterpret_cast<int32_t*>(take(4 * (size_t)K + 4));
  w.run_arrive = reinterpret_cast<int32_t*>(take(4 * (size_t)pc));
  w.S = reinterpret_cast<double*>(take(8 * (size_t)pnnz + 8));
  w.pnnz = pnnz;
  w.bs = reinterpret_cast<double*>(take(8 * (size_t)n + 8));
  w.fac = reinterpret_cast<double*>(
      take(n > kCoopLdsN ? 8 * ((size_t)pnnz + 15 * (size_t)n + 64) + 128 * kMaxGrid : 8));
  w.xp = reinterpret_cast<double*>(take(8 * (size_t)n + 8));
  w.part = reinterpret_cast<double*>(take(8 * 8 * (size_t)(G + 1)));
  w.bar = reinterpret_cast<uint32_t*>(take(64));
  w.ctl = reinterpret_cast<int32_t*>(take(64));
  w.prof = reinterpret_cast<double*>(take(128));
  w.pairs_cap = pc;
  w.end_bit = key_bits(K);
  w.cub_bytes = cub_bytes_needed(pc, w.end_bit);
  w.cub_tmp = take(w.cub_bytes + 256);
  if (bytes) *bytes = off + 256;
  return w;
}

const void* coop_kernel_ptr() { return reinterpret_cast<const void*>(&ba_coop_kernel); }

hipError_t launch_coop_ba(const PoseParams& P, const CoopProblem& pb, const CoopWs& w,
                          const CoopPhase* phases, int n_phases, bool outlier_pass,
                          const int32_t* d_stop, int G, hipStream_t st) {
  auto blocks = [](int n) { return dim3((unsigned)std::max(1, (n + 255) / 256)); };
  const int nmax = std::max(std::max(pb.n_kf, pb.n_pts), std::max(pb.n_obs, 6 * pb.K + 8));
  SLAMGPU_LAUNCH("ba_coop_setup", st, coop_setup_kernel, blocks(nmax), dim3(256), 0, st, pb, w);
  {
    // structure of the first phase's active edge set: pairs per point -> offsets -> keys ->
    // sorted runs -> chunks (the second phase filters these lists in the kernel)
    SLAMGPU_LAUNCH("ba_coop_sort", st, coop_sort_kernel, blocks(pb.n_pts + 1), dim3(256), 0, st,
                   pb, w);
    size_t tb = w.cub_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, tb, w.npairs, w.poff,
                                                    pb.n_pts + 1, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.keys[0], 0xff, 4 * (size_t)w.pairs_cap, st)) != hipSuccess) return e;
    SLAMGPU_LAUNCH("ba_coop_emit", st, coop_emit_kernel, blocks(pb.n_pts), dim3(256), 0, st, pb, w);
    tb = w.cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(w.cub_tmp, tb, w.keys[0], w.keys[1], w.vals[0],
                                           w.vals[1], w.pairs_cap, 0, w.end_bit, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.run_cnt, 0, 4 * (size_t)w.pairs_cap, st)) != hipSuccess) return e;
    tb = w.cub_bytes;
    e = hipcub::DeviceRunLengthEncode::Encode(w.cub_tmp, tb, w.keys[1], w.run_key, w.run_cnt,
                                              w.n_runs, w.pairs_cap, st);
    if (e != hipSuccess) return e;
    tb = w.cub_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, tb, w.run_cnt, w.run_off, w.pairs_cap, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.diag_run, 0xff, 4 * (size_t)pb.K + 4, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.S, 0, 8 * (size_t)w.pnnz + 8, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.run_arrive, 0, 4 * (size_t)w.pairs_cap, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.kf_arrive, 0, 4 * (size_t)pb.K + 4, st)) != hipSuccess) return e;
    SLAMGPU_LAUNCH("ba_coop_runs", st, coop_runs_kernel, blocks(w.pairs_cap), dim3(256), 0, st, w);
    tb = w.cub_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, tb, w.run_nch, w.run_ch0, w.pairs_cap, st);
    if (e != hipSuccess) return e;
    SLAMGPU_LAUNCH("ba_coop_chunks", st, coop_chunks_kernel, blocks(w.pairs_cap), dim3(256), 0, st,
                   w);
    // the whole LM schedule in one launch. Its G work-groups (16 by default, at most the number
    // the device holds resident at once, optimizer_runtime.cpp coop_grid) are all dispatched
    // while the first spin at a grid barrier: they only wait for CUs that non-spinning kernels
    // free, and a barrier that still does not fill raises CTL_ERR (bounded spin) rather than
    // hanging. A plain launch: the runtime's cooperative launch costs ~50 us per call, and under
    // rocprofv3 a process that had used it crashed at exit (r2s/r2t; cause not established, so
    // the cooperative launch is not offered).
    CoopSchedule sch{};
    sch.n_phases = n_phases;
    sch.outlier_pass = outlier_pass ? 1 : 0;
    for (int ph = 0; ph < n_phases && ph < 2; ph++) sch.ph[ph] = phases[ph];
    PoseParams Pc = P;
    CoopProblem pbc = pb;
    CoopWs wc = w;
    const int32_t* stop = d_stop;
    void* args[] = {&Pc, &pbc, &wc, &sch, &stop};
    if (g_timer) g_timer->begin("ba_coop", st);
    e = hipLaunchKernel(reinterpret_cast<const void*>(&ba_coop_kernel), dim3(G), dim3(kT), args,
                        0, st);
    if (g_timer) g_timer->end("ba_coop", st);
    if (e != hipSuccess) return e;
  }
  SLAMGPU_LAUNCH("ba_coop_finish", st, coop_finish_kernel, blocks(nmax), dim3(256), 0, st, P, pb, w);
  return hipGetLastError();
}

}  // namespace slamgpu
