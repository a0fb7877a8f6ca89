// host_stage_check.cpp -- the staging layouts of every synchronous wrapper and the shared
// FeatureVector validator, driven on the CPU (built with -fsanitize=address,undefined by
// slam_framework_amd.build.build_host_stage_check; run by tests/test_host_stage.py).
//
// The wrappers call the same layout_* / place_* functions, so what holds here holds for the
// offsets they hand to the device: every slot 256-aligned, slots disjoint (zero-byte ones
// included) and in take order, every slot inside size().
#include <cstdio>
#include <cstring>
#include <string>

#include "stage_layout.h"

using namespace slamgpu;

static int g_failed = 0, g_layouts = 0;

#define EXPECT(cond, ...)                   \
  do {                                      \
    if (!(cond)) {                          \
      g_failed++;                           \
      std::printf("FAIL %s: ", #cond);      \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
    }                                       \
  } while (0)

struct Walk {
  StageLayout L;
  std::vector<std::pair<size_t, size_t>> log;
  Walk() { L.log = &log; }
  // n_slots: how many takes the layout is made of
  void check(const char* what, size_t n_slots) {
    g_layouts++;
    EXPECT(log.size() == n_slots, "%s: %zu slots, expected %zu", what, log.size(), n_slots);
    size_t end = 0;
    for (size_t i = 0; i < log.size(); i++) {
      const size_t at = log[i].first, bytes = log[i].second;
      EXPECT(at % 256 == 0, "%s: slot %zu at %zu", what, i, at);
      EXPECT(at >= end, "%s: slot %zu at %zu overlaps the previous one ending at %zu", what, i, at, end);
      EXPECT(i == 0 || at > log[i - 1].first, "%s: slot %zu shares offset %zu", what, i, at);
      EXPECT(at + bytes <= L.size(), "%s: slot %zu ends at %zu > size %zu", what, i, at + bytes, L.size());
      end = at + bytes;
    }
  }
  // the recorded offset of take number i, to tie a layout's named fields to the log
  size_t at(size_t i) const { return i < log.size() ? log[i].first : kNoSlot; }
};

static void check_kf_place(const char* what, const Walk& w, size_t first, const KfPlace& p,
                           KfParts parts, int n_nodes) {
  EXPECT(p.kps == w.at(first) && p.desc == w.at(first + 1), "%s: kps / desc", what);
  EXPECT((p.u_right != kNoSlot) == (parts >= kKfStereo), "%s: u_right", what);
  EXPECT((p.has_mp != kNoSlot) == (parts >= kKfFeatureVector), "%s: has_mp", what);
  const bool fv = parts >= kKfFeatureVector && n_nodes > 0;
  EXPECT((p.nodes != kNoSlot) == fv && (p.node_start != kNoSlot) == fv &&
             (p.node_feats != kNoSlot) == fv, "%s: FeatureVector slots", what);
}

static size_t kf_slots(KfParts parts, int n_nodes) {
  return 2 + (parts >= kKfStereo) + (parts >= kKfFeatureVector) * (1 + (n_nodes > 0 ? 3 : 0));
}

static void walk_layouts() {
  const int ns[] = {0, 1, 255, 256, 257};
  const int pts[] = {0, 1, 64, 65};
  char what[128];
  for (int n : ns) {
    {  // PoseOptimization (48-byte edges, Tcw) and OptimizeSim3 (matches, S12)
      Walk w;
      const SolveLayout s = layout_solve(w.L, n, sizeof(slamgpu_pose_edge), 64);
      std::snprintf(what, sizeof(what), "pose n=%d", n);
      w.check(what, 5);
      EXPECT(s.start == 0 && s.items == w.at(1) && s.state == w.at(2) && s.flags == w.at(3) &&
                 s.result == w.at(4), "%s: fields", what);
      Walk w2;
      layout_solve(w2.L, n, sizeof(slamgpu_sim3_match), 64);
      std::snprintf(what, sizeof(what), "sim3 n=%d", n);
      w2.check(what, 5);
    }
    {  // bow transform (cap = max(n, 1)), distinctive, gray
      Walk w;
      const BowTransformLayout t = layout_bow_transform(w.L, n > 0 ? n : 1);
      std::snprintf(what, sizeof(what), "bow_transform n=%d", n);
      w.check(what, 11);
      EXPECT(t.desc == 0 && t.feat_node == w.at(10), "%s: fields", what);
      for (int total : {0, 1, 3 * n}) {
        Walk d;
        const DistinctiveLayout dl = layout_distinctive(d.L, n, total);
        std::snprintf(what, sizeof(what), "distinctive n_points=%d total=%d", n, total);
        d.check(what, 4);
        EXPECT(dl.out == d.at(3), "%s: fields", what);
      }
      Walk g;
      const GrayLayout gl = layout_gray(g.L, (size_t)n * 3 * 5, (size_t)n * 5);
      std::snprintf(what, sizeof(what), "gray cols=%d", n);
      g.check(what, 2);
      EXPECT(gl.src == 0 && gl.dst == g.at(1), "%s: fields", what);
    }
    const int nodes[] = {0, 1, n};
    for (int nn : nodes) {
      if (nn > n) continue;
      {  // SearchByBoW: both sets of this shape
        Walk w;
        const BowSearchLayout s = layout_search_by_bow(w.L, n, nn, n, nn);
        std::snprintf(what, sizeof(what), "search_by_bow n=%d n_nodes=%d", n, nn);
        w.check(what, 17);
        EXPECT(s.a.desc == 0 && s.b.desc == w.at(7) && s.views == w.at(14) && s.nmatches == w.at(16),
               "%s: fields", what);
      }
      {  // SearchForTriangulation: kf2 of the same shape, every feature listed once
        Walk w;
        const int n2[2] = {n, n}, nn2[2] = {nn, nn}, nf2[2] = {nn > 0 ? n : 0, nn > 0 ? n : 0};
        const TriLayout t = layout_search_tri(w.L, n2, nn2, nf2);
        std::snprintf(what, sizeof(what), "search_tri n=%d n_nodes=%d", n, nn);
        const size_t k = kf_slots(kKfFeatureVector, nn);
        w.check(what, 2 * k + 4);
        check_kf_place(what, w, 0, t.kf[0], kKfFeatureVector, nn);
        check_kf_place(what, w, k, t.kf[1], kKfFeatureVector, nn);
        EXPECT(t.kfs == w.at(2 * k) && t.nmatches == w.at(2 * k + 3), "%s: fields", what);
      }
    }
    for (int np : pts) {
      for (KfParts parts : {kKfStereo, kKfLoop}) {  // Fuse and the Sim3 Fuse
        Walk w;
        const FuseLayout f = layout_fuse(w.L, parts, n, np);
        std::snprintf(what, sizeof(what), "fuse parts=%d n=%d n_pts=%d", (int)parts, n, np);
        const size_t k = kf_slots(parts, 0);
        w.check(what, k + 4);
        check_kf_place(what, w, 0, f.kf, parts, 0);
        EXPECT(f.kfs == w.at(k) && f.best_dist == w.at(k + 3), "%s: fields", what);
      }
      {
        Walk w;
        const SbpSim3Layout s = layout_sbp_sim3(w.L, n, np, (size_t)np * 12);
        std::snprintf(what, sizeof(what), "sbp_sim3 n=%d n_pts=%d", n, np);
        w.check(what, 2 + 8);
        check_kf_place(what, w, 0, s.kf, kKfLoop, 0);
        EXPECT(s.kfs == w.at(2) && s.scratch == w.at(9), "%s: fields", what);
      }
    }
    for (int n2 : ns) {
      Walk w;
      const SearchSim3Layout s = layout_search_sim3(w.L, n, n2);
      std::snprintf(what, sizeof(what), "search_sim3 n1=%d n2=%d", n, n2);
      w.check(what, 4 + 9);
      check_kf_place(what, w, 0, s.kf[0], kKfLoop, 0);
      check_kf_place(what, w, 2, s.kf[1], kKfLoop, 0);
      EXPECT(s.kfs == w.at(4) && s.nfound == w.at(12), "%s: fields", what);
      const size_t stride = (size_t)(n > n2 ? n : n2);
      EXPECT(s.already2 - s.already1 > stride && s.vn_match2 - s.vn_match1 > 4 * stride,
             "%s: strided arrays", what);
    }
  }
  // the frame matchers' query buffer: the three SearchByProjection calls (64- and 80-byte queries,
  // a 72-byte pose record or none) and SearchForInitialization
  for (int nq : {0, 1, 3, 4097}) {
    for (size_t query_bytes : {sizeof(slamgpu_f2f_query), sizeof(slamgpu_mps_query)})
      for (size_t extra : {(size_t)0, (size_t)72}) {
        Walk w;
        const FrameSearchLayout s = layout_frame_search(w.L, nq, query_bytes, extra);
        std::snprintf(what, sizeof(what), "frame_search nq=%d query_bytes=%zu extra_bytes=%zu", nq,
                      query_bytes, extra);
        w.check(what, 2);
        EXPECT(s.queries == 0 && s.extra == w.at(1), "%s: fields", what);
        EXPECT(s.extra >= (size_t)nq * query_bytes && s.extra + extra <= w.L.size(),
               "%s: pose record at %zu", what, s.extra);
      }
    Walk w;
    const InitSearchLayout s = layout_init_search(w.L, nq);
    std::snprintf(what, sizeof(what), "init_search n1=%d", nq);
    w.check(what, 4);
    EXPECT(s.queries == 0 && s.params == w.at(1) && s.prev_matched == w.at(2) &&
               s.matches12 == w.at(3), "%s: fields", what);
    EXPECT(s.matches12 - s.prev_matched >= 8 * (size_t)nq &&
               s.matches12 + 4 * (size_t)nq <= w.L.size(), "%s: per-query arrays", what);
  }
  // local / global BA: the I/O block is one contiguous region [0, io), the workspace starts at io
  const int small[] = {0, 1, 7};
  for (int n_kf : small)
    for (int K : small)
      for (int n_points : small)
        for (int n_obs : small) {
          if (K > n_kf) continue;
          Walk w;
          const CoopLayout c = layout_coop(w.L, n_kf, K, n_points, n_obs, 1000);
          std::snprintf(what, sizeof(what), "coop n_kf=%d K=%d n_points=%d n_obs=%d", n_kf, K,
                        n_points, n_obs);
          w.check(what, 12);
          const size_t f[] = {c.T, c.mode, c.pts, c.ps, c.obs, c.free_of, c.kf_of, c.pfirst,
                              c.prow, c.er, c.ctl, c.ws};
          for (size_t i = 0; i < 12; i++) EXPECT(f[i] == w.at(i), "%s: field %zu", what, i);
          EXPECT(c.T == 0, "%s: block starts at %zu", what, c.T);
          for (size_t i = 0; i + 1 < 12; i++) {
            // no gap a copy of [0, er) or [0, io) would not cover: the next slot starts at the
            // 256-byte boundary after this one's last byte + 1
            const size_t next = (w.log[i].first + w.log[i].second + 256) / 256 * 256;
            EXPECT(w.log[i + 1].first == next, "%s: gap after field %zu", what, i);
          }
          EXPECT(c.ctl + 8 * sizeof(int32_t) <= c.io, "%s: control words end after io", what);
          EXPECT(c.er + (size_t)n_obs <= c.ctl, "%s: erase flags reach the control words", what);
          EXPECT(c.ws == c.io, "%s: workspace at %zu, io %zu", what, c.ws, c.io);
          EXPECT(c.ws + 1000 <= w.L.size(), "%s: workspace past size", what);
        }
}

// The message texts are those check_set (BoW) and check_kf (kfmatch) have always reported.
static const char* kBowFmt = "%s: feature index %u >= n";
static const char* kKfFmt = "%s: feature index >= n";

static void expect_fv(const char* name, const char* fmt, int n, int n_nodes, const uint32_t* nodes,
                      const int32_t* start, const uint32_t* feats, int rc, const char* msg) {
  ErrorSlot err;
  err.msg = "untouched";
  const int got = check_feature_vector(err, name, n, n_nodes, nodes, start, feats, fmt);
  EXPECT(got == rc, "validator returned %d, expected %d (%s)", got, rc, msg);
  EXPECT(err.msg == msg, "validator said '%s', expected '%s'", err.c_str(), msg);
}

static void walk_validator() {
  const int n = 4;
  const uint32_t nodes[2] = {3, 9}, feats[4] = {0, 2, 1, 3};
  const int32_t start[3] = {0, 2, 4};
  expect_fv("a", kBowFmt, n, 2, nodes, start, feats, 0, "untouched");
  expect_fv("kf1", kKfFmt, n, 2, nodes, start, feats, 0, "untouched");
  const int32_t start_nz[3] = {1, 2, 4};
  expect_fv("a", kBowFmt, n, 2, nodes, start_nz, feats, SLAMGPU_EINVAL, "a: node_start[0] != 0");
  expect_fv("kf1", kKfFmt, n, 2, nodes, start_nz, feats, SLAMGPU_EINVAL, "kf1: node_start[0] != 0");
  const int32_t start_desc[3] = {0, 3, 2};
  expect_fv("b", kBowFmt, n, 2, nodes, start_desc, feats, SLAMGPU_EINVAL,
            "b: node_start not ascending within [0, n]");
  expect_fv("kf2", kKfFmt, n, 2, nodes, start_desc, feats, SLAMGPU_EINVAL,
            "kf2: node_start not ascending within [0, n]");
  const int32_t start_past[3] = {0, 2, 5};
  expect_fv("b", kBowFmt, n, 2, nodes, start_past, feats, SLAMGPU_EINVAL,
            "b: node_start not ascending within [0, n]");
  const uint32_t nodes_eq[2] = {3, 3};
  expect_fv("a", kBowFmt, n, 2, nodes_eq, start, feats, SLAMGPU_EINVAL,
            "a: nodes not strictly ascending");
  expect_fv("kf1", kKfFmt, n, 2, nodes_eq, start, feats, SLAMGPU_EINVAL,
            "kf1: nodes not strictly ascending");
  const uint32_t feats_n[4] = {0, 2, 4, 3};
  expect_fv("a", kBowFmt, n, 2, nodes, start, feats_n, SLAMGPU_EINVAL, "a: feature index 4 >= n");
  expect_fv("kf1", kKfFmt, n, 2, nodes, start, feats_n, SLAMGPU_EINVAL, "kf1: feature index >= n");
  expect_fv("a", kBowFmt, n, 2, nullptr, start, feats, SLAMGPU_EINVAL, "a: NULL FeatureVector");
}

int main() {
  walk_layouts();
  walk_validator();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok: %d layouts\n", g_layouts);
  return 0;
}
