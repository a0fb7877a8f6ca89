// kfdb_adapter_check.cpp -- LoopDetectorCore and gather_detect_loop_candidates of
// include/slamgpu_adapters.hpp driven from C++ on the CPU (tests/test_kfdb_ref.py compares the
// output with a Python statement of LoopCloser::DetectLoop's group logic).
// Input file: "threshold n_connected n_queries", then n_connected lines "id n ids..."
// (GetConnectedKeyFrames of a candidate), then n_queries lines "kf n candidates...".
// Output: JSON on stdout.
#include <cstdio>
#include <fstream>
#include <map>

#include "slamgpu_adapters.hpp"

using namespace slamgpu_adapter;

static void print_ids(const std::vector<int32_t>& v) {
  std::printf("[");
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%d", i ? ", " : "", v[i]);
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int threshold = 0, n_connected = 0, n_queries = 0;
  in >> threshold >> n_connected >> n_queries;
  std::map<int32_t, std::vector<int32_t>> connected;
  for (int i = 0; i < n_connected; i++) {
    int id = 0, n = 0;
    in >> id >> n;
    std::vector<int32_t>& v = connected[id];
    v.resize(n);
    for (int& x : v) in >> x;
  }
  LoopDetectorCore core(threshold);
  std::printf("{\"queries\": [");
  for (int q = 0; q < n_queries; q++) {
    int kf = 0, n = 0;
    in >> kf >> n;
    std::vector<int32_t> cand(n);
    for (int& x : cand) in >> x;
    if (!in) return 3;
    if (core.too_soon(kf)) return 4;  // the sequence's keyframe ids are past the early exit
    const LoopDetectorCore::Result r = core.update(
        cand.data(), n, [&](int32_t id, std::vector<int32_t>& out) {
          const std::vector<int32_t>& c = connected[id];
          out.insert(out.end(), c.begin(), c.end());
        });
    if (!r.add_current_keyframe || r.detected != !r.consistent_enough.empty()) return 5;
    std::vector<LoopDetectorCore::Group> groups = core.groups();
    std::sort(groups.begin(), groups.end());
    std::printf("%s{\"enough\": ", q ? ", " : "");
    print_ids(r.consistent_enough);
    std::printf(", \"groups\": [");
    for (size_t g = 0; g < groups.size(); g++) {
      std::printf("%s[", g ? ", " : "");
      print_ids(groups[g].first);
      std::printf(", %d]", groups[g].second);
    }
    std::printf("]}");
  }
  LoopDetectorCore fresh(threshold);
  std::printf("], \"early\": {\"too_soon_5\": %s, \"too_soon_10\": %s, \"add\": %s}",
              fresh.too_soon(5) ? "true" : "false", fresh.too_soon(10) ? "true" : "false",
              LoopDetectorCore::early_exit().add_current_keyframe ? "true" : "false");

  // gather: keyframe 0 with covisible {1 (bad), 2}, connected {2, 1}; ids are 10 * index + 7
  KeyFrameView kfs[3] = {};
  const int32_t cov[2] = {1, 2}, con[2] = {2, 1};
  for (int i = 0; i < 3; i++) kfs[i].id = 10 * i + 7;
  kfs[1].bad = true;
  kfs[0].covisible = cov;
  kfs[0].n_covisible = 2;
  const LoopQueryIds ids = gather_detect_loop_candidates(0, kfs, con, 2);
  std::printf(", \"gather\": {\"kf_id\": %d, \"connected\": ", ids.kf_id);
  print_ids(ids.connected);
  std::printf(", \"covisible\": ");
  print_ids(ids.covisible);
  std::printf("}}\n");
  return 0;
}
