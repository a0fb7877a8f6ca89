// PnPSolverCore (include/slamgpu_adapters.hpp) driven from C++ on the device in the round robin of
// Tracker::Relocalization (tracker.cpp:904-988): the frame's undistorted keypoints, the map points
// and one vpMapPointMatches per candidate come from a JSON scenario (a flat object of number
// arrays, written by tests/test_pnpsolver_adapter.py); the solvers run with srand(1) and the
// default rand() functor. Prints each gather (mvKeyPointIndices), every iterate(5) outcome in the
// order the round robin makes them, and at the end each solver's draws and device calls; the
// Python side feeds the draws to the CPU restatement and requires equality.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "slamgpu_adapters.hpp"

namespace A = slamgpu_adapter;

using Arrays = std::map<std::string, std::vector<double>>;

// {"name": [1, 2.5, ...], ...}: nothing else is understood.
static bool parse(const std::string& s, Arrays& out) {
  size_t i = 0;
  auto ws = [&] { while (i < s.size() && std::isspace((unsigned char)s[i])) ++i; };
  ws();
  if (i >= s.size() || s[i++] != '{') return false;
  for (;;) {
    ws();
    if (i < s.size() && s[i] == '}') return true;
    if (i >= s.size() || s[i++] != '"') return false;
    const size_t e = s.find('"', i);
    if (e == std::string::npos) return false;
    std::vector<double>& v = out[s.substr(i, e - i)];
    i = e + 1;
    ws();
    if (i >= s.size() || s[i++] != ':') return false;
    ws();
    if (i >= s.size() || s[i++] != '[') return false;
    for (;;) {
      ws();
      if (i < s.size() && s[i] == ']') { ++i; break; }
      char* end = nullptr;
      v.push_back(std::strtod(s.c_str() + i, &end));
      if (end == s.c_str() + i) return false;
      i = end - s.c_str();
      ws();
      if (i < s.size() && s[i] == ',') ++i;
    }
    ws();
    if (i < s.size() && s[i] == ',') ++i;
  }
}

template <typename T>
static std::vector<T> as(const Arrays& a, const std::string& name) {
  const std::vector<double>& v = a.at(name);
  return std::vector<T>(v.begin(), v.end());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::string text;
  char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  std::fclose(f);
  Arrays a;
  if (!parse(text, a)) {
    std::printf("FAILED to parse %s\n", argv[1]);
    return 2;
  }
  // the frame: kps [n][3] = x, y, octave (undistorted)
  const std::vector<float> kraw = as<float>(a, "kps");
  std::vector<slamgpu_keypoint> kps(kraw.size() / 3);
  for (size_t i = 0; i < kps.size(); ++i) {
    kps[i] = slamgpu_keypoint{};
    kps[i].x = kraw[3 * i];
    kps[i].y = kraw[3 * i + 1];
    kps[i].octave = (int)kraw[3 * i + 2];
  }
  A::FrameView F = {};
  F.undist_kps = kps.data();
  F.n_kps = (int)kps.size();
  // map points: xyz [M][3], bad [M]
  const std::vector<float> xyz = as<float>(a, "mp_xyz");
  const std::vector<int32_t> bad = as<int32_t>(a, "mp_bad");
  std::vector<A::MapPointView> mps(bad.size());
  for (size_t m = 0; m < mps.size(); ++m) {
    mps[m] = A::MapPointView{};
    mps[m].id = (int64_t)m;
    mps[m].bad = bad[m] != 0;
    for (int r = 0; r < 3; ++r) mps[m].xyz[r] = xyz[3 * m + r];
  }
  const std::vector<float> K = as<float>(a, "K"), sigma2 = as<float>(a, "sigma2");
  // probability, minInliers, maxIterations, minSet, epsilon, th2
  const std::vector<double> ransac = a.at("ransac");
  const int n_cand = (int)a.at("candidates")[0], max_calls = (int)a.at("max_calls")[0];

  std::srand(1);
  std::vector<std::unique_ptr<A::PnPSolverCore>> solvers;
  std::vector<std::vector<int32_t>> matched(n_cand);
  for (int c = 0; c < n_cand; ++c) {
    matched[c] = as<int32_t>(a, "matches" + std::to_string(c));
    solvers.emplace_back(new A::PnPSolverCore(F, mps.data(), matched[c].data(),
                                              (int)matched[c].size(), K.data(), sigma2.data(),
                                              (int)sigma2.size()));
    A::PnPSolverCore& s = *solvers.back();
    s.SetRansacParameters(ransac[0], (int)ransac[1], (int)ransac[2], (int)ransac[3],
                          (float)ransac[4], (float)ransac[5]);
    std::printf("candidate %d n %zu min_inliers %d max_its %d indices", c, s.matches().size(),
                s.min_inliers(), s.max_iterations());
    for (int32_t i : s.indices()) std::printf(" %d", i);
    std::printf("\n");
  }
  std::vector<bool> discarded(n_cand, false);
  std::vector<int> calls(n_cand, 0);
  for (bool any = true; any;) {
    any = false;
    for (int c = 0; c < n_cand; ++c) {
      if (discarded[c]) continue;
      bool no_more = false;
      std::vector<bool> vb;
      int n_inliers = 0;
      float T[16] = {0};
      const bool ok = solvers[c]->iterate(5, no_more, vb, n_inliers, T);
      std::printf("iterate %d %d %d %d %d ", c, ok ? 1 : 0, no_more ? 1 : 0, n_inliers,
                  solvers[c]->iterations());
      std::putchar('b');
      for (bool b : vb) std::putchar(b ? '1' : '0');
      for (int i = 0; i < 12; ++i) std::printf(" %.9g", T[i]);
      std::printf("\n");
      if (no_more || ++calls[c] >= max_calls) discarded[c] = true;
      any = any || !discarded[c];
    }
  }
  for (int c = 0; c < n_cand; ++c) {
    std::printf("draws %d", c);
    for (int32_t d : solvers[c]->draws()) std::printf(" %d", d);
    std::printf("\ndevice_calls %d %d\n", c, solvers[c]->device_calls());
  }
  // any other minSet is refused
  try {
    solvers[0]->SetRansacParameters(0.99, 10, 300, 5, 0.5f, 5.991f);
    std::printf("minset accepted\n");
  } catch (const std::invalid_argument& e) {
    std::printf("minset refused: %s\n", e.what());
  }
  return 0;
}
