// Sim3SolverCore (include/slamgpu_adapters.hpp) driven from C++ on the device: the KeyFrameViews,
// map points and vpMatched12 come from a JSON scenario (a flat object of number arrays, written by
// tests/test_sim3solver_adapter.py); the solver runs with srand(1) and the default rand() functor.
// Prints the gather (mvnIndices1), the draws it made and every iterate(5) outcome with the
// estimate it leaves; the Python side feeds the draws to the CPU restatement and requires equality.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <map>
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
static std::vector<T> as(const Arrays& a, const char* name) {
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
  // keyframes 0 and 1: Tcw [16], kps [n][3] = x, y, octave, map_points [n]
  std::vector<float> Tcw[2] = {as<float>(a, "Tcw1"), as<float>(a, "Tcw2")};
  std::vector<float> kraw[2] = {as<float>(a, "kps1"), as<float>(a, "kps2")};
  std::vector<int32_t> mp_of[2] = {as<int32_t>(a, "map_points1"), as<int32_t>(a, "map_points2")};
  std::vector<slamgpu_keypoint> kps[2];
  A::KeyFrameView kfs[2] = {};
  for (int k = 0; k < 2; ++k) {
    kps[k].resize(mp_of[k].size());
    for (size_t i = 0; i < kps[k].size(); ++i) {
      kps[k][i] = slamgpu_keypoint{};
      kps[k][i].x = kraw[k][3 * i];
      kps[k][i].y = kraw[k][3 * i + 1];
      kps[k][i].octave = (int)kraw[k][3 * i + 2];
    }
    kfs[k].id = k;
    kfs[k].Tcw = Tcw[k].data();
    kfs[k].undist_kps = kps[k].data();
    kfs[k].map_points = mp_of[k].data();
    kfs[k].n_kps = (int)kps[k].size();
  }
  // map points: xyz [M][3], bad [M], obs [..][3] = map point, keyframe, keypoint
  const std::vector<float> xyz = as<float>(a, "mp_xyz");
  const std::vector<int32_t> bad = as<int32_t>(a, "mp_bad"), obs = as<int32_t>(a, "mp_obs");
  const int M = (int)bad.size();
  std::vector<std::vector<A::ObsRef>> mobs(M);
  for (size_t o = 0; o + 2 < obs.size(); o += 3) mobs[obs[o]].push_back({obs[o + 1], obs[o + 2]});
  std::vector<A::MapPointView> mps(M);
  for (int m = 0; m < M; ++m) {
    mps[m] = A::MapPointView{};
    mps[m].id = m;
    mps[m].bad = bad[m] != 0;
    for (int r = 0; r < 3; ++r) mps[m].xyz[r] = xyz[3 * m + r];
    mps[m].obs = mobs[m].data();
    mps[m].n_obs = (int)mobs[m].size();
  }
  const std::vector<int32_t> matched = as<int32_t>(a, "matched12");
  const std::vector<float> K = as<float>(a, "K"), sigma2 = as<float>(a, "sigma2");
  const std::vector<double> ransac = a.at("ransac");  // probability, minInliers, maxIterations
  const bool fix_scale = a.at("fix_scale")[0] != 0;

  std::srand(1);
  A::Sim3SolverCore solver(0, 1, kfs, mps.data(), matched.data(), (int)matched.size(), K.data(),
                           K.data(), sigma2.data(), sigma2.data(), (int)sigma2.size(), fix_scale);
  solver.SetRansacParameters(ransac[0], (int)ransac[1], (int)ransac[2]);
  std::printf("n %zu n_its %d\nindices1", solver.matches().size(), solver.max_iterations());
  for (int32_t i : solver.indices1()) std::printf(" %d", i);
  std::printf("\ndraws");
  for (int32_t d : solver.draws()) std::printf(" %d", d);
  std::printf("\n");
  for (int call = 0; call < 400; ++call) {
    bool no_more = false;
    std::vector<bool> vb;
    int n_inliers = 0;
    const int k = solver.iterate(5, no_more, vb, n_inliers);
    std::printf("iterate %d %d %d ", k, no_more ? 1 : 0, n_inliers);
    for (bool b : vb) std::putchar(b ? '1' : '0');
    float R[9] = {0}, t[3] = {0};
    const bool has = solver.GetEstimatedRotation(R) && solver.GetEstimatedTranslation(t);
    std::printf(" best %d", has ? 1 : 0);
    for (float x : R) std::printf(" %.9g", x);
    for (float x : t) std::printf(" %.9g", x);
    std::printf(" %.9g\n", solver.GetEstimatedScale());
    if (no_more) break;
  }
  return 0;
}
