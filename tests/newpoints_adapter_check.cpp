// newpoints_adapter_check.cpp -- compute_fundamental_matrix and create_new_map_points of
// include/slamgpu_adapters.hpp driven from C++ against libslamgpu.so, no Python in between.
// tests/test_newpoints_adapter.py writes the inputs as raw arrays into a directory and reads the
// results back:
//   newpoints_adapter_check fmat <dir>     (no device)
//     poses.f32    Tcw of keyframe 1 and 2 (2 x 16), cams.f32  fx fy cx cy bf of both (2 x 5)
//     -> F12.f32
//   newpoints_adapter_check chain <dir>
//     params.i32   n_kf, is_monocular, n_neighbours, then the neighbours, then first_obs
//     median.f32   [n_neighbours] ComputeSceneMedianDepth(2) of each neighbour
//     kf<i>_kps.bin, _desc.u8, _ur.f32, _depth.f32, _mp.i32 (map point index or -1), _nodes.u32,
//     _start.i32, _feats.u32, _pose.f32 (Tcw 16, Ow 3, fx fy cx cy mbf, mb)
//     -> points.bin (slamgpu_adapter::NewPoint records), skipped.u8, status.i8; prints
//        "n_new N skipped S"
// The current keyframe is keyframe 0.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slamgpu_adapters.hpp"

namespace A = slamgpu_adapter;

template <typename T>
static std::vector<T> read_all(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)bytes / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

template <typename T>
static void write_all(const std::string& path, const T* p, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || (n && std::fwrite(p, sizeof(T), n, f) != n)) std::exit(2);
  std::fclose(f);
}

static slamgpu_camera camera(const float* c) { return {c[0], c[1], c[2], c[3], c[4]}; }

static int fmat(const std::string& dir) {
  const auto poses = read_all<float>(dir + "/poses.f32");
  const auto cams = read_all<float>(dir + "/cams.f32");
  if (poses.size() != 32 || cams.size() != 10) return 2;
  A::KeyFrameView k1{}, k2{};
  k1.Tcw = poses.data();
  k2.Tcw = poses.data() + 16;
  float F12[9];
  A::compute_fundamental_matrix(k1, k2, camera(cams.data()), camera(cams.data() + 5), F12);
  write_all(dir + "/F12.f32", F12, 9);
  return 0;
}

struct Kf {
  std::vector<slamgpu_keypoint> kps;
  std::vector<uint8_t> desc;
  std::vector<float> ur, depth, pose;
  std::vector<int32_t> mp, start;
  std::vector<uint32_t> nodes, feats;
};

static int chain(const std::string& dir) {
  const auto params = read_all<int32_t>(dir + "/params.i32");
  const auto median = read_all<float>(dir + "/median.f32");
  if (params.size() < 3) return 2;
  const int n_kf = params[0], n_nb = params[2];
  const bool mono = params[1] != 0;
  if ((int)params.size() != 3 + 2 * n_nb || (int)median.size() != n_nb) return 2;
  std::vector<Kf> data(n_kf);
  std::vector<A::KeyFrameView> views(n_kf);
  std::vector<A::KeyFrameFeatures> feats(n_kf);
  std::vector<A::KeyFrameStereo> stereo(n_kf);
  for (int i = 0; i < n_kf; ++i) {
    const std::string b = dir + "/kf" + std::to_string(i);
    Kf& d = data[i];
    d.kps = read_all<slamgpu_keypoint>(b + "_kps.bin");
    d.desc = read_all<uint8_t>(b + "_desc.u8");
    d.ur = read_all<float>(b + "_ur.f32");
    d.depth = read_all<float>(b + "_depth.f32");
    d.mp = read_all<int32_t>(b + "_mp.i32");
    d.nodes = read_all<uint32_t>(b + "_nodes.u32");
    d.start = read_all<int32_t>(b + "_start.i32");
    d.feats = read_all<uint32_t>(b + "_feats.u32");
    d.pose = read_all<float>(b + "_pose.f32");
    const size_t n = d.kps.size();
    if (d.desc.size() != n * 32 || d.ur.size() != n || d.depth.size() != n || d.mp.size() != n ||
        d.pose.size() != 25 || d.start.size() != d.nodes.size() + 1) {
      std::fprintf(stderr, "keyframe %d: input sizes do not fit\n", i);
      return 2;
    }
    A::KeyFrameView& v = views[i];
    v.id = i;
    v.bad = false;
    v.Tcw = d.pose.data();
    v.undist_kps = d.kps.data();
    v.right_coords = d.ur.data();
    v.map_points = d.mp.data();
    v.n_kps = (int)n;
    v.covisible = nullptr;
    v.n_covisible = 0;
    feats[i].desc = d.desc.data();
    feats[i].fv.nodes = d.nodes.data();
    feats[i].fv.node_start = d.start.data();
    feats[i].fv.node_feats = d.feats.data();
    feats[i].fv.n_nodes = (int)d.nodes.size();
    feats[i].Ow = d.pose.data() + 16;
    stereo[i].depths = d.depth.data();
    stereo[i].kps = nullptr;
    stereo[i].cam = camera(d.pose.data() + 19);
    stereo[i].mb = d.pose[24];
  }
  slamgpu_levels lv{};
  lv.nlevels = 8;
  lv.log_scale_factor = std::log(1.2f);
  lv.scale[0] = 1.0f;
  for (int i = 1; i < 8; ++i) lv.scale[i] = lv.scale[i - 1] * 1.2f;
  for (int i = 0; i < 8; ++i) {
    lv.sigma2[i] = lv.scale[i] * lv.scale[i];
    lv.inv_sigma2[i] = 1.0f / lv.sigma2[i];
  }
  A::NewPointsResult r;
  try {
    r = A::create_new_map_points(0, views.data(), feats.data(), stereo.data(), params.data() + 3,
                                 n_nb, mono, median.data(), params.data() + 3 + n_nb, lv);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "create_new_map_points: %s\n", e.what());
    return 1;
  }
  write_all(dir + "/points.bin", r.points.data(), r.points.size());
  write_all(dir + "/skipped.u8", r.skipped.data(), r.skipped.size());
  write_all(dir + "/status.i8", r.status.data(), r.status.size());
  int skipped = 0;
  for (uint8_t s : r.skipped) skipped += s;
  std::printf("n_new %zu skipped %d\n", r.points.size(), skipped);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s fmat|chain dir\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  if (mode == "fmat") return fmat(argv[2]);
  if (mode == "chain") return chain(argv[2]);
  return 2;
}
