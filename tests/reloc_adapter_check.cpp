// reloc_adapter_check.cpp -- relocalization_refine of include/slamgpu_adapters.hpp
// (Tracker::Relocalization's refinement of one candidate, tracker.cpp:924-975) driven from C++
// against libslamgpu.so, no Python in between. tests/test_reloc_adapter.py writes the inputs as
// raw arrays into a directory and reads the recorded steps back:
//   reloc_adapter_check <dir> <cols> <rows> <n_keyframe_keypoints>
//   <dir>/left.u8, right.u8   the current frame's stereo pair (rows x cols)
//   kf_kps.bin                the keyframe's undistorted keypoints (slamgpu_keypoint)
//   queries.bin               one slamgpu_reloc_query per keyframe keypoint: its map point (skip =
//                             no point); map point index = keypoint index
//   init_mp.i32               the frame's slots after the PnP step (map point index or -1)
//   found.i32                 sFound; Tcw0.f32 the PnP pose (4x4); inv_sigma2.f32 (8 levels)
// Output: "nkps N ngood G steps K" and <dir>/trace.bin, K records of
//   int32 kind, result; float Tcw_in[16], Tcw_out[16]; slamgpu_reloc_pose; int32 n_found,
//   found[nk]; int32 map_points_in[N], map_points_out[N]; uint8 outlier[N].
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

static void check(int rc, const char* what, const char* msg) {
  if (rc != SLAMGPU_OK) {
    std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, msg ? msg : "");
    std::exit(1);
  }
}

template <typename T>
static void put(FILE* f, const T* p, size_t n) {
  if (n && std::fwrite(p, sizeof(T), n, f) != n) std::exit(2);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s dir cols rows n_keyframe_keypoints\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int cols = std::atoi(argv[2]), rows = std::atoi(argv[3]), nk = std::atoi(argv[4]);
  const auto left = read_all<uint8_t>(dir + "/left.u8"), right = read_all<uint8_t>(dir + "/right.u8");
  const auto kf_kps = read_all<slamgpu_keypoint>(dir + "/kf_kps.bin");
  const auto queries = read_all<slamgpu_reloc_query>(dir + "/queries.bin");
  auto map_points = read_all<int32_t>(dir + "/init_mp.i32");
  const auto found = read_all<int32_t>(dir + "/found.i32");
  auto Tcw = read_all<float>(dir + "/Tcw0.f32");
  const auto inv_sigma2 = read_all<float>(dir + "/inv_sigma2.f32");
  if ((int)left.size() != cols * rows || right.size() != left.size() || (int)kf_kps.size() != nk ||
      (int)queries.size() != nk || Tcw.size() != 16 || inv_sigma2.size() != 8) {
    std::fprintf(stderr, "input sizes do not fit\n");
    return 2;
  }

  const slamgpu_orb_params prm = {2000, 1.2f, 8, 20, 7};
  const slamgpu_camera cam = {718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f};
  slamgpu_ctx* ctx = nullptr;
  check(slamgpu_create(0, &prm, cols, rows, 1, &ctx), "slamgpu_create", slamgpu_last_error(nullptr));
  check(slamgpu_frame_stereo(ctx, left.data(), right.data(), (size_t)cols, &cam),
        "slamgpu_frame_stereo", slamgpu_last_error(ctx));
  const int cap = slamgpu_kp_capacity(ctx);
  std::vector<slamgpu_keypoint> kps(cap);
  std::vector<uint8_t> desc((size_t)cap * 32);
  std::vector<float> ur(cap), depth(cap);
  int n = 0, n2 = 0;
  check(slamgpu_download_keypoints(ctx, 0, kps.data(), desc.data(), cap, &n),
        "slamgpu_download_keypoints", slamgpu_last_error(ctx));
  check(slamgpu_download_stereo(ctx, 0, ur.data(), depth.data(), cap, &n2), "slamgpu_download_stereo",
        slamgpu_last_error(ctx));
  if ((int)map_points.size() != n || n2 != n) {
    std::fprintf(stderr, "the frame has %d keypoints, init_mp.i32 %zu\n", n, map_points.size());
    return 1;
  }

  // the map: point i is keyframe keypoint i's (absent where the record says skip)
  std::vector<A::MapPointView> mps(nk);
  std::vector<A::MapPointGeometry> geom(nk);
  std::vector<int32_t> kf_mp(nk);
  for (int i = 0; i < nk; ++i) {
    const slamgpu_reloc_query& q = queries[i];
    mps[i] = A::MapPointView{i, false, {q.xyz[0], q.xyz[1], q.xyz[2]}, q.desc, nullptr, 0};
    geom[i] = A::MapPointGeometry{{0, 0, 0}, q.min_dist, q.max_dist, 1};
    kf_mp[i] = q.skip ? -1 : i;
  }
  const float kf_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const A::KeyFrameView kf = {0, false, kf_pose, kf_kps.data(), nullptr, kf_mp.data(), nk, nullptr, 0};
  std::vector<uint8_t> outlier(n, 0);
  const A::FrameView current = {Tcw.data(), kps.data(), kps.data(), ur.data(), map_points.data(),
                                outlier.data(), n};
  std::vector<A::RelocRefineStep> trace;
  int n_good = 0;
  try {
    n_good = A::relocalization_refine(ctx, 0, cam, inv_sigma2.data(), 8, current, Tcw.data(),
                                      map_points.data(), outlier.data(), kf, mps.data(), geom.data(),
                                      found, true, &trace);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "relocalization_refine: %s\n", e.what());
    return 1;
  }
  FILE* out = std::fopen((dir + "/trace.bin").c_str(), "wb");
  if (!out) return 2;
  for (const A::RelocRefineStep& s : trace) {
    put(out, &s.kind, 1);
    put(out, &s.result, 1);
    put(out, s.Tcw_in, 16);
    put(out, s.Tcw_out, 16);
    put(out, &s.pose, 1);
    const int32_t nf = (int32_t)s.found.size();
    put(out, &nf, 1);
    std::vector<int32_t> f(nk, -1);
    for (int i = 0; i < nf && i < nk; ++i) f[i] = s.found[i];
    put(out, f.data(), f.size());
    put(out, s.map_points_in.data(), s.map_points_in.size());
    put(out, s.map_points_out.data(), s.map_points_out.size());
    put(out, s.outlier_out.data(), s.outlier_out.size());
  }
  std::fclose(out);
  std::printf("nkps %d ngood %d steps %zu\n", n, n_good, trace.size());
  slamgpu_destroy(ctx);
  return 0;
}
