// initmatch_adapter_check.cpp -- the first two device calls of Tracker::MonocularInitialization
// (tracker.cpp:297-364) driven from C++ against libslamgpu.so, no Python in between:
// slamgpu_frame_mono on the current image, then search_for_initialization of
// include/slamgpu_adapters.hpp with the initial frame the caller kept.
// tests/test_initmatch_gpu.py writes the inputs as raw arrays into a directory and reads the
// results back:
//   initmatch_adapter_check <dir> <cols> <rows> <windowSize> <nnratio> <checkOri>
//   <dir>/image.u8            the current frame's image (rows x cols)
//   f1_kps.bin, f1_desc.u8    the initial frame's undistorted keypoints and descriptors
//   prev.f32                  vbPrevMatched at entry ([n1][2])
// Output: "nkps N nmatches M", <dir>/matches12.i32, <dir>/prev_out.f32, and the frame's keypoints
// as downloaded (<dir>/f2_kps.bin, f2_desc.u8, f2_ur.f32, f2_depth.f32).
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

static void check(int rc, const char* what, const char* msg) {
  if (rc != SLAMGPU_OK) {
    std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, msg ? msg : "");
    std::exit(1);
  }
}

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s dir cols rows windowSize nnratio checkOri\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int cols = std::atoi(argv[2]), rows = std::atoi(argv[3]), window = std::atoi(argv[4]);
  const float nnratio = (float)std::atof(argv[5]);
  const bool check_ori = std::atoi(argv[6]) != 0;
  const auto image = read_all<uint8_t>(dir + "/image.u8");
  const auto f1_kps = read_all<slamgpu_keypoint>(dir + "/f1_kps.bin");
  const auto f1_desc = read_all<uint8_t>(dir + "/f1_desc.u8");
  auto prev = read_all<float>(dir + "/prev.f32");
  const int n1 = (int)f1_kps.size();
  if ((int)image.size() != cols * rows || f1_desc.size() != (size_t)n1 * 32 ||
      prev.size() != (size_t)n1 * 2) {
    std::fprintf(stderr, "input sizes do not fit\n");
    return 2;
  }
  const slamgpu_orb_params prm = {2000, 1.2f, 8, 20, 7};
  const slamgpu_camera cam = {718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f};
  slamgpu_ctx* ctx = nullptr;
  check(slamgpu_create(0, &prm, cols, rows, 1, &ctx), "slamgpu_create", slamgpu_last_error(nullptr));
  check(slamgpu_frame_mono(ctx, image.data(), (size_t)cols, &cam), "slamgpu_frame_mono",
        slamgpu_last_error(ctx));
  const int cap = slamgpu_kp_capacity(ctx);
  std::vector<slamgpu_keypoint> kps(cap);
  std::vector<uint8_t> desc((size_t)cap * 32);
  std::vector<float> ur(cap), depth(cap);
  int n = 0, n2 = 0;
  check(slamgpu_download_keypoints(ctx, 0, kps.data(), desc.data(), cap, &n),
        "slamgpu_download_keypoints", slamgpu_last_error(ctx));
  check(slamgpu_download_stereo(ctx, 0, ur.data(), depth.data(), cap, &n2), "slamgpu_download_stereo",
        slamgpu_last_error(ctx));
  if (n2 != n) return 1;

  const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const A::FrameView F1 = {identity, f1_kps.data(), f1_kps.data(), nullptr, nullptr, nullptr, n1};
  std::vector<int32_t> matches12(n1 > 0 ? n1 : 1, -7);
  int nm = 0;
  try {
    nm = A::search_for_initialization(ctx, 0, F1, f1_desc.data(), prev.data(), matches12.data(),
                                      window, nnratio, check_ori);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "search_for_initialization: %s\n", e.what());
    return 1;
  }
  write_all(dir + "/matches12.i32", matches12.data(), (size_t)n1);
  write_all(dir + "/prev_out.f32", prev.data(), prev.size());
  write_all(dir + "/f2_kps.bin", kps.data(), (size_t)n);
  write_all(dir + "/f2_desc.u8", desc.data(), (size_t)n * 32);
  write_all(dir + "/f2_ur.f32", ur.data(), (size_t)n);
  write_all(dir + "/f2_depth.f32", depth.data(), (size_t)n);
  std::printf("nkps %d nmatches %d\n", n, nm);
  slamgpu_destroy(ctx);
  return 0;
}
