// The OpenCV-free cores of the loop closer's adapters (include/slamgpu_adapters.hpp) that need
// no device: the record gather (loop_point, loop_kf) and the Fuse(pKF, Scw, ...) tail
// (fuse_sim3_apply, orb_matcher.cpp:1061-1075) on a hand-made map. Prints "ok" or the failed check.
#include <cstdio>
#include <cstring>
#include <vector>

#include "slamgpu_adapters.hpp"

namespace A = slamgpu_adapter;

#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                       \
    }                                                 \
  } while (0)

int main() {
  uint8_t desc[32];
  for (int i = 0; i < 32; ++i) desc[i] = (uint8_t)(i * 7);
  A::MapPointView mp{};
  mp.id = 5;
  mp.xyz[0] = 1.f, mp.xyz[1] = 2.f, mp.xyz[2] = 3.f;
  mp.desc = desc;
  A::MapPointGeometry g{{0.f, 0.f, 1.f}, 0.5f, 9.f, 2};
  slamgpu_fuse_point q = A::loop_point(&mp, &g, 0, false);
  CHECK(q.skip == 0 && q.xyz[2] == 3.f && q.normal[2] == 1.f && q.min_dist == 0.5f &&
        q.max_dist == 9.f && std::memcmp(q.desc, desc, 32) == 0);
  CHECK(A::loop_point(&mp, &g, 0, true).skip == 1);
  CHECK(A::loop_point(&mp, &g, -1, false).skip == 1);

  float Tcw[16] = {1, 0, 0, 4, 0, 1, 0, 5, 0, 0, 1, 6, 0, 0, 0, 1};
  float Ow[3] = {-4, -5, -6};
  A::KeyFrameView kv{};
  kv.Tcw = Tcw;
  kv.n_kps = 7;
  A::KeyFrameFeatures kf{};
  kf.Ow = Ow;
  const slamgpu_kf k = A::loop_kf(kv, kf);
  CHECK(k.n == 7 && k.Rcw[4] == 1.f && k.tcw[1] == 5.f && k.Ow[2] == -6.f && k.u_right == nullptr);

  // points 0..5 offered; slots: keypoint 5 holds point 9, keypoint 6 holds the bad point 8
  const int32_t best[6] = {3, -1, 3, 5, 6, 7};
  const int32_t points[6] = {0, 1, 2, 3, 4, 5};
  std::vector<uint8_t> bad(10, 0), in_kf(6, 0);
  bad[8] = 1;
  in_kf[5] = 1;  // point 5 already sits in the keyframe
  std::vector<int32_t> slot(10, -1);
  slot[5] = 9;
  slot[6] = 8;
  const A::FuseSim3Result r = A::fuse_sim3_apply(best, points, 6, bad.data(), slot, in_kf);
  CHECK(r.nfused == 4);
  CHECK(r.added.size() == 1 && r.added[0].first == 0 && r.added[0].second == 3 && slot[3] == 0);
  const int32_t want[6] = {-1, -1, 0, 9, -1, -1};  // 2 -> the point just added, 3 -> 9
  for (int i = 0; i < 6; ++i) CHECK(r.replace[i] == want[i]);
  CHECK(slot[6] == 8 && slot[7] == -1);
  std::printf("ok\n");
  return 0;
}
