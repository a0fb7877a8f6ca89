// ransac_common_check.cpp -- the host-compilable part of csrc/ransac_device.h (resolve_sample,
// draw_in_range, check_draws) walked on the CPU by g++ alone, under the address and
// undefined-behaviour sanitizers (tests/test_ransac_common.py). No HIP, no libslamgpu.so.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ransac_device.h"

namespace {

int g_fail = 0;

#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond) && g_fail++ < 20) std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
  } while (0)

// The reference's sampling on a real vector.
template <int S>
void swap_and_pop(const int32_t* draws, int n, int (&idx)[S]) {
  std::vector<int> avail(n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int i = 0; i < S; i++) {
    const int r = draws[i];
    idx[i] = avail[r];
    avail[r] = avail.back();
    avail.pop_back();
  }
}

// The closed form for three draws that sim3_hyp_kernel held before resolve_sample<3> replaced it.
void closed_form3(const int32_t* draws, int n, int (&idx)[3]) {
  const int r0 = draws[0], r1 = draws[1], r2 = draws[2];
  idx[0] = r0;
  idx[1] = r1 == r0 ? n - 1 : r1;
  idx[2] = r2 == r1 ? (r0 == n - 2 ? n - 1 : n - 2) : (r2 == r0 ? n - 1 : r2);
}

// Every valid draw tuple of a sample of S out of n: draw i runs over [0, n - 1 - i].
template <int S>
long exhaustive(int n) {
  int32_t d[S] = {};
  long count = 0;
  for (;;) {
    int got[S], want[S];
    slamgpu::resolve_sample<S>(d, n, got);
    swap_and_pop<S>(d, n, want);
    CHECK(std::memcmp(got, want, sizeof(got)) == 0);
    if (S == 3) {
      int old[3];
      closed_form3(d, n, old);
      CHECK(std::memcmp(got, old, sizeof(old)) == 0);
    }
    for (int i = 0; i < S; i++) CHECK(slamgpu::draw_in_range<S>(d[i], i, n));
    count++;
    int i = S - 1;
    while (i >= 0 && d[i] == n - 1 - i) d[i--] = 0;
    if (i < 0) break;
    d[i]++;
  }
  return count;
}

template <int S>
void range_edges(int n) {
  for (int rep = 0; rep < 2; rep++)  // i and i + S are the same place in the sample
    for (int p = 0; p < S; p++) {
      const int i = rep * S + p;
      CHECK(!slamgpu::draw_in_range<S>(-1, i, n));
      CHECK(slamgpu::draw_in_range<S>(0, i, n));
      CHECK(slamgpu::draw_in_range<S>(n - 1 - p, i, n));
      CHECK(!slamgpu::draw_in_range<S>(n - p, i, n));
    }
}

long product(int n, int s) {
  long p = 1;
  for (int i = 0; i < s; i++) p *= n - i;
  return p;
}

}  // namespace

int main() {
  for (int n = 3; n <= 7; n++) CHECK(exhaustive<3>(n) == product(n, 3));
  for (int n = 4; n <= 8; n++) CHECK(exhaustive<4>(n) == product(n, 4));
  for (int n = 8; n <= 10; n++) CHECK(exhaustive<8>(n) == product(n, 8));
  for (int n : {3, 7, 64}) range_edges<3>(n);
  for (int n : {4, 8, 64}) range_edges<4>(n);
  for (int n : {8, 10, 64}) range_edges<8>(n);

  // the schedule of test_pnpsolver_gpu.py::test_synchronous_call_errors: 64 correspondences, four
  // iterations, the third draw of iteration 1 one past its range
  slamgpu::ErrorSlot err;
  std::vector<int32_t> d(16);
  for (int i = 0; i < 16; i++) d[i] = (7 * i + 3) % (64 - i % 4);
  CHECK(slamgpu::check_draws<4>(err, d.data(), 4, 64) == 0 && err.msg.empty());
  d[6] = 62;
  CHECK(slamgpu::check_draws<4>(err, d.data(), 4, 64) == SLAMGPU_EINVAL);
  CHECK(err.msg == "iteration 1: draw 2 = 62 outside [0, 61]");
  d[6] = 61;
  CHECK(slamgpu::check_draws<4>(err, d.data(), 4, 64) == 0);
  d[15] = -1;  // the first bad draw is the one reported
  d[9] = 63;
  CHECK(slamgpu::check_draws<4>(err, d.data(), 4, 64) == SLAMGPU_EINVAL);
  CHECK(err.msg == "iteration 2: draw 1 = 63 outside [0, 62]");
  CHECK(slamgpu::check_draws<4>(err, d.data(), 2, 64) == 0);  // stops at n_its
  CHECK(slamgpu::check_draws<3>(err, d.data(), 0, 3) == 0);

  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
