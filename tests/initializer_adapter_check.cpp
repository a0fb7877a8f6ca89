// InitializerCore (include/slamgpu_adapters.hpp) driven from C++ on the device as
// Tracker::MonocularInitialization does (tracker.cpp:297-343): one reference frame, then one
// Initialize per current frame until one succeeds. The scenario is a binary file written by
// tests/test_initializer_adapter.py: int32 n1, n2, iterations, n_calls; float K[4], sigma,
// keys1[n1][2]; then per call float keys2[n2][2] and int32 vMatches12[n1]. The core runs with the
// default rand() functor, so the first call seeds rand() with 0 (SeedRandOnce). Prints, per call,
// the outcome, the draws, and R21 / t21 / vP3D as the bit patterns of their floats; the Python
// side feeds the draws to the CPU restatement and requires equality.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slamgpu_adapters.hpp"

namespace A = slamgpu_adapter;

template <typename T>
static bool get(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

static unsigned bits_of(float x) {
  unsigned u;
  std::memcpy(&u, &x, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[4];
  float K[4], sigma;
  if (!get(f, head, 4) || !get(f, K, 4) || !get(f, &sigma, 1)) return 2;
  const int n1 = head[0], n2 = head[1], iterations = head[2], n_calls = head[3];
  std::vector<float> keys1(2 * (size_t)n1), keys2(2 * (size_t)n2);
  std::vector<int32_t> m12(n1);
  if (!get(f, keys1.data(), keys1.size())) return 2;
  std::srand(1);  // SeedRandOnce(0) must replace this
  try {
    A::InitializerCore init(keys1.data(), n1, K, sigma, iterations);
    for (int c = 0; c < n_calls; ++c) {
      if (!get(f, keys2.data(), keys2.size()) || !get(f, m12.data(), m12.size())) return 2;
      float R21[9] = {0}, t21[3] = {0};
      std::vector<float> vP3D;
      std::vector<bool> vbTriangulated;
      const bool ok = init.Initialize(keys2.data(), n2, std::vector<int>(m12.begin(), m12.end()),
                                      R21, t21, vP3D, vbTriangulated);
      std::printf("call %d ok %d model %d n_motions %d device_calls %d\n", c, ok ? 1 : 0,
                  init.result().model, init.result().n_motions, init.device_calls());
      std::printf("draws");
      for (int d : init.draws()) std::printf(" %d", d);
      std::printf("\n");
      if (!ok) continue;
      std::printf("pose");
      for (float x : R21) std::printf(" %08x", bits_of(x));
      for (float x : t21) std::printf(" %08x", bits_of(x));
      std::printf("\ntriangulated");
      for (int i = 0; i < n1; ++i)
        if (vbTriangulated[i]) std::printf(" %d", i);
      std::printf("\np3d");
      for (float x : vP3D) std::printf(" %08x", bits_of(x));
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 1;
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
