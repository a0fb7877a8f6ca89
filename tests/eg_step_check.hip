// eg_step_check.hip -- one linear step of OptimizeEssentialGraph run alone, for
// tests/test_eg_step.py and tests/test_eg_step_gpu.py:
//   eg_step_check in.bin out.bin              the records below on the device
//   eg_step_check --structure in.bin out.bin  the structure arrays of every step record; HIP is
//                                             never initialised
// eg_kernels.hip is included, not linked, so its kernels and eg_meta_bytes are reachable; the
// structure comes from csrc/eg_structure.h, the function the runtime calls. File formats (all
// fields 8 bytes, little endian; tests/eg_step_spec.py writes and reads them): magic, record
// count, then per record its kind and
//   1 step    n_kf, n_edges, fix_scale, n_lambda, fixed[n_kf], (i, j)[n_edges], lambda[n_lambda],
//             J[n_edges][98], err[n_edges][7]
//             -> n_edges, F, n_blocks, n_lambda, staged variant chosen (1 / 0), its LDS bytes,
//                contrib, H, b, then per lambda and per way (the launcher, <true>, <false>):
//                ran (1 / 0), x[7F], out[1], out[2]
//   2 chi2    n, chi2[n] -> the sum
//   3 update  n_kf, fix_scale, n_points, fixed[n_kf], S[n_kf][8], S_fin[n_kf][8], x[7F],
//             points[n_points][3] (floats held in doubles), point_ref[n_points]
//             -> n_kf, n_points, S_trial of launch_eg_update(S, x), then launch_eg_finish with
//                S_fin as the optimised and S as the initial estimates: Tcw[n_kf][16] and the
//                corrected points (floats in doubles)
// Outputs start as a pattern that shows untouched storage: contrib, H, b, L, y as a NaN with a
// payload, x as the sentinel. Every count is checked against the file length before anything
// touches the GPU; a malformed file ends the program with status 1 and no output file.
#include "../slam_framework_amd/csrc/eg_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../slam_framework_amd/csrc/eg_structure.h"

namespace slamgpu {
namespace {

constexpr uint64_t kMagic = 0x3130504554534745ull;  // "EGSTEP01"
constexpr uint64_t kNanBits = 0x7FF8000000E6E600ull;
constexpr double kSentinel = -12345.0;
constexpr uint64_t kMaxRecords = 256, kMaxKf = 1u << 16, kMaxEdges = 1u << 20, kMaxLambda = 8,
                   kMaxChi2 = 1u << 20, kMaxPoints = 1u << 20;
enum : uint64_t { kStep = 1, kChi2 = 2, kUpdate = 3 };

[[noreturn]] void die(const char* what) {
  std::fprintf(stderr, "eg_step_check: %s\n", what);
  std::exit(1);
}
void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    std::fprintf(stderr, "eg_step_check: %s: %s\n", what, hipGetErrorString(e));
    std::exit(1);  // nothing more is started after an error
  }
}

struct Record {
  uint64_t kind;
  uint64_t n_kf = 0, n_edges = 0, fix_scale = 0, n_lambda = 0, n = 0, n_points = 0;
  int F = 0;
  size_t at = 0;  // the record's first word after its header
};

// device buffer of `bytes` (at least 8, so empty arrays still have an address)
template <class T>
T* dalloc(size_t count) {
  void* p = nullptr;
  hip_ok(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 8)), "hipMalloc");
  return static_cast<T*>(p);
}
template <class T>
T* upload(const std::vector<T>& v) {
  T* p = dalloc<T>(v.size());
  if (!v.empty())
    hip_ok(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "copy in");
  return p;
}
void fill_words(double* d, size_t n, uint64_t bits) {
  std::vector<uint64_t> h(n, bits);
  if (n) hip_ok(hipMemcpy(d, h.data(), n * 8, hipMemcpyHostToDevice), "fill");
}
void fill_value(double* d, size_t n, double v) {
  uint64_t bits;
  std::memcpy(&bits, &v, 8);
  fill_words(d, n, bits);
}
void download(std::vector<uint64_t>& o, const double* d, size_t n) {
  const size_t at = o.size();
  o.resize(at + n);
  if (n) hip_ok(hipMemcpy(&o[at], d, n * 8, hipMemcpyDeviceToHost), "copy out");
}
void push_double(std::vector<uint64_t>& o, double v) {
  uint64_t bits;
  std::memcpy(&bits, &v, 8);
  o.push_back(bits);
}

std::vector<slamgpu_sim3_edge> edges_of(const std::vector<uint64_t>& w, const Record& r) {
  std::vector<slamgpu_sim3_edge> e(r.n_edges);
  const size_t at = r.at + r.n_kf;
  for (size_t k = 0; k < r.n_edges; k++) {
    std::memset(&e[k], 0, sizeof(e[k]));
    e[k].i = (int32_t)w[at + 2 * k];
    e[k].j = (int32_t)w[at + 2 * k + 1];
  }
  return e;
}
std::vector<uint8_t> fixed_of(const std::vector<uint64_t>& w, const Record& r) {
  std::vector<uint8_t> f(r.n_kf);
  for (size_t v = 0; v < r.n_kf; v++) f[v] = (uint8_t)w[r.at + v];
  return f;
}

struct DeviceGraph {
  EgGraph G;
  std::vector<void*> owned;
  template <class T>
  const T* put(const std::vector<T>& v) {
    T* p = upload(v);
    owned.push_back(p);
    return p;
  }
  void release() {
    for (void* p : owned) hip_ok(hipFree(p), "hipFree");
  }
};

DeviceGraph device_graph(const EgStructure& s, const std::vector<slamgpu_sim3_edge>& edges,
                         int n_kf, int fix_scale) {
  DeviceGraph D;
  EgGraph& G = D.G;
  G.n = n_kf;
  G.n_edges = (int)edges.size();
  G.F = s.F;
  G.fix_scale = fix_scale ? 1 : 0;
  G.edges = D.put(edges);
  G.fidx = D.put(s.fidx);
  G.start = D.put(s.start);
  G.off = D.put(s.off);
  G.n_targets = (int)s.tgt_block.size();
  G.tgt_block = D.put(s.tgt_block);
  G.tgt_vertex = D.put(s.tgt_vertex);
  G.tgt_ptr = D.put(s.tgt_ptr);
  G.tgt_items = D.put(s.tgt_items);
  G.ext_ptr = D.put(s.ext_ptr);
  G.ext_rows = D.put(s.ext_rows);
  G.ext_base = D.put(s.ext_base);
  G.n_ext = (int)s.ext_rows.size();
  G.n_blocks = s.n_blocks;
  return D;
}

void run_step(const std::vector<uint64_t>& w, const Record& r, std::vector<uint64_t>& o) {
  const std::vector<uint8_t> fixed = fixed_of(w, r);
  const std::vector<slamgpu_sim3_edge> edges = edges_of(w, r);
  const EgStructure s = eg_build_structure((int)r.n_kf, fixed.data(), edges.data(), (int)r.n_edges);
  DeviceGraph D = device_graph(s, edges, (int)r.n_kf, (int)r.fix_scale);
  const EgGraph& G = D.G;
  const size_t E = r.n_edges, P7 = 7 * (size_t)s.F, NB = (size_t)s.n_blocks * 49;
  const size_t at_lambda = r.at + r.n_kf + 2 * E, at_J = at_lambda + r.n_lambda, at_err = at_J + 98 * E;
  EgState W{};
  W.J = dalloc<double>(98 * E);
  W.err = dalloc<double>(7 * E);
  W.contrib = dalloc<double>(kEgContrib * E);
  W.H = dalloc<double>(NB);
  W.L = dalloc<double>(NB);
  W.b = dalloc<double>(P7);
  W.x = dalloc<double>(P7);
  W.y = dalloc<double>(P7);
  W.out = dalloc<double>(4);
  if (E) {
    hip_ok(hipMemcpy(W.J, &w[at_J], 98 * E * 8, hipMemcpyHostToDevice), "copy in");
    hip_ok(hipMemcpy(W.err, &w[at_err], 7 * E * 8, hipMemcpyHostToDevice), "copy in");
  }
  fill_words(W.contrib, kEgContrib * E, kNanBits);
  fill_words(W.H, NB, kNanBits);
  fill_words(W.b, P7, kNanBits);
  if (E) {
    hipLaunchKernelGGL(eg_products_kernel, dim3(blocks_of((int)E * 7, 256)), dim3(256), 0, 0, G, W);
    hip_ok(hipGetLastError(), "eg_products");
  }
  hip_ok(launch_eg_assemble(G, W, s.n_blocks, 0), "eg_assemble");
  hip_ok(hipDeviceSynchronize(), "products and assembly");
  const size_t meta = eg_meta_bytes(G);
  o.push_back(E);
  o.push_back((uint64_t)s.F);
  o.push_back((uint64_t)s.n_blocks);
  o.push_back(r.n_lambda);
  o.push_back(meta > 0 ? 1 : 0);
  o.push_back(meta);
  download(o, W.contrib, kEgContrib * E);
  download(o, W.H, NB);
  download(o, W.b, P7);
  for (uint64_t l = 0; l < r.n_lambda; l++) {
    double lambda;
    std::memcpy(&lambda, &w[at_lambda + l], 8);
    for (int way = 0; way < 3; way++) {
      fill_words(W.L, NB, kNanBits);
      fill_words(W.y, P7, kNanBits);
      fill_words(W.out, 4, kNanBits);
      fill_value(W.x, P7, kSentinel);
      const bool ran = way != 1 || meta > 0;
      if (way == 0) {
        hip_ok(launch_eg_factor_solve(G, W, s.n_blocks, lambda, 0), "eg_factor_solve");
      } else if (ran) {  // the launcher's copy of H, launch shape and dynamic LDS
        if (NB) hip_ok(hipMemcpy(W.L, W.H, NB * 8, hipMemcpyDeviceToDevice), "copy H");
        if (way == 1)
          hipLaunchKernelGGL(eg_factor_solve_kernel<true>, dim3(1), dim3(kFacThreads), meta, 0, G,
                             W, s.n_blocks, lambda);
        else
          hipLaunchKernelGGL(eg_factor_solve_kernel<false>, dim3(1), dim3(kFacThreads), 0, 0, G, W,
                             s.n_blocks, lambda);
        hip_ok(hipGetLastError(), "eg_factor_solve_kernel");
      }
      hip_ok(hipDeviceSynchronize(), "factor and solve");
      o.push_back(ran ? 1 : 0);
      download(o, W.x, P7);
      download(o, W.out + 1, 2);
    }
  }
  for (double* p : {W.J, W.err, W.contrib, W.H, W.L, W.b, W.x, W.y, W.out})
    hip_ok(hipFree(p), "hipFree");
  D.release();
}

void run_chi2(const std::vector<uint64_t>& w, const Record& r, std::vector<uint64_t>& o) {
  EgGraph G{};
  EgState W{};
  G.n_edges = (int)r.n;
  W.chi2 = dalloc<double>(r.n);
  W.out = dalloc<double>(4);
  if (r.n) hip_ok(hipMemcpy(W.chi2, &w[r.at], r.n * 8, hipMemcpyHostToDevice), "copy in");
  fill_words(W.out, 4, kNanBits);
  hip_ok(launch_eg_chi2_sum(G, W, 0), "eg_chi2_sum");
  hip_ok(hipDeviceSynchronize(), "eg_chi2_sum");
  download(o, W.out, 1);
  hip_ok(hipFree(W.chi2), "hipFree");
  hip_ok(hipFree(W.out), "hipFree");
}

void run_update(const std::vector<uint64_t>& w, const Record& r, std::vector<uint64_t>& o) {
  const std::vector<uint8_t> fixed = fixed_of(w, r);
  const EgStructure s = eg_build_structure((int)r.n_kf, fixed.data(), nullptr, 0);
  DeviceGraph D = device_graph(s, {}, (int)r.n_kf, (int)r.fix_scale);
  const EgGraph& G = D.G;
  const size_t N = r.n_kf, P7 = 7 * (size_t)s.F, M = r.n_points;
  const size_t at_S = r.at + N, at_F = at_S + 8 * N, at_x = at_F + 8 * N, at_p = at_x + P7,
               at_ref = at_p + 3 * M;
  EgState W{};
  W.S = dalloc<double>(8 * N);
  W.S_trial = dalloc<double>(8 * N);
  W.x = dalloc<double>(P7);
  double* d_fin = dalloc<double>(8 * N);
  if (N) hip_ok(hipMemcpy(W.S, &w[at_S], 8 * N * 8, hipMemcpyHostToDevice), "copy in");
  if (N) hip_ok(hipMemcpy(d_fin, &w[at_F], 8 * N * 8, hipMemcpyHostToDevice), "copy in");
  if (P7) hip_ok(hipMemcpy(W.x, &w[at_x], P7 * 8, hipMemcpyHostToDevice), "copy in");
  fill_words(W.S_trial, 8 * N, kNanBits);
  std::vector<float> pts(3 * M), T(16 * N, -12345.f);
  std::vector<int32_t> ref(M);
  for (size_t q = 0; q < 3 * M; q++) {
    double v;
    std::memcpy(&v, &w[at_p + q], 8);
    pts[q] = (float)v;
  }
  for (size_t q = 0; q < M; q++) ref[q] = (int32_t)w[at_ref + q];
  float* d_pts = upload(pts);
  float* d_T = upload(T);
  int32_t* d_ref = upload(ref);
  hip_ok(launch_eg_update(G, W, 0), "eg_update");
  hip_ok(launch_eg_finish(G, d_fin, W.S, d_T, d_pts, d_ref, (int)M, 0), "eg_finish");
  hip_ok(hipDeviceSynchronize(), "update and finish");
  o.push_back(N);
  o.push_back(M);
  download(o, W.S_trial, 8 * N);
  if (N) hip_ok(hipMemcpy(T.data(), d_T, 16 * N * 4, hipMemcpyDeviceToHost), "copy out");
  if (M) hip_ok(hipMemcpy(pts.data(), d_pts, 3 * M * 4, hipMemcpyDeviceToHost), "copy out");
  for (float v : T) push_double(o, (double)v);
  for (float v : pts) push_double(o, (double)v);
  for (void* p : {(void*)W.S, (void*)W.S_trial, (void*)W.x, (void*)d_fin, (void*)d_pts, (void*)d_T, (void*)d_ref})
    hip_ok(hipFree(p), "hipFree");
  D.release();
}

void write_structure(const std::vector<uint64_t>& w, const Record& r, std::vector<uint64_t>& o) {
  const std::vector<uint8_t> fixed = fixed_of(w, r);
  const std::vector<slamgpu_sim3_edge> edges = edges_of(w, r);
  const EgStructure s = eg_build_structure((int)r.n_kf, fixed.data(), edges.data(), (int)r.n_edges);
  o.push_back(r.n_kf);
  o.push_back((uint64_t)s.F);
  o.push_back((uint64_t)s.n_blocks);
  o.push_back(s.tgt_block.size());
  o.push_back(s.tgt_items.size());
  o.push_back(s.ext_rows.size());
  auto put = [&](const auto& v) {
    for (auto x : v) o.push_back((uint64_t)(int64_t)x);
  };
  put(s.fidx);
  put(s.start);
  put(s.off);
  put(s.tgt_block);
  put(s.tgt_vertex);
  put(s.tgt_ptr);
  put(s.tgt_items);
  put(s.ext_ptr);
  put(s.ext_rows);
  put(s.ext_base);
}

}  // namespace
}  // namespace slamgpu

int main(int argc, char** argv) {
  using namespace slamgpu;
  const bool structure_only = argc == 4 && std::strcmp(argv[1], "--structure") == 0;
  if (!structure_only && argc != 3) die("usage: eg_step_check [--structure] in.bin out.bin");
  const char* in_path = argv[argc - 2];
  const char* out_path = argv[argc - 1];
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f) die("cannot open the case file");
  std::vector<uint64_t> w;
  {
    if (std::fseek(f, 0, SEEK_END) != 0) die("seek");
    const long bytes = std::ftell(f);
    if (bytes < 16 || bytes % 8 != 0 || bytes > (1l << 28)) die("case file length");
    std::rewind(f);
    w.resize((size_t)bytes / 8);
    if (std::fread(w.data(), 8, w.size(), f) != w.size()) die("short read");
    std::fclose(f);
  }
  // every count, size and index against the file length, before any HIP call
  if (w[0] != kMagic) die("bad magic");
  const uint64_t nrec = w[1];
  if (nrec > kMaxRecords) die("too many records");
  std::vector<Record> recs;
  size_t at = 2;
  auto need = [&](size_t words, const char* what) {
    if (words > w.size() - at) die(what);
  };
  auto count_free = [&](Record& r) {  // fixed[] at r.at: flags 0 / 1
    int F = 0;
    for (uint64_t v = 0; v < r.n_kf; v++) {
      if (w[r.at + v] > 1) die("fixed flag");
      F += w[r.at + v] == 0;
    }
    r.F = F;
  };
  for (uint64_t q = 0; q < nrec; q++) {
    need(1, "truncated record header");
    Record r;
    r.kind = w[at];
    if (r.kind == kStep) {
      need(5, "truncated record header");
      r.n_kf = w[at + 1];
      r.n_edges = w[at + 2];
      r.fix_scale = w[at + 3];
      r.n_lambda = w[at + 4];
      at += 5;
      if (r.n_kf > kMaxKf || r.n_edges > kMaxEdges) die("too many keyframes or edges");
      if (r.n_lambda > kMaxLambda) die("too many lambdas");
      if (r.fix_scale > 1) die("fix_scale flag");
      r.at = at;
      need(r.n_kf + r.n_edges * (2 + 98 + 7) + r.n_lambda, "truncated record");
      count_free(r);
      for (uint64_t k = 0; k < r.n_edges; k++) {
        const uint64_t i = w[at + r.n_kf + 2 * k], j = w[at + r.n_kf + 2 * k + 1];
        if (i >= r.n_kf || j >= r.n_kf || i == j) die("edge index");
      }
      at += r.n_kf + r.n_edges * (2 + 98 + 7) + r.n_lambda;
    } else if (r.kind == kChi2) {
      need(2, "truncated record header");
      r.n = w[at + 1];
      at += 2;
      if (r.n > kMaxChi2) die("too many chi2 values");
      r.at = at;
      need(r.n, "truncated record");
      at += r.n;
    } else if (r.kind == kUpdate) {
      need(4, "truncated record header");
      r.n_kf = w[at + 1];
      r.fix_scale = w[at + 2];
      r.n_points = w[at + 3];
      at += 4;
      if (r.n_kf > kMaxKf || r.n_points > kMaxPoints) die("too many keyframes or points");
      if (r.fix_scale > 1) die("fix_scale flag");
      r.at = at;
      need(r.n_kf, "truncated record");
      count_free(r);
      const size_t words = r.n_kf + 16 * r.n_kf + 7 * (size_t)r.F + 4 * r.n_points;
      need(words, "truncated record");
      for (uint64_t p = 0; p < r.n_points; p++)
        if (w[at + words - r.n_points + p] >= r.n_kf) die("point reference");
      at += words;
    } else {
      die("unknown record kind");
    }
    recs.push_back(r);
  }
  if (at != w.size()) die("trailing bytes");

  std::vector<uint64_t> o;
  o.push_back(kMagic);
  if (structure_only) {
    uint64_t n_step = 0;
    for (const Record& r : recs) n_step += r.kind == kStep;
    o.push_back(n_step);
    for (const Record& r : recs)
      if (r.kind == kStep) write_structure(w, r, o);
  } else {
    o.push_back(nrec);
    for (const Record& r : recs) {
      o.push_back(r.kind);
      if (r.kind == kStep) run_step(w, r, o);
      else if (r.kind == kChi2) run_chi2(w, r, o);
      else run_update(w, r, o);
    }
  }
  std::FILE* g = std::fopen(out_path, "wb");
  if (!g) die("cannot open the output file");
  if (std::fwrite(o.data(), 8, o.size(), g) != o.size()) die("short write");
  if (std::fclose(g) != 0) die("close");
  return 0;
}
