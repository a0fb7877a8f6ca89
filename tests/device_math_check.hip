// device_math_check.hip -- the optimizers' device helpers run one case per thread, for
// tests/test_device_math_gpu.py: device_math_check in.bin out.bin (layout: device_math_check.h).
// The library sources are included, not linked, so the helpers of their anonymous namespaces are
// reachable and libslamgpu.so stays as it is; the library's own compiler flags apply (the
// pragmas inside the helpers decide FMA contraction, as in the library). This unit holds main and
// the helpers of pose_kernels.hip, se3_device.h, sim3_device.h and ba_ldlt.h.
#include "../slam_framework_amd/csrc/pose_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../slam_framework_amd/csrc/ba_ldlt.h"
#include "../slam_framework_amd/csrc/sim3_device.h"
#include "device_math_check.h"

namespace slamgpu {
namespace {

using sim3::Sim3;

__device__ __forceinline__ SE3 load_se3(const double* v) {  // q (x, y, z, w), t
  SE3 T;
  T.r.x = v[0];
  T.r.y = v[1];
  T.r.z = v[2];
  T.r.w = v[3];
  T.t[0] = v[4];
  T.t[1] = v[5];
  T.t[2] = v[6];
  return T;
}
__device__ __forceinline__ void store_se3(const SE3& T, double* v) {
  v[0] = T.r.x;
  v[1] = T.r.y;
  v[2] = T.r.z;
  v[3] = T.r.w;
  v[4] = T.t[0];
  v[5] = T.t[1];
  v[6] = T.t[2];
}

struct OpRcp {
  static constexpr int kIn = 1, kOut = 1;
  __device__ static void run(const double* in, double* out) { out[0] = rcp_nr(in[0]); }
};
struct OpRsq {
  static constexpr int kIn = 1, kOut = 1;
  __device__ static void run(const double* in, double* out) { out[0] = rsq_nr(in[0]); }
};
struct OpHuber {  // (e, delta) -> rho0, rho0_sel, rho01's r0 and r1
  static constexpr int kIn = 2, kOut = 4;
  __device__ static void run(const double* in, double* out) {
    out[0] = huber_rho0(in[0], in[1]);
    out[1] = huber_rho0_sel(in[0], in[1]);
    huber_rho01(in[0], in[1], out[2], out[3]);
  }
};
struct OpLdlt6 {  // H (21, packed upper), lambda, b (6) -> ok, x (6)
  static constexpr int kIn = 28, kOut = 7;
  __device__ static void run(const double* in, double* out) {
    double H[kNH], b[6], x[6];
    for (int i = 0; i < kNH; i++) H[i] = in[i];
    for (int i = 0; i < 6; i++) {
      b[i] = in[22 + i];
      x[i] = dmc::kSentinel;
    }
    out[0] = ldlt_solve6(H, in[21], b, x) ? 1.0 : 0.0;
    for (int i = 0; i < 6; i++) out[1 + i] = x[i];
  }
};
struct OpLeftUpdate {  // u (6), T (7) -> pose_left_update (7), se3::se3_left_update (7)
  static constexpr int kIn = 13, kOut = 14;
  __device__ static void run(const double* in, double* out) {
    double u[6];
    for (int i = 0; i < 6; i++) u[i] = in[i];
    const SE3 T = load_se3(in + 6);
    store_se3(pose_left_update(u, T), out);
    store_se3(se3::se3_left_update(u, T), out + 7);
  }
};
struct OpQuatFromR {
  static constexpr int kIn = 9, kOut = 4;
  __device__ static void run(const double* in, double* out) {
    double R[9];
    for (int i = 0; i < 9; i++) R[i] = in[i];
    const Quat q = quat_from_R(R);
    out[0] = q.x;
    out[1] = q.y;
    out[2] = q.z;
    out[3] = q.w;
  }
};
struct OpNormalizeRot {
  static constexpr int kIn = 4, kOut = 4;
  __device__ static void run(const double* in, double* out) {
    Quat q = {in[0], in[1], in[2], in[3]};
    normalize_rotation(q);
    out[0] = q.x;
    out[1] = q.y;
    out[2] = q.z;
    out[3] = q.w;
  }
};
struct OpQuatRotate {  // q (4), v (3) -> q * v
  static constexpr int kIn = 7, kOut = 3;
  __device__ static void run(const double* in, double* out) {
    const Quat q = {in[0], in[1], in[2], in[3]};
    const double v[3] = {in[4], in[5], in[6]};
    double o[3];
    se3::quat_rotate(q, v, o);
    for (int i = 0; i < 3; i++) out[i] = o[i];
  }
};
struct OpQuatToR {
  static constexpr int kIn = 4, kOut = 9;
  __device__ static void run(const double* in, double* out) {
    const Quat q = {in[0], in[1], in[2], in[3]};
    double R[9];
    quat_to_R(q, R);
    for (int i = 0; i < 9; i++) out[i] = R[i];
  }
};
struct OpSim3Exp {
  static constexpr int kIn = 7, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double u[7], v[8];
    for (int i = 0; i < 7; i++) u[i] = in[i];
    sim3::sim3_store(sim3::sim3_exp(u), v);
    for (int i = 0; i < 8; i++) out[i] = v[i];
  }
};
struct OpSim3Log {
  static constexpr int kIn = 8, kOut = 7;
  __device__ static void run(const double* in, double* out) {
    double v[8], u[7];
    for (int i = 0; i < 8; i++) v[i] = in[i];
    sim3::sim3_log(sim3::sim3_load(v), u);
    for (int i = 0; i < 7; i++) out[i] = u[i];
  }
};
struct OpSim3Mul {
  static constexpr int kIn = 16, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double a[8], b[8], v[8];
    for (int i = 0; i < 8; i++) {
      a[i] = in[i];
      b[i] = in[8 + i];
    }
    sim3::sim3_store(sim3::sim3_mul(sim3::sim3_load(a), sim3::sim3_load(b)), v);
    for (int i = 0; i < 8; i++) out[i] = v[i];
  }
};
struct OpSim3Inv {
  static constexpr int kIn = 8, kOut = 8;
  __device__ static void run(const double* in, double* out) {
    double a[8], v[8];
    for (int i = 0; i < 8; i++) a[i] = in[i];
    sim3::sim3_store(sim3::sim3_inverse(sim3::sim3_load(a)), v);
    for (int i = 0; i < 8; i++) out[i] = v[i];
  }
};
struct OpSim3Affine {
  static constexpr int kIn = 8, kOut = 12;
  __device__ static void run(const double* in, double* out) {
    double a[8], M[12];
    for (int i = 0; i < 8; i++) a[i] = in[i];
    sim3::sim3_affine(sim3::sim3_load(a), M);
    for (int i = 0; i < 12; i++) out[i] = M[i];
  }
};
struct OpLu3 {  // W (9, row-major), b (3) -> x
  static constexpr int kIn = 12, kOut = 3;
  __device__ static void run(const double* in, double* out) {
    double W[9], b[3], x[3];
    for (int i = 0; i < 9; i++) W[i] = in[i];
    for (int i = 0; i < 3; i++) b[i] = in[9 + i];
    sim3::lu3_solve(W, b, x);
    for (int i = 0; i < 3; i++) out[i] = x[i];
  }
};
struct OpTriRc {
  static constexpr int kIn = 1, kOut = 2;
  __device__ static void run(const double* in, double* out) {
    int r, c;
    ba::tri_rc((int)in[0], r, c);
    out[0] = r;
    out[1] = c;
  }
};
struct OpDiagLdlt {  // A (21, packed lower), y (6) -> good, A, y, rdg
  static constexpr int kIn = 27, kOut = 34;
  __device__ static void run(const double* in, double* out) {
    double A[21], y[6], rdg[6];
    for (int i = 0; i < 21; i++) A[i] = in[i];
    for (int i = 0; i < 6; i++) y[i] = in[21 + i];
    out[0] = ba::diag_ldlt(A, y, rdg) ? 1.0 : 0.0;
    for (int i = 0; i < 21; i++) out[1 + i] = A[i];
    for (int i = 0; i < 6; i++) {
      out[22 + i] = y[i];
      out[28 + i] = rdg[i];
    }
  }
};
struct OpPanelRow {  // a (6), Ljj (15), rdg (6), yj (6), r -> v (6), l (6), r
  static constexpr int kIn = 34, kOut = 13;
  __device__ static void run(const double* in, double* out) {
    double a[6], Ljj[15], rdg[6], yj[6], v[6], l[6], r = in[33];
    for (int i = 0; i < 6; i++) {
      a[i] = in[i];
      rdg[i] = in[21 + i];
      yj[i] = in[27 + i];
    }
    for (int i = 0; i < 15; i++) Ljj[i] = in[6 + i];
    ba::panel_row(a, Ljj, rdg, yj, v, l, r);
    for (int i = 0; i < 6; i++) {
      out[i] = v[i];
      out[6 + i] = l[i];
    }
    out[12] = r;
  }
};
struct OpBlockBack6 {  // Lb (15), z (6) -> x
  static constexpr int kIn = 21, kOut = 6;
  __device__ static void run(const double* in, double* out) {
    double Lb[15], x[6];
    for (int i = 0; i < 15; i++) Lb[i] = in[i];
    for (int i = 0; i < 6; i++) x[i] = in[15 + i];
    ba::block_back6(Lb, x);
    for (int i = 0; i < 6; i++) out[i] = x[i];
  }
};
// factor_diag_block<double*, DenseRows> and load_strict_lower on block 1 of a 12x12 packed-lower
// factor storage: Lp (78), rhs (12) -> good, Lp (78), rhs (12), dg (12), idg (12), L (15). dg
// and idg start at the sentinel: only rows 6..11 may change.
struct OpFactorDiagBlock {
  static constexpr int kIn = 90, kOut = 130;
  __device__ static void run(const double* in, double* out) {
    double Lp[78], rhs[12], dg[12], idg[12], L[15];
    for (int i = 0; i < 78; i++) Lp[i] = in[i];
    for (int i = 0; i < 12; i++) {
      rhs[i] = in[78 + i];
      dg[i] = idg[i] = dmc::kSentinel;
    }
    double* lp = Lp;
    double* rp = rhs;
    double* dp = dg;
    double* ip = idg;
    out[0] = ba::factor_diag_block(lp, ba::DenseRows{}, rp, dp, ip, 6) ? 1.0 : 0.0;
    ba::load_strict_lower(lp, ba::DenseRows{}, 6, L);
    for (int i = 0; i < 78; i++) out[1 + i] = Lp[i];
    for (int i = 0; i < 12; i++) {
      out[79 + i] = rhs[i];
      out[91 + i] = dg[i];
      out[103 + i] = idg[i];
    }
    for (int i = 0; i < 15; i++) out[115 + i] = L[i];
  }
};
// The dense 6K x 6K factor-and-solve of ba_coop.hip's factor_solve, composed by one thread from
// ba_ldlt.h's pieces in factor_solve's order (diagonal block, panel rows, trailing update with
// block J + 1 factored right after its own update, z = D^-1 y, backward by blocks); the
// statements between the pieces are factor_solve's, with its contraction.
// K, S (171, packed lower, the first 3K (6K + 1) used), rhs (18) -> ok, x (18).
struct OpBlockSolve {
  static constexpr int kIn = 190, kOut = 19;
  __device__ static void run(const double* in, double* out) {
#pragma clang fp contract(fast)
    const int K = (int)in[0];
    for (int i = 0; i < kOut; i++) out[i] = 0.0;
    if (K < 1 || K > 3) return;
    const int n = 6 * K;
    double Lp[171], rhs[18], dg[18], idg[18], V[18 * 6];
    for (int i = 0; i < n * (n + 1) / 2; i++) Lp[i] = in[1 + i];
    for (int i = 0; i < n; i++) rhs[i] = in[172 + i];
    double* lp = Lp;
    double* rp = rhs;
    double* dp = dg;
    double* ip = idg;
    const ba::DenseRows rows;
    bool ok = ba::factor_diag_block(lp, rows, rp, dp, ip, 0);
    for (int J = 0; J < K && ok; J++) {
      const int j0 = 6 * J;
      double Ljj[15], rdg[6], yj[6];
      ba::load_strict_lower(lp, rows, j0, Ljj);
      for (int c = 0; c < 6; c++) {
        rdg[c] = idg[j0 + c];
        yj[c] = rhs[j0 + c];
      }
      for (int i = j0 + 6; i < n; i++) {
        const int ro = rows.off(i) + j0;
        double a[6], v[6], l[6];
        for (int c = 0; c < 6; c++) a[c] = Lp[ro + c];
        double r = rhs[i];
        ba::panel_row(a, Ljj, rdg, yj, v, l, r);
        for (int c = 0; c < 6; c++) {
          V[i * 6 + c] = v[c];
          Lp[ro + c] = l[c];
        }
        rhs[i] = r;
      }
      if (J + 1 < K) {
        for (int e = 0; e < 21; e++) {
          int r, c;
          ba::tri_rc(e, r, c);
          const int i = j0 + 6 + r, k = j0 + 6 + c, ro = ba::tri(i);
          double s = Lp[ro + k];
          for (int m = 0; m < 6; m++) s -= Lp[ro + j0 + m] * V[k * 6 + m];
          Lp[ro + k] = s;
        }
        ok = ba::factor_diag_block(lp, rows, rp, dp, ip, j0 + 6);
      }
      for (int i = j0 + 12; i < n; i++) {
        const int ro = ba::tri(i);
        for (int k = j0 + 6; k <= i; k++) {
          double s = Lp[ro + k];
          for (int c = 0; c < 6; c++) s -= Lp[ro + j0 + c] * V[k * 6 + c];
          Lp[ro + k] = s;
        }
      }
    }
    out[0] = ok ? 1.0 : 0.0;
    if (!ok) return;
    for (int i = 0; i < n; i++) rhs[i] /= dg[i];
    for (int J = K - 1; J >= 0; J--) {
      const int j0 = 6 * J;
      double Lb[15], x[6];
      ba::load_strict_lower(lp, rows, j0, Lb);
      for (int r = 0; r < 6; r++) x[r] = rhs[j0 + r];
      ba::block_back6(Lb, x);
      for (int r = 0; r < 6; r++) rhs[j0 + r] = x[r];
      for (int i = 0; i < j0; i++) {
        double sx = rhs[i];
        for (int c = 0; c < 6; c++) sx -= Lp[ba::tri(j0 + c) + i] * x[c];
        rhs[i] = sx;
      }
    }
    for (int i = 0; i < n; i++) out[1 + i] = rhs[i];
  }
};
// eval_edge with 8 levels of 1.2^-2l: xw (3), u, v, ur, octave, R (9), t (3), camera (fx, fy, cx,
// cy, bf) -> chi2, e (3), x, y, iz, stereo, info. The float fields arrive as doubles that hold
// float values.
struct OpEvalEdge {
  static constexpr int kIn = 24, kOut = 9;
  __device__ static void run(const double* in, double* out) {
    slamgpu_pose_edge E;
    for (int i = 0; i < 3; i++) E.xw[i] = (float)in[i];
    E.u = (float)in[3];
    E.v = (float)in[4];
    E.ur = (float)in[5];
    E.octave = (int32_t)in[6];
    PoseParams P;
    P.fx = (float)in[19];
    P.fy = (float)in[20];
    P.cx = (float)in[21];
    P.cy = (float)in[22];
    P.bf = (float)in[23];
    P.nlevels = 8;
    float s2 = 1.0f;
    for (int l = 0; l < 8; l++) {
      P.inv_sigma2[l] = 1.0f / s2;
      s2 *= 1.44f;
    }
    PassPose T;
    for (int i = 0; i < 9; i++) T.R[i] = in[7 + i];
    for (int i = 0; i < 3; i++) T.t[i] = in[16 + i];
    EdgeEval v;
    out[0] = eval_edge(E, P, P.inv_sigma2, T, v);
    out[1] = v.e[0];
    out[2] = v.e[1];
    out[3] = v.e[2];
    out[4] = v.x;
    out[5] = v.y;
    out[6] = v.iz;
    out[7] = v.stereo ? 1.0 : 0.0;
    out[8] = v.info;
  }
};

struct OpEntry {
  uint64_t op;
  int in, out;
  hipError_t (*run)(const double*, double*, int);
};
#define DMC_OP(id, T) {id, T::kIn, T::kOut, dmc::run_cases<T>}
const OpEntry kOps[] = {
    DMC_OP(dmc::kRcp, OpRcp),
    DMC_OP(dmc::kRsq, OpRsq),
    DMC_OP(dmc::kHuber, OpHuber),
    DMC_OP(dmc::kLdlt6, OpLdlt6),
    DMC_OP(dmc::kLeftUpdate, OpLeftUpdate),
    DMC_OP(dmc::kQuatFromR, OpQuatFromR),
    DMC_OP(dmc::kNormalizeRot, OpNormalizeRot),
    DMC_OP(dmc::kQuatRotate, OpQuatRotate),
    DMC_OP(dmc::kQuatToR, OpQuatToR),
    DMC_OP(dmc::kSim3Exp, OpSim3Exp),
    DMC_OP(dmc::kSim3Log, OpSim3Log),
    DMC_OP(dmc::kSim3Mul, OpSim3Mul),
    DMC_OP(dmc::kSim3Inv, OpSim3Inv),
    DMC_OP(dmc::kSim3Affine, OpSim3Affine),
    DMC_OP(dmc::kLu3, OpLu3),
    DMC_OP(dmc::kTriRc, OpTriRc),
    DMC_OP(dmc::kDiagLdlt, OpDiagLdlt),
    DMC_OP(dmc::kPanelRow, OpPanelRow),
    DMC_OP(dmc::kBlockBack6, OpBlockBack6),
    DMC_OP(dmc::kFactorDiagBlock, OpFactorDiagBlock),
    DMC_OP(dmc::kBlockSolve, OpBlockSolve),
    DMC_OP(dmc::kEvalEdge, OpEvalEdge),
    {dmc::kLdlt7, 36, 8, dmc::run_ldlt7},
    {dmc::kHuberSim3, 2, 2, dmc::run_huber_sim3},
    {dmc::kEgEdgeError, 24, 8, dmc::run_eg_edge_error},
    {dmc::kEgOplusAxis, 11, 8, dmc::run_eg_oplus_axis},
};
#undef DMC_OP

const OpEntry* find_op(uint64_t op) {
  for (const OpEntry& e : kOps)
    if (e.op == op) return &e;
  return nullptr;
}

struct Record {
  const OpEntry* op;
  uint64_t n;
  size_t in_at;  // index of the record's first input double in the file's words
};

[[noreturn]] void die(const char* what) {
  std::fprintf(stderr, "device_math_check: %s\n", what);
  std::exit(1);
}
void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    std::fprintf(stderr, "device_math_check: %s: %s\n", what, hipGetErrorString(e));
    std::exit(1);  // nothing more is started after an error
  }
}

}  // namespace
}  // namespace slamgpu

int main(int argc, char** argv) {
  using namespace slamgpu;
  if (argc != 3) die("usage: device_math_check in.bin out.bin");
  std::FILE* f = std::fopen(argv[1], "rb");
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
  // every count and size against the file length, before any launch
  if (w[0] != dmc::kMagic) die("bad magic");
  const uint64_t nrec = w[1];
  if (nrec > dmc::kMaxRecords) die("too many records");
  std::vector<Record> recs;
  size_t at = 2, out_words = 2;
  for (uint64_t r = 0; r < nrec; r++) {
    if (at + 4 > w.size()) die("truncated record header");
    const OpEntry* op = find_op(w[at]);
    if (!op) die("unknown operation");
    const uint64_t n = w[at + 1];
    if (n > dmc::kMaxCases) die("too many cases");
    if (w[at + 2] != (uint64_t)op->in || w[at + 3] != (uint64_t)op->out) die("case width");
    at += 4;
    const size_t need = (size_t)n * op->in;
    if (need > w.size() - at) die("truncated record");
    recs.push_back({op, n, at});
    at += need;
    out_words += 4 + (size_t)n * op->out;
  }
  if (at != w.size()) die("trailing bytes");

  std::vector<uint64_t> o(out_words);
  o[0] = dmc::kMagic;
  o[1] = nrec;
  size_t oat = 2;
  for (const Record& r : recs) {
    const size_t ib = (size_t)r.n * r.op->in * 8, ob = (size_t)r.n * r.op->out * 8;
    o[oat] = r.op->op;
    o[oat + 1] = r.n;
    o[oat + 2] = (uint64_t)r.op->in;
    o[oat + 3] = (uint64_t)r.op->out;
    oat += 4;
    if (r.n > 0) {
      double *d_in = nullptr, *d_out = nullptr;
      hip_ok(hipMalloc(&d_in, ib), "hipMalloc");
      hip_ok(hipMalloc(&d_out, ob), "hipMalloc");
      hip_ok(hipMemcpy(d_in, &w[r.in_at], ib, hipMemcpyHostToDevice), "copy in");
      hip_ok(hipMemset(d_out, 0, ob), "hipMemset");
      hip_ok(r.op->run(d_in, d_out, (int)r.n), "kernel");
      hip_ok(hipMemcpy(&o[oat], d_out, ob, hipMemcpyDeviceToHost), "copy out");
      hip_ok(hipFree(d_in), "hipFree");
      hip_ok(hipFree(d_out), "hipFree");
    }
    oat += (size_t)r.n * r.op->out;
  }
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) die("cannot open the output file");
  if (std::fwrite(o.data(), 8, o.size(), g) != o.size()) die("short write");
  if (std::fclose(g) != 0) die("close");
  return 0;
}
