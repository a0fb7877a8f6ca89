"""Build libslamgpu.so (HIP kernels + C++ runtime) in-tree for gfx950.

`python -m slam_framework_amd.build` or `__graft_entry__.build()`. hipcc cross-compiles without a
GPU. -ffp-contract=off keeps float results bit-identical to the reference's expression-by-
expression semantics (explicit fmaf() only where the reference's Release build fuses).
"""
from __future__ import annotations

import glob
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libslamgpu.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("SLAMGPU_ARCH", "gfx950")

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", f"--offload-arch={ARCH}",
         "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))
    deps += glob.glob(os.path.join(os.path.dirname(PKG), "include", "*.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        build_capi_check()
        build_adapter_check()
        build_geometry_check()
        build_host_stage_check()
        build_sim3solver_adapter_check()
        build_pnpsolver_adapter_check()
        build_initializer_adapter_check()
        build_reloc_adapter_check()
        build_initmatch_adapter_check()
        build_newpoints_adapter_check()
        build_kfdb_adapter_check()
        build_device_math_check()
        build_eg_step_check()
        return LIB
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    procs, objs = [], []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        cmd = [HIPCC, *FLAGS, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = []
    for src, p in procs:
        out = p.communicate()[0].decode(errors="replace")
        if p.returncode != 0:
            failed.append(f"{src}:\n{out}")
        elif verbose and out.strip():
            print(out, file=sys.stderr)
    if failed:
        raise RuntimeError("hipcc failed:\n" + "\n".join(failed))
    tmp = LIB + ".tmp"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp, *objs, "-lz"],
                   check=True)
    os.replace(tmp, LIB)
    build_capi_check()
    build_adapter_check()
    build_geometry_check()
    build_host_stage_check()
    build_sim3solver_adapter_check()
    build_pnpsolver_adapter_check()
    build_initializer_adapter_check()
    build_reloc_adapter_check()
    build_initmatch_adapter_check()
    build_newpoints_adapter_check()
    build_kfdb_adapter_check()
    build_device_math_check()
    build_eg_step_check()
    return LIB


ROOT = os.path.dirname(PKG)
CAPI_SRC = os.path.join(ROOT, "tests", "capi_check.cpp")
CAPI_BIN = os.path.join(ROOT, "tests", "capi_check")
CAPI_KF_SRC = os.path.join(ROOT, "tests", "capi_kf_check.cpp")
CAPI_KF_BIN = os.path.join(ROOT, "tests", "capi_kf_check")


def build_capi_check() -> str:
    """g++ builds of tests/capi_check.cpp and tests/capi_kf_check.cpp against include/*.h*,
    linked to libslamgpu.so: the C++ caller side of the drop-in boundary, with no HIP or Python
    in between."""
    headers = glob.glob(os.path.join(ROOT, "include", "*.h*"))
    for src, exe in ((CAPI_SRC, CAPI_BIN), (CAPI_KF_SRC, CAPI_KF_BIN)):
        if os.path.exists(exe) and os.path.getmtime(exe) >= max(
                os.path.getmtime(d) for d in [src, LIB] + headers):
            continue
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                        src, "-L", PKG, "-lslamgpu",
                        "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", exe], check=True)
    return CAPI_BIN


ADAPTER_SRC = os.path.join(ROOT, "tests", "adapter_check.cpp")
ADAPTER_BIN = os.path.join(ROOT, "tests", "adapter_check")


def build_adapter_check() -> str:
    """g++ build of tests/adapter_check.cpp: include/slamgpu_adapters.hpp (the OpenCV-free graph
    gathering of the reference-side adapters) compiled and driven on the CPU."""
    deps = [ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(ADAPTER_BIN) and os.path.getmtime(ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", ADAPTER_BIN], check=True)
    return ADAPTER_BIN


SIM3SOLVER_ADAPTER_SRC = os.path.join(ROOT, "tests", "sim3solver_adapter_check.cpp")
SIM3SOLVER_ADAPTER_BIN = os.path.join(ROOT, "tests", "sim3solver_adapter_check")


def build_sim3solver_adapter_check() -> str:
    """g++ build of tests/sim3solver_adapter_check.cpp: Sim3SolverCore of
    include/slamgpu_adapters.hpp (the gather, the eager draws, the iterate / find replay) driven
    from C++ against libslamgpu.so."""
    deps = [SIM3SOLVER_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(SIM3SOLVER_ADAPTER_BIN) and os.path.getmtime(SIM3SOLVER_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return SIM3SOLVER_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), SIM3SOLVER_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", SIM3SOLVER_ADAPTER_BIN],
                   check=True)
    return SIM3SOLVER_ADAPTER_BIN


PNPSOLVER_ADAPTER_SRC = os.path.join(ROOT, "tests", "pnpsolver_adapter_check.cpp")
PNPSOLVER_ADAPTER_BIN = os.path.join(ROOT, "tests", "pnpsolver_adapter_check")


def build_pnpsolver_adapter_check() -> str:
    """g++ build of tests/pnpsolver_adapter_check.cpp: PnPSolverCore of
    include/slamgpu_adapters.hpp (the gather, the eager draws, the iterate / find replay with its
    schedule extension) driven from C++ against libslamgpu.so."""
    deps = [PNPSOLVER_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(PNPSOLVER_ADAPTER_BIN) and os.path.getmtime(PNPSOLVER_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return PNPSOLVER_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), PNPSOLVER_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", PNPSOLVER_ADAPTER_BIN],
                   check=True)
    return PNPSOLVER_ADAPTER_BIN


INITIALIZER_ADAPTER_SRC = os.path.join(ROOT, "tests", "initializer_adapter_check.cpp")
INITIALIZER_ADAPTER_BIN = os.path.join(ROOT, "tests", "initializer_adapter_check")


def build_initializer_adapter_check() -> str:
    """g++ build of tests/initializer_adapter_check.cpp: InitializerCore of
    include/slamgpu_adapters.hpp (the eager draws after SeedRandOnce(0), the one device call, the
    replay of the ReconstructH / ReconstructF tails) driven from C++ against libslamgpu.so."""
    deps = [INITIALIZER_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(INITIALIZER_ADAPTER_BIN) and os.path.getmtime(INITIALIZER_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return INITIALIZER_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), INITIALIZER_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", INITIALIZER_ADAPTER_BIN],
                   check=True)
    return INITIALIZER_ADAPTER_BIN


RELOC_ADAPTER_SRC = os.path.join(ROOT, "tests", "reloc_adapter_check.cpp")
RELOC_ADAPTER_BIN = os.path.join(ROOT, "tests", "reloc_adapter_check")


def build_reloc_adapter_check() -> str:
    """g++ build of tests/reloc_adapter_check.cpp: relocalization_refine of
    include/slamgpu_adapters.hpp (PoseOptimization and the two relocalisation searches of
    tracker.cpp:924-975 on the frame the context holds) driven from C++ against libslamgpu.so."""
    deps = [RELOC_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(RELOC_ADAPTER_BIN) and os.path.getmtime(RELOC_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return RELOC_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), RELOC_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", RELOC_ADAPTER_BIN],
                   check=True)
    return RELOC_ADAPTER_BIN


INITMATCH_ADAPTER_SRC = os.path.join(ROOT, "tests", "initmatch_adapter_check.cpp")
INITMATCH_ADAPTER_BIN = os.path.join(ROOT, "tests", "initmatch_adapter_check")


def build_initmatch_adapter_check() -> str:
    """g++ build of tests/initmatch_adapter_check.cpp: slamgpu_frame_mono and
    search_for_initialization of include/slamgpu_adapters.hpp (the first two calls of
    Tracker::MonocularInitialization, tracker.cpp:297-364) driven from C++ against libslamgpu.so."""
    deps = [INITMATCH_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(INITMATCH_ADAPTER_BIN) and os.path.getmtime(INITMATCH_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return INITMATCH_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), INITMATCH_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", INITMATCH_ADAPTER_BIN],
                   check=True)
    return INITMATCH_ADAPTER_BIN


NEWPOINTS_ADAPTER_SRC = os.path.join(ROOT, "tests", "newpoints_adapter_check.cpp")
NEWPOINTS_ADAPTER_BIN = os.path.join(ROOT, "tests", "newpoints_adapter_check")


def build_newpoints_adapter_check() -> str:
    """g++ build of tests/newpoints_adapter_check.cpp: compute_fundamental_matrix and
    create_new_map_points of include/slamgpu_adapters.hpp (LocalMapper::CreateNewMapPoints,
    local_mapper.cpp:258-492: the baseline tests, the one device call, the NewPoint actions)
    driven from C++ against libslamgpu.so."""
    deps = [NEWPOINTS_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(NEWPOINTS_ADAPTER_BIN) and os.path.getmtime(NEWPOINTS_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return NEWPOINTS_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), NEWPOINTS_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", NEWPOINTS_ADAPTER_BIN],
                   check=True)
    return NEWPOINTS_ADAPTER_BIN


KFDB_ADAPTER_SRC = os.path.join(ROOT, "tests", "kfdb_adapter_check.cpp")
KFDB_ADAPTER_BIN = os.path.join(ROOT, "tests", "kfdb_adapter_check")


def build_kfdb_adapter_check() -> str:
    """g++ build of tests/kfdb_adapter_check.cpp: gather_detect_loop_candidates and
    LoopDetectorCore of include/slamgpu_adapters.hpp (LoopCloser::DetectLoop's consistency groups,
    loop_closer.cpp:194-297, around the database query) driven from C++ on the CPU."""
    deps = [KFDB_ADAPTER_SRC, LIB] + glob.glob(os.path.join(ROOT, "include", "*.h*"))
    if os.path.exists(KFDB_ADAPTER_BIN) and os.path.getmtime(KFDB_ADAPTER_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return KFDB_ADAPTER_BIN
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I",
                    os.path.join(ROOT, "include"), KFDB_ADAPTER_SRC, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", KFDB_ADAPTER_BIN],
                   check=True)
    return KFDB_ADAPTER_BIN


GEOMETRY_SRC = os.path.join(ROOT, "tests", "geometry_check.cpp")
GEOMETRY_BIN = os.path.join(ROOT, "tests", "geometry_check")


def build_geometry_check() -> str:
    """Host-only hipcc build (orb_geometry.h includes hip_runtime.h) of tests/geometry_check.cpp +
    csrc/orb_geometry.cpp: compute_geometry / build_cells printed as JSON, no device code and no
    libslamgpu.so. Same -ffp-contract=off as the library."""
    geo = os.path.join(CSRC, "orb_geometry.cpp")
    deps = [GEOMETRY_SRC, geo] + glob.glob(os.path.join(CSRC, "orb_*.h"))
    if os.path.exists(GEOMETRY_BIN) and os.path.getmtime(GEOMETRY_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return GEOMETRY_BIN
    tmp = GEOMETRY_BIN + ".tmp"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-I", CSRC, GEOMETRY_SRC, geo, "-o", tmp],
                   check=True)
    os.replace(tmp, GEOMETRY_BIN)
    return GEOMETRY_BIN


HOST_STAGE_SRC = os.path.join(ROOT, "tests", "host_stage_check.cpp")
HOST_STAGE_BIN = os.path.join(ROOT, "tests", "host_stage_check")


def build_host_stage_check() -> str:
    """g++ build of tests/host_stage_check.cpp with the address and undefined-behaviour
    sanitizers: csrc/stage_layout.h (the staging layouts of every synchronous wrapper and the
    FeatureVector validator, HIP-free) walked on the CPU, no libslamgpu.so. The sanitizer
    runtimes are linked statically: the program runs as it is, whatever else is preloaded."""
    deps = [HOST_STAGE_SRC, os.path.join(CSRC, "stage_layout.h"),
            os.path.join(CSRC, "host_common.h")] + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if os.path.exists(HOST_STAGE_BIN) and os.path.getmtime(HOST_STAGE_BIN) >= max(
            os.path.getmtime(d) for d in deps):
        return HOST_STAGE_BIN
    tmp = HOST_STAGE_BIN + ".tmp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", CSRC,
                    HOST_STAGE_SRC, "-o", tmp], check=True)
    os.replace(tmp, HOST_STAGE_BIN)
    return HOST_STAGE_BIN


def _build_device_harness(exe: str, srcs, deps) -> str:
    """hipcc build, with the library's own FLAGS, of a stand-alone program under tests/ that
    includes library .hip files and links libslamgpu.so; skipped while `exe` is no older than any
    of `deps`."""
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    tmp = exe + ".tmp"
    subprocess.run([HIPCC, *FLAGS, *srcs, "-L", PKG, "-lslamgpu",
                    "-Wl,-rpath,$ORIGIN/../slam_framework_amd", "-o", tmp], check=True)
    os.replace(tmp, exe)
    return exe


DEVICE_MATH_SRCS = [os.path.join(ROOT, "tests", n) for n in (
    "device_math_check.hip", "device_math_check_sim3.hip", "device_math_check_eg.hip")]
DEVICE_MATH_BIN = os.path.join(ROOT, "tests", "device_math_check")


def build_device_math_check() -> str:
    """hipcc build of tests/device_math_check*.hip with the library's own FLAGS: a stand-alone
    program that includes pose_kernels.hip, sim3_kernels.hip, eg_kernels.hip and the device
    headers (one translation unit per .hip) and runs their helpers one case per thread. Linked to
    libslamgpu.so only for the symbols the included launchers refer to."""
    deps = DEVICE_MATH_SRCS + [os.path.join(ROOT, "tests", "device_math_check.h"), LIB]
    deps += glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))
    deps += glob.glob(os.path.join(ROOT, "include", "*.h"))
    return _build_device_harness(DEVICE_MATH_BIN, DEVICE_MATH_SRCS, deps)


EG_STEP_SRC = os.path.join(ROOT, "tests", "eg_step_check.hip")
EG_STEP_BIN = os.path.join(ROOT, "tests", "eg_step_check")


def build_eg_step_check():
    """hipcc build of tests/eg_step_check.hip with the library's own FLAGS: a stand-alone program
    that includes eg_kernels.hip and csrc/eg_structure.h and runs one linear step of
    OptimizeEssentialGraph (products, assembly, both factor-solve variants) and the small kernels
    around it on given graphs. Linked to libslamgpu.so only for the symbols the included
    launchers refer to. The program belongs to the tests: in a tree that does not hold its source
    there is nothing to build and None is returned (the tests that run it assert that it exists)."""
    if not os.path.exists(EG_STEP_SRC):
        return None
    deps = [EG_STEP_SRC, LIB] + glob.glob(os.path.join(CSRC, "*.h"))
    deps += [os.path.join(CSRC, "eg_kernels.hip")] + glob.glob(os.path.join(ROOT, "include", "*.h"))
    return _build_device_harness(EG_STEP_BIN, [EG_STEP_SRC], deps)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
