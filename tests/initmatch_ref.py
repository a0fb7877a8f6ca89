"""Builds tests/initmatch_ref.c on demand (gcc, the oracle Makefile's CFLAGS, linked against
oracle/liborb_oracle.so with an rpath) and wraps its call: the CPU restatement of
OrbMatcher::SearchForInitialization the device path is compared against bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from relocmatch_ref import _cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "initmatch_ref.c")
LIB = os.path.join(HERE, "libinitmatch_ref.so")  # not "initmatch_ref.so": import would load it

_lib = None


def build():
    O.build()
    deps = [SRC, os.path.join(O.ORACLE_DIR, "orb_oracle.h"), O.LIB_PATH]
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *_cflags(), "-shared", "-o", tmp, SRC,
                    "-L", O.ORACLE_DIR, "-l:liborb_oracle.so", "-Wl,-rpath,$ORIGIN/../oracle", "-lm"],
                   check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        build()
        O.lib()
        L = C.CDLL(LIB)
        vp, ip, fp = C.c_void_p, C.c_int, C.c_float
        L.ir_search_for_initialization.argtypes = [vp, vp, ip, C.POINTER(O.GridGeom), vp, ip, fp,
                                                   ip, ip, vp, vp, vp, vp]
        _lib = L
    return _lib


def search_for_initialization(kps2, desc2, grid, queries, nnratio, window_size, check_ori,
                              prev_matched):
    """kps2 / desc2: F2's undistorted keypoints and descriptors; queries: INIT_QUERY records of
    F1; prev_matched [n1][2] float32 (not modified). Returns (nmatches, matches12, prev_matched',
    accept_kp, dict(skipped, takeovers, removed, max_candidates))."""
    n2 = len(desc2)
    kps2 = np.ascontiguousarray(kps2).view(O.KP_DTYPE) if n2 else np.zeros(1, O.KP_DTYPE)
    desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32) if n2 else np.zeros((1, 32), np.uint8)
    q = np.ascontiguousarray(queries)
    assert q.dtype.itemsize == 64
    n1 = len(q)
    q = q if n1 else np.zeros(1, q.dtype)
    prev = np.ascontiguousarray(prev_matched, np.float32).reshape(-1, 2).copy()
    assert len(prev) == n1
    prev_buf = prev if n1 else np.zeros((1, 2), np.float32)
    m12, ak = np.zeros(max(n1, 1), np.int32), np.zeros(max(n1, 1), np.int32)
    cnt = np.zeros(4, np.int32)
    nm = lib().ir_search_for_initialization(
        O.ptr(kps2), O.ptr(desc2), n2, C.byref(grid), O.ptr(q), n1, float(np.float32(nnratio)),
        int(window_size), int(check_ori), O.ptr(prev_buf), O.ptr(m12), O.ptr(ak), O.ptr(cnt))
    return nm, m12[:n1], prev, ak[:n1], dict(skipped=int(cnt[0]), takeovers=int(cnt[1]),
                                              removed=int(cnt[2]), max_candidates=int(cnt[3]))
