"""Builds tests/relocmatch_ref.c on demand (gcc, the oracle Makefile's CFLAGS, linked against
oracle/liborb_oracle.so with an rpath) and wraps its call: the CPU restatement of the
relocalisation SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) the device path is
compared against bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "relocmatch_ref.c")
LIB = os.path.join(HERE, "librelocmatch_ref.so")  # not "relocmatch_ref.so": import would load it

_lib = None


def _cflags():
    text = open(os.path.join(O.ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS \?= (.*)$", text, re.M).group(1).split()


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
        L.rr_search_by_projection_reloc.argtypes = [
            vp, vp, ip, C.POINTER(O.GridGeom), fp, fp, fp, fp, vp, ip, fp, vp, vp, vp, fp, ip, ip,
            vp, ip, vp, vp, vp, vp]
        _lib = L
    return _lib


def logf(x):
    """std::log(float) as the oracle states it (glibc's logf)."""
    return float(np.float32(O._kf_lib().oc_logf(float(np.float32(x)))))


def search_by_projection_reloc(kps, desc, grid, cam, scale, log_scale_factor, queries, pose,
                               map_point):
    """queries: RELOC_QUERY records, pose: one RELOC_POSE record, map_point: the frame's slots
    (int32, -1 = none), not modified. Returns (nmatches, map_point', query_kp, passed_over,
    n_removed)."""
    kps = np.ascontiguousarray(kps).view(O.KP_DTYPE) if len(kps) else np.zeros(1, O.KP_DTYPE)
    n = len(desc)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    desc = desc if n else np.zeros((1, 32), np.uint8)
    q = np.ascontiguousarray(queries)
    assert q.dtype.itemsize == 64
    m = len(q)
    q = q if m else np.zeros(1, q.dtype)
    p = np.atleast_1d(pose)[0]
    keep = [np.ascontiguousarray(p[k], np.float32).reshape(-1) for k in ("Rcw", "tcw", "Ow")]
    sc = np.ascontiguousarray(scale, np.float32)
    mp = np.ascontiguousarray(map_point, np.int32).copy()
    assert len(mp) == n
    mp_buf = mp if n else np.zeros(1, np.int32)
    qk, po = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
    rem = np.zeros(1, np.int32)
    fx, fy, cx, cy = [float(np.float32(c)) for c in cam[:4]]
    nm = lib().rr_search_by_projection_reloc(
        O.ptr(kps), O.ptr(desc), n, C.byref(grid), fx, fy, cx, cy, O.ptr(sc), len(sc),
        float(np.float32(log_scale_factor)), O.ptr(keep[0]), O.ptr(keep[1]), O.ptr(keep[2]),
        float(p["th"]), int(p["orb_dist"]), int(p["check_ori"]), O.ptr(q), m, O.ptr(mp_buf),
        O.ptr(qk), O.ptr(po), O.ptr(rem))
    return nm, mp, qk[:m], po[:m], int(rem[0])
