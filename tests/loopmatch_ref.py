"""Builds tests/loopmatch_ref.c on demand (gcc, the oracle Makefile's CFLAGS, linked against
oracle/liborb_oracle.so with an rpath) and wraps its three calls: the CPU restatement of the
LoopCloser's Sim3 matchers the device paths are compared against bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "loopmatch_ref.c")
LIB = os.path.join(HERE, "libloopmatch_ref.so")  # not "loopmatch_ref.so": import would load it

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
        gp = C.POINTER(O.GridGeom)
        L.lr_fuse_sim3.argtypes = [vp, vp, ip, gp, vp, vp, vp, fp, fp, fp, fp, vp, ip, fp, vp, ip,
                                   fp, vp, vp]
        L.lr_search_by_projection_sim3.argtypes = [vp, vp, ip, gp, vp, vp, vp, fp, fp, fp, fp, vp,
                                                   ip, fp, vp, ip, vp, fp, vp, vp, vp]
        L.lr_search_by_sim3.argtypes = [vp, vp, ip, vp, vp, ip, gp, vp, vp, vp, vp, vp, vp, vp, vp,
                                        vp, vp, fp, fp, fp, fp, vp, ip, fp, fp, vp, vp, vp]
        _lib = L
    return _lib


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def _kf(k):
    kps = np.ascontiguousarray(k["kps"]).view(O.KP_DTYPE) if len(k["kps"]) else \
        np.zeros(1, O.KP_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    return kps, desc if len(desc) else np.zeros((1, 32), np.uint8), len(k["desc"])


def _cam4(cam):
    return [float(np.float32(c)) for c in cam[:4]]


def fuse_sim3(k, grid, Rcw, tcw, Ow, cam, scale, log_scale_factor, points, th):
    """k = dict(kps, desc). Returns (nfused, best_idx, best_dist)."""
    kps, desc, n = _kf(k)
    keep = [_f(Rcw), _f(tcw), _f(Ow), _f(scale)]
    pts = np.ascontiguousarray(points)
    m = len(pts)
    bi, bd = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
    nf = lib().lr_fuse_sim3(O.ptr(kps), O.ptr(desc), n, C.byref(grid), O.ptr(keep[0]),
                            O.ptr(keep[1]), O.ptr(keep[2]), *_cam4(cam), O.ptr(keep[3]),
                            len(keep[3]), float(log_scale_factor), O.ptr(pts), m, float(th),
                            O.ptr(bi), O.ptr(bd))
    return nf, bi[:m], bd[:m]


def search_by_projection_sim3(k, grid, Rcw, tcw, Ow, cam, scale, log_scale_factor, points,
                              matched_in, th):
    """Returns (nmatches, kp_point, point_kp, passed_over)."""
    kps, desc, n = _kf(k)
    keep = [_f(Rcw), _f(tcw), _f(Ow), _f(scale)]
    pts = np.ascontiguousarray(points)
    m = len(pts)
    mi = np.ascontiguousarray(matched_in, np.uint8)
    mi = mi if len(mi) else np.zeros(1, np.uint8)
    kpp = np.zeros(max(n, 1), np.int32)
    pkp, po = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
    nm = lib().lr_search_by_projection_sim3(
        O.ptr(kps), O.ptr(desc), n, C.byref(grid), O.ptr(keep[0]), O.ptr(keep[1]), O.ptr(keep[2]),
        *_cam4(cam), O.ptr(keep[3]), len(keep[3]), float(log_scale_factor), O.ptr(pts), m,
        O.ptr(mi), float(th), O.ptr(kpp), O.ptr(pkp), O.ptr(po))
    return nm, kpp[:n], pkp[:m], po[:m]


def search_by_sim3(k1, k2, grid, T1, T2, mp1, mp2, already1, already2, sR12, t12, sR21, t21, cam,
                   scale, log_scale_factor, th):
    """T1 / T2: 4x4 f32 poses of the keyframes. Returns (nfound, match12, vn_match1, vn_match2)."""
    a, da, n1 = _kf(k1)
    b, db, n2 = _kf(k2)
    Tw = [np.concatenate([np.asarray(T, np.float32)[:3, :3].reshape(-1),
                          np.asarray(T, np.float32)[:3, 3]]) for T in (T1, T2)]
    keep = [_f(Tw[0]), _f(Tw[1]), _f(sR12), _f(t12), _f(sR21), _f(t21), _f(scale)]
    p1, p2 = np.ascontiguousarray(mp1), np.ascontiguousarray(mp2)
    a1 = np.ascontiguousarray(already1, np.uint8)
    a2 = np.ascontiguousarray(already2, np.uint8)
    a1 = a1 if len(a1) else np.zeros(1, np.uint8)
    a2 = a2 if len(a2) else np.zeros(1, np.uint8)
    m12, v1 = np.zeros(max(n1, 1), np.int32), np.zeros(max(n1, 1), np.int32)
    v2 = np.zeros(max(n2, 1), np.int32)
    nf = lib().lr_search_by_sim3(
        O.ptr(a), O.ptr(da), n1, O.ptr(b), O.ptr(db), n2, C.byref(grid), O.ptr(keep[0]),
        O.ptr(keep[1]), O.ptr(p1), O.ptr(p2), O.ptr(a1), O.ptr(a2), O.ptr(keep[2]),
        O.ptr(keep[3]), O.ptr(keep[4]), O.ptr(keep[5]), *_cam4(cam), O.ptr(keep[6]), len(keep[6]),
        float(log_scale_factor), float(th), O.ptr(m12), O.ptr(v1), O.ptr(v2))
    return nf, m12[:n1], v1[:n1], v2[:n2]
