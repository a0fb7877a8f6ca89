"""Builds tests/newpoints_ref.c on demand (gcc, the oracle Makefile's CFLAGS) and wraps it: the CPU
restatement of LocalMapper::CreateNewMapPoints' triangulation (local_mapper.cpp:332-490) and, with
the oracle's SearchForTriangulation (oracle/kfmatch_oracle.c), of the chain over the neighbour
keyframes that slamgpu_create_new_map_points is compared against bit for bit.

A keyframe is a dict: kps (KP_DTYPE), raw (KP_DTYPE or None), desc [n][32] u8, ur, depth f32 [n],
mp u8 [n], fv = (nodes, node_start, node_feats), T (4x4 f32 Tcw), Ow f32 [3], cam = (fx, fy, cx,
cy, mbf), mb."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "newpoints_ref.c")
LIB = os.path.join(HERE, "libnewpoints_ref.so")
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
FUSE_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"),
                             ("max_dist", "<f4"), ("skip", "<i4"), ("pad", "<i4", (3,)),
                             ("desc", "u1", (32,))])
NEW_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"),
                            ("source", "<i4")])
assert KP_DTYPE.itemsize == 28 and FUSE_POINT_DTYPE.itemsize == 80
MAX_FEATURES = 4096

DLT, STEREO1, STEREO2 = 1, 2, 3
W_ZERO, LOW_PARALLAX, BEHIND1, BEHIND2 = -1, -2, -3, -4
REPROJ1_STEREO, REPROJ1_MONO, REPROJ2_STEREO, REPROJ2_MONO = -5, -6, -7, -8
DIST_ZERO, SCALE, NO_DEPTH, MALFORMED = -9, -10, -11, -12


class Kf(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("kps", "raw_kps", "u_right", "depth", "desc")] + [
        ("n", C.c_int32), ("pad", C.c_int32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
        ("Ow", C.c_float * 3)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mbf", "mb")]


_lib = None


def _cflags():
    text = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS \?= (.*)$", text, re.M).group(1).split()


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *_cflags(), "-shared", "-o", tmp, SRC, "-lm"],
                   check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        vp, ip, fp, kp = C.c_void_p, C.c_int, C.c_float, C.POINTER(Kf)
        L.np_jacobi_sweeps.restype = ip
        for name in ("np_cos_stereo", "np_cos_stereo_libm"):
            getattr(L, name).argtypes = [fp, fp]
            getattr(L, name).restype = fp
        L.np_cos_stereo_many.argtypes = [fp, vp, ip, vp, vp]
        L.np_cos_stereo_many.restype = None
        L.np_dlt.argtypes = [kp, kp, ip, ip, ip, vp, vp]
        L.np_dlt.restype = None
        L.np_pair_one.argtypes = [kp, kp, ip, ip, vp, vp, ip, fp, ip, ip, ip, vp]
        L.np_pair_one.restype = ip
        L.np_pair.argtypes = [kp, kp, vp, ip, vp, vp, ip, fp, ip, ip, ip, vp, vp, vp, vp, vp]
        L.np_pair.restype = None
        _lib = L
    return _lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def jacobi_sweeps():
    return lib().np_jacobi_sweeps()


def cos_stereo(mb, depth):
    return np.float32(lib().np_cos_stereo(float(np.float32(mb)), float(np.float32(depth))))


def cos_stereo_libm(mb, depth):
    return np.float32(lib().np_cos_stereo_libm(float(np.float32(mb)), float(np.float32(depth))))


def cos_stereo_many(mb, depth):
    """(identity, libm) of np_cos_stereo over an array of depths."""
    d = np.ascontiguousarray(depth, np.float32)
    a, b = np.zeros(len(d), np.float32), np.zeros(len(d), np.float32)
    lib().np_cos_stereo_many(float(np.float32(mb)), ptr(d), len(d), ptr(a), ptr(b))
    return a, b


def c_kf(k):
    """(Kf, keep) of a keyframe dict."""
    kps = np.ascontiguousarray(k["kps"]).view(KP_DTYPE) if len(k["kps"]) else np.zeros(1, KP_DTYPE)
    raw = None if k.get("raw") is None else np.ascontiguousarray(k["raw"]).view(KP_DTYPE)
    ur = np.ascontiguousarray(k["ur"], np.float32)
    depth = np.ascontiguousarray(k["depth"], np.float32)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    s = Kf()
    s.kps, s.raw_kps, s.u_right, s.depth, s.desc = ptr(kps), ptr(raw), ptr(ur), ptr(depth), ptr(desc)
    s.n = len(desc)
    T = np.asarray(k["T"], np.float32)
    s.Rcw[:] = [float(x) for x in T[:3, :3].reshape(-1)]
    s.tcw[:] = [float(x) for x in T[:3, 3]]
    s.Ow[:] = [float(x) for x in np.asarray(k["Ow"], np.float32)]
    s.fx, s.fy, s.cx, s.cy, s.mbf = [float(np.float32(c)) for c in k["cam"]]
    s.mb = float(np.float32(k["mb"]))
    return s, [kps, raw, ur, depth, desc]


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def dlt(k1, k2, idx1, idx2, sweeps=None):
    """(A float 4x4, null vector in double) of one pair."""
    a, b = c_kf(k1), c_kf(k2)
    A, x = np.zeros(16, np.float32), np.zeros(4, np.float64)
    lib().np_dlt(C.byref(a[0]), C.byref(b[0]), idx1, idx2,
                 jacobi_sweeps() if sweeps is None else sweeps, ptr(A), ptr(x))
    return A.reshape(4, 4), x


def pair_one(k1, k2, idx1, idx2, scale, sigma2, first_obs=0, libm_cos=False, sweeps=None):
    """(status, FUSE_POINT record) of one pair."""
    a, b = c_kf(k1), c_kf(k2)
    sc, s2 = _f(scale), _f(sigma2)
    out = np.zeros(1, FUSE_POINT_DTYPE)
    sf = float(sc[1]) if len(sc) > 1 else float(sc[0])
    st = lib().np_pair_one(C.byref(a[0]), C.byref(b[0]), int(idx1), int(idx2), ptr(sc), ptr(s2),
                           len(sc), sf, int(first_obs), int(bool(libm_cos)),
                           jacobi_sweeps() if sweeps is None else int(sweeps), ptr(out))
    return st, out[0]


def pair(k1, k2, match12, neighbour, scale, sigma2, first_obs, points, news, n_new, has_mp1,
         libm_cos=False, sweeps=None):
    """One neighbour's triangulation; appends to points / news from n_new on and sets has_mp1.
    Returns (n_new, status[n1])."""
    a, b = c_kf(k1), c_kf(k2)
    sc, s2 = _f(scale), _f(sigma2)
    m = np.ascontiguousarray(match12, np.int32)
    status = np.zeros(max(a[0].n, 1), np.int8)
    nn = np.array([n_new], np.int32)
    sf = float(sc[1]) if len(sc) > 1 else float(sc[0])
    lib().np_pair(C.byref(a[0]), C.byref(b[0]), ptr(m), int(neighbour), ptr(sc), ptr(s2), len(sc),
                  sf, int(first_obs), int(bool(libm_cos)),
                  jacobi_sweeps() if sweeps is None else int(sweeps), ptr(points), ptr(news),
                  ptr(nn), ptr(status), ptr(has_mp1))
    return int(nn[0]), status[:a[0].n]


def newpoints_chain(cur, nbors, scale, sigma2, check_ori=True, libm_cos=False, sweeps=None):
    """The loop of local_mapper.cpp:284-491 over nbors = [dict(kf=, F12=, skip=, first_obs=)]:
    the oracle's SearchForTriangulation on the current has_mp, then the pair routine. Returns
    dict(n_new, points, news, status [len(nbors)][n1], has_mp1, matches); n_new = -1 (and nothing
    else defined past that neighbour) when a keyframe exceeds MAX_FEATURES."""
    import oracle_lib
    oracle_lib.build()
    n1 = len(cur["desc"])
    has_mp1 = np.ascontiguousarray(cur["mp"], np.uint8).copy()
    points = np.zeros(max(n1, 1), FUSE_POINT_DTYPE)
    news = np.zeros(max(n1, 1), NEW_POINT_DTYPE)
    status = np.zeros((len(nbors), max(n1, 1)), np.int8)
    matches = []
    n_new = 0
    for k, nb in enumerate(nbors):
        if nb["skip"]:
            matches.append(None)
            continue
        kf2 = nb["kf"]
        if n1 > MAX_FEATURES or len(kf2["desc"]) > MAX_FEATURES:
            n_new = -1
            break
        T2 = np.asarray(kf2["T"], np.float32)
        T2w = np.concatenate([T2[:3, :3].reshape(-1), T2[:3, 3]]).astype(np.float32)
        k1 = dict(cur, mp=has_mp1)
        _, m = oracle_lib.search_for_triangulation(k1, kf2, cur["Ow"], T2w, kf2["cam"][:4], scale,
                                                   sigma2, nb["F12"], False, check_ori)
        matches.append(m.copy())
        n_new, st = pair(cur, kf2, m, k, scale, sigma2, nb["first_obs"], points, news, n_new,
                         has_mp1, libm_cos, sweeps)
        status[k, :n1] = st
    n = max(n_new, 0)
    return dict(n_new=n_new, points=points[:n], news=news[:n], status=status[:, :n1],
                has_mp1=has_mp1, matches=matches)
