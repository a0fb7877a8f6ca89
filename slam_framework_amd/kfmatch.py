"""The LocalMapper's keyframe-rate matchers on the device: ctypes binding of
include/slamgpu_kfmatch.h with reference-shaped names.

  search_for_triangulation   OrbMatcher::SearchForTriangulation (orb_matcher.cpp:634-802)
  fuse                       OrbMatcher::Fuse(pKF, vpMapPoints, th) (orb_matcher.cpp:804-954),
                             the candidate search; fuse_apply is the reference's sequential
                             Replace / AddObservation walk over its result
and of include/slamgpu_loopmatch.h, the LoopCloser's three Sim3 matchers:
  search_by_sim3             OrbMatcher::SearchBySim3 (orb_matcher.cpp:1081-1310)
  search_by_projection_sim3  OrbMatcher::SearchByProjection(pKF, Scw, ...) (:384-497)
  fuse_sim3                  OrbMatcher::Fuse(pKF, Scw, ...) (:956-1079), the candidate search;
                             fuse_sim3_apply is the reference's per-point tail (:1061-1075)
  create_new_map_points      LocalMapper::CreateNewMapPoints (local_mapper.cpp:258-492): the chain
                             over the neighbours, search and triangulation, in one device call;
                             compute_fundamental_matrix is its ComputeFundamentalMatrix (:615-630)
libslamgpu.so is the only compute path (no CPU fallback); errors raise SlamGpuError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import slamgpu as G

MAX_FEATURES = 4096
TH_LOW = 50

FUSE_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"),
                             ("max_dist", "<f4"), ("skip", "<i4"), ("pad", "<i4", (3,)),
                             ("desc", "u1", (32,))])
TRI_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("F12", "<f4", (9,)),
                           ("only_stereo", "<i4")])
# slamgpu_kf with device addresses (the *_device calls)
KF_DTYPE = np.dtype([("kps", "<u8"), ("desc", "<u8"), ("u_right", "<u8"), ("has_mp", "<u8"),
                     ("nodes", "<u8"), ("node_start", "<u8"), ("node_feats", "<u8"),
                     ("n", "<i4"), ("n_nodes", "<i4"), ("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)),
                     ("Ow", "<f4", (3,)), ("pad", "<f4")])
SBP_JOB_DTYPE = np.dtype([("kf", "<i4"), ("pt_begin", "<i4"), ("n_pts", "<i4"),
                          ("kp_begin", "<i4")])
SIM3_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("mp1_begin", "<i4"),
                            ("mp2_begin", "<i4"), ("sR12", "<f4", (9,)), ("t12", "<f4", (3,)),
                            ("sR21", "<f4", (9,)), ("t21", "<f4", (3,))])
assert FUSE_POINT_DTYPE.itemsize == 80 and TRI_PAIR_DTYPE.itemsize == 48
assert SBP_JOB_DTYPE.itemsize == 16 and SIM3_PAIR_DTYPE.itemsize == 112
assert KF_DTYPE.itemsize == 128
# CreateNewMapPoints: slamgpu_kf_stereo (device addresses), slamgpu_newpoints_nbor / _job,
# slamgpu_new_point
KF_STEREO_DTYPE = np.dtype([("depth", "<u8"), ("raw_kps", "<u8"), ("cam", "<f4", (5,)),
                            ("mb", "<f4")])
NP_NBOR_DTYPE = np.dtype([("kf2", "<i4"), ("F12", "<f4", (9,)), ("skip", "<i4"),
                          ("first_obs", "<i4")])
NP_JOB_DTYPE = np.dtype([("kf1", "<i4"), ("first_nbor", "<i4"), ("n_nbors", "<i4"),
                         ("pad", "<i4"), ("has_mp1", "<u8")])
NEW_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"),
                            ("source", "<i4")])
assert KF_STEREO_DTYPE.itemsize == 40 and NP_NBOR_DTYPE.itemsize == 48
assert NP_JOB_DTYPE.itemsize == 24 and NEW_POINT_DTYPE.itemsize == 16
# per-keypoint status of one neighbour (SLAMGPU_NP_*)
NP_DLT, NP_STEREO1, NP_STEREO2 = 1, 2, 3
NP_W_ZERO, NP_LOW_PARALLAX, NP_BEHIND1, NP_BEHIND2 = -1, -2, -3, -4
NP_REPROJ1_STEREO, NP_REPROJ1_MONO, NP_REPROJ2_STEREO, NP_REPROJ2_MONO = -5, -6, -7, -8
NP_DIST_ZERO, NP_SCALE, NP_NO_DEPTH, NP_MALFORMED = -9, -10, -11, -12


class Levels(C.Structure):
    """slamgpu_levels: a KeyFrame's per-level tables."""
    _fields_ = [("nlevels", C.c_int32), ("log_scale_factor", C.c_float),
                ("scale", C.c_float * 32), ("sigma2", C.c_float * 32),
                ("inv_sigma2", C.c_float * 32)]


class KfGrid(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("min_x", "max_x", "min_y", "max_y", "cell_w", "cell_h")]


class Kf(C.Structure):
    """slamgpu_kf (host pointers in the synchronous calls)."""
    _fields_ = [(n, C.c_void_p) for n in ("kps", "desc", "u_right", "has_mp", "nodes",
                                          "node_start", "node_feats")] + [
        ("n", C.c_int32), ("n_nodes", C.c_int32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
        ("Ow", C.c_float * 3), ("pad", C.c_float)]


class KfStereo(C.Structure):
    """slamgpu_kf_stereo (host pointers in the synchronous call)."""
    _fields_ = [("depth", C.c_void_p), ("raw_kps", C.c_void_p), ("cam", G.Camera),
                ("mb", C.c_float)]


class NewPointsNbor(C.Structure):
    _fields_ = [("kf2", C.c_int32), ("F12", C.c_float * 9), ("skip", C.c_int32),
                ("first_obs", C.c_int32)]


def levels(scale_factor=1.2, nlevels=8):
    """The extractor's tables as KeyFrame copies them (orb_extractor.cpp:357-369, f32; log via
    the float std::log of Frame)."""
    lv = Levels()
    lv.nlevels = nlevels
    sf = np.float32(scale_factor)
    lv.log_scale_factor = float(np.float32(np.log(np.float64(sf))))
    sc = np.float32(1.0)
    for i in range(nlevels):
        if i:
            sc = np.float32(float(sc) * float(np.float32(scale_factor)))
        lv.scale[i] = float(sc)
        s2 = np.float32(sc * sc)
        lv.sigma2[i] = float(s2)
        lv.inv_sigma2[i] = float(np.float32(1.0) / s2)
    return lv


def kf_grid(cols, rows):
    """KeyFrame::min_x_ .. max_y_ and the 64 x 48 cell sizes of an undistorted cols x rows
    image (Frame::ComputeImageBounds k1 == 0, frame.cpp:223-224)."""
    return KfGrid(0.0, float(int(cols)), 0.0, float(int(rows)),
                  float(np.float32(cols) / np.float32(64)), float(np.float32(rows) / np.float32(48)))


_bound = False


def lib():
    global _bound
    L = G.lib()
    if not _bound:
        vp, ip = C.c_void_p, C.c_int
        L.slamgpu_kfmatch_last_error.argtypes = []
        L.slamgpu_kfmatch_last_error.restype = C.c_char_p
        L.slamgpu_search_for_triangulation.argtypes = [
            C.POINTER(Kf), C.POINTER(Kf), vp, C.POINTER(G.Camera), C.POINTER(Levels), ip, ip, vp,
            C.POINTER(ip)]
        L.slamgpu_search_for_triangulation_device.argtypes = [
            vp, vp, ip, C.POINTER(G.Camera), C.POINTER(Levels), ip, vp, C.c_int64, vp, vp]
        L.slamgpu_fuse.argtypes = [C.POINTER(Kf), vp, ip, C.c_float, C.POINTER(G.Camera),
                                   C.POINTER(Levels), C.POINTER(KfGrid), vp, vp, C.POINTER(ip)]
        L.slamgpu_fuse_device.argtypes = [vp, vp, vp, ip, C.c_float, C.POINTER(G.Camera),
                                          C.POINTER(Levels), C.POINTER(KfGrid), vp, vp, vp]
        L.slamgpu_create_new_map_points_scratch_bytes.argtypes = [ip, ip]
        L.slamgpu_create_new_map_points_scratch_bytes.restype = C.c_size_t
        L.slamgpu_create_new_map_points_device.argtypes = [
            vp, vp, vp, ip, vp, ip, C.POINTER(G.Camera), C.POINTER(Levels), ip, vp, vp, vp,
            C.c_int64, vp, C.c_int64, vp, C.c_size_t, vp]
        L.slamgpu_create_new_map_points.argtypes = [
            C.POINTER(Kf), C.POINTER(KfStereo), C.POINTER(NewPointsNbor), ip, C.POINTER(G.Camera),
            C.POINTER(Levels), ip, vp, vp, vp, vp, C.POINTER(ip)]
        cp, lp, gp, fl = C.POINTER(G.Camera), C.POINTER(Levels), C.POINTER(KfGrid), C.c_float
        L.slamgpu_loopmatch_last_error.argtypes = []
        L.slamgpu_loopmatch_last_error.restype = C.c_char_p
        L.slamgpu_fuse_sim3.argtypes = [C.POINTER(Kf), vp, ip, fl, cp, lp, gp, vp, vp,
                                        C.POINTER(ip)]
        L.slamgpu_fuse_sim3_device.argtypes = [vp, ip, vp, ip, vp, fl, cp, lp, gp, vp, vp, vp]
        L.slamgpu_search_by_projection_sim3.argtypes = [C.POINTER(Kf), vp, ip, vp, fl, cp, lp, gp,
                                                        vp, vp, C.POINTER(ip)]
        L.slamgpu_search_by_projection_sim3_scratch_bytes.argtypes = [ip]
        L.slamgpu_search_by_projection_sim3_scratch_bytes.restype = C.c_size_t
        L.slamgpu_search_by_projection_sim3_device.argtypes = [
            vp, vp, ip, vp, ip, ip, vp, ip, fl, cp, lp, gp, vp, vp, vp, vp, C.c_size_t, vp]
        L.slamgpu_search_by_sim3.argtypes = [C.POINTER(Kf), C.POINTER(Kf), vp, vp, vp, vp, vp, vp,
                                             vp, vp, fl, cp, lp, gp, vp, vp, vp, C.POINTER(ip)]
        L.slamgpu_search_by_sim3_device.argtypes = [vp, vp, ip, vp, ip, vp, vp, C.c_int64, fl, cp,
                                                    lp, gp, vp, vp, vp, vp, vp]
        _bound = True
    return L


def _check(rc):
    if rc != 0:
        raise G.SlamGpuError(f"slamgpu error {rc}: {lib().slamgpu_kfmatch_last_error().decode()}")


_p = G._ptr


def _cam(cam):
    return G.Camera(*[float(np.float32(c)) for c in cam])


def host_kf(kps, desc, u_right, Tcw, has_mp=None, feature_vec=None):
    """A slamgpu_kf over host arrays (kept alive in the returned tuple). Tcw: 4x4 f32 pose;
    Ow = -R^T t as the caller's KeyFrame holds it (pass Ow explicitly via .Ow to override)."""
    k = np.ascontiguousarray(kps)
    if len(k) and k.dtype != G.KP_DTYPE:
        k = k.view(G.KP_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    ur = np.ascontiguousarray(u_right, np.float32)
    mp = None if has_mp is None else np.ascontiguousarray(has_mp, np.uint8)
    keep = [k, d, ur, mp]
    s = Kf()
    s.kps, s.desc, s.u_right, s.has_mp = _p(k), _p(d), _p(ur), _p(mp)
    s.n = len(d)
    if feature_vec is not None:
        nodes, start, feats = (np.ascontiguousarray(a, t) for a, t in zip(
            feature_vec.arrays(), (np.uint32, np.int32, np.uint32)))
        keep += [nodes, start, feats]
        s.nodes, s.node_start, s.node_feats = _p(nodes), _p(start), _p(feats)
        s.n_nodes = len(nodes)
    T = np.asarray(Tcw, np.float32)
    R, t = T[:3, :3], T[:3, 3]
    s.Rcw[:] = [float(x) for x in R.reshape(-1)]
    s.tcw[:] = [float(x) for x in t]
    s.Ow[:] = [float(x) for x in camera_center(T)]
    return s, keep


def camera_center(Tcw):
    """KeyFrame::SetPose's Ow = -Rcw^T tcw in float cv::Mat arithmetic (OpenCV gemm: float dot
    products added in double, as matcher_oracle.c restates Rcw * X + tcw)."""
    T = np.asarray(Tcw, np.float32)
    Rt = T[:3, :3].T
    t = T[:3, 3]
    out = np.zeros(3, np.float32)
    for r in range(3):
        dot = np.float32(np.float32(Rt[r, 0] * t[0]) + np.float32(Rt[r, 1] * t[1]))
        dot = np.float32(dot + np.float32(Rt[r, 2] * t[2]))
        out[r] = np.float32(-dot)
    return out


def search_for_triangulation(kf1, kf2, F12, cam, lv, only_stereo=False, check_ori=True):
    """kf1 / kf2: (Kf, keep) from host_kf (with has_mp and feature_vec). Returns (nmatches,
    match12) with match12[i] = vMatches12[i]."""
    s1, s2 = kf1[0], kf2[0]
    F = np.ascontiguousarray(F12, np.float32).reshape(9)
    m = np.full(max(s1.n, 1), -1, np.int32)
    nm = C.c_int()
    _check(lib().slamgpu_search_for_triangulation(C.byref(s1), C.byref(s2), _p(F),
                                                  C.byref(_cam(cam)), C.byref(lv),
                                                  int(bool(only_stereo)), int(bool(check_ori)),
                                                  _p(m), C.byref(nm)))
    return nm.value, m[:s1.n]


def search_for_triangulation_device(d_kfs, d_pairs, n_pairs, cam, lv, check_ori, d_match,
                                    match_stride, d_nmatches, stream=None):
    from .bow import _dev
    _check(lib().slamgpu_search_for_triangulation_device(
        _dev(d_kfs), _dev(d_pairs), n_pairs, C.byref(_cam(cam)), C.byref(lv),
        int(bool(check_ori)), _dev(d_match), match_stride, _dev(d_nmatches),
        C.c_void_p(stream or 0)))


def fuse(kf, points, th, cam, lv, grid):
    """kf: (Kf, keep) from host_kf; points: FUSE_POINT_DTYPE. Returns (nfused, best_idx,
    best_dist)."""
    pts = np.ascontiguousarray(points).view(FUSE_POINT_DTYPE)
    n = len(pts)
    bi, bd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nf = C.c_int()
    _check(lib().slamgpu_fuse(C.byref(kf[0]), _p(pts), n, float(th), C.byref(_cam(cam)),
                              C.byref(lv), C.byref(grid), _p(bi), _p(bd), C.byref(nf)))
    return nf.value, bi[:n], bd[:n]


def fuse_device(d_kfs, d_pts, d_point_kf, n_pts, th, cam, lv, grid, d_best_idx, d_best_dist,
                stream=None):
    from .bow import _dev
    _check(lib().slamgpu_fuse_device(_dev(d_kfs), _dev(d_pts), _dev(d_point_kf), n_pts, float(th),
                                     C.byref(_cam(cam)), C.byref(lv), C.byref(grid),
                                     _dev(d_best_idx), _dev(d_best_dist), C.c_void_p(stream or 0)))


# ---- CreateNewMapPoints ------------------------------------------------------------------------
def _mat3(a, b):
    """cv::Mat product of two 3 x 3 float matrices: double sums over ascending k, rounded once."""
    out = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += float(a[i, k]) * float(b[k, j])
            out[i, j] = np.float32(acc)
    return out


def compute_fundamental_matrix(Tcw1, Tcw2, cam1, cam2):
    """LocalMapper::ComputeFundamentalMatrix (local_mapper.cpp:615-630) under the cv::Mat rules of
    DESIGN.md "CreateNewMapPoints": R12 = R1w * R2w.t(); t12 = -R1w * R2w.t() * t2w + t1w;
    F12 = K1.t().inv() * t12x * R12 * K2.inv(), every product left to right as written, the two
    inverses in the closed (cofactor) form in double, rounded once. Bit for bit what
    compute_fundamental_matrix of include/slamgpu_adapters.hpp gives.
    cam = (fx, fy, cx, cy, ...). Returns 3 x 3 f32."""
    T1, T2 = np.asarray(Tcw1, np.float32), np.asarray(Tcw2, np.float32)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    R2t = np.ascontiguousarray(R2.T)
    R12 = _mat3(R1, R2t)
    nR1 = (-R1).astype(np.float32)
    m = _mat3(nR1, R2t)
    t12 = np.zeros(3, np.float32)
    for i in range(3):
        acc = 0.0
        for k in range(3):
            acc += float(m[i, k]) * float(t2[k])
        t12[i] = np.float32(np.float32(acc) + t1[i])
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], np.float32)

    def kmat(c):
        fx, fy, cx, cy = [np.float32(v) for v in c[:4]]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)

    def inv3(m):
        a = [float(v) for v in m.reshape(-1)]
        det = (a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
               a[2] * (a[3] * a[7] - a[4] * a[6]))
        cof = [a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
               a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
               a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
        return np.array([np.float32(c / det) for c in cof], np.float32).reshape(3, 3)
    K1ti = inv3(np.ascontiguousarray(kmat(cam1).T))
    return _mat3(_mat3(_mat3(K1ti, tx), R12), inv3(kmat(cam2)))


def host_kf_stereo(depth, cam, mb, raw_kps=None):
    """A slamgpu_kf_stereo over host arrays (kept alive in the returned tuple). cam = (fx, fy, cx,
    cy, mbf) of this keyframe."""
    d = np.ascontiguousarray(depth, np.float32)
    raw = None
    if raw_kps is not None:
        raw = np.ascontiguousarray(raw_kps)
        raw = raw if raw.dtype == G.KP_DTYPE else raw.view(G.KP_DTYPE)
    s = KfStereo()
    s.depth, s.raw_kps, s.cam, s.mb = _p(d), _p(raw), _cam(cam), float(np.float32(mb))
    return s, [d, raw]


def create_new_map_points(cur, cur_stereo, nbors, cam, lv, check_ori=True):
    """cur / cur_stereo: (Kf, keep) from host_kf (with has_mp and feature_vec) and host_kf_stereo.
    nbors: [(kf, kf_stereo, F12, skip, first_obs)] in GetBestCovisibilityKeyFrames order; skip =
    the baseline test of local_mapper.cpp:290-304 failed. cam: the neighbours' fx, fy, cx, cy.
    Returns (n_new, points FUSE_POINT_DTYPE, news NEW_POINT_DTYPE, status [len(nbors)][n1] i8,
    has_mp1 u8 [n1] after the call); n_new = -1 when a search reported -1."""
    n1, nn = cur[0].n, len(nbors)
    kfs = (Kf * (1 + nn))(cur[0], *[b[0][0] for b in nbors])
    sts = (KfStereo * (1 + nn))(cur_stereo[0], *[b[1][0] for b in nbors])
    hn = (NewPointsNbor * max(nn, 1))()
    for k, b in enumerate(nbors):
        hn[k].kf2 = 1 + k
        hn[k].F12[:] = [float(x) for x in np.asarray(b[2], np.float32).reshape(9)]
        hn[k].skip, hn[k].first_obs = int(bool(b[3])), int(b[4])
    has_mp1 = np.zeros(max(n1, 1), np.uint8)
    if n1:
        has_mp1[:n1] = np.ctypeslib.as_array(C.cast(cur[0].has_mp, C.POINTER(C.c_uint8)), (n1,))
    points = np.zeros(max(n1, 1), FUSE_POINT_DTYPE)
    news = np.zeros(max(n1, 1), NEW_POINT_DTYPE)
    status = np.zeros((max(nn, 1), max(n1, 1)), np.int8)
    out = C.c_int()
    _check(lib().slamgpu_create_new_map_points(kfs, sts, hn, nn, C.byref(_cam(cam)), C.byref(lv),
                                               int(bool(check_ori)), _p(has_mp1), _p(points),
                                               _p(news), _p(status), C.byref(out)))
    n = max(out.value, 0)
    st = status.reshape(-1)[:nn * n1].reshape(nn, n1)
    return out.value, points[:n], news[:n], st, has_mp1[:n1]


def create_new_map_points_scratch_bytes(n_jobs, max_nbors):
    return int(lib().slamgpu_create_new_map_points_scratch_bytes(int(n_jobs), int(max_nbors)))


def create_new_map_points_device(d_kfs, d_kf_stereo, d_jobs, n_jobs, d_nbors, max_nbors, cam, lv,
                                 check_ori, d_n_new, d_points, d_new, point_stride, d_status,
                                 status_stride, d_scratch, scratch_bytes, stream=None):
    """Every job's chain on `stream`, no synchronisation (include/slamgpu_kfmatch.h)."""
    from .bow import _dev
    _check(lib().slamgpu_create_new_map_points_device(
        _dev(d_kfs), _dev(d_kf_stereo), _dev(d_jobs), n_jobs, _dev(d_nbors), max_nbors,
        C.byref(_cam(cam)), C.byref(lv), int(bool(check_ori)), _dev(d_n_new), _dev(d_points),
        _dev(d_new), point_stride, _dev(d_status), status_stride, _dev(d_scratch), scratch_bytes,
        C.c_void_p(stream or 0)))


def fuse_apply(best_idx, kf_map_points, mp_ids, mp_nobs, mp_bad, mp_in_kf):
    """The reference's walk over Fuse's result (orb_matcher.cpp:821-951) on an id-based map:
    kf_map_points[j] = map point id of keypoint j (-1 none), mp_ids[i] = id of offered point i,
    mp_nobs / mp_bad / mp_in_kf indexed by id (mutated). Replace(a -> b) moves a's keyframe slot
    to b and marks a bad. Returns nFused."""
    nfused = 0
    for i, mid in enumerate(mp_ids):
        if mid < 0 or mp_bad[mid] or mp_in_kf[mid] or best_idx[i] < 0:
            continue
        j = int(best_idx[i])
        cur = int(kf_map_points[j])
        if cur >= 0:
            if not mp_bad[cur]:
                keep, drop = (cur, mid) if mp_nobs[cur] > mp_nobs[mid] else (mid, cur)
                mp_bad[drop] = True
                mp_nobs[keep] += mp_nobs[drop]
                kf_map_points[kf_map_points == drop] = keep
                mp_in_kf[keep] = True
        else:
            mp_nobs[mid] += 1
            mp_in_kf[mid] = True
            kf_map_points[j] = mid
        nfused += 1
    return nfused


# ---- the LoopCloser's Sim3 matchers (include/slamgpu_loopmatch.h) ------------------------------
TH_HIGH = 100
SBP_KEEP = 3  # SLAMGPU_SBP_KEEP
_f32 = np.float32


def host_kf_pose(kps, desc, Rcw, tcw, Ow):
    """A slamgpu_kf over host arrays with the pose blocks given as such (the decomposed Scw of
    the two Scw calls): no u_right, has_mp or FeatureVector, which the Sim3 matchers never read."""
    k = np.ascontiguousarray(kps)
    if len(k) and k.dtype != G.KP_DTYPE:
        k = k.view(G.KP_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    s = Kf()
    s.kps, s.desc, s.n = _p(k), _p(d), len(d)
    s.Rcw[:] = [float(x) for x in np.asarray(Rcw, np.float32).reshape(-1)]
    s.tcw[:] = [float(x) for x in np.asarray(tcw, np.float32).reshape(-1)]
    s.Ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(-1)]
    return s, [k, d]


def decompose_scw(Scw):
    """Rcw, tcw, Ow of a 4x4 f32 Scw in the reference's operation order (orb_matcher.cpp:393-397,
    :965-969) under OpenCV's float cv::Mat arithmetic: scw = (float)sqrt(row0 . row0) (Mat::dot,
    a double sum), Rcw = sRcw / scw and tcw = Scw[:3, 3] / scw as a multiplication by the float
    1/scw (MatExpr scaling), Ow = -Rcw^T tcw (camera_center). A convenience for Python callers
    and tests: the C ABI takes the blocks as the caller's own arithmetic made them."""
    S = np.asarray(Scw, np.float32)
    r0 = S[0, :3].astype(np.float64)
    scw = _f32(np.sqrt(float(r0[0] * r0[0]) + float(r0[1] * r0[1]) + float(r0[2] * r0[2])))
    inv = _f32(1.0 / float(scw))
    Rcw = (S[:3, :3] * inv).astype(np.float32)
    tcw = (S[:3, 3] * inv).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = Rcw, tcw
    return Rcw, tcw, camera_center(T)


def relative_sim3(s12, R12, t12):
    """sR12, t12, sR21, t21 as SearchBySim3 computes them (orb_matcher.cpp:1103-1105): sR12 =
    s12 * R12, sR21 = (1.0 / s12) * R12^T (scalings by a float factor), t21 = -sR21 * t12
    (OpenCV gemm: float dot products, negated)."""
    R = np.asarray(R12, np.float32).reshape(3, 3)
    t = np.asarray(t12, np.float32).reshape(3)
    s = _f32(s12)
    sR12 = (R * s).astype(np.float32)
    sR21 = (R.T * _f32(1.0 / float(s))).astype(np.float32)
    t21 = np.zeros(3, np.float32)
    for r in range(3):
        dot = _f32(_f32(sR21[r, 0] * t[0]) + _f32(sR21[r, 1] * t[1]))
        t21[r] = -_f32(dot + _f32(sR21[r, 2] * t[2]))
    return sR12, t.copy(), sR21, t21


def fuse_sim3(kf, points, th, cam, lv, grid):
    """kf: (Kf, keep) from host_kf_pose(decompose_scw(Scw)); points: FUSE_POINT_DTYPE with skip =
    isBad() or already in the keyframe. Returns (nfused, best_idx, best_dist)."""
    pts = np.ascontiguousarray(points).view(FUSE_POINT_DTYPE)
    n = len(pts)
    bi, bd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nf = C.c_int()
    _check(lib().slamgpu_fuse_sim3(C.byref(kf[0]), _p(pts), n, float(th), C.byref(_cam(cam)),
                                   C.byref(lv), C.byref(grid), _p(bi), _p(bd), C.byref(nf)))
    return nf.value, bi[:n], bd[:n]


def fuse_sim3_device(d_kfs, n_kfs, d_pts, n_pts, d_skip, th, cam, lv, grid, d_best_idx,
                     d_best_dist, stream=None):
    """n_kfs keyframes x one shared point array; d_skip [n_kfs][n_pts] u8 or None; outputs
    [n_kfs][n_pts]."""
    from .bow import _dev
    _check(lib().slamgpu_fuse_sim3_device(
        _dev(d_kfs), n_kfs, _dev(d_pts), n_pts, _dev(d_skip) if d_skip is not None else None,
        float(th), C.byref(_cam(cam)), C.byref(lv), C.byref(grid), _dev(d_best_idx),
        _dev(d_best_dist), C.c_void_p(stream or 0)))


def search_by_projection_sim3(kf, points, matched_in, th, cam, lv, grid):
    """matched_in[idx] = vpMatched[idx] != nullptr at entry. Returns (nmatches, kp_point,
    point_kp): kp_point[idx] = the point that claimed keypoint idx or -1."""
    pts = np.ascontiguousarray(points).view(FUSE_POINT_DTYPE)
    n, m = kf[0].n, len(pts)
    mi = np.ascontiguousarray(matched_in, np.uint8)
    if len(mi) != n:
        raise G.SlamGpuError(f"matched_in has {len(mi)} entries for {n} keypoints")
    kpp, pkp = np.zeros(max(n, 1), np.int32), np.zeros(max(m, 1), np.int32)
    nm = C.c_int()
    _check(lib().slamgpu_search_by_projection_sim3(
        C.byref(kf[0]), _p(pts), m, _p(mi), float(th), C.byref(_cam(cam)), C.byref(lv),
        C.byref(grid), _p(kpp), _p(pkp), C.byref(nm)))
    return nm.value, kpp[:n], pkp[:m]


def search_by_projection_sim3_scratch_bytes(n_pts_total):
    return int(lib().slamgpu_search_by_projection_sim3_scratch_bytes(int(n_pts_total)))


def search_by_projection_sim3_device(d_kfs, d_pts, n_pts_total, d_jobs, n_jobs, max_job_pts,
                                     d_matched_in, n_kp_total, th, cam, lv, grid, d_kp_point,
                                     d_point_kp, d_nmatches, d_scratch, scratch_bytes,
                                     stream=None):
    from .bow import _dev
    _check(lib().slamgpu_search_by_projection_sim3_device(
        _dev(d_kfs), _dev(d_pts), n_pts_total, _dev(d_jobs), n_jobs, max_job_pts,
        _dev(d_matched_in), n_kp_total, float(th), C.byref(_cam(cam)), C.byref(lv), C.byref(grid),
        _dev(d_kp_point), _dev(d_point_kp), _dev(d_nmatches), _dev(d_scratch), scratch_bytes,
        C.c_void_p(stream or 0)))


def search_by_sim3(kf1, kf2, mp1, mp2, already1, already2, sim3, th, cam, lv, grid):
    """kf1 / kf2: (Kf, keep) with Rcw / tcw = the keyframes' poses; mp1 / mp2: one
    FUSE_POINT_DTYPE record per feature (skip = no map point or bad); sim3 = (sR12, t12, sR21,
    t21) (relative_sim3). Returns (nfound, match12, vn_match1, vn_match2)."""
    p1 = np.ascontiguousarray(mp1).view(FUSE_POINT_DTYPE)
    p2 = np.ascontiguousarray(mp2).view(FUSE_POINT_DTYPE)
    n1, n2 = kf1[0].n, kf2[0].n
    a1, a2 = np.ascontiguousarray(already1, np.uint8), np.ascontiguousarray(already2, np.uint8)
    if (len(p1), len(a1), len(p2), len(a2)) != (n1, n1, n2, n2):
        raise G.SlamGpuError("search_by_sim3: one map point record and one flag per feature")
    blocks = [np.ascontiguousarray(b, np.float32).reshape(-1) for b in sim3]
    m12, v1 = np.zeros(max(n1, 1), np.int32), np.zeros(max(n1, 1), np.int32)
    v2 = np.zeros(max(n2, 1), np.int32)
    nf = C.c_int()
    _check(lib().slamgpu_search_by_sim3(
        C.byref(kf1[0]), C.byref(kf2[0]), _p(p1), _p(p2), _p(a1), _p(a2), _p(blocks[0]),
        _p(blocks[1]), _p(blocks[2]), _p(blocks[3]), float(th), C.byref(_cam(cam)), C.byref(lv),
        C.byref(grid), _p(m12), _p(v1), _p(v2), C.byref(nf)))
    return nf.value, m12[:n1], v1[:n1], v2[:n2]


def search_by_sim3_device(d_kfs, d_mp, n_mp_total, d_pairs, n_pairs, d_already1, d_already2,
                          stride, th, cam, lv, grid, d_match12, d_vn_match1, d_vn_match2,
                          d_nfound, stream=None):
    from .bow import _dev
    _check(lib().slamgpu_search_by_sim3_device(
        _dev(d_kfs), _dev(d_mp), n_mp_total, _dev(d_pairs), n_pairs, _dev(d_already1),
        _dev(d_already2), stride, float(th), C.byref(_cam(cam)), C.byref(lv), C.byref(grid),
        _dev(d_match12), _dev(d_vn_match1), _dev(d_vn_match2), _dev(d_nfound),
        C.c_void_p(stream or 0)))


def fuse_sim3_apply(best_idx, kf_map_points, mp_ids, mp_nobs, mp_bad, mp_in_kf):
    """The reference's per-point tail of Fuse(pKF, Scw, ...) (orb_matcher.cpp:1061-1075) over the
    candidate search's result, on an id-based map (arrays as fuse_apply; kf_map_points, mp_nobs
    and mp_in_kf are mutated). "Bad" and "already in this keyframe" are re-checked here: in a
    SearchAndFuse batch the Replace calls after an earlier keyframe can have added observations
    to a loop point since the search ran. Returns (nFused, vpReplacePoint as ids, -1 = none)."""
    replace = np.full(len(mp_ids), -1, np.int64)
    nfused = 0
    for i, mid in enumerate(mp_ids):
        if mid < 0 or mp_bad[mid] or mp_in_kf[mid] or best_idx[i] < 0:
            continue
        j = int(best_idx[i])
        cur = int(kf_map_points[j])
        if cur >= 0:
            if not mp_bad[cur]:
                replace[i] = cur
        else:
            mp_nobs[mid] += 1
            mp_in_kf[mid] = True
            kf_map_points[j] = mid
        nfused += 1
    return nfused, replace
