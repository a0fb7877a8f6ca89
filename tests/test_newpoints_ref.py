"""The CPU restatement of CreateNewMapPoints' triangulation (tests/newpoints_ref.c) without a GPU.

  - A second, independent statement of local_mapper.cpp:335-485 in numpy scalars (py_pair below;
    only the 4 x 4 null vector is taken from the C) agrees with the C bit for bit on every matched
    pair of the scenes.
  - Every comparison of :340-470 is pinned by a constructed pair: the input just inside and the
    adjacent float32 input just outside, found by bisection over the float32 ordinals where the
    value is not constructed exactly; the expected status follows from the cited line, evaluated
    by py_pair's intermediates.
  - Geometry, the cos identity, the chain, the descriptor rule and the sanitizers as DESIGN.md
    "CreateNewMapPoints" records them."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import newpoints_ref as R
import newpoints_scenario as NS

f32 = np.float32
SC, S2 = NS.levels_arrays()
SCENES = [("mono", 51), ("stereo", 52), ("mixed", 53)]


# ---- exact float32 helpers -------------------------------------------------------------------------

def rnd32(fr):
    """The float32 nearest to the Fraction fr, ties to even."""
    d = f32(float(fr))
    cands = [np.nextafter(d, f32(-np.inf)), d, np.nextafter(d, f32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(c.view(np.uint32)) & 1))
    return best


def fmaf(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return f32(float(a) * float(b) + float(c))
    return rnd32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def ordinal(x):
    b = int(f32(x).view(np.int32))
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def from_ordinal(o):
    return np.int32(o).view(f32) if o >= 0 else np.uint32(0x80000000 | -o).view(f32)


def bisect_flip(fn, lo, hi):
    """Adjacent float32 a, b between lo and hi with fn(a) == fn(lo) != fn(b) == fn(hi)."""
    a, b = ordinal(lo), ordinal(hi)
    fa, fb = fn(from_ordinal(a)), fn(from_ordinal(b))
    assert fa != fb, (fa, fb)
    step = 1 if b > a else -1
    while abs(b - a) > 1:
        m = (a + b) // 2
        if fn(from_ordinal(m)) == fa:
            a = m
        else:
            b = m
    assert abs(b - a) == 1 and step
    return from_ordinal(a), from_ordinal(b)


# ---- the numpy statement of local_mapper.cpp:335-485 -----------------------------------------------

def dot3(a, b):
    acc = 0.0
    for k in range(3):
        acc += float(a[k]) * float(b[k])
    return acc


def py_pair(k1, k2, i, j, first_obs=0):
    """(status, intermediates, point) of one pair; every float line as the reference writes it."""
    q = {}
    kp1, kp2 = k1["kps"][i], k2["kps"][j]
    ur1, ur2 = f32(k1["ur"][i]), f32(k2["ur"][j])
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    fx1, fy1, cx1, cy1, mbf1 = [f32(c) for c in k1["cam"]]
    fx2, fy2, cx2, cy2, _ = [f32(c) for c in k2["cam"]]
    T1, T2 = np.asarray(k1["T"], f32), np.asarray(k2["T"], f32)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    O1, O2 = np.asarray(k1["Ow"], f32), np.asarray(k2["Ow"], f32)
    one = f32(1)
    xn1 = [(kp1["x"] - cx1) * (one / fx1), (kp1["y"] - cy1) * (one / fy1), one]
    xn2 = [(kp2["x"] - cx2) * (one / fx2), (kp2["y"] - cy2) * (one / fy2), one]
    ray1 = [f32(dot3(R1[:, c], xn1)) for c in range(3)]
    ray2 = [f32(dot3(R2[:, c], xn2)) for c in range(3)]
    den = math.sqrt(dot3(ray1, ray1)) * math.sqrt(dot3(ray2, ray2))
    cosRays = f32(dot3(ray1, ray2) / den) if den != 0 and den == den else f32(np.nan)

    def cos_stereo(mb, d):
        h = f32(mb) / f32(2)
        hh, dd = float(h) * float(h), float(d) * float(d)
        return f32((dd - hh) / (dd + hh)) if dd + hh != 0 else f32(np.nan)
    cosSt1 = cosSt2 = cosRays + one
    if st1:
        cosSt1 = cos_stereo(k1["mb"], k1["depth"][i])
    elif st2:
        cosSt2 = cos_stereo(k2["mb"], k2["depth"][j])
    cosSt = min(cosSt1, cosSt2) if not (cosSt2 != cosSt2 or cosSt1 != cosSt1) else (
        cosSt2 if cosSt2 < cosSt1 else cosSt1)
    q.update(st1=st1, st2=st2, cosRays=cosRays, cosSt1=cosSt1, cosSt2=cosSt2, cosSt=cosSt)

    def unproject(k, idx):
        z = f32(k["depth"][idx])
        if not z > 0:
            return None
        fx, fy, cx, cy, _ = [f32(c) for c in k["cam"]]
        raw = k["kps"] if k.get("raw") is None else k["raw"]
        c = [(raw[idx]["x"] - cx) * z * (one / fx), (raw[idx]["y"] - cy) * z * (one / fy), z]
        Rk = np.asarray(k["T"], f32)[:3, :3]
        return np.array([f32(dot3(Rk[:, a], c)) + f32(k["Ow"][a]) for a in range(3)], f32)

    if cosRays < cosSt and cosRays > 0 and (st1 or st2 or float(cosRays) < 0.9998):
        A, xd = R.dlt(k1, k2, i, j)
        rows = [[xn1[0] * T1[2, c] - T1[0, c] for c in range(4)],
                [xn1[1] * T1[2, c] - T1[1, c] for c in range(4)],
                [xn2[0] * T2[2, c] - T2[0, c] for c in range(4)],
                [xn2[1] * T2[2, c] - T2[1, c] for c in range(4)]]
        assert np.array_equal(np.array(rows, f32), A, equal_nan=True)
        x = xd.astype(f32)
        q["w"] = x[3]
        if x[3] == 0:
            return R.W_ZERO, q, None
        s = f32(1.0 / float(x[3]))
        x3D = np.array([x[0] * s, x[1] * s, x[2] * s], f32)
        source = R.DLT
    elif st1 and cosSt1 < cosSt2:
        x3D, source = unproject(k1, i), R.STEREO1
    elif st2 and cosSt2 < cosSt1:
        x3D, source = unproject(k2, j), R.STEREO2
    else:
        return R.LOW_PARALLAX, q, None
    if x3D is None:
        return R.NO_DEPTH, q, None
    q["x3D"] = x3D
    z1 = f32(dot3(R1[2], x3D) + float(t1[2]))
    q["z1"] = z1
    if z1 <= 0:
        return R.BEHIND1, q, None
    z2 = f32(dot3(R2[2], x3D) + float(t2[2]))
    q["z2"] = z2
    if z2 <= 0:
        return R.BEHIND2, q, None
    sig1 = f32(S2[kp1["octave"]])
    x1, y1 = f32(dot3(R1[0], x3D) + float(t1[0])), f32(dot3(R1[1], x3D) + float(t1[1]))
    u1, v1 = (fx1 * x1) / z1 + cx1, (fy1 * y1) / z1 + cy1
    ex, ey = u1 - kp1["x"], v1 - kp1["y"]
    if st1:
        er = (u1 - (mbf1 / z1)) - ur1
        q["e1"], q["sig1"] = fmaf(er, er, fmaf(ex, ex, ey * ey)), sig1
        if float(q["e1"]) > 7.8 * float(sig1):
            return R.REPROJ1_STEREO, q, None
    else:
        q["e1"], q["sig1"] = fmaf(ex, ex, ey * ey), sig1
        if float(q["e1"]) > 5.991 * float(sig1):
            return R.REPROJ1_MONO, q, None
    sig2 = f32(S2[kp2["octave"]])
    x2, y2 = f32(dot3(R2[0], x3D) + float(t2[0])), f32(dot3(R2[1], x3D) + float(t2[1]))
    u2, v2 = (fx2 * x2) / z2 + cx2, (fy2 * y2) / z2 + cy2
    ex, ey = u2 - kp2["x"], v2 - kp2["y"]
    if st2:
        er = (u2 - (mbf1 / z2)) - ur2
        q["e2"], q["sig2"] = fmaf(er, er, fmaf(ex, ex, ey * ey)), sig2
        if q["e2"] > f32(7.8) * sig2:
            return R.REPROJ2_STEREO, q, None
    else:
        q["e2"], q["sig2"] = fmaf(ex, ex, ey * ey), sig2
        if float(q["e2"]) > 5.991 * float(sig2):
            return R.REPROJ2_MONO, q, None
    n1, n2 = x3D - O1, x3D - O2
    nd1, nd2 = math.sqrt(dot3(n1, n1)), math.sqrt(dot3(n2, n2))
    dist1, dist2 = f32(nd1), f32(nd2)
    q.update(dist1=dist1, dist2=dist2)
    if dist1 == 0 or dist2 == 0:
        return R.DIST_ZERO, q, None
    ratioDist = dist2 / dist1
    ratioFactor = f32(1.5) * SC[1]
    ratioOctave = SC[kp1["octave"]] / SC[kp2["octave"]]
    q.update(lo=ratioDist * ratioFactor, hi=ratioDist / ratioFactor, ratioOctave=ratioOctave)
    if q["lo"] < ratioOctave or q["hi"] > ratioOctave:
        return R.SCALE, q, None
    pt = np.zeros(1, R.FUSE_POINT_DTYPE)[0]
    s1, s2 = f32(1.0 / nd1), f32(1.0 / nd2)
    pt["xyz"] = x3D
    pt["normal"] = [((f32(0) + n1[a] * s1) + n2[a] * s2) * f32(0.5) for a in range(3)]
    pt["max_dist"] = dist1 * SC[kp1["octave"]]
    pt["min_dist"] = pt["max_dist"] / SC[-1]
    pt["desc"] = k2["desc"][j] if first_obs else k1["desc"][i]
    return source, q, pt


def both(k1, k2, first_obs=0):
    """(status, intermediates) of the single-keypoint pair; the C and the numpy statement agree."""
    st_c, pt_c = R.pair_one(k1, k2, 0, 0, SC, S2, first_obs)
    with np.errstate(all="ignore"):
        st_p, q, pt_p = py_pair(k1, k2, 0, 0, first_obs)
    assert st_c == st_p, (st_c, st_p, q)
    if st_c > 0:
        assert pt_c.tobytes() == pt_p.tobytes()
    return st_c, q


# ---- constructed single-keypoint pairs (newpoints_scenario.py has the builders) -------------------

one_kf, wide_pair, with_, degenerate_pose_pair = NS.one_kf, NS.wide_pair, NS.with_, NS.degenerate_pose_pair


def axial_pair(z_cur=0.0, z_nb=0.0, d1=None, d2=None):
    """Both cameras on the z axis, unrotated, keypoints at the principal point: every ray is the z
    axis, cosParallaxRays = 1, so only a stereo unprojection can give the point, and z and the
    distances are exact differences."""
    cam = (NS.CAM[0], NS.CAM[1], 600.0, 180.0, NS.CAM[4])
    T1, T2 = np.eye(4, dtype=f32), np.eye(4, dtype=f32)
    T1[2, 3], T2[2, 3] = -z_cur, -z_nb
    k1 = one_kf(T1, (0, 0, z_cur), (600.0, 180.0), cam=cam)
    k2 = one_kf(T2, (0, 0, z_nb), (600.0, 180.0), cam=cam)
    for k, d in ((k1, d1), (k2, d2)):
        if d is not None:
            k["depth"][0] = d
            k["ur"][0] = f32(600.0) - f32(cam[4]) / f32(d)
    return k1, k2


# ---- the two statements agree ----------------------------------------------------------------------

@pytest.mark.parametrize("kind,seed", SCENES)
def test_numpy_statement_agrees_with_the_c(kind, seed):
    cur, nbors = NS.scene(150, seed, 3, kind)
    out = R.newpoints_chain(cur, nbors, SC, S2)
    seen = set()
    k1 = dict(cur)
    for k, nb in enumerate(nbors):
        at = {int(q["idx1"]): p for p, q in zip(out["points"], out["news"]) if q["neighbour"] == k}
        for i, j in enumerate(out["matches"][k]):
            if j < 0:
                continue
            with np.errstate(all="ignore"):
                st, _, pt = py_pair(k1, nb["kf"], i, int(j), nb["first_obs"])
            assert st == out["status"][k, i], (k, i, j)
            seen.add(st)
            if st > 0:
                assert pt.tobytes() == at[i].tobytes()
    assert len(seen) >= 4


# ---- boundaries (:340-470) -------------------------------------------------------------------------

def test_stereo_flag_is_ur_ge_zero():
    """:340, :344: bStereo = (ur >= 0). 0 and -0 are stereo, the largest negative float is not."""
    k1, k2 = wide_pair(X=(1.0, 0.5, 300.0))
    tiny = -np.nextafter(f32(0), f32(1))
    assert both(k1, k2)[0] == R.LOW_PARALLAX  # mono, mono, 0.9 m at 300 m
    for ur in (f32(0.0), f32(-0.0)):
        st, q = both(with_(k1, ur=ur, depth=300.0), k2)
        assert q["st1"] and st == R.REPROJ1_STEREO  # u_right = 0 is far from the projection
        st, q = both(k1, with_(k2, ur=ur, depth=300.0))
        assert q["st2"] and st == R.REPROJ2_STEREO
    st, q = both(with_(k1, ur=tiny, depth=300.0), with_(k2, ur=tiny, depth=300.0))
    assert not q["st1"] and not q["st2"] and st == R.LOW_PARALLAX


def test_else_if_stereo2_asymmetry():
    """:361-367: the neighbour's stereo parallax counts only when keypoint 1 is monocular. With a
    neighbour depth of 5 m (parallax far wider than the rays') the DLT is blocked only then."""
    k1, k2 = wide_pair(st1=True, st2=True)
    k2 = with_(k2, depth=5.0)
    st, q = both(k1, k2)
    assert st == R.DLT and q["cosSt2"] == q["cosRays"] + f32(1)
    assert R.cos_stereo(NS.MB, 5.0) < q["cosRays"] < q["cosSt1"]
    st, q = both(with_(k1, ur=-1.0), k2)
    assert q["cosSt2"] == R.cos_stereo(NS.MB, 5.0) and not q["cosRays"] < q["cosSt"]
    assert st != R.DLT and st in (R.STEREO2, R.REPROJ1_MONO)


def test_parallax_rays_below_stereo():
    """:372 cosParallaxRays < cosParallaxStereo, on the current keyframe's depth."""
    k1, k2 = wide_pair(X=(1.0, 0.5, 30.0), st1=True)
    fn = lambda d: both(with_(k1, depth=d), k2)[0] == R.DLT  # noqa: E731
    a, b = bisect_flip(fn, 100.0, 5.0)
    (sa, qa), (sb, qb) = both(with_(k1, depth=a), k2), both(with_(k1, depth=b), k2)
    assert sa == R.DLT and qa["cosRays"] < qa["cosSt1"]
    assert sb != R.DLT and not qb["cosRays"] < qb["cosSt1"] and sb != R.LOW_PARALLAX


def test_parallax_rays_positive():
    """:373 cosParallaxRays > 0: a neighbour turned by 80 degrees, its keypoint swept across."""
    T2, O2 = NS.pose((3.0, 0.0, 3.0), (0.0, math.radians(80), 0.0))
    k1, _ = wide_pair()
    k2 = one_kf(T2, O2, (600.0, 180.0))
    fn = lambda x: both(k1, with_(k2, x=x))[0] == R.LOW_PARALLAX  # noqa: E731
    a, b = bisect_flip(fn, 100.0, 1100.0) if fn(100.0) else bisect_flip(fn, 1100.0, 100.0)
    (sa, qa), (sb, qb) = both(k1, with_(k2, x=a)), both(k1, with_(k2, x=b))
    assert sa == R.LOW_PARALLAX and not qa["cosRays"] > 0
    assert sb != R.LOW_PARALLAX and qb["cosRays"] > 0


def test_mono_parallax_below_0_9998():
    """:374 cosParallaxRays < 0.9998 for two monocular keypoints. The literal is a double;
    float(0.9998) rounds up, so no float32 lies between them and `< 0.9998f` would decide every
    float32 cosine the same way: there is no input that tells the two types apart."""
    k1, k2 = wide_pair(X=(1.0, 0.5, 30.0))
    fn = lambda x: both(k1, with_(k2, x=x))[0] == R.LOW_PARALLAX  # noqa: E731
    x0 = k2["kps"]["x"][0]
    a, b = bisect_flip(fn, x0 + f32(25.0), x0) if fn(x0 + f32(25.0)) else bisect_flip(fn, x0 - f32(25.0), x0)
    (sa, qa), (sb, qb) = both(k1, with_(k2, x=a)), both(k1, with_(k2, x=b))
    assert sa == R.LOW_PARALLAX and not float(qa["cosRays"]) < 0.9998
    assert sb != R.LOW_PARALLAX and float(qb["cosRays"]) < 0.9998
    assert float(f32(0.9998)) > 0.9998
    for c in (f32(0.9998), np.nextafter(f32(0.9998), f32(0))):
        assert (float(c) < 0.9998) == bool(c < f32(0.9998))


def test_depth_in_the_current_keyframe():
    """:407 z <= 0: the neighbour's stereo point exactly in the current camera's plane is dropped,
    one float32 further it is not."""
    st, q = both(*axial_pair(z_cur=5.0, d2=5.0))
    assert q["z1"] == 0 and st == R.BEHIND1
    st, q = both(*axial_pair(z_cur=5.0, d2=np.nextafter(f32(5), f32(6))))
    assert q["z1"] > 0 and st not in (R.BEHIND1, R.LOW_PARALLAX)
    assert both(*axial_pair(z_cur=5.0, d2=4.0))[0] == R.BEHIND1


def test_depth_in_the_neighbour():
    """:412, the same for the neighbour with the current keyframe's stereo point."""
    st, q = both(*axial_pair(z_nb=5.0, d1=5.0))
    assert q["z1"] == 5 and q["z2"] == 0 and st == R.BEHIND2
    st, q = both(*axial_pair(z_nb=5.0, d1=np.nextafter(f32(5), f32(6))))
    assert q["z2"] > 0 and st not in (R.BEHIND1, R.BEHIND2, R.LOW_PARALLAX)


def near_pair(st1, st2, X=(-8.67, 0.5, 11.0)):
    """5 cm apart: less parallax than the stereo baseline's, so the stereo keyframe's own
    unprojection gives the point and the other view's test can be moved freely. Octave 0
    (sigma2 = 1); the projections lie near the left image border, where u_right is a small number
    with a fine float32 grid."""
    k1, k2 = wide_pair(X=X, st1=st1, st2=st2, center2=(-0.05, 0.0, 0.0), angles2=(0, 0, 0), octave=0)
    assert (k1["ur"][0] >= 0) == st1 and (k2["ur"][0] >= 0) == st2
    return k1, k2


def _threshold(make, lo, hi, code, key, sig, thr):
    """Bisects the parameter of make() between lo (accepted) and hi (code); thr(e, sigma2) is the
    cited line's comparison."""
    fn = lambda p: both(*make(p))[0] == code  # noqa: E731
    a, b = bisect_flip(fn, lo, hi)
    (sa, qa), (sb, qb) = both(*make(a)), both(*make(b))
    assert sa != code and not thr(qa[key], qa[sig])
    assert sb == code and thr(qb[key], qb[sig])
    return qa, qb


def test_reprojection_current_stereo():
    """:428 > 7.8 * sigma2 with a double literal."""
    k1, k2 = near_pair(True, False)
    ur = k1["ur"][0]
    _threshold(lambda p: (with_(k1, ur=p), k2), ur + f32(1), ur + f32(3.5), R.REPROJ1_STEREO,
               "e1", "sig1", lambda e, s: float(e) > 7.8 * float(s))


def test_reprojection_current_mono():
    """:432 > 5.991 * sigma2."""
    k1, k2 = near_pair(False, True)
    y = k1["kps"]["y"][0]
    _threshold(lambda p: (with_(k1, y=p), k2), y + f32(1), y + f32(5), R.REPROJ1_MONO,
               "e1", "sig1", lambda e, s: float(e) > 5.991 * float(s))


def test_reprojection_neighbour_stereo():
    """:449 > 7.8f * sigma2: a float product and a float comparison."""
    k1, k2 = near_pair(False, True)
    ur = k2["ur"][0]
    _threshold(lambda p: (k1, with_(k2, ur=p)), ur + f32(1), ur + f32(3.5), R.REPROJ2_STEREO,
               "e2", "sig2", lambda e, s: e > f32(7.8) * s)


def test_reprojection_neighbour_mono():
    """:453 > 5.991 * sigma2."""
    k1, k2 = near_pair(True, False)
    y = k2["kps"]["y"][0]
    _threshold(lambda p: (k1, with_(k2, y=p)), y + f32(1), y + f32(5), R.REPROJ2_MONO,
               "e2", "sig2", lambda e, s: float(e) > 5.991 * float(s))


def _scan_literal(make, ur, code, key, sig):
    """Looks, over 60 small shifts of the raw keypoint (UnprojectStereo reads it, so the point
    and with it the other error components move), for the accepted / rejected pair
    of adjacent u_right values whose squared error is exactly float(7.8) * sigma2 on one side:
    the one value that `> 7.8 * sigma2` (double) and `> 7.8f * sigma2` (float) decide differently
    at octave 0 (sigma2 = 1). Returns the intermediates found with e == float32(7.8)."""
    hits = []
    for c in range(60):
        mk = lambda p: make(p, f32(0.013) * c)  # noqa: E731
        fn = lambda p: both(*mk(p))[0] == code  # noqa: E731
        a, b = bisect_flip(fn, ur - f32(1), ur - f32(3.4))
        for p in (a, b):
            st, q = both(*mk(p))
            if q[key] == f32(7.8) and q[sig] == 1:
                hits.append((st, q))
    return hits


def test_stereo_thresholds_literal_types():
    """7.8 (:428, double) against 7.8f (:449, float): float32(7.8) = 7.80000019 > 7.8, so a
    squared error of exactly float32(7.8) at sigma2 = 1 is rejected in the current keyframe and
    accepted in the neighbour. Such inputs exist; the restatement follows the type as written."""
    k1, k2 = near_pair(True, False)

    def raw(k, dy):
        r = k["kps"].copy()
        r["y"] += dy
        return r
    hits = _scan_literal(lambda p, dy: (with_(k1, ur=p, raw=raw(k1, dy)), k2), k1["ur"][0],
                         R.REPROJ1_STEREO, "e1", "sig1")
    assert hits and all(st == R.REPROJ1_STEREO for st, _ in hits)
    k1, k2 = near_pair(False, True)
    hits = _scan_literal(lambda p, dy: (k1, with_(k2, ur=p, raw=raw(k2, dy))), k2["ur"][0],
                         R.REPROJ2_STEREO, "e2", "sig2")
    assert hits and all(st != R.REPROJ2_STEREO for st, _ in hits)


def test_neighbour_test_reads_the_current_mbf():
    """:447: u2_r = u2 - current_keyframe_->mbf / z_nbor. A neighbour with half the mbf whose
    u_right follows the current keyframe's mbf is accepted, one that follows its own is not."""
    k1, k2 = near_pair(False, True)
    cam2 = NS.CAM[:4] + (0.5 * NS.CAM[4],)
    z2 = float(k2["depth"][0])
    own = f32(k2["kps"]["x"][0]) - f32(cam2[4]) / f32(z2)
    assert both(k1, with_(k2, cam=cam2))[0] > 0
    assert both(k1, with_(k2, cam=cam2, ur=own))[0] == R.REPROJ2_STEREO


def test_zero_distance():
    """:462 dist1 == 0 || dist2 == 0: a camera centre equal to the point in every bit."""
    k1, k2 = wide_pair()
    st, pt = R.pair_one(k1, k2, 0, 0, SC, S2)
    assert st == R.DLT
    off = pt["xyz"].copy()
    off[0] = np.nextafter(off[0], f32(np.inf))
    for which in (0, 1):
        a, b = (with_(k1, Ow=pt["xyz"]), k2) if which == 0 else (k1, with_(k2, Ow=pt["xyz"]))
        st, q = both(a, b)
        assert st == R.DIST_ZERO and (q["dist1"], q["dist2"])[which] == 0
        a, b = (with_(k1, Ow=off), k2) if which == 0 else (k1, with_(k2, Ow=off))
        st, q = both(a, b)
        assert st == R.SCALE and (q["dist1"], q["dist2"])[which] > 0


def test_scale_consistency():
    """:469 both sides: the neighbour's centre moved along z changes dist2 alone."""
    k1, k2 = wide_pair()
    O2 = np.asarray(k2["Ow"], f32)

    def mk(z):
        return k1, with_(k2, Ow=np.array([O2[0], O2[1], z], f32))
    fn = lambda z: both(*mk(z))[0] == R.SCALE  # noqa: E731
    a, b = bisect_flip(fn, O2[2], f32(9.0))     # dist2 shrinks: dist_ratio * ratioFactor < ratioOctave
    (sa, qa), (sb, qb) = both(*mk(a)), both(*mk(b))
    assert sa == R.DLT and not qa["lo"] < qa["ratioOctave"]
    assert sb == R.SCALE and qb["lo"] < qb["ratioOctave"]
    a, b = bisect_flip(fn, O2[2], f32(-20.0))   # dist2 grows: dist_ratio / ratioFactor > ratioOctave
    (sa, qa), (sb, qb) = both(*mk(a)), both(*mk(b))
    assert sa == R.DLT and not qa["hi"] > qa["ratioOctave"]
    assert sb == R.SCALE and qb["hi"] > qb["ratioOctave"] and not qb["lo"] < qb["ratioOctave"]
    # ratioOctave: the octaves of both keypoints
    assert both(with_(k1, octave=7), with_(k2, octave=2))[0] == R.SCALE
    assert both(with_(k1, octave=3), with_(k2, octave=2))[0] == R.DLT


def test_w_zero():
    st, q = both(*degenerate_pose_pair())
    assert st == R.W_ZERO and q["w"] == 0 and 0 < q["cosRays"] < f32(0.9998)


def test_unproject_needs_depth_and_malformed():
    k1, k2 = near_pair(True, False)
    assert both(k1, k2)[0] == R.STEREO1
    assert both(with_(k1, depth=0.0), k2)[0] == R.NO_DEPTH
    assert R.pair_one(k1, k2, 0, 1, SC, S2)[0] == R.MALFORMED
    assert R.pair_one(with_(k1, octave=8), k2, 0, 0, SC, S2)[0] == R.MALFORMED
    # UnprojectStereo reads the raw keypoint, not the undistorted one
    raw = k1["kps"].copy()
    raw["x"] += 3.0
    moved = R.pair_one(with_(k1, raw=raw), k2, 0, 0, SC, S2)
    assert moved[0] != R.STEREO1 or not np.array_equal(moved[1]["xyz"],
                                                         R.pair_one(k1, k2, 0, 0, SC, S2)[1]["xyz"])


# ---- geometry ---------------------------------------------------------------------------------------

# The largest relative deviation of an accepted DLT point from the float64 numpy.linalg.svd
# triangulation of the same float32 matrix on the noise-free scenes below, measured with
#   python -m pytest tests/test_newpoints_ref.py -k geometry -s
# and the bound: 4 x that (the scene is fixed; the float32 rounding of the null vector and of the
# final divide is the only slack).
GEOMETRY_MEASURED = 1.33e-7
GEOMETRY_BOUND = 4 * GEOMETRY_MEASURED


def test_geometry_against_numpy_svd():
    worst, count = 0.0, 0
    for kind, seed in SCENES:
        cur, nbors = NS.scene(500, seed, 3, kind, noise=0.0, disturb=False)
        out = R.newpoints_chain(cur, nbors, SC, S2)
        for p, q in zip(out["points"], out["news"]):
            if q["source"] != R.DLT:
                continue
            A, _ = R.dlt(cur, nbors[q["neighbour"]]["kf"], int(q["idx1"]), int(q["idx2"]))
            x = np.linalg.svd(A.astype(np.float64))[2][3]
            X = x[:3] / x[3]
            worst = max(worst, float(np.linalg.norm(p["xyz"].astype(np.float64) - X) /
                                     np.linalg.norm(X)))
            count += 1
    print(f"geometry: {count} DLT points, largest relative deviation {worst:.3e}, "
          f"bound {GEOMETRY_BOUND:.3e}")
    assert count > 1000
    assert worst <= GEOMETRY_BOUND


# ---- the cos identity ---------------------------------------------------------------------------------

def _ulps(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_cos_identity_against_libm():
    """(d^2 - h^2) / (d^2 + h^2) against cosf(2 * atan2f(h, d)) over h in {0.05 .. 0.6} and every
    1000th float32 d in [0.1, 500]. The float chain's angle 2 * atan2f is off by up to 2^-22 for
    an atan2f good to an ulp of [1, 2), cosf adds 2^-24 and the identity's one rounding 2^-25:
    the two forms are within 2^-21 of each other. The largest distance goes to DESIGN.md, in
    absolute terms and in ulp where |cos| >= 0.5 (near d = h the cosine crosses 0 and an ulp
    count says nothing)."""
    lo, hi = int(f32(0.1).view(np.int32)), int(f32(500.0).view(np.int32))
    d = np.arange(lo, hi + 1, 1000, dtype=np.int32).view(f32)
    worst_ulp, worst_abs = 0, 0.0
    for h in (0.05, 0.1, 0.15, 0.2, 0.2686, 0.3, 0.4, 0.5, 0.6):
        a, b = R.cos_stereo_many(2 * h, d)
        worst_ulp = max(worst_ulp, int(_ulps(a, b)[np.abs(a) >= 0.5].max()))
        worst_abs = max(worst_abs, float(np.abs(a.astype(np.float64) - b).max()))
    print(f"cos identity: {len(d)} depths x 9 half-baselines, largest distance {worst_abs:.3e} "
          f"absolute, {worst_ulp} ulp where |cos| >= 0.5")
    assert worst_abs <= 2.0 ** -21


def test_cos_forms_give_the_same_status_rows():
    scenes = [NS.scene(300, seed, 3, kind) for kind, seed in SCENES]
    scenes.append(NS.scene(300, 31, 2))
    scenes.append(NS.scene(300, 54, 3, "stereo", noise=0.0, disturb=False))
    for cur, nbors in scenes:
        a = R.newpoints_chain(cur, nbors, SC, S2)
        b = R.newpoints_chain(cur, nbors, SC, S2, libm_cos=True)
        np.testing.assert_array_equal(a["status"], b["status"])
        assert a["n_new"] == b["n_new"]


# ---- the chain ------------------------------------------------------------------------------------------

def test_chain_uses_the_updated_has_mp():
    cur, nbors = NS.scene(300, 31, 2)
    out = R.newpoints_chain(cur, nbors, SC, S2)
    m0, m1 = out["matches"]
    acc0, rej0 = out["status"][0] > 0, out["status"][0] < 0
    assert acc0.sum() > 50 and (m0[acc0] >= 0).all()
    assert (m1[acc0] < 0).all(), "a keypoint accepted in the first neighbour matched again"
    assert (m1[rej0] >= 0).any(), "no rejected keypoint came back in the second neighbour"
    alone = R.newpoints_chain(cur, [nbors[1]], SC, S2)["matches"][0]
    assert (alone[acc0] >= 0).any()
    np.testing.assert_array_equal(out["has_mp1"], cur["mp"] | (out["status"] > 0).any(0))
    # skipped neighbours leave nothing
    cur, nbors = NS.scene(300, 21, 3, skips=(1,))
    out = R.newpoints_chain(cur, nbors, SC, S2)
    assert not out["status"][1].any() and 1 not in out["news"]["neighbour"]
    # the first k rows do not depend on the later neighbours (CheckNewKeyFrames' early return)
    first = R.newpoints_chain(cur, nbors[:1], SC, S2)
    np.testing.assert_array_equal(first["status"][0], out["status"][0])
    n = first["n_new"]
    assert out["points"][:n].tobytes() == first["points"].tobytes()


def test_descriptor_follows_first_obs():
    """map_point.cpp:249-304 with two observations: both medians are 0 and `median < best_median`
    keeps the first entry of the std::map<KeyFrame*, size_t>."""
    k1, k2 = wide_pair()
    k1, k2 = with_(k1, desc=np.full((1, 32), 0x11, np.uint8)), with_(k2, desc=np.full((1, 32), 0x22, np.uint8))
    a, b = R.pair_one(k1, k2, 0, 0, SC, S2, 0), R.pair_one(k1, k2, 0, 0, SC, S2, 1)
    assert a[0] == b[0] == R.DLT
    assert (a[1]["desc"] == 0x11).all() and (b[1]["desc"] == 0x22).all()
    for f in ("xyz", "normal", "min_dist", "max_dist"):
        np.testing.assert_array_equal(a[1][f], b[1][f])
    cur, nbors = NS.scene(100, 21, 2)
    out = R.newpoints_chain(cur, nbors, SC, S2)
    for p, q in zip(out["points"], out["news"]):
        nb = nbors[q["neighbour"]]
        want = nb["kf"]["desc"][q["idx2"]] if nb["first_obs"] else cur["desc"][q["idx1"]]
        np.testing.assert_array_equal(p["desc"], want)


# ---- sanitizers -----------------------------------------------------------------------------------------

def test_restatement_is_clean_under_the_sanitizers(tmp_path):
    """tests/newpoints_sanitizer_check.c (the restatement plus a main of its own: a regular pair,
    a row without matches, x3D(3) == 0, NaN poses, malformed matches and octaves) built with the
    address and undefined-behaviour sanitizers and run as a program; the runtimes are linked
    statically, so it runs as it is whatever else is preloaded."""
    exe = str(tmp_path / "newpoints_sanitizer_check")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",
                    os.path.join(R.HERE, "newpoints_sanitizer_check.c"), "-o", exe, "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", r.stdout + r.stderr
    assert not r.stderr.strip(), r.stderr
