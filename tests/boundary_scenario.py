"""Constructed boundary inputs of the Hamming matchers (plain numpy: neither the oracle nor the
device library is imported here). Every case is a small record: the inputs of one call of one
entry point, the features it designates, the output `expected` there, written down from the line
of src/orb_features/orb_matcher.cpp the case cites, and the output `alt` the nearest wrong rule
would give (first instead of last, `<` instead of `<=`, ...). expected != alt is what makes the case
a test; everything that is not designated is filler and must stay unmatched.

Keyframe matchers (hand-built keyframes): camera fx = fy = 512, cx = 320, cy = 240 on a 640 x 480
image, so the 64 x 48 grid has 10 x 10 px cells and a point ((u - 320) / 64, (v - 240) / 64, 8)
seen from the identity pose projects to (u, v) without rounding. A "site" is a point at (..3, ..3)
with keypoints 2 px to its left / above (the same cell) and 3 px to its right / below (x = ..6 is
cell round(..0.6): the next one), so GetFeaturesInArea's order (keyframe.cpp:442-476: cell x-major,
then y, then index) and the index order disagree wherever the case wants them to.

Frame matchers (the frame comes from an image): the caller passes the frame's keypoints and
descriptors; a site is a pair of close keypoints with no third one near, the query descriptor is
built at exact distances from both (desc_at2) and the projection is placed between them.

Families by entry point ("x" or the line of orb_matcher.cpp = built; "-" = the entry point has no
such rule; "n/a" = not applicable, see below). tri = SearchForTriangulation, sbp_sim3 =
SearchByProjection(pKF, Scw), sim3 = SearchBySim3, f2f = SearchByProjection(Frame, Frame), mps =
SearchByProjection(Frame, vpMapPoints), reloc = SearchByProjection(Frame, pKF, sAlreadyFound).
In the keyframe matchers' cases the families window .. off_grid share one case, "gates".

  family            tri    fuse   fuse_sim3  sbp_sim3  sim3        f2f    mps   reloc
  tie               :717   :923   :1053      :481      :1198/1278  :1406  :76   :1534
  threshold         :717   :930   :1061      :486      :1207/1287  :1415  :90   :1541
  best_dist = 256   -      x      x          -         -           -      -     -
  ratio             -      -      -          -         -           -      :84   -
  claims            -      -      -          :469      :1117 (a)   :1391  :60   :1526
  not searched (c)  :684   x      x          x         x           -      :26   :1470
  chain > top-K     -      -      -          x         -           x (d)  x (d) x
  window            -      x      x          x         x           x      x     x
  level_window      -      x      x          x         x           x (b)  x     x
  scale ceil/clamp  -      x      x          x         x           -      -     x
  scale[k] +- 1 ulp -      x      x          x         x           -      -     x
  depth_sign        -      :834   :995       :422      :1147       :1359  -     :1483 (no gate)
  image_bounds      -      x      x          x         x           n/a    -     n/a
  off_grid          -      x      x          x         x           n/a    n/a   n/a
  chi_square        -      :880   -          -         -           -      -     -
  u_right 0 / -1    :688   :884   -          -         -           n/a    n/a   -
  epipolar          :114   -      -          -         -           -      -     -
  epipole           :694   -      -          -         -           -      -     -
  den_zero          :124   -      -          -         -           -      -     -
  view_cos          -      -      -          -         -           -      :105  -
  histogram         x      -      -          -         -           x      -     x
  check_ori_off     x      -      -          -         -           x      -     x

SearchByBoW (entry "bow"; its tie order is constructed in test_bow_gpu.py) has the threshold's
strictness in its two overloads (<= TH_LOW :202, < TH_LOW :575), the ratio test at equality, a tied
minimum and a keypoint already taken (:186-204), and the histogram and check_ori_off families of
SearchForTriangulation on the same keyframes and angle sets (:210-220, :241-259).

(a) SearchBySim3 claims nothing; its vbAlreadyMatched flags are in its threshold case.
(b) with the forward and the backward window (:1371-1376).
(c) a point or query that would be the best match but is flagged: skip (bad, already in the
    keyframe, spAlreadyFound / sAlreadyFound), not in view, has_mp; the frame-to-frame queries
    carry no such flag (the caller leaves the point out).
(d) the query descriptor is the bitwise majority of seven keypoints of a wide window.

Not applicable, with the reason:
  - dsqr == 3.84 * sigma2 and e2 * invSigma2 == 5.99 / 7.8 exactly: the constants are no floats;
    the cases sit on the floats (one coordinate step) either side.
  - PredictScale clamped to 0: out of reach (dist3D <= 1.2 * max_dist keeps ceil(log(ratio) /
    log 1.2) >= -0). At scale[k] and one ulp either side the expected level is written from the
    correctly rounded logarithm (float64 log rounded to float), not from the oracle's logf.
  - frame matchers, image bounds and off-grid keypoints: a frame's keypoints lie >= 19 px inside
    the image, so no candidate exists where u == max_x would show, and none is off the grid.
  - frame matchers, u_right gates at their edge: the frame's u_right comes from its stereo
    matcher, not from the caller; the sites use keypoints with u_right <= 0, where the gate never
    applies (the chain cases work the gate out for every keypoint of their window).
  - `bin == 30`: rot * (1 / 30f) <= 12, unreachable in the reference too.
  - a pKF1 feature listed under two nodes of its FeatureVector: DBoW2 never produces it.
  - SearchByBoW's batched device form: not among the eight entry points; its cases run through
    the single call only.
"""
import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
FUSE_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"),
                             ("max_dist", "<f4"), ("skip", "<i4"), ("pad", "<i4", (3,)),
                             ("desc", "u1", (32,))])
CAM = (512.0, 512.0, 320.0, 240.0, 64.0)
W, H = 640, 480
Z = 8.0
N_KF = 130
TH_LOW, TH_HIGH = 50, 100


def scales(nlevels=8):
    sc = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sc[i] = f32(float(sc[i - 1]) * float(f32(1.2)))
    return sc


SC = scales()


class Case:
    """designated / expected / alt: the features the case is about, the output there by the cited
    line, and the output of the nearest wrong rule. support: {feature: output} of features that
    match under either rule and only set the stage (the bulk of a rotation histogram, the earlier
    claimants of a keypoint). Every other feature is filler: its output stays "unmatched"."""

    def __init__(self, entry, family, name, cite, inp, designated, expected, alt, output,
                 support=None):
        self.entry, self.family, self.name, self.cite = entry, family, name, cite
        self.inp, self.output = inp, output
        self.designated = np.asarray(list(designated), np.int64)
        self.expected = np.asarray(list(expected), np.int64)
        self.alt = np.asarray(list(alt), np.int64)
        self.support = dict(support or {})
        assert len(self.designated) == len(self.expected) == len(self.alt) > 0
        assert len(set(self.designated.tolist())) == len(self.designated)
        assert not set(self.designated.tolist()) & set(self.support)

    @property
    def id(self):
        return f"{self.entry}-{self.family}-{self.name}"


# ---- helper 1: descriptors at exact Hamming distances ---------------------------------------------
def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def rand_desc(rng, n=None):
    return rng.integers(0, 256, (32,) if n is None else (n, 32), dtype=np.uint8)


def _flip(d, bits):
    d = np.array(d, np.uint8)
    for b in bits:
        d[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return d


def desc_at(base, k, rng):
    """A descriptor at Hamming distance exactly k from `base`."""
    out = _flip(base, rng.choice(256, k, replace=False))
    assert hamming(out, base) == k
    return out


def desc_at2(a, b, ka, kb, rng):
    """A descriptor at distance ka from a and kb from b: x of the bits where a and b differ and y
    of the bits where they agree are flipped in a, x + y = ka, D - x + y = kb. None if (ka, kb, D)
    admit no such descriptor."""
    bits_a = np.unpackbits(np.asarray(a, np.uint8), bitorder="little")
    bits_b = np.unpackbits(np.asarray(b, np.uint8), bitorder="little")
    differ, agree = np.nonzero(bits_a != bits_b)[0], np.nonzero(bits_a == bits_b)[0]
    D = len(differ)
    if (ka - kb + D) % 2:
        return None
    x, y = (ka - kb + D) // 2, (ka + kb - D) // 2
    if not (0 <= x <= D and 0 <= y <= len(agree)):
        return None
    out = _flip(a, np.concatenate([rng.choice(differ, x, replace=False),
                                   rng.choice(agree, y, replace=False)]))
    assert hamming(out, a) == ka and hamming(out, b) == kb
    return out


# ---- helper 2: keypoints, poses and points that put a float gate where the case wants it --------
def norm3(p):
    p = np.asarray(p, f32).astype(np.float64)
    return f32(np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]))


LSF = f32(np.log(np.float64(f32(1.2))))      # log_scale_factor: std::log of the float 1.2f


def predicted_level(ratio, nlevels=8):
    """PredictScale (map_point.cpp:366-396) of a float ratio = max_dist / dist: ceil(logf(ratio) /
    log_scale_factor) in float arithmetic, clamped, with logf the correctly rounded logarithm
    (float64 log rounded to float)."""
    q = f32(f32(np.log(np.float64(f32(ratio)))) / LSF)
    return int(min(max(int(np.ceil(q)), 0), nlevels - 1))


def max_dist_for_ratio(d, target):
    """A float max_dist with (float)(max_dist / d) == target exactly, or None."""
    d, target = f32(d), f32(target)
    m = f32(d * target)
    for _ in range(4):
        m = np.nextafter(m, f32(-np.inf), dtype=f32)
    for _ in range(9):
        if f32(m / d) == target:
            return m
        m = np.nextafter(m, f32(np.inf), dtype=f32)
    return None


def ratio_edges(k, scale=None):
    """scale[k] and its float neighbours, each with the level PredictScale gives there."""
    s = f32((SC if scale is None else scale)[k])
    return [(t, predicted_level(t)) for t in (np.nextafter(s, f32(0), dtype=f32), s,
                                              np.nextafter(s, f32(np.inf), dtype=f32))]


def point(u, v, level, desc, z=Z, ratio=None, skip=0, max_dist=None):
    """A FUSE_POINT record that the identity pose projects to (u, v) exactly (u, v on the 1/64 px
    grid, z a power of two), seen head-on, whose PredictScale is `level` (max_dist / dist3D =
    1.2^(level - 0.5), or `ratio` as given)."""
    p = np.zeros(1, FUSE_POINT_DTYPE)
    xyz = np.array([(u - CAM[2]) * z / CAM[0], (v - CAM[3]) * z / CAM[1], z], f32)
    assert float(xyz[0]) * CAM[0] / z + CAM[2] == u and float(xyz[1]) * CAM[1] / z + CAM[3] == v
    d = norm3(xyz)
    p["xyz"][0] = xyz
    p["normal"][0] = (xyz.astype(np.float64) / float(d) * np.sign(z)).astype(f32)
    p["max_dist"] = f32(float(d) * (1.2 ** (level - 0.5) if ratio is None else ratio))
    if max_dist is not None:
        p["max_dist"] = max_dist
    p["min_dist"] = f32(float(p["max_dist"][0]) / 1.2 ** 7 * 0.9)
    p["skip"] = skip
    p["desc"][0] = desc
    return p[0]


def radius_th(level, near=3.0):
    """A window factor th (near `near`) whose radius th * scale[level], the float product the
    matchers form, lies on the 1/4096 px grid: a keypoint can then sit at exactly that distance from
    a projection on the same grid. Returns (th, r)."""
    for k in range(int(near * 4096), int(near * 4096) + 200000):
        th = f32(k / 4096.0)
        r = f32(th * SC[level])
        if float(r) * 4096.0 == int(float(r) * 4096.0):
            return float(th), float(r)
    raise AssertionError("no radius on the grid")


class KeyframeBuilder:
    """N_KF keypoints: fillers in a band along the bottom of the image (random descriptors, mono),
    designated ones moved to their sites by put()."""

    def __init__(self, rng, n=N_KF):
        self.rng, self.n = rng, n
        self.kps = np.zeros(n, KP_DTYPE)
        i = np.arange(n)
        self.kps["x"] = 20.25 + 10.0 * (i % 60)
        self.kps["y"] = 425.25 + 15.0 * (i // 60)
        self.kps["size"] = 31.0
        self.desc = rand_desc(rng, n)
        self.ur = np.full(n, -1.0, f32)
        self.placed = set()

    def put(self, idx, x, y, octave, desc, ur=-1.0, angle=0.0):
        assert idx not in self.placed and 0 <= idx < self.n
        self.placed.add(idx)
        self.kps[idx]["x"], self.kps[idx]["y"] = x, y
        self.kps[idx]["octave"], self.kps[idx]["angle"] = octave, angle
        self.kps[idx]["size"] = f32(31.0 * SC[octave])
        self.desc[idx] = desc
        self.ur[idx] = ur
        return idx

    def kf(self):
        return dict(kps=self.kps, desc=self.desc, ur=self.ur)

    def filler_points(self, count, first=0):
        """Points that land on filler keypoints with unrelated descriptors: they fuse nowhere."""
        out = []
        fill = [j for j in range(self.n) if j not in self.placed]
        for j in fill[first:first + count]:
            out.append(point(float(self.kps["x"][j]), float(self.kps["y"][j]), 0,
                             rand_desc(self.rng)))
        return out


I3 = np.eye(3, dtype=f32)
Z3 = np.zeros(3, f32)
T_ID = np.eye(4, dtype=f32)


# ---- the grid-ordered keyframe matchers: Fuse, Fuse(Scw), SearchByProjection(Scw) ---------------
class _Sites:
    """Designated points of one case: each add() puts one point (at (sx + 3, sy + 3)) and its
    candidate keypoints (offsets from the point, index, octave, distance, ...)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kb = KeyframeBuilder(self.rng)
        self.pts, self.exp, self.alt = [], [], []
        self.slot = 0

    def site_xy(self):
        s = self.slot
        self.slot += 1
        return 53.0 + 50.0 * (s % 10), 53.0 + 50.0 * (s // 10)

    def add(self, cands, level, expected, alt, uv=None, q=None, **pk):
        """cands: (dx, dy, idx, octave, dist[, ur]) relative to the point."""
        u, v = uv if uv is not None else self.site_xy()
        q = rand_desc(self.rng) if q is None else q
        for c in cands:
            dx, dy, idx, octave, dist = c[:5]
            self.kb.put(idx, u + dx, v + dy, octave, desc_at(q, dist, self.rng),
                        ur=c[5] if len(c) > 5 else -1.0)
        self.pts.append(point(u, v, level, q, **pk))
        self.exp.append(expected)
        self.alt.append(alt)
        return q

    def again(self, expected, alt):
        """The last point offered once more (expected None: it must stay unmatched, as filler)."""
        self.pts.append(self.pts[-1].copy())
        self.exp.append(expected)
        self.alt.append(alt)

    def finish(self, n_filler=8):
        """(points, designated, expected, alt): the sites' points in order, fillers between them
        (so that they sit in different blocks and waves). A point with an expectation and alt None
        goes to self.support, one with neither is filler."""
        m = len(self.pts)
        fill = self.kb.filler_points(n_filler)
        order, des, exp, alt = [], [], [], []
        self.support = {}
        for i in range(max(m, n_filler)):
            if i < n_filler:
                order.append(fill[i])
            if i < m:
                if self.exp[i] is not None and self.alt[i] is None:
                    self.support[len(order)] = self.exp[i]
                elif self.exp[i] is not None:
                    des.append(len(order))
                    exp.append(self.exp[i])
                    alt.append(self.alt[i])
                order.append(self.pts[i])
        pts = np.array(order, FUSE_POINT_DTYPE)
        assert len(pts) <= 40
        return pts, des, exp, alt


L3 = 3  # predicted level of the ordinary sites: r = 3 * 1.728 = 5.18 px, 5.99 * sigma2 = 17.9


def _tie_sites(S):
    """Tied minima at distance 20 whose position decides (first in GetFeaturesInArea order)."""
    S.add([(-2, 0, 100, L3, 20), (3, 0, 5, L3, 20)], L3, 100, 5)        # earlier cell (x), high idx
    S.add([(0, -2, 101, L3, 20), (0, 3, 6, L3, 20)], L3, 101, 6)        # earlier cell (y), high idx
    S.add([(3, -2, 7, L3, 20), (-2, 3, 8, L3, 20)], L3, 8, 7)           # x-major, not y-major
    S.add([(-2, 0, 9, L3, 20), (-1, -1, 73, L3, 20)], L3, 9, 73)        # one cell, lanes c / c + 64
    S.add([(-2, -1, 129, L3, 20), (-1, 0, 70, L3, 20)], L3, 70, 129)    # one cell, one round
    S.add([(3, 3, 2, L3, 20), (-2, 3, 66, L3, 20), (3, -2, 128, L3, 20), (-2, -2, 127, L3, 20),
           (0, 0, 126, L3, 21)], L3, 127, 2)                            # four cells, three rounds


def _threshold_sites(S, th_dist):
    S.add([(1, 1, 10, L3, th_dist)], L3, 10, -1)                         # dist == TH: kept (<=)
    S.add([(1, 1, 75, L3, th_dist + 1)], L3, -1, 75)                     # TH + 1: dropped
    S.add([(1, 1, 11, L3, th_dist - 1), (-1, 0, 76, L3, th_dist)], L3, 11, 76)
    S.add([], L3, -1, 0)                                                 # no candidate at all
    S.add([(1, 1, 12, L3 + 1, 3)], L3, -1, 12)                           # only a wrong-level one
    # a point flagged skip (bad, already in the keyframe, in spAlreadyFound) is not searched,
    # however good its candidate
    S.add([(1, 1, 13, L3, 3)], L3, -1, 13, skip=1)


def _gate_sites(S):
    # search window fabs(dx) < r, r = th * scale[0] on the grid (the case's th applies to all sites)
    r = S.r
    S.add([(r, 0, 20, 0, 5), (-1, 0, 84, 0, 30)], 0, 84, 20)             # |dx| == r: outside
    S.add([(r - 1 / 4096.0, 0, 21, 0, 5), (-1, 0, 85, 0, 30)], 0, 21, 85)
    S.add([(0, -r, 22, 0, 5), (0, 1, 86, 0, 30)], 0, 86, 22)             # |dy| == r: outside
    # level window lvl - 1 .. lvl
    S.add([(1, 0, 23, 1, 5), (-1, 0, 87, 2, 30)], 3, 87, 23)             # lvl - 2 is outside
    S.add([(1, 0, 24, 4, 5), (-1, 0, 88, 3, 30)], 3, 88, 24)             # lvl + 1 is outside
    # PredictScale: ceil (1.2^0.1 is level 1, not 0) and the clamp to nlevels - 1 (1.2^8.5 is level
    # 9 -> 7; the clamp to 0 is out of reach: dist3D <= 1.2 * max_dist keeps the level above -1)
    S.add([(1, 0, 25, 1, 30)], 1, 25, -1, ratio=1.2 ** 0.1)
    S.add([(1, 0, 26, 7, 30), (-1, 0, 89, 5, 5)], 7, 26, -1, ratio=1.2 ** 8.5)
    # max_dist / dist3D at scale[3] exactly and one ulp either side: the level is 3 or 4 as the
    # correctly rounded logf says; a keypoint of octave 2 is in the window of level 3 only, one of
    # octave 4 in that of level 4 only
    for i, (target, n) in enumerate(ratio_edges(3)):
        assert n in (3, 4)
        while True:
            u, v = S.site_xy()
            m = max_dist_for_ratio(norm3([(u - CAM[2]) * Z / CAM[0], (v - CAM[3]) * Z / CAM[1], Z]),
                                   target)
            if m is not None:
                break
        lo, hi = 40 + i, 110 + i
        S.add([(1, 0, lo, 2, 5), (-1, 0, hi, 4, 5)], 3, lo if n == 3 else hi,
              hi if n == 3 else lo, uv=(u, v), max_dist=m)
    # zc < 0: the mirrored point projects to the same pixel and is skipped
    S.add([(1, 0, 27, 3, 5)], 3, -1, 27, z=-Z)
    # u >= min_x, v >= min_y: on the bound is inside; u < max_x: on the bound is outside
    S.add([(1, 0, 28, 0, 5)], 0, 28, -1, uv=(0.0, 203.0))
    S.add([(0, 1, 29, 0, 5)], 0, 29, -1, uv=(253.0, 0.0))
    S.add([(-6, 0, 30, 7, 5)], 7, -1, 30, uv=(640.0, 203.0))
    S.add([(-6, 0, 31, 7, 5)], 7, 31, -1, uv=(640.0 - 1 / 64.0, 253.0))
    # PosInGrid: x = 636 is cell round(63.6) = 64, outside the grid: never a candidate
    S.add([(3, 0, 32, 7, 5), (-3, 0, 90, 7, 30)], 7, 90, 32, uv=(633.0, 303.0))


def _chi_sites(S):
    """Fuse's chi-square gates (:880-905): mono e2 * invSigma2 > 5.99, stereo > 7.8 (level 0:
    invSigma2 = 1), ex one step of the coordinate grid either side of sqrt(5.99) / sqrt(7.8); and
    which of the two gates a keypoint meets: u_right >= 0 (:884)."""
    g = 1 / 4096.0
    lo = np.floor(np.sqrt(5.99) / g) * g
    assert f32(lo * lo) < 5.99 < f32((lo + g) * (lo + g))
    S.add([(lo, 0, 33, 0, 5), (0, 1, 91, 0, 30)], 0, 33, 91)
    S.add([(lo + g, 0, 34, 0, 5), (0, 1, 92, 0, 30)], 0, 92, 34)
    lo = np.floor(np.sqrt(7.8) / g) * g
    assert f32(lo * lo) < 7.8 < f32((lo + g) * (lo + g))
    # stereo keypoint on the projection: ex = ey = 0, er = (u - bf / z) - ur
    u, v = S.site_xy()
    S.add([(0, 0, 35, 0, 5, u - CAM[4] / Z - lo), (0, 1, 93, 0, 30)], 0, 35, 93, uv=(u, v))
    u, v = S.site_xy()
    S.add([(0, 0, 36, 0, 5, u - CAM[4] / Z - (lo + g)), (0, 1, 94, 0, 30)], 0, 94, 36, uv=(u, v))
    # u_right exactly 0 is a stereo keypoint (>= 0: er is large, the gate drops it); -1 is mono
    S.add([(1, 0, 37, 0, 5, 0.0), (0, 1, 95, 0, 30)], 0, 95, 37)
    S.add([(1, 0, 38, 0, 5, -1.0), (0, 1, 96, 0, 30)], 0, 38, 96)


CITE = {"fuse": {"tie": ":923", "threshold": ":930", "gates": ":828-878", "chi_square": ":880-905"},
        "fuse_sim3": {"tie": ":1053", "threshold": ":1061", "gates": ":988-1044"},
        "sbp_sim3": {"tie": ":481", "threshold": ":486", "gates": ":415-478", "claims": ":469"}}


def _scw_case(entry, family, seed):
    S = _Sites(seed)
    th = 3.0
    if family == "tie":
        _tie_sites(S)
    elif family == "threshold":
        _threshold_sites(S, TH_LOW)
    elif family == "chi_square":
        _chi_sites(S)
    else:
        th, S.r = radius_th(0, 2.0)
        assert S.r * S.r < 5.99                       # the window's edge is inside Fuse's chi-square
        _gate_sites(S)
    pts, des, exp, alt = S.finish()
    kf = S.kb.kf()
    inp = dict(kf=kf, pts=pts, th=th, matched_in=np.zeros(N_KF, np.uint8))
    return Case(entry, family, "sites", CITE[entry][family], inp, des, exp, alt,
                "point_kp" if entry == "sbp_sim3" else "best_idx")


def _best_dist_case(entry, seed):
    """best_dist: 256 where no candidate passes the gates, else the minimum (also above TH_LOW)."""
    S = _Sites(seed)
    S.add([], L3, 256, -1)
    S.add([(1, 1, 12, L3 + 1, 3)], L3, 256, 3)
    S.add([(1, 1, 13, L3, 51)], L3, 51, 256)
    S.add([(1, 1, 14, L3, 50)], L3, 50, 256)
    pts, des, exp, alt = S.finish()
    inp = dict(kf=S.kb.kf(), pts=pts, th=3.0, matched_in=np.zeros(N_KF, np.uint8))
    return Case(entry, "threshold", "best_dist", CITE[entry]["threshold"], inp, des, exp, alt,
                "best_dist")


def _claims_case(seed):
    """SearchByProjection(pKF, Scw): the points claim keypoints in order (:469 skips vpMatched)."""
    S = _Sites(seed)
    # one point offered four times at three candidates (10 / 20 / 30): each offer takes the best
    # keypoint still free, i.e. the loser's next candidate is the later offer's best; the fourth
    # finds none
    S.add([(-2, 0, 40, L3, 10), (3, 0, 41, L3, 20), (0, 3, 42, L3, 30)], L3, 40, None)
    S.again(41, 40)
    S.again(42, 41)
    S.again(-1, 42)
    # two different points whose best is one keypoint, the loser's next candidate tied with the
    # third point's best: the loser takes it, the third point falls to its own second
    u, v = S.site_xy()
    q1 = S.add([(-2, 0, 50, L3, 10), (3, 0, 51, L3, 20)], L3, 50, None, uv=(u, v))
    S.pts.append(point(u, v, L3, desc_at2(S.kb.desc[50], S.kb.desc[51], 12, 20, S.rng)))
    S.exp.append(51); S.alt.append(50)                                    # noqa: E702
    q3 = desc_at2(S.kb.desc[51], q1, 20, 40, S.rng)
    S.kb.put(52, u, v + 3, L3, desc_at(q3, 30, S.rng))
    S.pts.append(point(u, v, L3, q3))
    S.exp.append(52); S.alt.append(51)                                    # noqa: E702
    # a chain longer than the kept top-K: six tied candidates, one point offered seven times; the
    # i-th offer takes the i-th keypoint in GetFeaturesInArea order (cell (c, r): 60 108 125, then
    # (c, r + 1): 43, (c + 1, r): 107, (c + 1, r + 1): 44), the seventh finds none
    S.add([(3, 3, 44, L3, 10), (-2, 3, 43, L3, 10), (3, -2, 107, L3, 10), (-2, -2, 108, L3, 10),
           (-1, -1, 60, L3, 10), (-2, 0, 125, L3, 10)], L3, 60, 43)
    for e, a in ((108, 44), (125, 60), (43, 107), (107, 108), (44, 125)):
        S.again(e, a)
    S.again(None, None)
    # keypoints matched at entry: the tied minimum that comes first, and a strictly better one
    S.add([(-2, 0, 46, L3, 10), (3, 0, 47, L3, 10)], L3, 47, 46)
    S.add([(-2, 0, 48, L3, 5), (3, 0, 49, L3, 45)], L3, 49, 48)
    # a skipped point (bad or in spAlreadyFound) claims nothing: the same point offered again
    # without the flag takes the keypoint
    S.add([(1, 1, 53, L3, 5)], L3, -1, 53, skip=1)
    S.again(53, -1)
    S.pts[-1]["skip"] = 0
    pts, des, exp, alt = S.finish(n_filler=6)
    mi = np.zeros(N_KF, np.uint8)
    mi[[46, 48]] = 1
    inp = dict(kf=S.kb.kf(), pts=pts, th=3.0, matched_in=mi)
    return Case("sbp_sim3", "claims", "in_order", ":469", inp, des, exp, alt, "point_kp",
                support=S.support)


# ---- SearchBySim3 -------------------------------------------------------------------------------
def _sim3_cases(seed):
    """Both keyframes at the identity pose, S12 the identity: a map point of one keyframe projects
    into the other at its own pixel. match12[i1] needs vnMatch1[i1] = i2 and vnMatch2[i2] = i1."""
    out = []
    for family in ("tie", "threshold", "gates"):
        rng = np.random.default_rng(seed)
        seed += 1
        k = [KeyframeBuilder(rng), KeyframeBuilder(rng)]
        mp = [np.zeros(N_KF, FUSE_POINT_DTYPE), np.zeros(N_KF, FUSE_POINT_DTYPE)]
        for m in mp:
            m["skip"] = 1
        des, exp, alt = [], [], []
        flag1, flag2 = [], []
        slot = [0]
        th = 3.0

        def site():
            s = slot[0]
            slot[0] += 1
            return 53.0 + 50.0 * (s % 10), 53.0 + 50.0 * (s // 10)

        def feat(kf, idx, x, y, octave, desc, level, mp_desc, **pk):
            """Feature idx of keyframe kf at (x, y) carrying a map point that projects to (x, y)."""
            k[kf].put(idx, x, y, octave, desc)
            mp[kf][idx] = point(x, y, level, mp_desc, **pk)

        def plain(kf, idx, x, y, octave, desc):
            k[kf].put(idx, x, y, octave, desc)

        if family == "tie":
            # 1: forward tie decided by grid order, backward unique: agreement only under the rule
            u, v = site()
            q, back = rand_desc(rng), rand_desc(rng)
            feat(0, 3, u, v, L3, desc_at(back, 0, rng), L3, q)
            feat(1, 100, u - 2, v, L3, desc_at(q, 20, rng), L3, back)        # earlier cell: wins
            plain(1, 5, u + 3, v, L3, desc_at(q, 20, rng))
            des.append(3); exp.append(100); alt.append(-1)                   # noqa: E702
            # 2: backward tie broken towards another feature of keyframe 1: agreement fails
            u, v = site()
            q, back = rand_desc(rng), rand_desc(rng)
            feat(0, 4, u + 3, v, L3, desc_at(back, 20, rng), L3, q)          # later cell, low idx
            plain(0, 90, u - 2, v, L3, desc_at(back, 20, rng))               # earlier cell: wins
            feat(1, 6, u, v, L3, desc_at(q, 10, rng), L3, back)
            des.append(4); exp.append(-1); alt.append(6)                     # noqa: E702
            # 3: ties in both directions, same lane of different rounds (c, c + 64), one cell
            u, v = site()
            q, back = rand_desc(rng), rand_desc(rng)
            feat(0, 7, u - 2, v, L3, desc_at(back, 20, rng), L3, q)
            plain(0, 71, u - 1, v - 1, L3, desc_at(back, 20, rng))
            feat(1, 8, u - 2, v - 1, L3, desc_at(q, 20, rng), L3, back)
            plain(1, 72, u - 1, v, L3, desc_at(q, 20, rng))
            des.append(7); exp.append(8); alt.append(-1)                     # noqa: E702
            # 4: the tied keypoint that is last in grid order carries the point that comes back
            u, v = site()
            q, back = rand_desc(rng), rand_desc(rng)
            feat(0, 9, u, v, L3, desc_at(back, 0, rng), L3, q)
            plain(1, 129, u - 2, v, L3, desc_at(q, 20, rng))
            feat(1, 10, u + 3, v, L3, desc_at(q, 20, rng), L3, back)
            des.append(9); exp.append(-1); alt.append(10)                    # noqa: E702
        elif family == "threshold":
            for idx, d_fwd, d_back, e, a in ((3, 100, 0, 20, -1), (4, 101, 0, -1, 21),
                                             (5, 0, 100, 22, -1), (6, 0, 101, -1, 23)):
                u, v = site()
                q, back = rand_desc(rng), rand_desc(rng)
                feat(0, idx, u, v, L3, desc_at(back, d_back, rng), L3, q)
                feat(1, 17 + idx, u + 1, v + 1, L3, desc_at(q, d_fwd, rng), L3, back)
                des.append(idx); exp.append(e); alt.append(a)                # noqa: E702
            # vbAlreadyMatched1 / 2 (:1117-1129): a flagged feature is not searched, in either
            # direction, however good its candidate
            flag1, flag2 = [7], [17 + 8]
            for idx in (7, 8, 9, 10):
                u, v = site()
                q, back = rand_desc(rng), rand_desc(rng)
                feat(0, idx, u, v, L3, back, L3, q)
                feat(1, 17 + idx, u + 1, v + 1, L3, desc_at(q, 5, rng), L3, back)
                des.append(idx); exp.append(-1); alt.append(17 + idx)        # noqa: E702
            # and so is a feature without a map point, or with a bad one (:1136, :1216)
            mp[0][9]["skip"] = 1
            mp[1][17 + 10]["skip"] = 1
        else:
            th, r = radius_th(0, 2.0)
            g = 1 / 4096.0
            # (dx of the keyframe-2 keypoint, its octave, level of the point, point kwargs, hit)
            # the gate under test is the forward one: keyframe 1's point projects to uv, keyframe
            # 2's keypoint sits at uv + d; its own point comes back onto keyframe 1's keypoint
            # (at the same pixel, distance 0), so the agreement hangs on the forward search alone
            # (uv or None = the next site, d, keypoint octave, point level, point kwargs, hit)
            rows = [(None, (r, 0), 0, 0, {}, False), (None, (r - g, 0), 0, 0, {}, True),
                    (None, (0, -r), 0, 0, {}, False),
                    (None, (1, 0), 1, 3, {}, False), (None, (1, 0), 2, 3, {}, True),
                    (None, (1, 0), 4, 3, {}, False), (None, (1, 0), 3, 3, {}, True),
                    (None, (1, 0), 1, 1, dict(ratio=1.2 ** 0.1), True),
                    (None, (1, 0), 7, 7, dict(ratio=1.2 ** 8.5), True),
                    (None, (1, 0), 3, 3, dict(z=-Z), False),
                    ((0.0, 203.0), (1, 0), 0, 0, {}, True),
                    ((253.0, 0.0), (0, 1), 0, 0, {}, True),
                    ((640.0, 253.0), (-6, 0), 7, 7, {}, False),
                    ((640.0 - 1 / 64.0, 303.0), (-6, 0), 7, 7, {}, True)]
            # max_dist / dist3D at scale[3] and one ulp either side: level 3 (octaves 2 .. 3) or 4
            # (3 .. 4) as the correctly rounded logf says
            for target, n in ratio_edges(3):
                assert n in (3, 4)
                rows += [(None, (1, 0), 2, 3, dict(edge=target), n == 3),
                         (None, (1, 0), 4, 3, dict(edge=target), n == 4)]
            for i, (uv, d, octave, level, pk, hit) in enumerate(rows):
                u, v = site() if uv is None else uv
                if "edge" in pk:
                    while True:
                        m = max_dist_for_ratio(norm3([(u - CAM[2]) * Z / CAM[0],
                                                      (v - CAM[3]) * Z / CAM[1], Z]), pk["edge"])
                        if m is not None:
                            break
                        u, v = site()
                    pk = dict(max_dist=m)
                q, back = rand_desc(rng), rand_desc(rng)
                x2, y2 = u + d[0], v + d[1]
                k[0].put(3 + i, x2, y2, octave, back)
                mp[0][3 + i] = point(u, v, level, q, **pk)
                k[1].put(40 + i, x2, y2, octave, desc_at(q, 5, rng))
                mp[1][40 + i] = point(u + int(d[0]), v + int(d[1]), octave, back)
                des.append(3 + i); exp.append(40 + i if hit else -1)         # noqa: E702
                alt.append(-1 if hit else 40 + i)
            # PosInGrid: x = 636 is cell 64, off the grid: never a candidate
            q, back = rand_desc(rng), rand_desc(rng)
            k[0].put(30, 630.0, 353.0, 7, back)
            mp[0][30] = point(633.0, 353.0, 7, q)
            k[1].put(70, 636.0, 353.0, 7, desc_at(q, 5, rng))
            k[1].put(71, 630.0, 353.0, 7, desc_at(q, 30, rng))
            mp[1][71] = point(630.0, 353.0, 7, back)
            des.append(30); exp.append(71); alt.append(-1)                   # noqa: E702
        a1, a2 = np.zeros(N_KF, np.uint8), np.zeros(N_KF, np.uint8)
        a1[flag1], a2[flag2] = 1, 1
        inp = dict(k1=k[0].kf(), k2=k[1].kf(), mp1=mp[0], mp2=mp[1], a1=a1, a2=a2, th=th)
        cite = {"tie": ":1198/:1278", "threshold": ":1207/:1287", "gates": ":1140-1196"}[family]
        out.append(Case("sim3", family, "sites", cite, inp, des, exp, alt, "match12"))
    return out


# ---- SearchForTriangulation ---------------------------------------------------------------------
def fundamental(T1, T2):
    """LocalMapper::ComputeF12 in float64, stored as float."""
    fx, fy, cx, cy, _ = CAM
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    R1, t1 = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64)
    R2, t2 = T2[:3, :3].astype(np.float64), T2[:3, 3].astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Ki = np.linalg.inv(K)
    return (Ki.T @ tx @ R12 @ Ki).astype(f32)


# pure x baseline of fy: F12 = [0 0 0; 0 0 -1; 0 1 0] exactly, the epipolar line of (x1, y1) is
# y = y1 with a = 0, b = 1, c = -y1, den = 1 and dsqr = (y2 - y1)^2 without rounding
F_X = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)


def _pose(t):
    T = np.eye(4, dtype=f32)
    T[:3, 3] = t
    return T


class _Tri:
    def __init__(self, seed, n1, nodes1, n2=N_KF):
        """nodes1: {node id: [pKF1 features]}; pKF2's candidates are added per node."""
        self.rng = np.random.default_rng(seed)
        self.n1, self.n2 = n1, n2
        mk = lambda n: dict(kps=np.zeros(n, KP_DTYPE), desc=rand_desc(self.rng, n),  # noqa: E731
                            ur=np.full(n, 5.0, f32), mp=np.zeros(n, np.uint8))
        self.k1, self.k2 = mk(n1), mk(n2)
        for k in (self.k1, self.k2):
            k["kps"]["x"] = 100.0 + np.arange(len(k["kps"]))
            k["kps"]["y"] = 100.0
        self.nodes1 = nodes1
        self.nodes2 = {n: [] for n in nodes1}
        self.used2 = set()

    def cand(self, node, idx2, q, dist, y=100.0, x=None, octave=0, ur=5.0, angle=0.0, mp=0):
        assert idx2 not in self.used2
        self.used2.add(idx2)
        k = self.k2
        k["desc"][idx2] = desc_at(q, dist, self.rng)
        k["kps"][idx2]["y"], k["kps"][idx2]["octave"] = y, octave
        if x is not None:
            k["kps"][idx2]["x"] = x
        k["kps"][idx2]["angle"] = angle
        k["ur"][idx2], k["mp"][idx2] = ur, mp
        self.nodes2[node].append(idx2)

    def fill2(self, node, upto):
        """Unrelated pKF2 features appended to the node until it holds `upto` candidates."""
        free = [j for j in range(self.n2) if j not in self.used2]
        while len(self.nodes2[node]) < upto:
            j = free.pop(0)
            self.used2.add(j)
            self.nodes2[node].append(j)

    def order2(self, node, order):
        assert sorted(order) == sorted(self.nodes2[node])
        self.nodes2[node] = list(order)

    def fv(self, nodes):
        ids = sorted(nodes)
        start = np.zeros(len(ids) + 1, np.int32)
        feats = []
        for i, n in enumerate(ids):
            feats += nodes[n]
            start[i + 1] = len(feats)
        return np.array(ids, np.uint32), start, np.array(feats, np.uint32)

    def inp(self, T1=None, T2=None, F=F_X, only_stereo=False, check_ori=False):
        self.k1["fv"], self.k2["fv"] = self.fv(self.nodes1), self.fv(self.nodes2)
        return dict(k1=self.k1, k2=self.k2, T1=_pose((0, 0, 0)) if T1 is None else T1,
                    T2=_pose((-CAM[1], 0, 0)) if T2 is None else T2, F=F,
                    only_stereo=only_stereo, check_ori=check_ori)


def _tri_cases(seed):
    out = []
    C = lambda fam, name, cite, inp, d, e, a: out.append(  # noqa: E731
        Case("tri", fam, name, cite, inp, d, e, a, "match12"))
    # -- tie: one node, 9 pKF1 features (more than the 8 waves), 130 candidates in three lane rounds
    T = _Tri(seed, 9, {7: list(range(9))})
    q = T.k1["desc"]
    # feature 0: tied at 20 in positions 3, 70, 129 of the node (lanes 3, 6, 1; rounds 0, 1, 2)
    # feature 1: exactly 50 (kept) ; feature 2: 51 only ; feature 3: tied in one lane (c, c + 64)
    # feature 4: tied in one round ; feature 5: distance 5 off the epipolar line + 30 on it
    # feature 6: the last tied candidate fails the epipolar gate: the one before it stays
    # feature 7: the last tied candidate has a map point ; feature 8: nothing in reach
    T.fill2(7, 130 - 16)
    for idx2, (f, d, kw) in zip(
            range(114, 130),
            [(0, 20, {}), (0, 20, {}), (0, 20, {}), (1, 50, {}), (2, 51, {}), (3, 20, {}),
             (3, 20, {}), (4, 20, {}), (4, 20, {}), (5, 5, dict(y=110.0)), (5, 30, {}),
             (6, 20, {}), (6, 20, dict(y=103.0)), (7, 20, {}), (7, 20, dict(mp=1)),
             (0, 21, {})]):
        T.cand(7, idx2, q[f], d, **kw)
    # node order: place the designated pKF2 features at chosen positions among the fillers
    fill = [j for j in T.nodes2[7] if j < 114]
    order = [None] * 130
    place = {3: 114, 70: 115, 129: 116, 10: 117, 20: 118, 5: 119, 69: 120, 64: 121, 100: 122,
             30: 123, 31: 124, 40: 125, 90: 126, 50: 127, 128: 128, 0: 129}
    for p, j in place.items():
        order[p] = j
    it = iter(fill)
    order = [next(it) if j is None else j for j in order]
    T.order2(7, order)
    C("tie", "one_node", ":717", T.inp(), range(9),
      [116, 117, -1, 120, 122, 124, 125, 127, -1], [114, -1, 118, 119, 121, 123, 126, 128, 0])
    # -- three nodes, 17 entries; a node pKF2 lacks and one pKF1 lacks; a better candidate in
    # another node is never seen (:671: only the features of the same node are compared)
    T = _Tri(seed + 1, 17, {3: list(range(6)), 9: list(range(6, 12)), 40: list(range(12, 17))})
    q = T.k1["desc"]
    T.nodes2 = {3: [], 40: [], 55: []}
    T.cand(3, 10, q[0], 20); T.cand(3, 11, q[0], 20)                       # noqa: E702
    T.cand(40, 12, q[0], 5)                                                  # another node
    T.cand(3, 13, q[5], 50)
    T.cand(40, 14, q[12], 20); T.cand(40, 80, q[12], 20)                   # noqa: E702
    T.cand(55, 15, q[6], 0)                                                  # node 9 != 55: no match
    T.fill2(3, 65); T.fill2(40, 64)                                        # noqa: E702
    T.order2(3, [10] + [j for j in T.nodes2[3] if j not in (10, 11, 13)] + [11, 13])
    T.order2(40, [14, 12] + [j for j in T.nodes2[40] if j not in (12, 14, 80)] + [80])
    C("tie", "three_nodes", ":717", T.inp(), [0, 5, 6, 12], [11, 13, -1, 80], [12, -1, 15, 14])
    # -- dist <= TH_LOW: 50 is kept, 51 is not, two candidates at 50 are a tie like any other
    T = _Tri(seed + 7, 9, {7: list(range(9))})
    q = T.k1["desc"]
    T.cand(7, 0, q[0], 50); T.cand(7, 1, q[1], 51)                         # noqa: E702
    T.cand(7, 4, q[3], 50); T.cand(7, 5, q[3], 50)                         # noqa: E702
    T.fill2(7, 70)
    C("threshold", "th_low", ":717", T.inp(), [0, 1, 3], [0, -1, 5], [-1, 1, 4])
    # -- u_right: >= 0 is stereo (exactly 0 included), -1 is mono; only_stereo drops the mono ones
    T = _Tri(seed + 2, 9, {7: list(range(9))})
    q = T.k1["desc"]
    T.cand(7, 0, q[0], 20); T.cand(7, 1, q[0], 20, ur=0.0); T.cand(7, 2, q[0], 20, ur=-1.0)  # noqa
    T.cand(7, 3, q[1], 20)
    T.k1["ur"][1] = -1.0                                                     # mono pKF1 feature
    T.cand(7, 4, q[2], 20)
    T.k1["ur"][2] = 0.0                                                      # stereo at exactly 0
    T.fill2(7, 70)
    C("u_right", "only_stereo", ":688/:708", T.inp(only_stereo=True), [0, 1, 2], [1, -1, 4],
      [0, 3, -1])
    # -- epipolar gate dsqr < 3.84 * sigma2 (y1 = 0: y2 itself is the distance, without rounding)
    T = _Tri(seed + 3, 9, {7: list(range(9))})
    q = T.k1["desc"]
    T.k1["kps"]["y"] = 0.0
    for octave, f_in, f_out in ((0, 0, 1), (2, 2, 3)):
        lim = 3.84 * float(f32(SC[octave] * SC[octave]))
        y = f32(np.sqrt(lim))
        while float(f32(y * y)) < lim:
            y = np.nextafter(y, f32(np.inf), dtype=f32)
        while not float(f32(y * y)) < lim:
            y = np.nextafter(y, f32(-np.inf), dtype=f32)
        T.cand(7, 10 + f_in, q[f_in], 5, y=float(y), octave=octave)              # largest inside
        T.cand(7, 20 + f_in, q[f_in], 30, y=0.0, octave=octave)
        T.cand(7, 10 + f_out, q[f_out], 5, octave=octave,
               y=float(np.nextafter(y, f32(np.inf), dtype=f32)))                # smallest outside
        T.cand(7, 20 + f_out, q[f_out], 30, y=0.0, octave=octave)
    # sigma2 is the candidate's level's: the same offset passes at level 2 and fails at level 0
    T.cand(7, 40, q[4], 5, y=2.5, octave=0); T.cand(7, 41, q[4], 30, y=0.0)   # noqa: E702
    T.cand(7, 42, q[5], 5, y=2.5, octave=2); T.cand(7, 43, q[5], 30, y=0.0)   # noqa: E702
    T.fill2(7, 70)
    C("epipolar", "edge", ":114-131", T.inp(), range(6), [10, 21, 12, 23, 41, 42],
      [20, 11, 22, 13, 40, 43])
    # -- den == 0: F12 = 0 makes every line degenerate, nothing matches (:124)
    T = _Tri(seed + 4, 9, {7: list(range(9))})
    T.cand(7, 3, T.k1["desc"][0], 20)
    T.fill2(7, 70)
    C("den_zero", "zero_F", ":124", T.inp(F=np.zeros((3, 3), f32)), [0], [-1], [3])
    # -- epipole exclusion, both features mono: dist^2 < 100 * scale[octave] is skipped. Forward
    # motion puts the epipole at (cx, cy); the lines are radial, all keypoints on y = cy.
    T = _Tri(seed + 5, 9, {7: list(range(9))})
    q = T.k1["desc"]
    T1, T2 = _pose((0, 0, 0)), _pose((0, 0, -1.0))
    for k in (T.k1, T.k2):
        k["kps"]["y"] = CAM[3]
        k["ur"][:] = -1.0
    T.k1["kps"]["x"] = 200.0
    cases = [(0, CAM[2] - 10.0, 0, True),                                       # d2 == 100: kept
             (1, float(np.nextafter(f32(CAM[2] - 10.0), f32(np.inf), dtype=f32)), 0, False),
             (2, CAM[2] - 11.5, 2, False), (3, CAM[2] - 12.5, 2, True)]          # 100 * 1.44 = 144
    for f, x, octave, hit in cases:
        T.cand(7, 10 + f, q[f], 5, x=x, y=CAM[3], octave=octave, ur=-1.0)
        T.cand(7, 20 + f, q[f], 30, x=100.0, y=CAM[3], ur=-1.0)
    # a stereo candidate inside the circle is not excluded (:694 needs both mono)
    T.cand(7, 14, q[4], 5, x=CAM[2] - 5.0, y=CAM[3], ur=3.0)
    T.cand(7, 24, q[4], 30, x=100.0, y=CAM[3], ur=-1.0)
    T.fill2(7, 70)
    C("epipole", "edge", ":694-700", T.inp(T1=T1, T2=T2, F=fundamental(T1, T2)), range(5),
      [10, 21, 22, 13, 14], [20, 11, 12, 23, 24])
    # -- rotation histogram
    out += _tri_hist_cases(seed + 6)
    return out


def half_rot(k):
    """A float rot with rot * (1 / 30f) == k + 0.5 exactly in float arithmetic."""
    factor = f32(1.0) / f32(30.0)
    r = f32((k + 0.5) * 30.0)
    for _ in range(64):
        p = f32(r * factor)
        if p == f32(k + 0.5):
            return float(r)
        r = np.nextafter(r, f32(-np.inf) if p > k + 0.5 else f32(np.inf), dtype=f32)
    raise AssertionError("no such rot")


HALF_ROT = half_rot(4)      # 135.0: 135 * (1 / 30f) is 4.5 exactly

def hist_plans():
    """name -> (list of (rot of the match, base angle), expected kept mask, alt kept mask). rot is
    angle1 - angle2 as the matchers form it; bin = round(rot' / 30) with rot' = rot + 360 if rot < 0."""
    plans = {}

    def plan(name, groups, kept_bins, alt_bins):
        rows, exp, alt = [], [], []
        for b, cnt, rot in groups:
            for _ in range(cnt):
                rows.append(rot)
                exp.append(b in kept_bins)
                alt.append(b in alt_bins)
        plans[name] = (rows, exp, alt)
    # max2 == 0.1f * max1 is kept (strict <): 10/1/1, 20/2, 30/3; 11/1 is dropped
    plan("ten_one_one", [(5, 10, 150.0), (9, 1, 270.0), (2, 1, 60.0)], {5, 9, 2}, {5})
    plan("twenty_two", [(5, 20, 150.0), (9, 2, 270.0)], {5, 9}, {5})
    plan("thirty_three", [(5, 30, 150.0), (9, 3, 270.0)], {5, 9}, {5})
    plan("eleven_one", [(5, 11, 150.0), (9, 1, 270.0)], {5}, {5, 9})
    # equal counts in four bins: strict > keeps the three earlier bins
    plan("four_equal", [(3, 5, 90.0), (7, 5, 210.0), (11, 5, 330.0), (1, 5, 30.0)], {1, 3, 7},
         {3, 7, 11})
    # two bins equal behind a larger one, a fourth equal bin later: the earlier two stay
    plan("two_equal", [(8, 6, 240.0), (4, 3, 120.0), (10, 3, 300.0), (12, 3, 355.0)], {8, 4, 10},
         {8, 10, 12})
    # rot exactly 0 (bin 0, 11 of them); a tiny negative rot becomes 360.0f, bin 12, alone: dropped
    # (a wrap to bin 0 would keep it); rot * (1 / 30f) == 4.5 rounds away from zero to bin 5, where
    # a rot of 150 keeps it company (rint would send it to bin 4, alone)
    plan("edges", [(0, 11, 0.0), (12, 1, -1.0e-6), (5, 1, HALF_ROT), (5, 1, 150.0)], {0, 5},
         {0, 5, 12})
    plans["edges"][2][12] = False        # alt: the 4.5 one lands in bin 4 and is dropped
    return plans


def _tri_hist_cases(seed, entry="tri", cite_off=":750", **extra):
    """The rotation-histogram plans as SearchForTriangulation pairs; with entry "bow" (and extra =
    its kf_kf and nnratio) the same keyframes, angle sets and expectations through SearchByBoW:
    every match is at distance 10 with no second candidate below 90."""
    out = []
    for name, (rots, exp, alt) in hist_plans().items():
        n1 = len(rots)
        T = _Tri(seed, n1, {7: list(range(n1))})
        seed += 1
        q = T.k1["desc"]
        for i, rot in enumerate(rots):
            a1, a2 = rot_angles(rot, i)
            T.k1["kps"][i]["angle"] = a1
            T.cand(7, i, q[i], 10, angle=a2)
        T.fill2(7, 70)
        e = [i if k else -1 for i, k in enumerate(exp)]
        a = [i if k else -1 for i, k in enumerate(alt)]
        des = [i for i in range(n1) if e[i] != a[i]]
        sup = {i: e[i] for i in range(n1) if e[i] == a[i]}
        out.append(Case(entry, "histogram", name, ":1584-1625", dict(T.inp(check_ori=True), **extra),
                        des, [e[i] for i in des], [a[i] for i in des], "match12", support=sup))
        if name == "edges":
            inp = dict(T.inp(), check_ori=False, **extra)
            des = [i for i in range(n1) if e[i] < 0]
            out.append(Case(entry, "check_ori_off", name, cite_off, inp, des, des,
                            [-1] * len(des), "match12",
                            support={i: i for i in range(n1) if e[i] >= 0}))
    return out


def rot_angles(rot, i):
    """(angle1, angle2), both in [0, 360), with angle1 - angle2 == rot in float arithmetic."""
    if rot < 0:
        a1, a2 = f32(0.0), f32(-rot)
    elif rot != int(rot):
        a1, a2 = f32(rot), f32(0.0)
    else:
        a2 = f32(i % 4)
        a1 = f32(a2 + f32(rot))
    assert float(f32(a1 - a2)) == float(f32(rot)) and 0 <= a1 < 360 and 0 <= a2 < 360
    return a1, a2


# ---- SearchByBoW (its ties are constructed in test_bow_gpu.py; here its comparisons) --------------
def _bow_cases(seed):
    """SearchByBoW (orb_matcher.cpp:133-262 Frame overload, :499-632 keyframe pair): bestDist1 <=
    TH_LOW (:202) against < TH_LOW (:575), the ratio test (float)bestDist1 < mfNNratio *
    (float)bestDist2 with a strict <, a tied minimum (bestDist2 == bestDist1: no match for any
    ratio <= 1), and a keypoint already taken by an earlier feature of the node."""
    out = []
    for kf_kf, rows, name in ((False, [(50, True), (51, False)], "frame_le"),
                              (True, [(50, False), (49, True)], "kf_kf_lt")):
        T = _Tri(seed, 9, {7: list(range(9))})
        q = T.k1["desc"]
        for f, (d, hit) in enumerate(rows):
            T.cand(7, 10 + f, q[f], d)
        T.fill2(7, 130)
        inp = dict(T.inp(), kf_kf=kf_kf, nnratio=1.0)
        out.append(Case("bow", "threshold", name, ":575" if kf_kf else ":202", inp, [0, 1],
                        [10 + f if hit else -1 for f, (d, hit) in enumerate(rows)],
                        [-1 if hit else 10 + f for f, (d, hit) in enumerate(rows)], "match12"))
    T = _Tri(seed + 1, 9, {7: list(range(9))})
    q = T.k1["desc"]
    T.cand(7, 10, q[0], 40); T.cand(7, 74, q[0], 50)      # 40 < 0.8f * 50 is false: no match
    T.cand(7, 11, q[1], 39); T.cand(7, 75, q[1], 50)      # noqa: E702
    T.cand(7, 12, q[2], 20); T.cand(7, 76, q[2], 20)      # a tie: bestDist2 == bestDist1
    # features 3 and 4 both want 13; 3 comes first in the node, 4 falls to 77
    T.cand(7, 13, q[3], 10)
    T.k1["desc"][4] = desc_at(T.k2["desc"][13], 5, T.rng)
    T.cand(7, 77, T.k1["desc"][4], 30)
    T.fill2(7, 130)
    inp = dict(T.inp(), kf_kf=False, nnratio=0.8)
    out.append(Case("bow", "ratio", "nn08", ":204/:186", inp, [0, 2, 4], [-1, -1, 77],
                    [10, 12, 13], "match12", support={1: 11, 3: 13}))
    # the rotation histogram (:210-220 bins, :241-259 removal) on the triangulation cases' angle
    # sets, and the same matches with mbCheckOrientation off
    out += _tri_hist_cases(seed + 2, "bow", ":241", kf_kf=False, nnratio=0.6)
    return out


# ---- all keyframe-matcher cases -------------------------------------------------------------------
_kf_cases = None


def kf_cases():
    global _kf_cases
    if _kf_cases is None:
        out = _tri_cases(100)
        for e, s in (("fuse", 200), ("fuse_sim3", 300), ("sbp_sim3", 400)):
            for i, fam in enumerate(("tie", "threshold", "gates")):
                out.append(_scw_case(e, fam, s + i))
        out.append(_scw_case("fuse", "chi_square", 205))
        out.append(_best_dist_case("fuse", 210))
        out.append(_best_dist_case("fuse_sim3", 310))
        out.append(_claims_case(410))
        out += _sim3_cases(500)
        out += _bow_cases(600)
        for c in out:
            assert (c.expected != c.alt).all(), c.id
        _kf_cases = out
    return _kf_cases


# ==== the frame matchers: frame-to-frame, local-map, relocalisation ==============================
# The frame is the left image of synthetic.stereo_pair(FRAME_SEED, 640, 240) through the extractor
# at FRAME_ORB; its keypoints, descriptors and u_right are the caller's (the oracle's, asserted
# equal to the device's). Camera fx = fy = 512, cx = 320, cy = 120: with z = 8 the identity pose
# projects ((u - 320) / 64, (v - 120) / 64, 8) to (u, v) on the 1/64 px grid without rounding.
FRAME_SEED, FW, FH = 77, 640, 240
FRAME_ORB = (600, 1.2, 4, 20, 7)
FCAM = (512.0, 512.0, 320.0, 120.0, 256.0)
F2F_QUERY_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("last_angle", "<f4"), ("last_octave", "<i4"),
                            ("mp_id", "<i4"), ("blocks", "<i4"), ("pad", "<i4"),
                            ("desc", "u1", (32,))])
F2F_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("tlc_z", "<f4"),
                           ("baseline", "<f4"), ("th", "<f4"), ("mono", "<i4"),
                           ("check_ori", "<i4"), ("pad", "<i4")])
MPS_QUERY_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"),
                            ("view_cos", "<f4"), ("level", "<i4"), ("in_view", "<i4"),
                            ("is_bad", "<i4"), ("mp_id", "<i4"), ("blocks", "<i4"),
                            ("pad", "<i4", (3,)), ("desc", "u1", (32,))])
RELOC_QUERY_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("max_dist", "<f4"), ("min_dist", "<f4"),
                              ("kf_angle", "<f4"), ("mp_id", "<i4"), ("skip", "<i4"),
                              ("desc", "u1", (32,))])
RELOC_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)),
                             ("th", "<f4"), ("orb_dist", "<i4"), ("check_ori", "<i4")])
PRE_ID = 5000         # map point ids of slots occupied at entry are PRE_ID + keypoint


def r64(x):
    return float(np.round(float(x) * 64.0) / 64.0)


def f_xyz(u, v, z=Z):
    xyz = np.array([(u - FCAM[2]) * z / FCAM[0], (v - FCAM[3]) * z / FCAM[1], z], f32)
    assert float(xyz[0]) * FCAM[0] / z + FCAM[2] == u and float(xyz[1]) * FCAM[1] / z + FCAM[3] == v
    return xyz


def angle_for(a2, rot):
    """angle1 in [0, 360) such that the matchers' rot = angle1 - angle2 (+ 360 if negative) is
    exactly `rot` in float arithmetic."""
    a2 = f32(a2)
    for base in (float(a2) + rot, float(a2) + rot - 360.0):
        if not 0 <= base < 360:
            continue
        a1 = f32(base)
        for _ in range(2):
            for cand in (a1, np.nextafter(a1, f32(np.inf), dtype=f32),
                         np.nextafter(a1, f32(-np.inf), dtype=f32)):
                r = f32(cand - a2)
                if r < 0:
                    r = f32(r + f32(360.0))
                if float(r) == float(f32(rot)) and 0 <= cand < 360:
                    return cand
            a1 = np.nextafter(np.nextafter(a1, f32(np.inf), dtype=f32), f32(np.inf), dtype=f32)
    raise AssertionError(f"no angle for rot {rot} from {a2}")


class FrameSites:
    """Sites of a frame: isolated keypoints and close pairs without a third keypoint near, all
    with u_right <= 0 (the u_right gate of :1395 / :65 then never applies)."""

    def __init__(self, kps, desc, ur, scale, seed):
        self.kps, self.desc, self.ur, self.scale = kps, desc, ur, np.asarray(scale, f32)
        self.n = len(kps)
        self.rng = np.random.default_rng(seed)
        x, y = kps["x"].astype(np.float64), kps["y"].astype(np.float64)
        D = np.maximum(np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :]))
        np.fill_diagonal(D, 1e9)
        self.D = D
        self.free = np.asarray(ur) <= 0
        self.inside = (x > 30) & (x < FW - 30) & (y > 30) & (y < FH - 30)
        self.used = set()
        self.cell = np.floor(x / (FW / 64.0) + 0.5).astype(int) * 48 + \
            np.floor(y / (FH / 48.0) + 0.5).astype(int)

    def single(self, iso=9.0, octave=None, pred=None):
        for j in range(self.n):
            if j in self.used or not (self.free[j] and self.inside[j]) or self.D[j].min() <= iso:
                continue
            if octave is not None and self.kps["octave"][j] not in np.atleast_1d(octave):
                continue
            if pred is not None and not pred(j):
                continue
            self.used.add(j)
            return j
        raise AssertionError("no isolated keypoint left")

    def pair(self, want, reach=3.0):
        """The next pair (a, b), a < b, at most `reach` px apart for which want(a, b) returns
        something (returned with the pair); want checks the window with alone()."""
        for a in range(self.n):
            if a in self.used or not (self.free[a] and self.inside[a]):
                continue
            for b in range(a + 1, self.n):
                if b in self.used or not self.free[b] or self.D[a, b] > reach:
                    continue
                w = want(a, b)
                if w is not None:
                    self.used.update((a, b))
                    return a, b, w
        raise AssertionError("no pair left")

    def thirds(self, a, b, r):
        """The other keypoints within r + 1 px (Chebyshev) of the pair's midpoint."""
        u, v = self.mid(a, b)
        x, y = self.kps["x"].astype(np.float64), self.kps["y"].astype(np.float64)
        near = (np.abs(x - u) < r + 1.0) & (np.abs(y - v) < r + 1.0)
        assert near[a] and near[b]
        return [int(j) for j in np.nonzero(near)[0] if j not in (a, b)]

    def alone(self, a, b, r):
        return not self.thirds(a, b, r)

    def mid(self, a, b):
        return (r64((self.kps["x"][a] + self.kps["x"][b]) / 2),
                r64((self.kps["y"][a] + self.kps["y"][b]) / 2))

    def at(self, j):
        return r64(self.kps["x"][j]), r64(self.kps["y"][j])

    def first(self, a, b):
        """The one GetFeaturesInArea (frame.cpp:348-403) returns first, and the other."""
        return (a, b) if (self.cell[a], a) < (self.cell[b], b) else (b, a)

    def octv(self, j):
        return int(self.kps["octave"][j])


class _FrameCase:
    """Queries of one call of a frame matcher; q() appends one for the entry point."""

    def __init__(self, entry, FS):
        self.entry, self.FS = entry, FS
        self.rows = []
        self.des, self.exp, self.alt, self.support = [], [], [], {}
        self.mp0 = np.full(FS.n, -1, np.int32)

    def q(self, u, v, level, desc, angle=0.0, blocks=1, z=Z, view_cos=0.9, px=None, ratio=None):
        """level: the last frame's octave (f2f), the predicted level (mps, reloc)."""
        i = len(self.rows)
        if self.entry == "f2f":
            r = np.zeros(1, F2F_QUERY_DTYPE)
            r["xyz"][0] = f_xyz(u, v, z)
            r["last_angle"], r["last_octave"], r["blocks"] = angle, level, blocks
        elif self.entry == "mps":
            r = np.zeros(1, MPS_QUERY_DTYPE)
            r["proj_x"], r["proj_y"] = (u if px is None else px), v
            r["proj_xr"] = r["proj_x"] - f32(FCAM[4] / Z)
            r["view_cos"], r["level"], r["in_view"], r["blocks"] = view_cos, level, 1, blocks
        else:
            r = np.zeros(1, RELOC_QUERY_DTYPE)
            xyz = f_xyz(u, v, z)
            d = norm3(xyz)
            r["xyz"][0] = xyz
            r["max_dist"] = f32(float(d) * (1.2 ** (level - 0.5) if ratio is None else ratio))
            r["min_dist"] = f32(float(r["max_dist"][0]) / 1.2 ** 7)
            r["kf_angle"] = angle
        r["mp_id"] = i
        r["desc"][0] = desc
        self.rows.append(r[0])
        return i

    def want(self, kp, expected, alt):
        if alt is None:
            self.support[kp] = expected
        else:
            self.des.append(kp); self.exp.append(expected); self.alt.append(alt)  # noqa: E702

    def occupy(self, kp):
        self.mp0[kp] = PRE_ID + kp
        self.support[kp] = PRE_ID + kp

    def case(self, family, name, cite, th, pose_kw=None, nnratio=0.8):
        dt = {"f2f": F2F_QUERY_DTYPE, "mps": MPS_QUERY_DTYPE, "reloc": RELOC_QUERY_DTYPE}
        q = np.array(self.rows, dt[self.entry])
        pk = dict(pose_kw or {})
        if self.entry == "f2f":
            pose = np.zeros(1, F2F_POSE_DTYPE)
            pose["Rcw"] = np.eye(3, dtype=f32).reshape(-1)
            pose["baseline"] = f32(FCAM[4]) / f32(FCAM[0])
            pose["th"], pose["check_ori"] = th, pk.get("check_ori", 0)
            pose["tlc_z"] = pk.get("tlc_z", 0.0)
        elif self.entry == "reloc":
            pose = np.zeros(1, RELOC_POSE_DTYPE)
            pose["Rcw"] = np.eye(3, dtype=f32).reshape(-1)
            pose["th"], pose["orb_dist"] = th, pk.get("orb_dist", 100)
            pose["check_ori"] = pk.get("check_ori", 0)
        else:
            pose = None
        inp = dict(q=q, pose=pose, mp0=self.mp0, th=th, nnratio=nnratio)
        return Case(self.entry, family, name, cite, inp, self.des, self.exp, self.alt, "map_point",
                    support=self.support)


FCITE = {"f2f": {"tie": ":1406", "threshold": ":1415", "claims": ":1391", "level_window": ":1378",
                 "depth_sign": ":1359", "histogram": ":1584-1625", "check_ori_off": ":1418"},
         "mps": {"tie": ":76", "threshold": ":90", "claims": ":60", "level_window": ":47",
                 "ratio": ":84-93", "window": "frame.cpp:390", "view_cos": ":105-111"},
         "reloc": {"tie": ":1534", "threshold": ":1541", "claims": ":1526", "level_window": ":1514",
                   "depth_sign": ":1483", "histogram": ":1584-1625", "check_ori_off": ":1546"}}
BOUND = {"f2f": TH_HIGH, "mps": TH_HIGH, "reloc": 64}       # reloc: the case's ORBdist


def _tie_distance(FS, a, b, hi):
    """k with a descriptor at distance k from both a and b."""
    D = hamming(FS.desc[a], FS.desc[b])
    if D % 2:
        return None
    k = D // 2 + 8
    return k if k <= hi else None


def _frame_entry_cases(entry, kps, desc, ur, scale, seed):
    out = []
    th = 1 if entry == "mps" else 3.0
    bound = BOUND[entry]
    pk = dict(orb_dist=bound)
    cite = FCITE[entry]
    new = lambda: _FrameCase(entry, FrameSites(kps, desc, ur, scale, seed))  # noqa: E731

    def levels_for(FS, a, b):
        """The query level at which both keypoints are in the entry point's level window."""
        oa, ob = FS.octv(a), FS.octv(b)
        if abs(oa - ob) <= 1:                                 # mps: level - 1 .. level
            lv = max(oa, ob)
        elif abs(oa - ob) == 2 and entry != "mps":            # the others: level - 1 .. level + 1
            lv = (oa + ob) // 2
        else:
            return None
        r = (4.0 if entry == "mps" else 3.0) * float(FS.scale[lv])
        return lv if FS.alone(a, b, r) else None

    # ---- tie: the first in GetFeaturesInArea order wins (strict <) ----
    B = new()
    FS = B.FS
    for order_differs in (True, False, False):
        def want(a, b):
            k = _tie_distance(FS, a, b, bound)
            lv = levels_for(FS, a, b)
            if k is None or lv is None:
                return None
            if entry == "mps" and FS.octv(a) == FS.octv(b):
                return None                       # equal levels: the ratio test rejects a tie
            if order_differs and FS.first(a, b)[0] == a:
                return None                       # the later index comes first in the grid
            return k, lv
        a, b, (k, lv) = FS.pair(want)
        u, v = FS.mid(a, b)
        B.q(u, v, lv, desc_at2(desc[a], desc[b], k, k, FS.rng))
        w, l = FS.first(a, b)
        B.want(w, len(B.rows) - 1, -1)
        B.want(l, -1, len(B.rows) - 1)
    out.append(B.case("tie", "pairs", cite["tie"], th, pk))

    # ---- threshold: dist <= bound ----
    B = new()
    FS = B.FS
    for d, hit in ((bound, True), (bound + 1, False), (bound - 1, True)):
        j = FS.single()
        u, v = FS.at(j)
        i = B.q(u, v, FS.octv(j), desc_at(desc[j], d, FS.rng))
        B.want(j, i if hit else -1, -1 if hit else i)
    out.append(B.case("threshold", "singles", cite["threshold"], th, pk))

    # ---- level window ----
    B = new()
    FS = B.FS
    if entry == "mps":
        rows = [(0, True), (1, True), (-1, False), (2, False)]          # level - octave
    else:
        rows = [(-1, True), (0, True), (1, True), (2, False), (-2, False)]
    for dl, hit in rows:
        j = FS.single(octave=[o for o in range(4) if 0 <= o + dl <= 3])
        u, v = FS.at(j)
        i = B.q(u, v, FS.octv(j) + dl, desc_at(desc[j], 10, FS.rng))
        B.want(j, i if hit else -1, -1 if hit else i)
    if entry == "reloc":
        # PredictScale(dist, Frame*) clamps to nlevels - 1 (map_point.cpp:382-396): 1.2^4.5 is level
        # 5 of 4 -> 3, window 2 .. 4; unclamped (4 .. 6, and scale[5]) nothing would match
        j = FS.single(octave=[2, 3])
        u, v = FS.at(j)
        i = B.q(u, v, 3, desc_at(desc[j], 10, FS.rng), ratio=1.2 ** 4.5)
        B.want(j, i, -1)
        # max_dist / dist3D at scale[1] exactly and one ulp either side: level 1 (octaves 0 .. 2)
        # or 2 (1 .. 3) as the correctly rounded logf says; the keypoint is of octave 0
        for target, n in ratio_edges(1, FS.scale):
            assert n in (1, 2)
            while True:
                j = FS.single(octave=0)
                u, v = FS.at(j)
                m = max_dist_for_ratio(norm3(f_xyz(u, v)), target)
                if m is not None:
                    break
            i = B.q(u, v, 1, desc_at(desc[j], 10, FS.rng))
            B.rows[i]["max_dist"] = m
            B.rows[i]["min_dist"] = f32(float(m) / 1.2 ** 7)
            B.want(j, i if n == 1 else -1, -1 if n == 1 else i)
    out.append(B.case("level_window", "pm1" if entry != "mps" else "lvl_minus_1",
                      cite["level_window"], th, pk))
    if entry != "mps":
        # search window fabs(dx) < r, r = th * scale[0] = 3 (frame.cpp:390): an octave-0 keypoint
        # (integer coordinates) exactly 3 px from the projection is outside, 1/64 px nearer inside
        B = new()
        FS = B.FS
        for off, axis, hit in ((3.0, 0, False), (3.0 - 1 / 64.0, 0, True), (3.0, 1, False)):
            j = FS.single(octave=0)
            u, v = FS.at(j)
            assert (u, v) == (float(FS.kps["x"][j]), float(FS.kps["y"][j]))
            i = B.q(u - off if axis == 0 else u, v - off if axis == 1 else v, 0,
                    desc_at(desc[j], 10, FS.rng))
            B.want(j, i if hit else -1, -1 if hit else i)
        out.append(B.case("window", "edge", "frame.cpp:390", th, pk))
    if entry == "f2f":
        # forward (tlc_z > baseline): octave >= last octave, any higher; backward: <= last octave
        for name, tlc, rows in (("forward", 1.0, [(0, True), (-2, True), (1, False)]),
                                ("backward", -1.0, [(0, True), (2, True), (-1, False)])):
            B = new()
            FS = B.FS
            for dl, hit in rows:
                j = FS.single(octave=[o for o in range(4) if 0 <= o + dl <= 3])
                u, v = FS.at(j)
                i = B.q(u, v, FS.octv(j) + dl, desc_at(desc[j], 10, FS.rng))
                B.want(j, i if hit else -1, -1 if hit else i)
            out.append(B.case("level_window", name, ":1371-1376", th, dict(tlc_z=tlc)))

    # ---- depth sign: frame-to-frame skips invzc < 0 (:1359); relocalisation has no such gate ----
    if entry in ("f2f", "reloc"):
        B = new()
        FS = B.FS
        j = FS.single()
        u, v = FS.at(j)
        i = B.q(u, v, FS.octv(j), desc_at(desc[j], 10, FS.rng), z=-Z)
        hit = entry == "reloc"
        B.want(j, i if hit else -1, -1 if hit else i)
        out.append(B.case("depth_sign", "mirrored", cite["depth_sign"], th, pk))

    # ---- claims in order ----
    B = new()
    FS = B.FS
    # two queries, one keypoint: the first keeps it (a query that blocks)
    j = FS.single()
    u, v = FS.at(j)
    i0 = B.q(u, v, FS.octv(j), desc_at(desc[j], 20, FS.rng))
    i1 = B.q(u, v, FS.octv(j), desc_at(desc[j], 10, FS.rng))
    B.want(j, i0, i1)
    if entry != "f2f":
        # queries that are not searched, though each is the keypoint's best match: a point in
        # sAlreadyFound / bad (reloc :1470-1474), not in view or bad (local map :26-31); the
        # searched query behind them takes the keypoint
        j = FS.single()
        u, v = FS.at(j)
        i0 = B.q(u, v, FS.octv(j), desc_at(desc[j], 5, FS.rng))
        i1 = B.q(u, v, FS.octv(j), desc_at(desc[j], 5, FS.rng))
        i2 = B.q(u, v, FS.octv(j), desc_at(desc[j], 20, FS.rng))
        if entry == "reloc":
            B.rows[i0]["skip"] = B.rows[i1]["skip"] = 1
        else:
            B.rows[i0]["in_view"], B.rows[i1]["is_bad"] = 0, 1
        B.want(j, i2, i0)
    if entry == "f2f":
        # a map point without observations does not block (:1391-1393): the later query overwrites
        j = FS.single()
        u, v = FS.at(j)
        i0 = B.q(u, v, FS.octv(j), desc_at(desc[j], 10, FS.rng), blocks=0)
        i1 = B.q(u, v, FS.octv(j), desc_at(desc[j], 20, FS.rng))
        B.want(j, i1, i0)

    def want_chain(a, b):
        lv = levels_for(FS, a, b)
        D = hamming(desc[a], desc[b])
        if lv is None or D % 2 or D < 10 or D // 2 + 14 > bound:
            return None
        return lv, D
    # keypoints a and b, D apart: query 0 (D/2 + 4, D/2 + 14) takes a; query 1 (D/2 + 6, D/2 + 10)
    # loses a and falls to b; query 2 (D/2 + 14, D/2 + 4), whose best is b, finds both taken
    a, b, (lv, D) = FS.pair(want_chain)
    u, v = FS.mid(a, b)
    k = D // 2
    i0 = B.q(u, v, lv, desc_at2(desc[a], desc[b], k + 4, k + 14, FS.rng))
    i1 = B.q(u, v, lv, desc_at2(desc[a], desc[b], k + 6, k + 10, FS.rng))
    i2 = B.q(u, v, lv, desc_at2(desc[a], desc[b], k + 14, k + 4, FS.rng))
    B.want(a, i0, i1)
    B.want(b, i1, i2)

    # a slot occupied at entry that is the tied minimum and first in order: the other one is taken
    def want_pre(a, b):
        lv = levels_for(FS, a, b)
        k = _tie_distance(FS, a, b, bound)
        if lv is None or k is None:
            return None
        return lv, k
    a, b, (lv, k) = FS.pair(want_pre)
    w, l = FS.first(a, b)
    u, v = FS.mid(a, b)
    B.occupy(w)
    i = B.q(u, v, lv, desc_at2(desc[a], desc[b], k, k, FS.rng))
    B.want(l, i, -1)
    out.append(B.case("claims", "in_order", cite["claims"], th, pk, nnratio=1.0))

    if entry == "reloc":
        out.append(_reloc_chain_case(new, desc))
    else:
        out.append(_majority_chain_case(entry, new, desc))
    if entry == "mps":
        out += _mps_only_cases(new, desc, cite)
    else:
        out += _frame_hist_cases(entry, new, desc, cite, pk)
    return out


def _reloc_chain_case(new, desc, keep=6):
    """More offers of one point than the kernels keep candidates per query (kTopK = 6), so that
    the rescan decides a tie: ORBdist = 256 lets every keypoint of a wide window (th = 12, level
    1) in, and offer i takes the i-th keypoint in (distance, GetFeaturesInArea order). The query
    descriptor is at one distance k from two keypoints a and b that rank behind the sixth place;
    the one that comes first in the grid is claimed first (:1534, strict <)."""
    B = new()
    FS = B.FS
    th, pred = 12.0, 1
    r = float(f32(th) * FS.scale[pred])
    x, y = FS.kps["x"].astype(np.float64), FS.kps["y"].astype(np.float64)
    lvl_ok = FS.kps["octave"] <= pred + 1
    for j in np.nonzero(FS.inside)[0]:
        u, v = FS.at(j)
        dx, dy = np.abs(x - u), np.abs(y - v)
        if (lvl_ok & ((np.abs(dx - r) < 0.05) | (np.abs(dy - r) < 0.05))).any():
            continue                                        # nothing near the window's edge
        idx = [int(i) for i in np.nonzero(lvl_ok & (dx < r) & (dy < r))[0]]
        if not 10 <= len(idx) <= 24:
            continue
        for a in idx:
            for b in idx:
                if a >= b or FS.first(a, b)[0] == a:
                    continue                                # the later index first in the grid
                for k in range(132, 150):
                    q = desc_at2(desc[a], desc[b], k, k, FS.rng)
                    if q is None:
                        continue
                    d = {i: hamming(q, desc[i]) for i in idx}
                    order = sorted(idx, key=lambda i: (d[i], FS.cell[i], i))
                    pa, pb = order.index(a), order.index(b)
                    if pb >= keep and pa == pb + 1 and max(d.values()) < 256:
                        n_offers = min(len(order), pa + 2)
                        for i in range(n_offers):
                            B.q(u, v, pred, q)
                            if order[i] == b:
                                B.want(b, i, i + 1)
                            elif order[i] == a:
                                B.want(a, i, i - 1)
                            else:
                                B.support[order[i]] = i
                        return B.case("claims", "chain", ":1526/:1534", th, dict(orb_dist=256))
    raise AssertionError("no window with a late tie")


def _majority_chain_case(entry, new, desc, keep=6):
    """Frame-to-frame / local map: more offers of one point than the kernels keep candidates per
    query (kTopK = 6). The query descriptor is the bitwise majority of seven keypoints of a wide
    window (about 88 bits from each, inside TH_HIGH); every keypoint of the window within TH_HIGH
    is claimed in (distance, GetFeaturesInArea order), one per offer, the seventh and later ones
    only by a rescan of the window (without it they stay unclaimed), the last offer finds none.
    The window's members, the u_right gate and the distances are worked out here, in numpy."""
    B = new()
    FS = B.FS
    mps = entry == "mps"
    th, level = (4, 1) if mps else (12.0, 1)
    r = float(f32(4.0) * f32(th) * FS.scale[level]) if mps else float(f32(th) * FS.scale[level])
    x, y = FS.kps["x"].astype(np.float64), FS.kps["y"].astype(np.float64)
    octv = FS.kps["octave"]
    lvl_ok = (octv >= level - 1) & (octv <= (level if mps else level + 1))
    for j in np.nonzero(FS.inside)[0]:
        u, v = FS.at(j)
        dx, dy = np.abs(x - u), np.abs(y - v)
        er = np.abs((u - FCAM[4] / Z) - FS.ur.astype(np.float64))     # the u_right gate's error
        gated = FS.ur > 0
        if (lvl_ok & ((np.abs(dx - r) < 0.05) | (np.abs(dy - r) < 0.05))).any() or \
                (gated & (np.abs(er - r) < 0.05)).any():
            continue                                        # nothing near an edge
        idx = [int(i) for i in np.nonzero(lvl_ok & (dx < r) & (dy < r) & ~(gated & (er > r)))[0]]
        if len(idx) < 7:
            continue
        near = sorted(idx, key=lambda i: hamming(desc[j], desc[i]))[:7]
        bits = np.unpackbits(desc[near], axis=1, bitorder="little").sum(0) >= 4
        q = np.packbits(bits, bitorder="little")
        d = {i: hamming(q, desc[i]) for i in idx}
        order = sorted([i for i in idx if d[i] <= TH_HIGH], key=lambda i: (d[i], FS.cell[i], i))
        if not keep < len(order) <= 12:
            continue
        for i in range(len(order) + 1):
            B.q(u, v, level, q)
        for i, kp in enumerate(order):
            if i < keep:
                B.support[kp] = i
            else:
                B.want(kp, i, -1)
        return B.case("claims", "chain", ":60/:76" if mps else ":1391/:1406", th, nnratio=1.0)
    raise AssertionError("no window with seven keypoints within TH_HIGH of one descriptor")


def _mps_only_cases(new, desc, cite):
    out = []
    # ---- second best and ratio (:84-93), nnratio 0.8 ----
    B = new()
    FS = B.FS

    def want_same(ka, kb, diff=0):
        """A pair `diff` levels apart and a query descriptor at (ka, kb) from it; every third
        keypoint in reach is further than kb + 10 from the query, so it is neither best nor
        second best."""
        def w(a, b):
            lv = max(FS.octv(a), FS.octv(b))
            if abs(FS.octv(a) - FS.octv(b)) != diff:
                return None
            q = desc_at2(desc[a], desc[b], ka, kb, FS.rng)
            if q is None:
                return None
            thirds = FS.thirds(a, b, 4.0 * float(FS.scale[lv]))
            return q if all(hamming(q, desc[j]) > kb + 10 for j in thirds) else None
        return w

    def want_diff(ka, kb):
        return want_same(ka, kb, 1)
    for ka, kb, same, hit in ((40, 50, True, True),      # 40 > 0.8f * 50 is false in float: kept
                              (41, 50, True, False),     # rejected
                              (41, 50, False, True),     # other level: no ratio test
                              (45, 45, True, False)):    # a tie: bestDist2 == bestDist, rejected
        a, b, q = FS.pair((want_same if same else want_diff)(ka, kb), reach=4.0)
        u, v = FS.mid(a, b)
        i = B.q(u, v, max(FS.octv(a), FS.octv(b)), q)
        best = a if ka < kb else FS.first(a, b)[0]
        B.want(best, i if hit else -1, -1 if hit else i)
    out.append(B.case("ratio", "nn08", cite["ratio"], 1, nnratio=0.8))

    # ---- search window fabs(dx) < r, r = 4 * scale[0] (frame.cpp:390); view_cos at 0.998 ----
    B = new()
    FS = B.FS
    for off, hit in ((4.0, False), (None, True)):
        j = FS.single(octave=0)
        x, y = float(FS.kps["x"][j]), r64(FS.kps["y"][j])
        px = f32(x - 4.0)
        if off is None:
            px = np.nextafter(px, f32(np.inf), dtype=f32)
        assert (float(f32(f32(x) - px)) < 4.0) == hit
        i = B.q(0.0, y, 0, desc_at(desc[j], 10, FS.rng), px=px)
        B.want(j, i if hit else -1, -1 if hit else i)
    out.append(B.case("window", "edge", cite["window"], 1))
    B = new()
    FS = B.FS
    # RadiusByViewingCos compares in double: float(0.998) > 0.998, so r = 2.5; a keypoint 3 px
    # (times the level's scale) away is outside; one float below, r = 4 and it is inside
    for vc, hit in ((f32(0.998), False), (np.nextafter(f32(0.998), f32(0), dtype=f32), True)):
        j = FS.single()
        o = FS.octv(j)
        u, v = r64(FS.kps["x"][j] - 3.0 * float(FS.scale[o])), r64(FS.kps["y"][j])
        i = B.q(u, v, o, desc_at(desc[j], 10, FS.rng), view_cos=vc)
        B.want(j, i if hit else -1, -1 if hit else i)
    assert float(f32(0.998)) > 0.998
    out.append(B.case("view_cos", "edge", cite["view_cos"], 1))
    return out


def _frame_hist_cases(entry, new, desc, cite, pk):
    """The rotation-histogram plans on isolated keypoints: th = 1 (a window of scale[level] px),
    every query lands on its keypoint at distance 10; the other frame's angle makes the rot."""
    out = []
    for name, (rots, exp, alt) in hist_plans().items():
        B = new()
        FS = B.FS
        ids = []
        for i, rot in enumerate(rots):
            j = FS.single(iso=3.5)
            u, v = FS.at(j)
            a2 = float(FS.kps["angle"][j])
            if rot < 0:                                     # the smallest negative rot there is
                a1 = np.nextafter(f32(a2), f32(-np.inf), dtype=f32)
            elif rot in (0.0, HALF_ROT):
                a1 = angle_for(a2, rot)                     # exactly
            else:
                a1 = f32((a2 + rot) % 360.0)                # the middle of the bin
            ids.append((j, B.q(u, v, FS.octv(j), desc_at(desc[j], 10, FS.rng), angle=a1)))
        for (j, i), e, a in zip(ids, exp, alt):
            if e == a:
                B.support[j] = i if e else -1
            else:
                B.want(j, i if e else -1, i if a else -1)
        out.append(B.case("histogram", name, cite["histogram"], 1.0, dict(pk, check_ori=1)))
        if name == "edges":
            C = out[-1]
            des = [j for (j, i), e in zip(ids, exp) if not e]
            idx = {j: i for j, i in ids}
            out.append(Case(entry, "check_ori_off", name, cite["check_ori_off"],
                            dict(C.inp, pose=_with(C.inp["pose"], check_ori=0)), des,
                            [idx[j] for j in des], [-1] * len(des), "map_point",
                            support={j: i for (j, i), e in zip(ids, exp) if e}))
    return out


def _with(pose, **kw):
    p = pose.copy()
    for k, v in kw.items():
        p[k] = v
    return p


# every (entry, family) the generator must produce: the tests compare the cases with these lists,
# so a family cannot drop out unnoticed, and parametrise by them, so a failure names the rule
KF_FAMILIES = {
    "tri": ("tie", "threshold", "u_right", "epipolar", "den_zero", "epipole", "histogram",
            "check_ori_off"),
    "fuse": ("tie", "threshold", "gates", "chi_square"),
    "fuse_sim3": ("tie", "threshold", "gates"),
    "sbp_sim3": ("tie", "threshold", "gates", "claims"),
    "sim3": ("tie", "threshold", "gates"),
    "bow": ("threshold", "ratio", "histogram", "check_ori_off")}
KF_CASE_IDS = ("fuse-threshold-best_dist", "fuse_sim3-threshold-best_dist", "tri-tie-one_node",
               "tri-tie-three_nodes", "bow-threshold-frame_le", "bow-threshold-kf_kf_lt")
FRAME_FAMILIES = {
    "f2f": ("tie", "threshold", "level_window", "window", "depth_sign", "claims", "histogram",
            "check_ori_off"),
    "mps": ("tie", "threshold", "level_window", "claims", "ratio", "window", "view_cos"),
    "reloc": ("tie", "threshold", "level_window", "window", "depth_sign", "claims", "histogram",
              "check_ori_off")}


def families(cases):
    return {(c.entry, c.family) for c in cases}


def listed(table):
    return {(e, f) for e, fs in table.items() for f in fs}


def frame_cases(kps, desc, ur, scale):
    """The frame matchers' cases on the frame (kps, desc, ur) whose level table is `scale`."""
    out = []
    for s, entry in enumerate(("f2f", "mps", "reloc")):
        out += _frame_entry_cases(entry, kps, desc, ur, scale, 900 + s)
    for c in out:
        assert (c.expected != c.alt).all(), c.id
    assert families(out) == listed(FRAME_FAMILIES)
    assert {"reloc-claims-chain", "f2f-claims-chain", "mps-claims-chain",
            "f2f-level_window-forward", "f2f-level_window-backward"} <= {c.id for c in out}
    return out
