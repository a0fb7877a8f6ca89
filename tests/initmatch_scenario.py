"""SearchForInitialization scenarios (test infrastructure), shared by test_initmatch_ref.py (CPU)
and test_initmatch_gpu.py: the tracker's call on the three-frame synthetic sequence (F1 = frame 0,
vbPrevMatched = F1's keypoint positions, tracker.cpp:313-318) and constructed queries on the real
oracle frame 1, one case per comparison of orb_matcher.cpp:264-382. A constructed query's
descriptor is an F2 keypoint's with k bits flipped (or, with two candidates in its window, at
chosen distances from both); its window holds the level-0 keypoints the case names and no other.
Every expected output is written down from the cited line, with numpy float32 where a float
expression decides -- never taken from the code under test."""
import numpy as np

import reloc_scenario as RS
from boundary_scenario import desc_at, desc_at2, hamming
from slam_framework_amd import slamgpu as G
from slam_framework_amd import synthetic as S

f32 = np.float32
W, H = S.KITTI_COLS, S.KITTI_ROWS
TH_LOW = 50
WIN = 12                      # windowSize of the constructed cases
INT_MAX = 2 ** 31 - 1


def frames(oracle, nfeatures=2000):
    return RS.frames(oracle, nfeatures)


def f1_queries(f):
    """The tracker's call: all keypoints of F1, vbPrevMatched[i] = F1's keypoint i."""
    q = G.init_queries(f["kl"], f["dl"])
    prev = np.stack([f["kl"]["x"], f["kl"]["y"]], 1).astype(np.float32)
    return q, np.ascontiguousarray(prev)


def accepts(best, second, nnratio):
    """:321-323 -- bestDist <= TH_LOW and (float)bestDist < (float)bestDist2 * mfNNratio."""
    return best <= TH_LOW and f32(best) < f32(f32(second) * f32(nnratio))


def cell_of(kps, cols=W, rows=H):
    """Frame::PosInGrid (frame.cpp:339-346) of undistorted keypoints on the k1 == 0 bounds:
    (cell = ix * 48 + iy, in the grid)."""
    cw, ch = f32(f32(cols) / f32(64)), f32(f32(rows) / f32(48))

    def rnd(v):                                   # roundf: half away from zero
        return np.where(v >= 0, np.floor(v + f32(0.5)), np.ceil(v - f32(0.5))).astype(np.int64)
    ix, iy = rnd(kps["x"].astype(f32) / cw), rnd(kps["y"].astype(f32) / ch)
    return ix * 48 + iy, (ix >= 0) & (ix < 64) & (iy >= 0) & (iy < 48)


def py_search(kps2, desc2, queries, nnratio, window_size, check_ori, prev_matched):
    """:264-382 in plain Python: the window by brute force over all keypoints (no cell walk; a
    keypoint outside the 64 x 48 grid is in no cell), candidates in GetFeaturesInArea's order
    (cell x-major then y, then index). Returns what initmatch_ref.search_for_initialization does."""
    n1, n2 = len(queries), len(kps2)
    cell, ingrid = cell_of(kps2) if n2 else (np.zeros(0, np.int64), np.zeros(0, bool))
    order = np.lexsort((np.arange(n2), cell))
    order = order[ingrid[order]]
    kx, ky, ko = kps2["x"][order], kps2["y"][order], kps2["octave"][order]
    bits2 = np.unpackbits(np.asarray(desc2, np.uint8).reshape(-1, 32), axis=1)
    md = np.full(n2, INT_MAX, np.int64)
    m21 = np.full(n2, -1, np.int64)
    m12 = np.full(n1, -1, np.int32)
    ak = np.full(n1, -1, np.int32)
    prev = np.array(prev_matched, np.float32).reshape(-1, 2).copy()
    hist = [[] for _ in range(30)]
    nm = skipped = takeovers = removed = maxc = 0
    r = f32(window_size)
    for i1 in range(n1):
        level1 = int(queries["octave"][i1])
        if level1 > 0:
            continue
        px, py = prev[i1]
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        sel = (np.abs(kx - px) < r) & (np.abs(ky - py) < r) & (ko == level1)
        cands = order[sel]
        if not len(cands):
            continue
        maxc = max(maxc, len(cands))
        qb = np.unpackbits(queries["desc"][i1])
        best, best2, idx = INT_MAX, INT_MAX, -1
        for i2 in cands:
            d = int((bits2[i2] != qb).sum())
            if md[i2] <= d:
                skipped += 1
                continue
            if d < best:
                best2, best, idx = best, d, int(i2)
            elif d < best2:
                best2 = d
        if accepts(best, best2, nnratio):
            if m21[idx] >= 0:
                m12[m21[idx]] = -1
                nm -= 1
                takeovers += 1
            m12[i1], m21[idx], md[idx], ak[i1] = idx, i1, best, idx
            nm += 1
            if check_ori:
                rot = f32(queries["angle"][i1] - kps2["angle"][idx])
                if rot < 0:
                    rot = f32(rot + f32(360.0))
                v = f32(rot * f32(f32(1.0) / f32(30)))
                b = int(np.floor(v + f32(0.5)))
                hist[0 if b == 30 else b].append(i1)
    if check_ori:
        m1 = m2 = m3 = 0
        j1 = j2 = j3 = -1
        for i, h in enumerate(hist):
            s = len(h)
            if s > m1:
                m3, m2, m1, j3, j2, j1 = m2, m1, s, j2, j1, i
            elif s > m2:
                m3, m2, j3, j2 = m2, s, j2, i
            elif s > m3:
                m3, j3 = s, i
        if f32(m2) < f32(f32(0.1) * f32(m1)):
            j2 = j3 = -1
        elif f32(m3) < f32(f32(0.1) * f32(m1)):
            j3 = -1
        for i, h in enumerate(hist):
            if i in (j1, j2, j3):
                continue
            for i1 in h:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nm -= 1
                    removed += 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1] = (kps2["x"][m12[i1]], kps2["y"][m12[i1]])
    return nm, m12, prev, ak, dict(skipped=skipped, takeovers=takeovers, removed=removed,
                                   max_candidates=maxc)


# ---- sites: level-0 keypoints alone, or two alone, in a WIN window -------------------------------
class Sites:
    def __init__(self, kps, desc, seed=7):
        self.kps, self.desc = kps, np.asarray(desc, np.uint8)
        self.rng = np.random.default_rng(seed)
        self.l0 = np.nonzero(kps["octave"] == 0)[0]
        self.x, self.y = kps["x"].astype(np.float64), kps["y"].astype(np.float64)
        x0, y0 = self.x[self.l0], self.y[self.l0]
        self.D0 = np.maximum(np.abs(x0[:, None] - x0[None, :]), np.abs(y0[:, None] - y0[None, :]))
        cell, ingrid = cell_of(kps)
        self.cell, self.ingrid = cell, ingrid
        inside = (self.x > 40) & (self.x < W - 40) & (self.y > 40) & (self.y < H - 40)
        # alone within 2 WIN + 2 px: a window centred up to WIN px away still holds it alone
        self.singles = [int(self.l0[i]) for i in range(len(self.l0))
                        if (self.D0[i] < 2 * WIN + 2).sum() == 1 and inside[self.l0[i]]]
        self.pairs = []
        for i in range(len(self.l0)):
            for j in range(i + 1, len(self.l0)):
                if self.D0[i, j] < 2 * (WIN - 2):
                    a, b = int(self.l0[i]), int(self.l0[j])
                    u, v = self.mid(a, b)
                    near = (np.abs(x0 - u) < WIN + 1) & (np.abs(y0 - v) < WIN + 1)
                    if near.sum() == 2 and inside[a] and inside[b]:
                        self.pairs.append((a, b))
        self.used = set()

    def mid(self, a, b):
        return (float(f32((self.x[a] + self.x[b]) / 2)), float(f32((self.y[a] + self.y[b]) / 2)))

    def at(self, j):
        return float(self.kps["x"][j]), float(self.kps["y"][j])

    def single(self):
        for j in self.singles:
            if j not in self.used:
                self.used.add(j)
                return j
        raise AssertionError("no isolated level-0 keypoint left")

    def pair(self, ka, kb):
        """An unused pair (a, b) and a descriptor at ka from a and kb from b."""
        for a, b in self.pairs:
            if a in self.used or b in self.used:
                continue
            for p, q in ((a, b), (b, a)):
                d = desc_at2(self.desc[p], self.desc[q], ka, kb, self.rng)
                if d is not None:
                    self.used.update((a, b))
                    return p, q, d
        raise AssertionError(f"no pair admits distances ({ka}, {kb})")

    def first(self, a, b):
        """The one GetFeaturesInArea returns first (frame.cpp:370-399), and the other."""
        return (a, b) if (self.cell[a], a) < (self.cell[b], b) else (b, a)


class Case:
    def __init__(self, name, cite, nnratio=0.9, window=WIN, check_ori=0):
        self.name, self.cite = name, cite
        self.nnratio, self.window, self.check_ori = nnratio, window, check_ori
        self.rows, self.prev, self.want = [], [], []
        self.counts = {}

    def q(self, desc, centre, want, angle=0.0, octave=0):
        r = np.zeros(1, G.INIT_QUERY_DTYPE)
        r["angle"], r["octave"], r["desc"][0] = angle, octave, desc
        self.rows.append(r[0])
        self.prev.append(centre)
        self.want.append(want)
        return len(self.rows) - 1

    def done(self, **counts):
        self.queries = np.array(self.rows, G.INIT_QUERY_DTYPE)
        self.prev0 = np.ascontiguousarray(np.array(self.prev, np.float32).reshape(-1, 2))
        self.want12 = np.array(self.want, np.int32).reshape(-1)
        self.counts = counts
        return self

    def check(self, kps2, nm, m12, prev, counts=None):
        """want12, nmatches == the number held (rule 9), vbPrevMatched written for survivors
        only (:377-379), every other entry bit for bit as it came."""
        try:
            np.testing.assert_array_equal(m12, self.want12)
            assert nm == int((self.want12 >= 0).sum())
            exp = self.prev0.copy()
            for i, j in enumerate(self.want12):
                if j >= 0:
                    exp[i] = (kps2["x"][j], kps2["y"][j])
            assert prev.tobytes() == exp.tobytes()
            if counts is not None:
                for k, v in self.counts.items():
                    assert counts[k] == v, (k, counts[k], v)
        except AssertionError as e:
            raise AssertionError(f"case {self.name} ({self.cite}): {e}") from e


def angle_for(a2, rot):
    """angle1 in [0, 360) whose rot = angle1 - angle2 (+ 360 if negative, :337-339) is within a
    hundredth of a degree of `rot`: the middle of a bin (rot is a multiple of 30)."""
    a1 = f32((float(a2) + rot) % 360.0)
    r = f32(a1 - f32(a2))
    if r < 0:
        r = f32(r + f32(360.0))
    assert 0 <= a1 < 360 and (abs(float(r) - rot) < 0.01 or abs(float(r) - rot - 360.0) < 0.01)
    return a1


def _edge_centre(kx, away):
    """p with float32(kx - p) == away exactly (|distx| == r: outside, frame.cpp:390) and its
    neighbour towards the keypoint (inside)."""
    p = f32(kx - f32(away))
    for _ in range(64):
        d = f32(f32(kx) - p)
        if d == f32(away):
            break
        p = np.nextafter(p, f32(np.inf) if d > away else f32(-np.inf), dtype=np.float32)
    assert f32(f32(kx) - p) == f32(away)
    q = p
    while not f32(f32(kx) - q) < f32(away):
        q = np.nextafter(q, f32(np.inf), dtype=np.float32)
    return float(p), float(q)


def rescan_site(kps, desc, window=100, keep=6):
    """A window of `window` px and a probe descriptor (the bitwise majority of a level-0
    keypoint's nearest descriptors) with more than `keep` level-0 candidates within TH_LOW of the
    probe: (centre, probe, candidates sorted by (distance, area order), their distances)."""
    l0 = np.nonzero(kps["octave"] == 0)[0]
    bits = np.unpackbits(np.asarray(desc, np.uint8)[l0], axis=1).astype(np.int32)
    x, y = kps["x"][l0], kps["y"][l0]
    cell, ingrid = cell_of(kps)
    best = None
    for i in range(len(l0)):
        if not (window < x[i] < W - window):
            continue
        r = f32(window)
        idx = np.nonzero((np.abs(x - x[i]) < r) & (np.abs(y - y[i]) < r) & ingrid[l0])[0]
        if len(idx) <= keep + 1:
            continue
        hd = (bits[idx] != bits[i]).sum(1)
        near = idx[np.argsort(hd, kind="stable")][:keep + 2]
        maj = (bits[near].sum(0) * 2 > len(near)).astype(np.int32)
        dist = (bits[idx] != maj).sum(1)
        o = np.lexsort((l0[idx], cell[l0[idx]], dist))
        ds = dist[o]
        second = int(ds[keep + 1]) if len(ds) > keep + 1 else INT_MAX
        if ds[keep] > ds[keep - 1] and ds[0] > 0 and accepts(int(ds[keep]), second, 0.9) and \
                (best is None or ds[keep] < best[3][keep]):
            best = ((float(x[i]), float(y[i])), np.packbits(maj.astype(np.uint8)), l0[idx][o], ds)
    assert best is not None, "no window with more than kTopK candidates within TH_LOW of a probe"
    return best


def cases(kps, desc):
    """The constructed cases on F2 = (kps, desc), a real oracle frame."""
    out = []
    ang = kps["angle"]

    def new(*a, **k):
        c = Case(*a, **k)
        out.append(c)
        return c, Sites(kps, desc)

    # 1. level1 > 0 is skipped (:283-285); an octave-1 keypoint in the window is no candidate
    c, S_ = new("level_above_0", ":283-285 / frame.cpp:380-386")
    s = S_.single()
    c.q(desc[s], S_.at(s), -1, octave=1)
    c.q(desc[s], S_.at(s), -1, octave=3)
    c.q(desc[s], S_.at(s), s)
    l0 = np.nonzero(kps["octave"] == 0)[0]
    for j in np.nonzero(kps["octave"] == 1)[0]:
        dx = np.maximum(np.abs(kps["x"][l0] - kps["x"][j]), np.abs(kps["y"][l0] - kps["y"][j]))
        if dx.min() > WIN + 1:
            c.q(desc[j], S_.at(j), -1)            # distance 0 to an octave-1 keypoint, alone
            break
    else:
        raise AssertionError("no octave-1 keypoint without a level-0 neighbour")
    c.done(takeovers=0, removed=0)

    # 2. |distx| < r is strict (frame.cpp:390); a window off the grid (:357-369)
    c, S_ = new("window_edge", "frame.cpp:357-369, :390")
    for axis in (0, 1):
        s = S_.single()
        x, y = S_.at(s)
        out_, in_ = _edge_centre((x, y)[axis], WIN)
        c.q(desc[s], (out_, y) if axis == 0 else (x, out_), -1)
        s2 = S_.single()
        x, y = S_.at(s2)
        out_, in_ = _edge_centre((x, y)[axis], WIN)
        c.q(desc[s2], (in_, y) if axis == 0 else (x, in_), s2)
    s = S_.single()
    for centre in ((-500.0, 100.0), (5000.0, 100.0), (600.0, -300.0), (600.0, 3000.0)):
        c.q(desc[s], centre, -1)
    c.done(takeovers=0, skipped=0)

    # 3. TH_LOW (:321): 50 accepted, 51 not
    c, S_ = new("th_low", ":321")
    for k in (50, 51, 0):
        s = S_.single()
        c.q(desc_at(desc[s], k, S_.rng), S_.at(s), s if k <= TH_LOW else -1)
    c.done()

    # 4. the ratio test (:323), strict '<' on a float product
    assert not accepts(45, 50, 0.9) and accepts(45, 51, 0.9)        # 50 * 0.9f rounds to 45.0f
    assert not accepts(45, 45, 0.9) and accepts(45, 45, 1.5)
    c, S_ = new("ratio_0.9", ":298-323", nnratio=0.9)
    a, b, d = S_.pair(45, 50)
    c.q(d, S_.mid(a, b), -1)
    a, b, d = S_.pair(45, 51)
    c.q(d, S_.mid(a, b), a)
    tie = S_.pair(45, 45)
    c.q(tie[2], S_.mid(tie[0], tie[1]), -1)
    c.done(takeovers=0, skipped=0)
    c, S_ = new("ratio_1.5_tie_goes_to_the_first", ":309-318", nnratio=1.5)
    a, b, d = tie
    c.q(d, S_.mid(a, b), S_.first(a, b)[0])
    c.done()

    # 5. rule 4's '<=' (:306-307)
    c, S_ = new("matched_distance", ":306-307")
    s = S_.single()
    c.q(desc_at(desc[s], 20, S_.rng), S_.at(s), -1)      # matched at 20, taken over below
    c.q(desc_at(desc[s], 20, S_.rng), S_.at(s), -1)      # 20 <= 20: skipped
    c.q(desc_at(desc[s], 25, S_.rng), S_.at(s), -1)      # 20 <= 25: skipped
    c.q(desc_at(desc[s], 19, S_.rng), S_.at(s), s)       # 20 <= 19 fails: takes it over
    # a skipped candidate is no second either: a is held at 10, so b at 45 has no rival
    # (with a at 47 as the second, 45 < 47 * 0.9f fails)
    assert not accepts(45, 47, 0.9) and accepts(45, INT_MAX, 0.9)
    a, b, d = S_.pair(47, 45)
    da = desc_at2(desc[a], desc[b], 10, hamming(desc[a], desc[b]) + 10, S_.rng)
    c.q(da, S_.mid(a, b), a)
    c.q(d, S_.mid(a, b), b)
    c.done(skipped=3, takeovers=1)

    # 6. a take-over (:325-333): the earlier query loses its match and keeps its vbPrevMatched
    c, S_ = new("take_over", ":325-333, :377-379")
    s = S_.single()
    x, y = S_.at(s)
    c.q(desc_at(desc[s], 20, S_.rng), (x + 1.5, y - 2.25), -1)
    c.q(desc_at(desc[s], 15, S_.rng), (x - 3.0, y + 1.0), s)
    c.done(takeovers=1, skipped=0)

    # 7. the histogram counts taken-over entries (:344, :357); the removal loop clears only
    #    matches that still hold (:366)
    assert not f32(2) < f32(f32(0.1) * f32(20)) and f32(1) < f32(f32(0.1) * f32(20))
    c, S_ = new("histogram_counts_taken_over", ":335-372", check_ori=1)

    def oq(s, k, rot, want):
        return c.q(desc_at(desc[s], k, S_.rng), S_.at(s), want, angle=angle_for(ang[s], rot))
    u, p, w, v = (S_.single() for _ in range(4))
    oq(u, 20, 90.0, -1)      # X: bin 3, taken over by Y below; still counted in bin 3
    oq(p, 20, 180.0, -1)     # P: bin 6 (rejected), taken over by Q below: not decremented again
    oq(w, 20, 270.0, -1)     # W: bin 9, one entry < 10 % of 20: removed
    oq(v, 20, 90.0, v)       # Z: bin 3 holds 2 = 10 % of 20 only with X counted: kept
    for _ in range(18):
        s = S_.single()
        oq(s, 5, 0.0, s)
    oq(u, 10, 0.0, u)        # Y
    oq(p, 10, 0.0, p)        # Q: bin 0 holds 20
    c.done(takeovers=2, removed=1)
    c2 = Case("histogram_off", ":335, :351", check_ori=0)
    c2.rows, c2.prev = list(c.rows), list(c.prev)
    c2.want = list(c.want)
    c2.want[2] = w
    out.append(c2.done(takeovers=2, removed=0))

    # 8. vbPrevMatched is written for survivors only; a non-finite entry matches nothing
    c, S_ = new("non_finite_prev_matched", ":287 (undefined), :377-379")
    ss = [S_.single() for _ in range(6)]
    bad = [None, (np.nan, None), (None, np.inf), (-np.inf, None), (np.nan, np.nan), None]
    for s, e in zip(ss, bad):
        x, y = S_.at(s)
        if e is None:
            c.q(desc_at(desc[s], 3, S_.rng), (x + 2.0, y - 1.0), s)
        else:
            c.q(desc[s], (x if e[0] is None else e[0], y if e[1] is None else e[1]), -1)
    c.done()

    # 9. 130 queries on one keypoint, distances falling from 50 to 0: every strict step takes the
    #    keypoint over (50 take-overs across both 64-query boundaries), a repeated distance is
    #    skipped by '<=' (TH_LOW leaves 51 distinct accepted distances, so 130 strict steps
    #    cannot exist)
    c, S_ = new("descending_on_one_keypoint", ":306-333")
    s = S_.single()
    dist = [50 - (i * 51) // 130 for i in range(130)]
    assert dist[0] == 50 and dist[-1] == 0 and sorted(set(dist)) == list(range(51))
    for i, d in enumerate(dist):
        first_of_d = i == 0 or dist[i - 1] != d
        c.q(desc_at(desc[s], d, S_.rng), S_.at(s), s if (d == 0 and first_of_d) else -1)
    c.done(takeovers=50, skipped=130 - 51)

    # 10. 130 queries on one pair, distances to a rising 0, 1, 2, ...: only the first holds a;
    #     the others fall to b, their second candidate -- above TH_LOW it is no match, from 50
    #     down to 0 each takes b over, then b is held at 0 and nothing matches
    c, S_ = new("ascending_on_one_keypoint", ":306-333")
    for a, b in S_.pairs:
        Dab = hamming(desc[a], desc[b])
        if 64 < Dab <= 100:
            break
    else:
        raise AssertionError("no pair 65..100 bits apart")
    want_b = -1
    for i in range(130):
        kb = abs(Dab - i)
        d = desc_at2(desc[a], desc[b], i, kb, S_.rng)
        c.q(d, S_.mid(a, b), -1)
        if kb == 0:
            want_b = i
    c.want[0] = a
    c.want[want_b] = b
    c.done(takeovers=TH_LOW)

    # 11. the kept candidates run out: the probe's six nearest are all held at distance 0 and a
    #     seventh within TH_LOW is free
    c, S_ = new("kept_candidates_all_held", ":298-319 (kTopK = 6)", window=100)
    centre, probe, cand, ds = rescan_site(kps, desc)
    for j in cand[:6]:
        c.q(desc[j], centre, int(j))
    second = int(ds[7]) if len(ds) > 7 else INT_MAX
    assert accepts(int(ds[6]), second, 0.9)
    c.q(probe, centre, int(cand[6]))
    c.done(takeovers=0)
    return out
