"""Pins tests/relocmatch_ref.c (the CPU restatement of the relocalisation matcher,
OrbMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist),
src/orb_features/orb_matcher.cpp:1455-1582) against an independent pure-Python statement of the
same method: the scenario of test_relocmatch_gpu.py, its hand-placed cases (with the queries the
reference leaves undefined), the rescan and rotation-tail inputs. No GPU. Parity against the
reference binary is unpinned (see the header of relocmatch_ref.c).

Scenario counts measured with the restatement (frame 1 against keyframe 0, 264 queries after the
20 % sAlreadyFound skips): (10, 100) on empty slots 231 matches without and 209 with the rotation
check (22 rotation-bin removals), 104 queries passed over a candidate an earlier query had taken;
20 % occupied slots 203 / 187 matches; (3, 64) 81 / 80 matches on empty, 65 / 64 on occupied
slots. The repeated point (th 20, ORBdist 128) is claimed 16 times in 40 offers: the later offers
pass over up to 16 taken candidates, more than the kTopK = 6 the device scan keeps."""
import math

import numpy as np
import pytest

import reloc_scenario as RS
import test_bow_oracle as TB
from test_kfmatch_oracle import fmaf, gemm_row
from test_loopmatch_ref import PyGrid

f32 = np.float32
W, H = 1241, 376
K_TOP = 6   # match_kernels.h kTopK


def _fma(a, b, c):
    """fmaf for operands that may be NaN or infinite (the shared helper is exact-rational)."""
    if np.isfinite(a) and np.isfinite(b) and np.isfinite(c):
        return fmaf(a, b, c)
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def py_reloc(oracle, kps, desc, grid, cam, scale, lsf, queries, pose, map_point):
    """:1455-1582 in plain Python with float32 scalars. Returns (nmatches, map_point', query_kp,
    passed_over, n_removed)."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    p = np.atleast_1d(pose)[0]
    R, t, Ow = p["Rcw"], p["tcw"], p["Ow"]
    th, orb_dist, check_ori = f32(p["th"]), int(p["orb_dist"]), int(p["check_ori"])
    logf = oracle._kf_lib().oc_logf
    pg = PyGrid(kps, grid)
    mp = np.array(map_point, np.int32)
    entry = mp >= 0
    nlevels = len(scale)
    hist = [[] for _ in range(30)]
    qk, passed = [], []
    nmatches = 0
    with np.errstate(all="ignore"):
        for q in queries:
            qk.append(-1)
            passed.append(0)
            if q["skip"]:
                continue
            x = q["xyz"]
            xc, yc, zc = (gemm_row(R, r, x, t[r]) for r in range(3))
            invzc = f32(np.float64(1.0) / np.float64(zc))
            u, v = _fma(f32(fx * xc), invzc, cx), _fma(f32(fy * yc), invzc, cy)
            if not (np.isfinite(invzc) and np.isfinite(u) and np.isfinite(v)):
                continue
            if u < f32(grid.min_x) or u > f32(grid.max_x) or v < f32(grid.min_y) or v > f32(grid.max_y):
                continue
            po = [f32(x[k] - Ow[k]) for k in range(3)]
            d3 = f32(math.sqrt(sum(float(c) * float(c) for c in po)))
            if not np.isfinite(d3):
                continue
            if d3 < f32(f32(0.8) * q["min_dist"]) or d3 > f32(f32(1.2) * q["max_dist"]):
                continue
            ratio = f32(q["max_dist"] / d3)
            if not np.isfinite(ratio) or not ratio > 0:
                continue
            lvl = math.ceil(f32(f32(logf(float(ratio))) / f32(lsf)))
            lvl = min(max(lvl, 0), nlevels - 1)
            radius = f32(th * scale[lvl])
            cands = [j for j in pg.area(u, v, radius) if lvl - 1 <= int(kps[j]["octave"]) <= lvl + 1]
            best, idx = 256, -1
            for j in cands:
                d = TB.hamming(q["desc"], desc[j])
                if mp[j] >= 0:
                    if not entry[j] and d <= orb_dist:
                        passed[-1] += 1
                    continue
                if d < best:
                    best, idx = d, j
            if best <= orb_dist and idx >= 0:
                mp[idx] = q["mp_id"]
                qk[-1] = idx
                nmatches += 1
                if check_ori:
                    rot = f32(q["kf_angle"] - kps[idx]["angle"])
                    if rot < 0:
                        rot = f32(rot + f32(360.0))
                    b = TB.roundf(f32(rot * f32(f32(1.0) / f32(30))))
                    hist[0 if b == 30 else b].append(idx)
    removed = 0
    if check_ori:
        m1 = m2 = m3 = 0
        i1 = i2 = i3 = -1
        for i, h in enumerate(hist):
            s = len(h)
            if s > m1:
                m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
            elif s > m2:
                m3, m2, i3, i2 = m2, s, i2, i
            elif s > m3:
                m3, i3 = s, i
        if f32(m2) < f32(f32(0.1) * f32(m1)):
            i2 = i3 = -1
        elif f32(m3) < f32(f32(0.1) * f32(m1)):
            i3 = -1
        for i, h in enumerate(hist):
            if i not in (i1, i2, i3):
                for j in h:
                    mp[j] = -1
                    nmatches -= 1
                    removed += 1
    return nmatches, mp, np.array(qk, np.int32), np.array(passed, np.int32), removed


@pytest.fixture(scope="module")
def world(oracle):
    import relocmatch_ref
    relocmatch_ref.lib()
    t, _, _, fr = RS.frames(oracle)
    sc, lsf = RS.scale_table(t), RS.log_scale_factor()
    grid = oracle.grid_geom(W, H)

    def both(cur, q, pose, mp0):
        f = fr[cur]
        a = relocmatch_ref.search_by_projection_reloc(f["kl"], f["dl"], grid, RS.CAM, sc, lsf, q,
                                                      pose, mp0)
        b = py_reloc(oracle, f["kl"], f["dl"], grid, RS.CAM, sc, lsf, q, pose, mp0)
        assert a[0] == b[0] and a[4] == b[4]
        for x, y in zip(a[1:4], b[1:4]):
            np.testing.assert_array_equal(x, y)
        return a

    def ref(cur, q, pose, mp0):
        f = fr[cur]
        return relocmatch_ref.search_by_projection_reloc(f["kl"], f["dl"], grid, RS.CAM, sc, lsf,
                                                         q, pose, mp0)
    return fr, sc, both, ref


def test_log_scale_factor_is_the_frames():
    """Frame::log_scale_factor_ = std::log(1.2f) in float."""
    assert RS.log_scale_factor() == float(f32(math.log(float(f32(1.2)))))


@pytest.mark.parametrize("th,orb_dist,floor", [(10.0, 100, 50), (3.0, 64, 20)])
@pytest.mark.parametrize("check_ori", [0, 1])
@pytest.mark.parametrize("occ", [0.0, 0.2])
def test_scenario_matches_python(world, th, orb_dist, floor, check_ori, occ):
    fr, sc, both, _ = world
    q = RS.kf_queries(fr[0], 0, sc, 0.2, seed=1)
    mp0 = RS.occupied(len(fr[1]["kl"]), occ, 3)
    nm, mp, qk, po, rem = both(1, q, RS.pose(1, th, orb_dist, check_ori), mp0)
    np.testing.assert_array_equal(mp[mp0 >= 0], mp0[mp0 >= 0])     # entry slots never taken
    assert nm == int(((mp >= 0) & (mp0 < 0)).sum())
    assert (qk[q["skip"] != 0] == -1).all()
    if occ == 0.0:                                                 # the issue's scenario conditions
        assert nm >= floor
        if orb_dist == 100:
            assert int((po > 0).sum()) >= 20
            assert rem >= 1 if check_ori else rem == 0


def test_small_cases_match_python(world):
    fr, sc, both, ref = world
    f = fr[1]
    cases = RS.small_cases(f["kl"], f["dl"], lambda q, p, mp0: ref(1, q, p, mp0))
    assert len(cases) == 20
    for name, q, pose, mp0, want in cases:
        nm, mp, _, _, _ = both(1, q, pose, mp0)
        try:
            RS.check_case(want, mp0, nm, mp)
        except AssertionError as e:
            raise AssertionError(f"case {name}: {e}") from e


def test_one_point_many_times(world):
    """One point offered 40 times walks down its candidate list, one claim per offer, deeper than
    the device scan's kept candidates."""
    fr, sc, both, ref = world
    q = RS.kf_queries(fr[0], 0, sc)
    pose = RS.pose(1, 20.0, 128, 0)
    rep, depth = RS.repeated_point(q, pose, len(fr[1]["kl"]), lambda a, b, c: ref(1, a, b, c))
    nm, mp, qk, po, _ = both(1, rep, pose, np.full(len(fr[1]["kl"]), -1, np.int32))
    assert nm == depth > K_TOP
    assert int(po.max()) > K_TOP
    np.testing.assert_array_equal(po[:nm], np.arange(nm))   # offer k passes over k taken ones
    assert len(set(qk[:nm])) == nm and (qk[nm:] == -1).all()


def test_rotation_tail(world):
    fr, sc, both, _ = world
    f = fr[1]
    q, iso = RS.rotation_queries(f["kl"], f["dl"])
    empty = np.full(len(f["kl"]), -1, np.int32)
    nm0, mp_off, _, _, rem0 = both(1, q, RS.identity_pose(3.0, 20, 0), empty)
    nm1, mp_on, qk, _, rem1 = both(1, q, RS.identity_pose(3.0, 20, 1), empty)
    assert nm0 == len(q) and rem0 == 0
    assert rem1 >= 1 and nm1 == nm0 - rem1
    gone = (mp_off >= 0) & (mp_on < 0)
    assert int(gone.sum()) == rem1 and gone[iso[7]]         # the 200 degree query's slot is cleared
