"""Parity of the device relocalisation matcher, OrbMatcher::SearchByProjection(CurrentFrame, pKF,
sAlreadyFound, th, ORBdist) (src/orb_features/orb_matcher.cpp:1455-1582), against its CPU
restatement tests/relocmatch_ref.c, bit for bit: slamgpu_search_by_projection_reloc and its
batched _device form on the KITTI-size context and three-frame synthetic sequence of
test_match_gpu.py. The scenario, the hand-placed cases and their measured counts are those of
test_relocmatch_ref.py (which pins the restatement on the CPU): 231 / 209 matches at (10, 100)
on empty slots without / with the rotation check (22 removals), 104 queries passing over a taken
candidate, 81 / 80 matches at (3, 64); the repeated point is claimed 16 times in 40 offers."""
import ctypes as C

import numpy as np
import pytest

import reloc_scenario as RS
from slam_framework_amd import synthetic as S

pytestmark = pytest.mark.gpu
CAM = S.KITTI_CAM
W, H = S.KITTI_COLS, S.KITTI_ROWS


@pytest.fixture(scope="module")
def world(oracle, gpu_lib):
    """The oracle's frames, the restatement bound to frame `cur`, and one context per test
    module (frame_stereo(cur) makes frame `cur` the context's frame 0)."""
    import relocmatch_ref
    relocmatch_ref.lib()
    t, L, R, fr = RS.frames(oracle)
    sc, lsf = RS.scale_table(t), RS.log_scale_factor()
    grid = oracle.grid_geom(W, H)
    ctx = gpu_lib.Context(W, H)
    state = {"cur": None}

    def ref(cur, q, pose, mp0):
        f = fr[cur]
        return relocmatch_ref.search_by_projection_reloc(f["kl"], f["dl"], grid, CAM, sc, lsf, q,
                                                         pose, mp0)

    def dev(cur, q, pose, mp0):
        if state["cur"] != cur:
            ctx.frame_stereo(L[cur], R[cur], CAM)
            kl, dl = ctx.keypoints(0)
            assert kl.tobytes() == fr[cur]["kl"].tobytes() and (dl == fr[cur]["dl"]).all()
            state["cur"] = cur
        mp = mp0.copy()
        blk = np.full(len(mp), 7, np.uint8)      # derived from map_point at entry, whatever it held
        nm = ctx.search_by_projection_reloc(0, q, pose, mp, blk)
        np.testing.assert_array_equal(blk, (mp >= 0).astype(np.uint8))
        return nm, mp

    def both(cur, q, pose, mp0):
        nm_r, mp_r, qk, po, rem = ref(cur, q, pose, mp0)
        nm_d, mp_d = dev(cur, q, pose, mp0)
        assert nm_d == nm_r
        np.testing.assert_array_equal(mp_d, mp_r)
        return nm_r, mp_r, qk, po, rem
    return dict(fr=fr, sc=sc, lsf=lsf, grid=grid, ctx=ctx, ref=ref, dev=dev, both=both, L=L, R=R,
                t=t)


@pytest.mark.parametrize("th,orb_dist,floor", [(10.0, 100, 50), (3.0, 64, 20)])
@pytest.mark.parametrize("check_ori", [0, 1])
@pytest.mark.parametrize("occ", [0.0, 0.2])
def test_scenario(world, th, orb_dist, floor, check_ori, occ):
    """Frame c against keyframe c-1 at a perturbed pose, 20 % of the points in sAlreadyFound."""
    fr, sc = world["fr"], world["sc"]
    for cur in (1, 2):
        q = RS.kf_queries(fr[cur - 1], cur - 1, sc, 0.2, seed=cur)
        mp0 = RS.occupied(len(fr[cur]["kl"]), occ, 3)
        nm, mp, qk, po, rem = world["both"](cur, q, RS.pose(cur, th, orb_dist, check_ori), mp0)
        print(f"frame {cur} ({th}, {orb_dist}) ori {check_ori} occ {occ}: nmatches {nm}, "
              f"passed-over queries {int((po > 0).sum())}, removed {rem}")
        np.testing.assert_array_equal(mp[mp0 >= 0], mp0[mp0 >= 0])
        if occ == 0.0:
            assert nm >= floor
            if orb_dist == 100:
                assert int((po > 0).sum()) >= 20
                assert rem >= 1 if check_ori else rem == 0


def test_two_stages_chained(world):
    """(10, 100), then (3, 64) on the slots the first search left, sFound rebuilt in between
    (tracker.cpp:940-962)."""
    fr, sc = world["fr"], world["sc"]
    q = RS.kf_queries(fr[0], 0, sc, 0.2, seed=1)
    mp0 = RS.occupied(len(fr[1]["kl"]), 0.2, 3)
    nm1, mp1, qk1, _, _ = world["both"](1, q, RS.pose(1, 10.0, 100, 1), mp0)
    q2 = q.copy()
    q2["skip"][np.isin(q2["mp_id"], mp1[mp1 >= 0])] = 1
    nm2, mp2, _, _, _ = world["both"](1, q2, RS.pose(1, 3.0, 64, 1), mp1)
    np.testing.assert_array_equal(mp2[mp1 >= 0], mp1[mp1 >= 0])
    assert nm1 >= 50


def test_small_cases(world):
    """The hand-placed queries: the ORBdist boundary, the octave window level-1 .. level+1, two
    queries for one keypoint, an occupied slot, a skip query, a point behind the camera (searched:
    no depth gate), the distance range's two ends, and the queries the reference leaves undefined
    (they write nothing, their neighbours match)."""
    f = world["fr"][1]
    cases = RS.small_cases(f["kl"], f["dl"], lambda q, p, mp0: world["ref"](1, q, p, mp0))
    assert len(cases) == 20
    for name, q, pose, mp0, want in cases:
        try:
            nm, mp, _, _, _ = world["both"](1, q, pose, mp0)
            RS.check_case(want, mp0, nm, mp)
        except AssertionError as e:
            raise AssertionError(f"case {name}: {e}") from e


def test_rescan_path(world):
    """One point offered 40 times: the later copies exhaust their kTopK kept candidates and are
    rescanned at their place in the order."""
    fr, sc = world["fr"], world["sc"]
    q = RS.kf_queries(fr[0], 0, sc)
    pose = RS.pose(1, 20.0, 128, 0)
    n = len(fr[1]["kl"])
    rep, depth = RS.repeated_point(q, pose, n, lambda a, b, c: world["ref"](1, a, b, c))
    nm, mp, qk, po, _ = world["both"](1, rep, pose, np.full(n, -1, np.int32))
    assert nm == depth and int(po.max()) > 6            # deeper than kTopK
    # and mixed into the scenario's queries, with the rotation check
    mix = np.concatenate([q[:len(q) // 2], rep, q[len(q) // 2:]])
    mix["mp_id"] = np.arange(len(mix))
    world["both"](1, mix, RS.pose(1, 20.0, 128, 1), RS.occupied(n, 0.2, 5))


def test_rotation_tail(world):
    """Keyframe angles spread over three bins, one of them below 10 % of the largest: its slot
    returns to -1 / unblocked and nmatches is decremented."""
    f = world["fr"][1]
    q, iso = RS.rotation_queries(f["kl"], f["dl"])
    empty = np.full(len(f["kl"]), -1, np.int32)
    nm0, mp_off, _, _, rem0 = world["both"](1, q, RS.identity_pose(3.0, 20, 0), empty)
    nm1, mp_on, _, _, rem1 = world["both"](1, q, RS.identity_pose(3.0, 20, 1), empty)
    assert nm0 == len(q) and rem0 == 0
    assert rem1 >= 1 and nm1 == nm0 - rem1
    assert mp_off[iso[7]] >= 0 and mp_on[iso[7]] == -1


def test_wide_keys(oracle, gpu_lib):
    """A 4000-feature context (kp_cap > 2048: the 64-bit candidate keys), frames from the device
    front-end itself."""
    import relocmatch_ref
    ctx = gpu_lib.Context(W, H, nfeatures=4000)
    assert ctx.kp_cap > 2048
    L, R = S.sequence(2000, 2)
    ctx.frame_stereo(L[0], R[0], CAM)
    kl, dl = (a.copy() for a in ctx.keypoints(0))
    depth = ctx.stereo(0)[1].copy()
    ctx.frame_stereo(L[1], R[1], CAM)
    ck, cd = (a.copy() for a in ctx.keypoints(0))
    assert len(ck) > 2048
    sc = RS.scale_table(oracle.tables(nfeatures=4000))
    q = RS.kf_queries(dict(kl=kl, dl=dl, depth=depth), 0, sc, 0.2, seed=4, twice=True)
    grid = oracle.grid_geom(W, H)
    for th, od, ori in ((10.0, 100, 1), (3.0, 64, 0)):
        pose = RS.pose(1, th, od, ori)
        mp0 = RS.occupied(len(ck), 0.2, 9)
        nm_r, mp_r, _, po, _ = relocmatch_ref.search_by_projection_reloc(
            ck, cd, grid, CAM, sc, RS.log_scale_factor(), q, pose, mp0)
        mp = mp0.copy()
        blk = np.zeros(len(mp), np.uint8)
        assert ctx.search_by_projection_reloc(0, q, pose, mp, blk) == nm_r
        np.testing.assert_array_equal(mp, mp_r)
        assert nm_r >= 50 and int((po > 0).sum()) >= 20


GUARD = 0x5A5A5A5A


def test_batched_device_form(world, gpu_lib):
    """Three frames in one call (frame 1 has no queries), guard words around every output row,
    equality with three synchronous calls, and the same call on a second stream."""
    import torch
    G = gpu_lib
    fr, sc, L, R = world["fr"], world["sc"], world["L"], world["R"]
    dev = torch.device("cuda", 0)
    ctx = G.Context(W, H, max_frames=3)
    kc = ctx.kp_cap
    pitch = 1280
    hl, hr = np.zeros((3, H, pitch), np.uint8), np.zeros((3, H, pitch), np.uint8)
    hl[:, :, :W], hr[:, :, :W] = L, R
    d_l, d_r = torch.from_numpy(hl).to(dev), torch.from_numpy(hr).to(dev)
    ctx.frontend_device(d_l, d_r, H * pitch, pitch, 3, CAM)
    ctx.sync()
    n = [len(ctx.keypoints(2 * f)[0]) for f in range(3)]
    assert n == [len(f["kl"]) for f in fr]
    # frame 0 <- keyframe 1, frame 1: no queries, frame 2 <- keyframe 1 (offered twice)
    qs = [RS.kf_queries(fr[1], 1, sc, 0.2, seed=1), np.zeros(0, G.RELOC_QUERY_DTYPE),
          RS.kf_queries(fr[1], 1, sc, 0.0, twice=True)]
    poses = np.concatenate([RS.pose(0, 10.0, 100, 1), RS.pose(1, 10.0, 100, 1),
                            RS.pose(2, 3.0, 64, 0)])
    gap = 5                                       # unused query records between the frames' lists
    q_start = np.array([gap, 0, gap + len(qs[0]) + gap], np.int32)
    q_count = np.array([len(x) for x in qs], np.int32)
    total = int(q_start[2] + q_count[2])
    qall = np.zeros(total, G.RELOC_QUERY_DTYPE)
    for f in (0, 2):
        qall[q_start[f]:q_start[f] + q_count[f]] = qs[f]
    mp0 = [RS.occupied(n[f], 0.2, 20 + f) for f in range(3)]
    stride = kc + 8                               # rows with 4 guard words on each side
    mp_h = np.full((4, stride), GUARD, np.int32)  # row 3: a frame the call must not touch
    blk_h = np.full((4, stride), 0xA5, np.uint8)
    for f in range(3):
        mp_h[f, 4:4 + kc] = -1
        mp_h[f, 4:4 + n[f]] = mp0[f]
        blk_h[f, 4:4 + kc] = 0
        blk_h[f, 4:4 + n[f]] = mp0[f] >= 0
    ref = [world["ref"](f, qs[f], poses[f:f + 1], mp0[f]) for f in range(3)]
    sync = []
    for f in range(3):                            # three synchronous calls on the same context
        mp, blk = mp0[f].copy(), np.zeros(n[f], np.uint8)
        sync.append((ctx.search_by_projection_reloc(f, qs[f], poses[f:f + 1], mp, blk), mp, blk))
    d_q = torch.from_numpy(qall.view(np.uint8).copy()).to(dev)
    d_p = torch.from_numpy(poses.view(np.uint8).copy()).to(dev)
    d_qs, d_qc = torch.from_numpy(q_start).to(dev), torch.from_numpy(q_count).to(dev)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    outs = []
    torch.cuda.synchronize()
    for i, st in enumerate(streams):
        if i:
            st.wait_stream(streams[0])            # one context: its calls run one after the other
        with torch.cuda.stream(st):
            d_mp = torch.from_numpy(mp_h.copy()).to(dev, non_blocking=False)
            d_blk = torch.from_numpy(blk_h.copy()).to(dev, non_blocking=False)
            d_nm = torch.full((5,), GUARD, dtype=torch.int32, device=dev)
            ctx.search_by_projection_reloc_device(
                d_q, total, d_qs, d_qc, int(q_count.max()), d_p,
                d_mp.view(-1)[4:], d_blk.view(-1)[4:], stride, d_nm[1:], 3, st.cuda_stream)
            outs.append((d_mp, d_blk, d_nm))
    for st in streams:
        st.synchronize()
    ctx.sync()
    for d_mp, d_blk, d_nm in outs:
        mp_g, blk_g, nm_g = d_mp.cpu().numpy(), d_blk.cpu().numpy(), d_nm.cpu().numpy()
        assert nm_g[0] == GUARD and nm_g[4] == GUARD
        assert (mp_g[:, :4] == GUARD).all() and (mp_g[:, 4 + kc:] == GUARD).all()
        assert (blk_g[:, :4] == 0xA5).all() and (blk_g[:, 4 + kc:] == 0xA5).all()
        assert (mp_g[3] == GUARD).all() and (blk_g[3] == 0xA5).all()
        for f in range(3):
            assert nm_g[1 + f] == ref[f][0] == sync[f][0]
            np.testing.assert_array_equal(mp_g[f, 4:4 + n[f]], ref[f][1])
            np.testing.assert_array_equal(mp_g[f, 4:4 + n[f]], sync[f][1])
            np.testing.assert_array_equal(blk_g[f, 4:4 + n[f]], sync[f][2])
            assert (mp_g[f, 4 + n[f]:4 + kc] == -1).all() and (blk_g[f, 4 + n[f]:4 + kc] == 0).all()
        np.testing.assert_array_equal(mp_g[1, 4:4 + n[1]], mp0[1])    # no queries: untouched
        assert nm_g[2] == 0
    assert ref[0][0] >= 50 and ref[2][0] >= 20


def test_error_codes(world, gpu_lib):
    """Each loud error returns SLAMGPU_EINVAL with a message and writes nothing."""
    G = gpu_lib
    world["dev"](1, np.zeros(0, G.RELOC_QUERY_DTYPE), RS.identity_pose(3.0, 20),
                 np.full(len(world["fr"][1]["kl"]), -1, np.int32))   # frame 1 in the context
    ctx, f = world["ctx"], world["fr"][1]
    n = len(f["kl"])
    q = np.ascontiguousarray(RS.on_keypoint(f["kl"], f["dl"], 0, int(f["kl"]["octave"][0])))
    good = RS.identity_pose(10.0, 100)
    L = G.lib()

    def call(frame=0, queries=q, nq=1, pose=good, mp=True, blk=True, n_=n, nm=True):
        mp_a, blk_a = np.full(n + 1, 41, np.int32), np.full(n + 1, 42, np.uint8)
        out = C.c_int(-77)
        rc = L.slamgpu_search_by_projection_reloc(
            ctx.h, frame, G._ptr(queries) if queries is not None else None, nq,
            G._ptr(pose) if pose is not None else None, G._ptr(mp_a) if mp else None,
            G._ptr(blk_a) if blk else None, n_, C.byref(out) if nm else None)
        assert (mp_a == 41).all() and (blk_a == 42).all() and out.value == -77
        return rc

    def pose_with(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[k] = v
        return p
    assert call(queries=None) == -1
    assert call(pose=None) == -1
    assert call(mp=False) == -1
    assert call(blk=False) == -1
    assert call(nm=False) == -1
    assert call(nq=-1) == -1
    assert call(frame=-1) == -1 and call(frame=1) == -1
    assert b"frame" in L.slamgpu_last_error(ctx.h)
    assert call(n_=n - 1) == -1 and call(n_=n + 1) == -1
    assert b"keypoints" in L.slamgpu_last_error(ctx.h)
    assert call(pose=pose_with(orb_dist=-1)) == -1 and call(pose=pose_with(orb_dist=257)) == -1
    assert b"orb_dist" in L.slamgpu_last_error(ctx.h)
    for bad in (np.nan, np.inf, -np.inf):
        assert call(pose=pose_with(th=bad)) == -1
    assert b"th" in L.slamgpu_last_error(ctx.h)
    assert L.slamgpu_search_by_projection_reloc(None, 0, None, 0, None, None, None, 0, None) == -1
    # the batched form: null pointers, frame count and stride out of range
    z = C.c_void_p(0)
    one = C.c_void_p(16)   # never dereferenced: the call fails before any launch
    dcall = lambda *a: L.slamgpu_search_by_projection_reloc_device(ctx.h, *a)  # noqa: E731
    assert dcall(one, 1, one, one, 1, one, one, one, ctx.kp_cap, one, 0, z) == -1
    assert dcall(one, 1, one, one, 1, one, one, one, ctx.kp_cap, one, 2, z) == -1
    assert dcall(one, 1, one, one, 1, one, one, one, ctx.kp_cap - 1, one, 1, z) == -1
    assert dcall(z, 1, one, one, 1, one, one, one, ctx.kp_cap, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, z, one, one, ctx.kp_cap, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, one, z, one, ctx.kp_cap, one, 1, z) == -1
    assert dcall(one, 1 << 30, one, one, 1, one, one, one, ctx.kp_cap, one, 1, z) == -3
    # and a valid call still works afterwards
    nm, mp = world["dev"](1, q, good, np.full(n, -1, np.int32))
    assert nm == world["ref"](1, q, good, np.full(n, -1, np.int32))[0]


def test_orbmatcher_method(world, gpu_lib):
    """OrbMatcher.SearchByProjectionReloc: the keyframe's map point table gathered into queries,
    ids written into the frame's id-per-keypoint array in place."""
    G = gpu_lib
    fr, sc = world["fr"], world["sc"]
    kf = fr[0]
    q = RS.kf_queries(kf, 0, sc)

    class KF:
        keypoints = kf["kl"]
        map_points = np.where(q["skip"] == 0, q["mp_id"] + 1000, -1)
        points = {int(q["mp_id"][i]) + 1000: (q["xyz"][i], q["max_dist"][i], q["min_dist"][i],
                                              q["desc"][i]) for i in np.nonzero(q["skip"] == 0)[0]}
    found = [int(m) for m in KF.map_points[KF.map_points >= 0][::5]]
    pose = RS.pose(1, 10.0, 100, 1)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = pose["Rcw"][0].reshape(3, 3), pose["tcw"][0]
    world["dev"](1, q[:0], pose, np.full(len(fr[1]["kl"]), -1, np.int32))   # frame 1 in the context
    mp0 = RS.occupied(len(fr[1]["kl"]), 0.2, 3)
    vp = mp0.copy()
    nm = G.OrbMatcher(0.9, True).SearchByProjectionReloc(world["ctx"], 0, KF, found, 10.0, 100, T, vp)
    q2 = q.copy()
    q2["mp_id"] += 1000
    q2["skip"][np.isin(q2["mp_id"], found)] = 1
    nm_r, mp_r, _, _, _ = world["ref"](1, q2, pose, mp0)
    assert nm == nm_r and nm >= 50
    np.testing.assert_array_equal(vp, mp_r)
