"""Parity of the device path of OrbMatcher::SearchForInitialization
(src/orb_features/orb_matcher.cpp:264-382) and of the monocular frame call against the CPU
restatement tests/initmatch_ref.c, bit for bit (vnMatches12, the bytes of vbPrevMatched,
nmatches): slamgpu_frame_mono, slamgpu_search_for_initialization and its batched _device form on
the KITTI-size context and the three-frame synthetic sequence of test_match_gpu.py. The scenario,
the constructed cases and their measured counts are those of test_initmatch_ref.py (which pins the
restatement on the CPU): windowSize 100, frames 0 -> 1, 184 / 180 matches without / with the
orientation check, 3 take-overs, 4 removals, 3008 rule-4 skips; at 4000 features 373 / 358
matches, 12 take-overs, 15 removals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import initmatch_scenario as IS
import scenario
from slam_framework_amd import synthetic as S

pytestmark = pytest.mark.gpu
CAM = S.KITTI_CAM
W, H = S.KITTI_COLS, S.KITTI_ROWS


@pytest.fixture(scope="module")
def world(oracle, gpu_lib):
    """The oracle's frames, the restatement, and one context per test module (frame_mono(cur)
    makes frame `cur` the context's frame 0)."""
    import initmatch_ref
    initmatch_ref.lib()
    G = gpu_lib
    t, L, R, fr = IS.frames(oracle)
    grid = oracle.grid_geom(W, H)
    ctx = G.Context(W, H)
    state = {"cur": None}

    def ref(cur, q, nnratio, window, ori, prev):
        f = fr[cur]
        return initmatch_ref.search_for_initialization(f["kl"], f["dl"], grid, q, nnratio, window,
                                                       ori, prev)

    def load(cur):
        if state["cur"] != cur:
            ctx.frame_mono(L[cur], CAM)
            kl, dl = ctx.keypoints(0)
            assert kl.tobytes() == fr[cur]["kl"].tobytes() and (dl == fr[cur]["dl"]).all()
            state["cur"] = cur

    def dev(cur, q, nnratio, window, ori, prev):
        load(cur)
        p = np.ascontiguousarray(prev, np.float32).copy()
        nm, m12 = ctx.search_for_initialization(0, q, G.init_search(nnratio, window, ori), p)
        return nm, m12, p

    def both(cur, q, nnratio, window, ori, prev):
        r = ref(cur, q, nnratio, window, ori, prev)
        nm, m12, p = dev(cur, q, nnratio, window, ori, prev)
        assert nm == r[0]
        np.testing.assert_array_equal(m12, r[1])
        assert p.tobytes() == r[2].tobytes()
        return r
    return dict(fr=fr, grid=grid, ctx=ctx, ref=ref, dev=dev, both=both, load=load, L=L, R=R, t=t,
                state=state)


@pytest.mark.parametrize("window", [100, 30])
@pytest.mark.parametrize("check_ori", [0, 1])
def test_scenario(world, window, check_ori):
    """The tracker's call: frames 0 -> 1, then 0 -> 2 with the vbPrevMatched the first returned."""
    fr = world["fr"]
    q, prev0 = IS.f1_queries(fr[0])
    nm, m12, prev1, _, cnt = world["both"](1, q, 0.9, window, check_ori, prev0)
    print(f"0->1 window {window} ori {check_ori}: nmatches {nm} {cnt}")
    assert nm == int((m12 >= 0).sum())
    if window == 100:
        assert nm >= 100                                          # tracker.cpp:331
        assert cnt["takeovers"] >= 1 and cnt["skipped"] >= 1
        assert cnt["removed"] >= 1 if check_ori else cnt["removed"] == 0
    nm2, m12b, _, _, cnt2 = world["both"](2, q, 0.9, window, check_ori, prev1)
    print(f"0->2 window {window} ori {check_ori}: nmatches {nm2} {cnt2}")
    assert nm2 == int((m12b >= 0).sum())


@pytest.mark.parametrize("nnratio", [0.6, 1.5, 0.0, -1.0, 1e-9, 3.0e38])
def test_every_finite_ratio(world, nnratio):
    """The scan drops candidates by (float)dist * nnratio > 50: the result is the restatement's
    for ratios above 1, zero, negative, and so small that an absent second fails the test."""
    q, prev0 = IS.f1_queries(world["fr"][0])
    nm = world["both"](1, q, nnratio, 100, 1, prev0)[0]
    if nnratio in (0.6, 1.5, 3.0e38):
        assert nm >= 50
    elif nnratio <= 0:
        assert nm == 0        # bestDist < bestDist2 * nnratio <= 0 never holds


def test_constructed_cases(world):
    f2 = world["fr"][1]
    cs = IS.cases(f2["kl"], f2["dl"])
    assert len(cs) == 13
    for c in cs:
        nm, m12, prev = world["dev"](1, c.queries, c.nnratio, c.window, c.check_ori, c.prev0)
        c.check(f2["kl"], nm, m12, prev)
        world["both"](1, c.queries, c.nnratio, c.window, c.check_ori, c.prev0)


def test_constructed_cases_in_one_list(world):
    """The cases of one window size concatenated behind the scenario's queries: more than 64
    queries per round, conflicts, take-overs and the rescan at places other than the first."""
    fr = world["fr"]
    cs = [c for c in IS.cases(fr[1]["kl"], fr[1]["dl"]) if c.nnratio == 0.9 and c.check_ori == 0]
    for window in (IS.WIN, 100):
        sel = [c for c in cs if c.window == window]
        q0, p0 = IS.f1_queries(fr[0])
        q = np.concatenate([q0[:300]] + [c.queries for c in sel] + [q0[300:]])
        prev = np.concatenate([p0[:300]] + [c.prev0 for c in sel] + [p0[300:]])
        r = world["both"](1, q, 0.9, window, 1, prev)
        assert r[0] >= 50


def test_empty_inputs(world, gpu_lib):
    """n1 = 0, and a frame without keypoints (a black image): valid, nothing found."""
    fr = world["fr"]
    q, prev0 = IS.f1_queries(fr[0])
    r = world["both"](1, q[:0], 0.9, 100, 1, prev0[:0])
    assert r[0] == 0
    ctx = world["ctx"]
    ctx.frame_mono(np.zeros((H, W), np.uint8), CAM)
    world["state"]["cur"] = None
    assert len(ctx.keypoints(0)[0]) == 0 and len(ctx.stereo(0)[0]) == 0
    p = prev0.copy()
    nm, m12 = ctx.search_for_initialization(0, q, gpu_lib.init_search(0.9, 100, 1), p)
    assert nm == 0 and (m12 == -1).all() and p.tobytes() == prev0.tobytes()
    mp, blk = np.full(0, -1, np.int32), np.zeros(0, np.uint8)
    vq = scenario.vo_queries(fr[0]["kl"], fr[0]["dl"], fr[0]["depth"], 0)[0]
    assert ctx.search_by_projection_frame(0, vq, scenario.pose(1, 15.0, mono=1), mp, blk) == 0


def test_frame_mono_wide_keys(oracle, gpu_lib):
    """nfeatures = 4000 (kp_cap > 2048: the 64-bit candidate keys): frame_mono's keypoints and
    descriptors are slamgpu_extract's byte for byte, u_right / depth all -1, the frame-to-frame
    search with mono = 1 on it is the oracle's, and SearchForInitialization the restatement's."""
    import initmatch_ref
    G = gpu_lib
    ctx = G.Context(W, H, nfeatures=4000)
    assert ctx.kp_cap > 2048
    L, R = S.sequence(2000, 2)
    ek, ed = ctx.extract(L[1])
    ctx.frame_stereo(L[0], R[0], CAM)
    k0, d0 = (a.copy() for a in ctx.keypoints(0))
    depth0 = ctx.stereo(0)[1].copy()
    ctx.frame_mono(L[1], CAM)
    k1, d1 = (a.copy() for a in ctx.keypoints(0))
    assert len(k1) > 2048
    assert k1.tobytes() == ek.tobytes() and d1.tobytes() == ed.tobytes()
    assert ctx.undistorted_keypoints(0).tobytes() == k1.tobytes()
    ur, depth = ctx.stereo(0)
    assert len(ur) == len(k1) and (ur == -1).all() and (depth == -1).all()
    # SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) on the mono frame
    t = oracle.tables(nfeatures=4000)
    grid = oracle.grid_geom(W, H)
    q, last_mp, last_out, xyz, mdesc, nobs = scenario.vo_queries(
        k0, d0, depth0, 0, np.random.default_rng(3), 0.5)
    p = scenario.pose(1, th=15.0, mono=1, check_ori=1)
    n = len(k1)
    mp_o = np.full(n, -1, np.int32)
    nm_o = oracle.search_frame(t, grid, k1, d1, np.full(n, -1, np.float32), mp_o, k0, last_mp,
                               last_out, xyz, mdesc, nobs, p["Rcw"][0].reshape(3, 3), p["tcw"][0],
                               float(p["tlc_z"][0]), float(p["baseline"][0]), CAM, 15.0, 1, 1)
    mp_g = np.full(n, -1, np.int32)
    nm_g = ctx.search_by_projection_frame(0, q, p, mp_g, np.zeros(n, np.uint8))
    assert nm_g == nm_o and nm_o >= 100
    np.testing.assert_array_equal(mp_g, mp_o)
    # SearchForInitialization, F1 = frame 0
    iq, prev0 = IS.f1_queries(dict(kl=k0, dl=d0))
    for ori in (0, 1):
        r = initmatch_ref.search_for_initialization(k1, d1, grid, iq, 0.9, 100, ori, prev0)
        pv = prev0.copy()
        nm, m12 = ctx.search_for_initialization(0, iq, G.init_search(0.9, 100, ori), pv)
        print(f"4000 features ori {ori}: nmatches {r[0]} {r[4]}")
        assert nm == r[0] and nm >= 100
        np.testing.assert_array_equal(m12, r[1])
        assert pv.tobytes() == r[2].tobytes()
        assert r[4]["takeovers"] >= 1 and r[4]["max_candidates"] > 64


def test_distortion(world, oracle, gpu_lib):
    """With a distortion set the window and the written vbPrevMatched use the undistorted keys
    (and the grid the undistorted image bounds)."""
    import initmatch_ref
    from test_undistort import DISTS
    G = gpu_lib
    fr, L = world["fr"], world["L"]
    dist = DISTS[0]
    ctx = G.Context(W, H)
    ctx.set_distortion(dist)
    ctx.frame_mono(L[1], CAM)
    un = ctx.undistorted_keypoints(0)
    ref_un = oracle.undistort_keypoints(CAM, dist, fr[1]["kl"])
    assert un.tobytes() == ref_un.tobytes() and un.tobytes() != fr[1]["kl"].tobytes()
    assert ctx.keypoints(0)[0].tobytes() == fr[1]["kl"].tobytes()
    grid = oracle.grid_geom(W, H, CAM, dist)
    un0 = oracle.undistort_keypoints(CAM, dist, fr[0]["kl"])
    q, prev0 = IS.f1_queries(dict(kl=un0, dl=fr[0]["dl"]))
    for window in (100, 30):
        r = initmatch_ref.search_for_initialization(ref_un, fr[1]["dl"], grid, q, 0.9, window, 1,
                                                    prev0)
        pv = prev0.copy()
        nm, m12 = ctx.search_for_initialization(0, q, G.init_search(0.9, window, 1), pv)
        assert nm == r[0] and nm >= 50
        np.testing.assert_array_equal(m12, r[1])
        assert pv.tobytes() == r[2].tobytes()
        held = m12 >= 0
        np.testing.assert_array_equal(pv[held, 0], ref_un["x"][m12[held]])


GUARD = 0x5A5A5A5A


def test_batched_device_form(world, gpu_lib):
    """Three frames in one call (frame 1 has no queries), gaps between the query lists, guard
    words around every output range, equality with three synchronous calls, and the same call on
    a second stream."""
    import torch
    G = gpu_lib
    fr, L, R = world["fr"], world["L"], world["R"]
    dev = torch.device("cuda", 0)
    ctx = G.Context(W, H, max_frames=3)
    pitch = 1280
    hl, hr = np.zeros((3, H, pitch), np.uint8), np.zeros((3, H, pitch), np.uint8)
    hl[:, :, :W], hr[:, :, :W] = L, R
    d_l, d_r = torch.from_numpy(hl).to(dev), torch.from_numpy(hr).to(dev)
    ctx.frontend_device(d_l, d_r, H * pitch, pitch, 3, CAM)
    ctx.sync()
    assert [len(ctx.keypoints(2 * f)[0]) for f in range(3)] == [len(f["kl"]) for f in fr]
    # frame 0 <- F1 = frame 1 (window 100, orientation check), frame 1: no queries,
    # frame 2 <- F1 = frame 0 (window 30, no check)
    src = [1, None, 0]
    qs, pv = [], []
    for s in src:
        q, p = IS.f1_queries(fr[s]) if s is not None else (np.zeros(0, G.INIT_QUERY_DTYPE),
                                                            np.zeros((0, 2), np.float32))
        qs.append(q)
        pv.append(p)
    params = np.concatenate([G.init_search(0.9, 100, 1), G.init_search(0.9, 100, 1),
                             G.init_search(0.8, 30, 0)])
    gap = 5
    q_start = np.array([gap, 0, gap + len(qs[0]) + gap], np.int32)
    q_count = np.array([len(x) for x in qs], np.int32)
    total = int(q_start[2] + q_count[2]) + gap
    qall = np.zeros(total, G.INIT_QUERY_DTYPE)
    prev_h = np.full((total, 2), np.float32(-12345.5), np.float32)
    m12_h = np.full(total, GUARD, np.int32)
    for f in (0, 2):
        qall[q_start[f]:q_start[f] + q_count[f]] = qs[f]
        prev_h[q_start[f]:q_start[f] + q_count[f]] = pv[f]
    # the gaps hold level-0 queries on real keypoints: a stray read of them would match
    qall[:gap] = qs[0][:gap]
    prev_h[:gap] = pv[0][:gap]
    ref = [world["ref"](f, qs[f], float(params["nnratio"][f]), int(params["window_size"][f]),
                        int(params["check_ori"][f]), pv[f]) for f in range(3)]
    sync = []
    for f in range(3):
        p = pv[f].copy()
        nm, m12 = ctx.search_for_initialization(f, qs[f], params[f:f + 1], p)
        sync.append((nm, m12, p))
    d_q = torch.from_numpy(qall.view(np.uint8).copy()).to(dev)
    d_p = torch.from_numpy(params.view(np.uint8).copy()).to(dev)
    d_qs, d_qc = torch.from_numpy(q_start).to(dev), torch.from_numpy(q_count).to(dev)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    outs = []
    torch.cuda.synchronize()
    for i, st in enumerate(streams):
        if i:
            st.wait_stream(streams[0])            # one context: its calls run one after the other
        with torch.cuda.stream(st):
            d_prev = torch.from_numpy(prev_h.copy()).to(dev, non_blocking=False)
            d_m12 = torch.from_numpy(m12_h.copy()).to(dev, non_blocking=False)
            d_nm = torch.full((5,), GUARD, dtype=torch.int32, device=dev)
            ctx.search_for_initialization_device(d_q, total, d_qs, d_qc, int(q_count.max()), d_p,
                                                 d_prev, d_m12, d_nm[1:], 3, st.cuda_stream)
            outs.append((d_prev, d_m12, d_nm))
    for st in streams:
        st.synchronize()
    ctx.sync()
    inside = np.zeros(total, bool)
    for f in (0, 2):
        inside[q_start[f]:q_start[f] + q_count[f]] = True
    for d_prev, d_m12, d_nm in outs:
        prev_g, m12_g, nm_g = d_prev.cpu().numpy(), d_m12.cpu().numpy(), d_nm.cpu().numpy()
        assert nm_g[0] == GUARD and nm_g[4] == GUARD
        assert (m12_g[~inside] == GUARD).all()
        assert prev_g[~inside].tobytes() == prev_h[~inside].tobytes()
        for f in range(3):
            sl = slice(q_start[f], q_start[f] + q_count[f])
            assert nm_g[1 + f] == ref[f][0] == sync[f][0]
            np.testing.assert_array_equal(m12_g[sl], ref[f][1])
            np.testing.assert_array_equal(m12_g[sl], sync[f][1])
            assert prev_g[sl].tobytes() == ref[f][2].tobytes() == sync[f][2].tobytes()
        assert nm_g[2] == 0
    assert ref[0][0] >= 100 and ref[2][0] >= 50


def test_error_codes(world, gpu_lib):
    """Each loud error returns SLAMGPU_EINVAL with a message and writes nothing."""
    G = gpu_lib
    world["load"](1)
    ctx, f = world["ctx"], world["fr"][1]
    q, prev0 = IS.f1_queries(world["fr"][0])
    q, prev0 = np.ascontiguousarray(q[:8]), np.ascontiguousarray(prev0[:8])
    good = G.init_search(0.9, 100, 1)
    L = G.lib()

    def call(frame=0, queries=q, n1=8, params=good, prev=True, m12=True, nm=True):
        pv, mm = prev0.copy(), np.full(8, 41, np.int32)
        out = C.c_int(-77)
        rc = L.slamgpu_search_for_initialization(
            ctx.h, frame, G._ptr(queries) if queries is not None else None, n1,
            G._ptr(params) if params is not None else None, G._ptr(pv) if prev else None,
            G._ptr(mm) if m12 else None, C.byref(out) if nm else None)
        assert pv.tobytes() == prev0.tobytes() and (mm == 41).all() and out.value == -77
        return rc

    def with_(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[k] = v
        return p
    assert call(queries=None) == -1
    assert call(params=None) == -1
    assert call(prev=False) == -1
    assert call(m12=False) == -1
    assert call(nm=False) == -1
    assert b"null" in L.slamgpu_last_error(ctx.h)
    assert call(n1=-1) == -1
    assert call(frame=-1) == -1 and call(frame=1) == -1
    assert b"frame" in L.slamgpu_last_error(ctx.h)
    assert call(params=with_(window_size=-1)) == -1
    assert b"window_size" in L.slamgpu_last_error(ctx.h)
    for bad in (np.nan, np.inf, -np.inf):
        assert call(params=with_(nnratio=bad)) == -1
    assert b"nnratio" in L.slamgpu_last_error(ctx.h)
    assert L.slamgpu_search_for_initialization(None, 0, None, 0, None, None, None, None) == -1
    assert L.slamgpu_frame_mono(None, None, 0, None) == -1
    assert L.slamgpu_frame_mono(ctx.h, None, W, C.byref(ctx.cam)) == -1
    # the batched form: null pointers, frame count out of range, more queries than the workspace
    z = C.c_void_p(0)
    one = C.c_void_p(16)   # never dereferenced: the call fails before any launch
    dcall = lambda *a: L.slamgpu_search_for_initialization_device(ctx.h, *a)  # noqa: E731
    assert dcall(one, 1, one, one, 1, one, one, one, one, 0, z) == -1
    assert dcall(one, 1, one, one, 1, one, one, one, one, 2, z) == -1
    assert dcall(z, 1, one, one, 1, one, one, one, one, 1, z) == -1
    assert dcall(one, 1, z, one, 1, one, one, one, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, z, one, one, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, one, z, one, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, one, one, z, one, 1, z) == -1
    assert dcall(one, 1, one, one, 1, one, one, one, z, 1, z) == -1
    assert dcall(one, -1, one, one, 1, one, one, one, one, 1, z) == -1
    assert dcall(one, 1 << 30, one, one, 1, one, one, one, one, 1, z) == -3
    # and a valid call still works afterwards
    nm, m12, pv = world["dev"](1, q, 0.9, 100, 1, prev0)
    r = world["ref"](1, q, 0.9, 100, 1, prev0)
    assert nm == r[0] and (m12 == r[1]).all()


def test_orbmatcher_method(world, gpu_lib):
    """OrbMatcher.SearchForInitialization: nnratio and checkOri from the instance, vbPrevMatched
    updated in place."""
    G = gpu_lib
    fr = world["fr"]
    world["load"](1)

    class F1:
        keypoints, descriptors = fr[0]["kl"], fr[0]["dl"]
    _, prev0 = IS.f1_queries(fr[0])
    vb = prev0.copy()
    nm, m12 = G.OrbMatcher(0.9, True).SearchForInitialization(world["ctx"], 0, F1, vb, 100)
    r = world["ref"](1, G.init_queries(F1.keypoints, F1.descriptors), 0.9, 100, 1, prev0)
    assert nm == r[0] >= 100
    np.testing.assert_array_equal(m12, r[1])
    assert vb.tobytes() == r[2].tobytes()
    vb = prev0.copy()
    nm10, _ = G.OrbMatcher(0.9, False).SearchForInitialization(world["ctx"], 0, F1, vb)
    assert nm10 == world["ref"](1, G.init_queries(F1.keypoints, F1.descriptors), 0.9, 10, 0, prev0)[0]


def test_adapter_check_program(world, gpu_lib, tmp_path):
    """slamgpu_frame_mono and slamgpu_adapter::search_for_initialization driven from C++
    (tests/initmatch_adapter_check.cpp), no Python in between."""
    from slam_framework_amd import build
    fr, L = world["fr"], world["L"]
    exe = build.build_initmatch_adapter_check()
    d = str(tmp_path)
    _, prev0 = IS.f1_queries(fr[0])
    L[1].tofile(os.path.join(d, "image.u8"))
    fr[0]["kl"].tofile(os.path.join(d, "f1_kps.bin"))
    fr[0]["dl"].tofile(os.path.join(d, "f1_desc.u8"))
    prev0.tofile(os.path.join(d, "prev.f32"))
    out = subprocess.run([exe, d, str(W), str(H), "100", "0.9", "1"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = world["ref"](1, gpu_lib.init_queries(fr[0]["kl"], fr[0]["dl"]), 0.9, 100, 1, prev0)
    assert out.stdout.split() == ["nkps", str(len(fr[1]["kl"])), "nmatches", str(r[0])]
    np.testing.assert_array_equal(np.fromfile(os.path.join(d, "matches12.i32"), np.int32), r[1])
    assert np.fromfile(os.path.join(d, "prev_out.f32"), np.float32).tobytes() == r[2].tobytes()
    assert np.fromfile(os.path.join(d, "f2_kps.bin"), np.uint8).tobytes() == fr[1]["kl"].tobytes()
    assert (np.fromfile(os.path.join(d, "f2_ur.f32"), np.float32) == -1).all()
    assert (np.fromfile(os.path.join(d, "f2_depth.f32"), np.float32) == -1).all()


@pytest.mark.parametrize("cur", [1, 2])
def test_monocular_initialization_chain(world, gpu_lib, cur):
    """Tracker::MonocularInitialization (tracker.cpp:297-364) as device calls: frame_mono ->
    SearchForInitialization -> Initializer::Initialize, against initmatch_ref -> initializer_ref.
    Equal results whether or not it initialises."""
    import initializer_ref as R
    import initializer_scenario as ISC
    G = gpu_lib
    fr = world["fr"]
    world["load"](cur)
    ctx = world["ctx"]

    class F1:
        keypoints, descriptors = fr[0]["kl"], fr[0]["dl"]
    _, prev0 = IS.f1_queries(fr[0])
    vb = prev0.copy()
    nm, m12 = G.OrbMatcher(0.9, True).SearchForInitialization(ctx, 0, F1, vb, 100)
    r = world["ref"](cur, G.init_queries(F1.keypoints, F1.descriptors), 0.9, 100, 1, prev0)
    assert nm == r[0] >= 100 and (m12 == r[1]).all()
    keys1 = prev0
    k2 = ctx.undistorted_keypoints(0)
    keys2 = np.ascontiguousarray(np.stack([k2["x"], k2["y"]], 1), np.float32)
    K = np.array(CAM[:4], np.float32)
    init = G.Initializer(keys1, K, 1.0, 200, random_int=ISC.Lcg(5))
    got = init.Initialize(keys2, m12)
    ref_keys2 = np.ascontiguousarray(np.stack([fr[cur]["kl"]["x"], fr[cur]["kl"]["y"]], 1))
    want, _ = R.initialize(keys1, ref_keys2, r[1], K, 1.0, 200, ISC.Lcg(5))
    print(f"frame {cur}: {nm} matches, initialised {want[0]}")
    assert got[0] == want[0] and init.device_calls == 1
    if want[0]:
        for g, w in zip(got[1:4], want[1:4]):
            ga, wa = np.asarray(g, np.float32), np.asarray(w, np.float32)
            na, nb = np.isnan(ga), np.isnan(wa)
            assert np.array_equal(na, nb)
            assert np.array_equal(ga.view(np.uint32)[~na], wa.view(np.uint32)[~nb])
        assert np.array_equal(got[4], want[4])
