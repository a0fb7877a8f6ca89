"""GPU parity of the LoopCloser's three Sim3 matchers (include/slamgpu_loopmatch.h) against the
CPU restatement tests/loopmatch_ref.c (pinned by tests/test_loopmatch_ref.py): bit-exact
OrbMatcher::Fuse(pKF, Scw, ...) candidates (orb_matcher.cpp:956-1079), the in-order claims of
SearchByProjection(pKF, Scw, ...) (:384-497) and both directions plus the agreement of
SearchBySim3 (:1081-1310), on the kf_scenario keyframes: single calls, the smallest shapes that
can go wrong, the batched device forms with guard words, loud errors, the OrbMatcher surface.

The lower bounds on match counts were checked on the restatement alone before they were fixed
(full keyframes, 335 offered points): nfused 201 at s = 1 (8 best keypoints / 19 best distances
differ from the plain Fuse in each scale case), 175 claims with 219 points passing over a
claimed candidate, nfound 109 / 107."""
import types

import numpy as np
import pytest

import kf_scenario as KS
import loop_scenario as LS

pytestmark = pytest.mark.gpu

W, H = 1241, 376
GUARD = 64


@pytest.fixture(scope="module")
def K(gpu_lib):
    from slam_framework_amd import kfmatch
    return kfmatch


@pytest.fixture(scope="module")
def scene(oracle):
    kfs, _ = KS.keyframes(oracle)
    return kfs


@pytest.fixture(scope="module")
def ref(oracle):
    import loopmatch_ref
    loopmatch_ref.lib()
    return loopmatch_ref


@pytest.fixture(scope="module")
def env(oracle, K):
    return types.SimpleNamespace(grid_o=oracle.grid_geom(W, H), grid=K.kf_grid(W, H),
                                 lv=K.levels(), lva=KS.levels_arrays())


@pytest.fixture(scope="module")
def fpts(scene):
    return KS.fuse_points(scene[0], KS.pose(0))


def _ref_fuse(ref, env, k, blocks, pts, th):
    return ref.fuse_sim3(k, env.grid_o, *blocks, KS.CAM, env.lva[0], env.lva[3], pts, th)


def _ref_sbp(ref, env, k, blocks, pts, matched_in, th):
    return ref.search_by_projection_sim3(k, env.grid_o, *blocks, KS.CAM, env.lva[0], env.lva[3],
                                         pts, matched_in, th)


def _ref_sim3(ref, env, k1, k2, T1, T2, mp1, mp2, a1, a2, sim3, th):
    return ref.search_by_sim3(k1, k2, env.grid_o, T1, T2, mp1, mp2, a1, a2, *sim3, KS.CAM,
                              env.lva[0], env.lva[3], th)


def _pose_kf(K, k, T):
    return K.host_kf_pose(k["kps"], k["desc"], T[:3, :3], T[:3, 3], K.camera_center(T))


# ---- 1. fuse_sim3 -----------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, 0.8, 1.3])
def test_fuse_sim3(oracle, K, ref, env, scene, fpts, s):
    T1 = KS.pose(1)
    blocks = K.decompose_scw(LS.scw(T1, s))
    nf_o, bi_o, bd_o = _ref_fuse(ref, env, scene[1], blocks, fpts, 4.0)
    kf = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *blocks)
    nf_g, bi_g, bd_g = K.fuse_sim3(kf, fpts, 4.0, KS.CAM, env.lv, env.grid)
    print(f"s={s}: nfused {nf_g} (restatement {nf_o})")
    assert nf_g == nf_o
    np.testing.assert_array_equal(bi_g, bi_o)
    np.testing.assert_array_equal(bd_g, bd_o)
    # the chi-square gates of the plain Fuse are really absent
    R, t, Ow = blocks
    _, bi_p, bd_p = oracle.fuse(scene[1]["kps"], scene[1]["desc"], scene[1]["ur"], env.grid_o,
                                R.reshape(-1), t, Ow, KS.CAM, env.lva[0], env.lva[2], env.lva[3],
                                fpts, 4.0)
    assert int(((bi_g != bi_p) | (bd_g != bd_p)).sum()) >= 1
    if s == 1.0:
        assert nf_o > 100


# ---- 2. search_by_projection_sim3 -----------------------------------------------------------
def test_search_by_projection_sim3(K, ref, env, scene, fpts):
    blocks = K.decompose_scw(LS.scw(KS.pose(1), 1.0))
    pts = np.concatenate([fpts, fpts])       # every point meets its own earlier claim
    matched_in = LS.flags(len(scene[1]["desc"]), 0.2, 11)
    nm_o, kpp_o, pkp_o, po = _ref_sbp(ref, env, scene[1], blocks, pts, matched_in, 10.0)
    kf = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *blocks)
    nm_g, kpp_g, pkp_g = K.search_by_projection_sim3(kf, pts, matched_in, 10.0, KS.CAM, env.lv,
                                                     env.grid)
    print(f"nmatches {nm_g} (restatement {nm_o}), {int((po > 0).sum())} points passed over a "
          f"claimed candidate, at most {po.max()}")
    assert nm_g == nm_o
    np.testing.assert_array_equal(kpp_g, kpp_o)
    np.testing.assert_array_equal(pkp_g, pkp_o)
    assert nm_o > 100 and int((po > 0).sum()) > 100
    assert (kpp_g[matched_in > 0] == -1).all()


def test_search_by_projection_sim3_one_point_many_times(oracle, K, ref, env, scene):
    """One point offered 40 times, more than the scan keeps: it walks down its candidate list
    exactly as the sequential loop does (the resolve's rescan path)."""
    from test_loopmatch_ref import repeated_point
    blocks = K.decompose_scw(LS.scw(KS.pose(1), 1.0))
    pts, depth = repeated_point(ref, oracle, scene, blocks, 40)
    assert depth > K.SBP_KEEP
    none = np.zeros(len(scene[1]["desc"]), np.uint8)
    nm_o, kpp_o, pkp_o, _ = _ref_sbp(ref, env, scene[1], blocks, pts, none, 10.0)
    kf = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *blocks)
    nm_g, kpp_g, pkp_g = K.search_by_projection_sim3(kf, pts, none, 10.0, KS.CAM, env.lv, env.grid)
    assert nm_g == nm_o == depth
    np.testing.assert_array_equal(kpp_g, kpp_o)
    np.testing.assert_array_equal(pkp_g, pkp_o)


# ---- 3. search_by_sim3 ------------------------------------------------------------------------
def _sim3_case(K, scene, perturbed):
    T1, T2 = KS.pose(0), KS.pose(1)
    mp1, mp2 = LS.mp_records(scene[0], T1), LS.mp_records(scene[1], T2)
    a1, a2 = LS.flags(len(mp1), 0.15, 21), LS.flags(len(mp2), 0.15, 22)
    sim3 = K.relative_sim3(*LS.relative_pose(T1, T2, *((1.05, 0.2) if perturbed else ())))
    return T1, T2, mp1, mp2, a1, a2, sim3


@pytest.mark.parametrize("perturbed", [False, True])
def test_search_by_sim3(K, ref, env, scene, perturbed):
    T1, T2, mp1, mp2, a1, a2, sim3 = _sim3_case(K, scene, perturbed)
    nf_o, m_o, v1_o, v2_o = _ref_sim3(ref, env, scene[0], scene[1], T1, T2, mp1, mp2, a1, a2, sim3,
                                      7.5)
    nf_g, m_g, v1_g, v2_g = K.search_by_sim3(_pose_kf(K, scene[0], T1), _pose_kf(K, scene[1], T2),
                                             mp1, mp2, a1, a2, sim3, 7.5, KS.CAM, env.lv, env.grid)
    print(f"perturbed={perturbed}: nfound {nf_g} (restatement {nf_o})")
    assert nf_g == nf_o
    np.testing.assert_array_equal(v1_g, v1_o)
    np.testing.assert_array_equal(v2_g, v2_o)
    np.testing.assert_array_equal(m_g, m_o)
    assert nf_o > 50


# ---- 4. the smallest shapes that can go wrong ---------------------------------------------------
def _small(ref, env, K, scene, fpts, n, n_pts):
    """n keypoints of keyframe 1 and n_pts points, chosen so that they still meet: the points the
    full search fuses first, and the keypoints they fuse into first."""
    blocks = K.decompose_scw(LS.scw(KS.pose(1), 1.0))
    _, bi, _ = _ref_fuse(ref, env, scene[1], blocks, fpts, 10.0)
    order = np.concatenate([np.nonzero(bi >= 0)[0], np.nonzero(bi < 0)[0]])[:n_pts]
    pts = fpts[np.sort(order)]
    hit = list(dict.fromkeys(int(j) for j in bi[np.sort(order)] if j >= 0))
    rest = [j for j in range(len(scene[1]["desc"])) if j not in set(hit)]
    idx = np.sort(np.array((hit + rest)[:n]))
    sub = {k: scene[1][k][idx] for k in ("kps", "desc", "ur", "depth")}
    return blocks, sub, pts


SHAPES = list(zip([1, 63, 64, 65, 130], [1, 63, 64, 65, 129]))


@pytest.mark.parametrize("n,n_pts", SHAPES)
def test_small_shapes_scw(K, ref, env, scene, fpts, n, n_pts):
    blocks, sub, pts = _small(ref, env, K, scene, fpts, n, n_pts)
    kf = K.host_kf_pose(sub["kps"], sub["desc"], *blocks)
    nf_o, bi_o, bd_o = _ref_fuse(ref, env, sub, blocks, pts, 4.0)
    nf_g, bi_g, bd_g = K.fuse_sim3(kf, pts, 4.0, KS.CAM, env.lv, env.grid)
    assert nf_g == nf_o
    np.testing.assert_array_equal(bi_g, bi_o)
    np.testing.assert_array_equal(bd_g, bd_o)
    half = (n_pts + 1) // 2                  # n_pts offers, the second half repeating the first
    twice = np.concatenate([pts[:half], pts[:n_pts - half]])
    matched_in = LS.flags(n, 0.2, 5)
    nm_o, kpp_o, pkp_o, _ = _ref_sbp(ref, env, sub, blocks, twice, matched_in, 10.0)
    nm_g, kpp_g, pkp_g = K.search_by_projection_sim3(kf, twice, matched_in, 10.0, KS.CAM, env.lv,
                                                     env.grid)
    assert nm_g == nm_o
    np.testing.assert_array_equal(kpp_g, kpp_o)
    np.testing.assert_array_equal(pkp_g, pkp_o)
    if n >= 63:
        assert nf_o >= 10


@pytest.mark.parametrize("n2,n1", SHAPES)
def test_small_shapes_sim3(K, ref, env, scene, n2, n1):
    T1, T2 = KS.pose(0), KS.pose(1)
    with_depth = np.nonzero(scene[0]["depth"] > 0)[0]
    i1 = np.sort(with_depth[:n1])
    k1 = {k: scene[0][k][i1] for k in ("kps", "desc", "ur", "depth")}
    mp1 = LS.mp_records(k1, T1)
    sim3 = K.relative_sim3(*LS.relative_pose(T1, T2))
    # keyframe 2: the features keyframe 1's points land on in the full keyframe first
    none1 = np.zeros(n1, np.uint8)
    full_mp2 = LS.mp_records(scene[1], T2)
    _, _, v1, _ = _ref_sim3(ref, env, k1, scene[1], T1, T2, mp1, full_mp2, none1,
                            np.zeros(len(full_mp2), np.uint8), sim3, 7.5)
    hit = list(dict.fromkeys(int(j) for j in v1 if j >= 0))
    rest = [j for j in range(len(scene[1]["desc"])) if j not in set(hit)]
    i2 = np.sort(np.array((hit + rest)[:n2]))
    k2 = {k: scene[1][k][i2] for k in ("kps", "desc", "ur", "depth")}
    mp2 = full_mp2[i2]
    a1, a2 = LS.flags(n1, 0.15, 31), LS.flags(n2, 0.15, 32)
    nf_o, m_o, v1_o, v2_o = _ref_sim3(ref, env, k1, k2, T1, T2, mp1, mp2, a1, a2, sim3, 7.5)
    nf_g, m_g, v1_g, v2_g = K.search_by_sim3(_pose_kf(K, k1, T1), _pose_kf(K, k2, T2), mp1, mp2,
                                             a1, a2, sim3, 7.5, KS.CAM, env.lv, env.grid)
    assert nf_g == nf_o
    np.testing.assert_array_equal(v1_g, v1_o)
    np.testing.assert_array_equal(v2_g, v2_o)
    np.testing.assert_array_equal(m_g, m_o)
    if n1 >= 63:
        assert nf_o >= 10


def test_empty_inputs(K, env, scene, fpts):
    """n = 0 keypoints: nothing matches; n_pts = 0: returns 0 and writes nothing."""
    T1 = KS.pose(1)
    blocks = K.decompose_scw(LS.scw(T1, 1.0))
    empty_kf = K.host_kf_pose(scene[1]["kps"][:0], scene[1]["desc"][:0], *blocks)
    full_kf = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *blocks)
    nf, bi, bd = K.fuse_sim3(empty_kf, fpts[:70], 4.0, KS.CAM, env.lv, env.grid)
    assert nf == 0 and (bi == -1).all() and (bd == 256).all()
    nf, bi, bd = K.fuse_sim3(full_kf, fpts[:0], 4.0, KS.CAM, env.lv, env.grid)
    assert nf == 0 and len(bi) == 0 and len(bd) == 0
    nm, kpp, pkp = K.search_by_projection_sim3(empty_kf, fpts[:70], np.zeros(0, np.uint8), 10.0,
                                               KS.CAM, env.lv, env.grid)
    assert nm == 0 and len(kpp) == 0 and (pkp == -1).all()
    nm, kpp, pkp = K.search_by_projection_sim3(full_kf, fpts[:0],
                                               np.zeros(full_kf[0].n, np.uint8), 10.0, KS.CAM,
                                               env.lv, env.grid)
    assert nm == 0 and (kpp == -1).all() and len(pkp) == 0
    mp2 = LS.mp_records(scene[1], T1)
    sim3 = K.relative_sim3(*LS.relative_pose(KS.pose(0), T1))
    nf, m, v1, v2 = K.search_by_sim3(_pose_kf(K, {k: scene[0][k][:0] for k in ("kps", "desc")},
                                              KS.pose(0)), _pose_kf(K, scene[1], T1), mp2[:0], mp2,
                                     np.zeros(0, np.uint8), np.zeros(len(mp2), np.uint8), sim3,
                                     7.5, KS.CAM, env.lv, env.grid)
    assert nf == 0 and len(m) == 0 and len(v1) == 0 and (v2 == -1).all()
    # the device forms return 0 before touching any pointer
    K.fuse_sim3_device(None, 0, None, 0, None, 4.0, KS.CAM, env.lv, env.grid, None, None)
    K.fuse_sim3_device(None, 3, None, 0, None, 4.0, KS.CAM, env.lv, env.grid, None, None)
    K.search_by_projection_sim3_device(None, None, 0, None, 0, 0, None, 0, 10.0, KS.CAM, env.lv,
                                       env.grid, None, None, None, None, 0)
    K.search_by_sim3_device(None, None, 0, None, 0, None, None, 0, 7.5, KS.CAM, env.lv, env.grid,
                            None, None, None, None)


# ---- 5. batched device forms --------------------------------------------------------------------
class Dev:
    def __init__(self):
        import torch
        self.torch, self.dev, self.keep = torch, torch.device("cuda", 0), []

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(
            self.dev)
        self.keep.append(t)
        return t

    def out(self, n):
        """n int32 outputs followed by GUARD guard words, all -9."""
        return self.torch.full((n + GUARD,), -9, dtype=self.torch.int32, device=self.dev)

    def kfs(self, K, frames):
        """frames: (kf dict, Rcw, tcw, Ow)."""
        rec = np.zeros(len(frames), K.KF_DTYPE)
        for i, (k, R, t, Ow) in enumerate(frames):
            rec[i]["kps"], rec[i]["desc"] = self.up(k["kps"]).data_ptr(), self.up(k["desc"]).data_ptr()
            rec[i]["n"] = len(k["desc"])
            rec[i]["Rcw"], rec[i]["tcw"], rec[i]["Ow"] = R.reshape(-1), t, Ow
        return self.up(rec)

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream


def _guard_ok(t, n):
    return bool((t[n:] == -9).all().item())


def test_batched_fuse_sim3_device(K, ref, env, scene, fpts):
    D = Dev()
    T0, T1 = KS.pose(0), KS.pose(1)
    cases = [(scene[1], K.decompose_scw(LS.scw(T1, 1.0))),
             (scene[1], K.decompose_scw(LS.scw(KS.pose(1, (0.02, -0.01, 0.05)), 0.8))),
             (scene[0], K.decompose_scw(LS.scw(T0, 1.3)))]
    d_kfs = D.kfs(K, [(k, *b) for k, b in cases])
    n = len(fpts)
    skip = np.stack([LS.flags(n, 0.1 * (q + 1), 40 + q) for q in range(3)])
    d_pts, d_skip = D.up(fpts), D.up(skip)          # ONE point array for the three keyframes
    d_bi, d_bd = D.out(3 * n), D.out(3 * n)
    K.fuse_sim3_device(d_kfs, 3, d_pts, n, d_skip, 4.0, KS.CAM, env.lv, env.grid, d_bi, d_bd,
                       D.stream)
    D.torch.cuda.synchronize()
    assert _guard_ok(d_bi, 3 * n) and _guard_ok(d_bd, 3 * n)
    bi, bd = d_bi.cpu().numpy()[:3 * n].reshape(3, n), d_bd.cpu().numpy()[:3 * n].reshape(3, n)
    total = 0
    for q, (k, b) in enumerate(cases):
        p = fpts.copy()
        p["skip"] = skip[q]
        nf_o, bi_o, bd_o = _ref_fuse(ref, env, k, b, p, 4.0)
        np.testing.assert_array_equal(bi[q], bi_o)
        np.testing.assert_array_equal(bd[q], bd_o)
        total += nf_o
    assert total > 200
    # d_skip = NULL: the records' own skip flags, for every keyframe
    d_bi2, d_bd2 = D.out(3 * n), D.out(3 * n)
    K.fuse_sim3_device(d_kfs, 3, d_pts, n, None, 4.0, KS.CAM, env.lv, env.grid, d_bi2, d_bd2,
                       D.stream)
    D.torch.cuda.synchronize()
    assert _guard_ok(d_bi2, 3 * n) and _guard_ok(d_bd2, 3 * n)
    for q, (k, b) in enumerate(cases):
        _, bi_o, bd_o = _ref_fuse(ref, env, k, b, fpts, 4.0)
        np.testing.assert_array_equal(d_bi2.cpu().numpy()[q * n:(q + 1) * n], bi_o)
        np.testing.assert_array_equal(d_bd2.cpu().numpy()[q * n:(q + 1) * n], bd_o)


def test_batched_search_by_projection_sim3_device(K, ref, env, scene, fpts):
    D = Dev()
    T0, T1 = KS.pose(0), KS.pose(1)
    b1, b0 = K.decompose_scw(LS.scw(T1, 1.0)), K.decompose_scw(LS.scw(T0, 0.8))
    d_kfs = D.kfs(K, [(scene[1], *b1), (scene[0], *b0)])
    n1, n0 = len(scene[1]["desc"]), len(scene[0]["desc"])
    pts_a = np.concatenate([fpts, fpts])
    pts_b = np.concatenate([fpts[::-1], fpts[:100]])
    allp = np.concatenate([pts_a, pts_b])
    jobs = np.zeros(2, K.SBP_JOB_DTYPE)
    jobs[0] = (0, 0, len(pts_a), 0)
    jobs[1] = (1, len(pts_a), len(pts_b), n1)
    mi = np.concatenate([LS.flags(n1, 0.2, 51), LS.flags(n0, 0.3, 52)])
    sb = K.search_by_projection_sim3_scratch_bytes(len(allp))
    d_scr = D.torch.zeros(sb, dtype=D.torch.uint8, device=D.dev)
    d_kpp, d_pkp, d_nm = D.out(n1 + n0), D.out(len(allp)), D.out(2)
    K.search_by_projection_sim3_device(d_kfs, D.up(allp), len(allp), D.up(jobs), 2,
                                       max(len(pts_a), len(pts_b)), D.up(mi), n1 + n0, 10.0,
                                       KS.CAM, env.lv, env.grid, d_kpp, d_pkp, d_nm, d_scr, sb,
                                       D.stream)
    D.torch.cuda.synchronize()
    assert _guard_ok(d_kpp, n1 + n0) and _guard_ok(d_pkp, len(allp)) and _guard_ok(d_nm, 2)
    kpp, pkp, nm = d_kpp.cpu().numpy(), d_pkp.cpu().numpy(), d_nm.cpu().numpy()
    for j, (k, b, p, m, kb, kn, pb) in enumerate([
            (scene[1], b1, pts_a, mi[:n1], 0, n1, 0),
            (scene[0], b0, pts_b, mi[n1:], n1, n0, len(pts_a))]):
        nm_o, kpp_o, pkp_o, _ = _ref_sbp(ref, env, k, b, p, m, 10.0)
        assert nm[j] == nm_o and nm_o > 100
        np.testing.assert_array_equal(kpp[kb:kb + kn], kpp_o)
        np.testing.assert_array_equal(pkp[pb:pb + len(p)], pkp_o)


def test_batched_search_by_sim3_device(K, ref, env, scene):
    D = Dev()
    T1, T2 = KS.pose(0), KS.pose(1)
    frames = [(scene[0], T1[:3, :3], T1[:3, 3], K.camera_center(T1)),
              (scene[1], T2[:3, :3], T2[:3, 3], K.camera_center(T2))]
    d_kfs = D.kfs(K, frames)
    mp = [LS.mp_records(scene[0], T1), LS.mp_records(scene[1], T2)]
    n = [len(mp[0]), len(mp[1])]
    begin = [0, n[0]]
    Ts = [T1, T2]
    plist = [(0, 1, (1.0, 0.0)), (1, 0, (1.0, 0.0)), (0, 1, (1.05, 0.2))]
    stride = 2100
    pairs = np.zeros(3, K.SIM3_PAIR_DTYPE)
    a1, a2 = np.zeros((3, stride), np.uint8), np.zeros((3, stride), np.uint8)
    sims = []
    for p, (a, b, pert) in enumerate(plist):
        sim3 = K.relative_sim3(*LS.relative_pose(Ts[a], Ts[b], *pert))
        sims.append(sim3)
        pairs[p] = (a, b, begin[a], begin[b], sim3[0].reshape(-1), sim3[1], sim3[2].reshape(-1),
                    sim3[3])
        a1[p, :n[a]], a2[p, :n[b]] = LS.flags(n[a], 0.15, 60 + p), LS.flags(n[b], 0.15, 70 + p)
    d_m, d_v1, d_v2, d_nf = D.out(3 * stride), D.out(3 * stride), D.out(3 * stride), D.out(3)
    K.search_by_sim3_device(d_kfs, D.up(np.concatenate(mp)), n[0] + n[1], D.up(pairs), 3,
                            D.up(a1), D.up(a2), stride, 7.5, KS.CAM, env.lv, env.grid, d_m, d_v1,
                            d_v2, d_nf, D.stream)
    D.torch.cuda.synchronize()
    for t in (d_m, d_v1, d_v2):
        assert _guard_ok(t, 3 * stride)
    assert _guard_ok(d_nf, 3)
    m, v1, v2, nf = (t.cpu().numpy() for t in (d_m, d_v1, d_v2, d_nf))
    for p, (a, b, _) in enumerate(plist):
        nf_o, m_o, v1_o, v2_o = _ref_sim3(ref, env, scene[a], scene[b], Ts[a], Ts[b], mp[a], mp[b],
                                          a1[p, :n[a]], a2[p, :n[b]], sims[p], 7.5)
        assert nf[p] == nf_o and nf_o > 50
        row = slice(p * stride, p * stride + n[a])
        np.testing.assert_array_equal(m[row], m_o)
        np.testing.assert_array_equal(v1[row], v1_o)
        np.testing.assert_array_equal(v2[p * stride:p * stride + n[b]], v2_o)
        assert (m[p * stride + n[a]:(p + 1) * stride] == -9).all()   # past n: untouched


# ---- 6. loud errors ---------------------------------------------------------------------------
def test_errors_are_loud(K, env, scene, fpts):
    import ctypes as C
    from slam_framework_amd.slamgpu import SlamGpuError
    blocks = K.decompose_scw(LS.scw(KS.pose(1), 1.0))
    kf = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *blocks)
    pts = fpts[:8]
    # n > SLAMGPU_KF_MAX_FEATURES
    big = K.host_kf_pose(np.resize(scene[1]["kps"], 4097), np.resize(scene[1]["desc"], (4097, 32)),
                         *blocks)
    with pytest.raises(SlamGpuError, match="outside"):
        K.fuse_sim3(big, pts, 4.0, KS.CAM, env.lv, env.grid)
    with pytest.raises(SlamGpuError, match="outside"):
        K.search_by_projection_sim3(big, pts, np.zeros(4097, np.uint8), 10.0, KS.CAM, env.lv,
                                    env.grid)
    mp = np.resize(fpts, 4097)
    with pytest.raises(SlamGpuError, match="outside"):
        K.search_by_sim3(big, kf, mp, mp[:kf[0].n], np.zeros(4097, np.uint8),
                         np.zeros(kf[0].n, np.uint8), K.relative_sim3(1.0, np.eye(3), np.zeros(3)),
                         7.5, KS.CAM, env.lv, env.grid)
    # nlevels = 0
    lv0 = K.levels()
    lv0.nlevels = 0
    with pytest.raises(SlamGpuError, match="nlevels"):
        K.fuse_sim3(kf, pts, 4.0, KS.CAM, lv0, env.grid)
    with pytest.raises(SlamGpuError, match="nlevels"):
        K.search_by_projection_sim3(kf, pts, np.zeros(kf[0].n, np.uint8), 10.0, KS.CAM, lv0,
                                    env.grid)
    with pytest.raises(SlamGpuError, match="nlevels"):
        K.fuse_sim3_device(1, 1, 1, 1, None, 4.0, KS.CAM, lv0, env.grid, 1, 1)
    # NULL arrays and negative counts, straight at the C ABI
    L, cam = K.lib(), K._cam(KS.CAM)
    out = np.zeros(16, np.int32)
    n_out = C.c_int()
    args = (C.byref(cam), C.byref(env.lv), C.byref(env.grid))
    with pytest.raises(SlamGpuError, match="NULL"):
        K._check(L.slamgpu_fuse_sim3(C.byref(kf[0]), None, 8, 4.0, *args, K._p(out), K._p(out),
                                     C.byref(n_out)))
    with pytest.raises(SlamGpuError, match="< 0"):
        K._check(L.slamgpu_fuse_sim3(C.byref(kf[0]), K._p(pts), -1, 4.0, *args, K._p(out),
                                     K._p(out), C.byref(n_out)))
    with pytest.raises(SlamGpuError, match="NULL"):
        K._check(L.slamgpu_search_by_projection_sim3(C.byref(kf[0]), K._p(pts), 8, None, 10.0,
                                                     *args, K._p(out), K._p(out), C.byref(n_out)))
    with pytest.raises(SlamGpuError, match="< 0"):
        K.fuse_sim3_device(1, -1, 1, 1, None, 4.0, KS.CAM, env.lv, env.grid, 1, 1)
    with pytest.raises(SlamGpuError, match="NULL"):
        K.fuse_sim3_device(None, 1, None, 1, None, 4.0, KS.CAM, env.lv, env.grid, None, None)
    with pytest.raises(SlamGpuError, match="negative"):
        K.search_by_sim3_device(1, 1, 1, 1, -2, 1, 1, 8, 7.5, KS.CAM, env.lv, env.grid, 1, 1, 1, 1)
    with pytest.raises(SlamGpuError, match="scratch"):
        K.search_by_projection_sim3_device(1, 1, 100, 1, 1, 100, 1, 10, 10.0, KS.CAM, env.lv,
                                           env.grid, 1, 1, 1, 1, 16)
    assert K.lib().slamgpu_loopmatch_last_error().decode() != ""


# ---- 7. the OrbMatcher surface ---------------------------------------------------------------
def test_orb_matcher_surface(K, env, scene, fpts):
    from slam_framework_amd.slamgpu import OrbMatcher
    T1, T2 = KS.pose(0), KS.pose(1)
    M = OrbMatcher(0.75, True)
    Scw = LS.scw(T2, 0.8)
    kf = types.SimpleNamespace(keypoints=scene[1]["kps"], descriptors=scene[1]["desc"])
    hk = K.host_kf_pose(scene[1]["kps"], scene[1]["desc"], *K.decompose_scw(Scw))
    nf, bi = M.FuseSim3(kf, Scw, fpts, 4.0, KS.CAM, env.lv, env.grid)
    nf2, bi2, _ = K.fuse_sim3(hk, fpts, 4.0, KS.CAM, env.lv, env.grid)
    assert nf == nf2 > 100
    np.testing.assert_array_equal(bi, bi2)
    # SearchByProjection: vpMatched holds map point ids, -1 = none
    matched_in = LS.flags(len(scene[1]["desc"]), 0.2, 11)
    vpMatched = np.where(matched_in > 0, 900000, -1)
    ids = 1000 + np.arange(len(fpts))
    nm = M.SearchByProjectionSim3(kf, Scw, fpts, vpMatched, 10.0, KS.CAM, env.lv, env.grid, ids)
    nm2, kpp, _ = K.search_by_projection_sim3(hk, fpts, matched_in, 10.0, KS.CAM, env.lv, env.grid)
    assert nm == nm2 > 100
    np.testing.assert_array_equal(vpMatched[kpp >= 0], ids[kpp[kpp >= 0]])
    assert (vpMatched[matched_in > 0] == 900000).all()
    assert ((vpMatched == -1) == ((kpp < 0) & (matched_in == 0))).all()
    # SearchBySim3: map point ids per feature; vpMatches12 pre-filled on a few features
    mp1, mp2 = LS.mp_records(scene[0], T1), LS.mp_records(scene[1], T2)
    id1 = np.where(mp1["skip"] == 0, 5000 + np.arange(len(mp1)), -1)
    id2 = np.where(mp2["skip"] == 0, 7000 + np.arange(len(mp2)), -1)
    mk = lambda k, T, ids_, rec: types.SimpleNamespace(  # noqa: E731
        keypoints=k["kps"], descriptors=k["desc"], Tcw=T, map_points=ids_, mp_records=rec)
    vp12 = np.full(len(mp1), -1, np.int64)
    pre2 = np.nonzero(id2 >= 0)[0][:20]
    pre1 = np.nonzero(id1 >= 0)[0][:20]
    vp12[pre1] = id2[pre2]
    before = vp12.copy()
    s12, R12, t12 = LS.relative_pose(T1, T2)
    nfound = M.SearchBySim3(mk(scene[0], T1, id1, mp1), mk(scene[1], T2, id2, mp2), vp12, s12, R12,
                            t12, 7.5, KS.CAM, env.lv, env.grid)
    a1 = (before >= 0).astype(np.uint8)
    a2 = np.zeros(len(mp2), np.uint8)
    a2[pre2] = 1
    nf3, m12, _, _ = K.search_by_sim3(_pose_kf(K, scene[0], T1), _pose_kf(K, scene[1], T2), mp1,
                                      mp2, a1, a2, K.relative_sim3(s12, R12, t12), 7.5, KS.CAM,
                                      env.lv, env.grid)
    assert nfound == nf3 > 50
    sel = m12 >= 0
    np.testing.assert_array_equal(vp12[sel], id2[m12[sel]])
    np.testing.assert_array_equal(vp12[~sel], before[~sel])
