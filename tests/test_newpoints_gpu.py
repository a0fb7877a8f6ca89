"""GPU parity of CreateNewMapPoints (include/slamgpu_kfmatch.h, csrc/newpoints.hip) against the
CPU chain newpoints_ref.newpoints_chain (the oracle's SearchForTriangulation + tests/newpoints_ref.c)
bit for bit: n_new, the slamgpu_fuse_point and slamgpu_new_point lists, the status rows and the
updated has_mp1, on the synthetic scenes of newpoints_scenario.py. Every output of every device
call here lies between 64-byte guards of 0xA5 and is pre-filled with 0xA5, so a write outside a
row or past n_new shows."""
import functools

import numpy as np
import pytest

import newpoints_ref as R
import newpoints_scenario as NS

pytestmark = pytest.mark.gpu

BLOCK = 512  # new_points_kernel's workgroup size (kNpThreads)
GUARD = 64
SC, S2 = NS.levels_arrays()


@pytest.fixture(scope="module")
def K(gpu_lib):
    from slam_framework_amd import kfmatch
    return kfmatch


@functools.lru_cache(maxsize=None)
def scene(n1, seed, n_nbors=1, kind="mixed", skips=(), mp_frac=0.1, n2=None):
    cur, nbors = NS.scene(n1, seed, n_nbors, kind, skips=skips, mp_frac=mp_frac, n2=n2)
    return cur, nbors, R.newpoints_chain(cur, nbors, SC, S2)


class Guarded:
    """A device buffer of `nbytes` 0xA5 bytes between two guards."""

    def __init__(self, torch, dev, nbytes, init=None):
        self.nbytes = nbytes
        self.t = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        if init is not None:
            self.t[GUARD:GUARD + nbytes] = torch.from_numpy(
                np.ascontiguousarray(init).view(np.uint8).reshape(-1).copy()).to(dev)
        self.ptr = int(self.t.data_ptr()) + GUARD

    def get(self, dtype=np.uint8):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == 0xA5).all() and (a[GUARD + self.nbytes:] == 0xA5).all(), "guard hit"
        return a[GUARD:GUARD + self.nbytes].copy().view(dtype)


def run_device(K, jobs, check_ori=True, point_stride=None):
    """jobs = [(cur, nbors)]. One slamgpu_create_new_map_points_device call; returns per job
    dict(n_new, points, news, status, has_mp1, d_points (device address), tail_clean) and the
    objects that keep the device memory alive."""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
        keep.append(t)
        return int(t.data_ptr())

    all_kfs = []
    jrec, nrec, mps = [], [], []
    for cur, nbors in jobs:
        jrec.append((len(all_kfs), len(nrec), len(nbors)))
        all_kfs.append(cur)
        for nb in nbors:
            nrec.append((len(all_kfs), nb))
            all_kfs.append(nb["kf"])
    kfs = np.zeros(len(all_kfs), K.KF_DTYPE)
    kst = np.zeros(len(all_kfs), K.KF_STEREO_DTYPE)
    for i, k in enumerate(all_kfs):
        T = np.asarray(k["T"], np.float32)
        kfs[i]["kps"], kfs[i]["desc"] = up(k["kps"]), up(k["desc"])
        kfs[i]["u_right"], kfs[i]["has_mp"] = up(k["ur"]), up(k["mp"])
        kfs[i]["nodes"] = up(k["fv"][0].astype(np.uint32))
        kfs[i]["node_start"] = up(k["fv"][1].astype(np.int32))
        kfs[i]["node_feats"] = up(k["fv"][2].astype(np.uint32))
        kfs[i]["n"], kfs[i]["n_nodes"] = len(k["desc"]), len(k["fv"][0])
        kfs[i]["Rcw"], kfs[i]["tcw"], kfs[i]["Ow"] = T[:3, :3].reshape(-1), T[:3, 3], k["Ow"]
        kst[i]["depth"] = up(k["depth"])
        kst[i]["raw_kps"] = 0 if k.get("raw") is None else up(k["raw"])
        kst[i]["cam"], kst[i]["mb"] = k["cam"], k["mb"]
    jarr = np.zeros(len(jobs), K.NP_JOB_DTYPE)
    for j, (kf1, first, nn) in enumerate(jrec):
        g = Guarded(torch, dev, len(jobs[j][0]["desc"]), jobs[j][0]["mp"])
        mps.append(g)
        kfs[kf1]["has_mp"] = g.ptr
        jarr[j] = (kf1, first, nn, 0, g.ptr)
    narr = np.zeros(max(len(nrec), 1), K.NP_NBOR_DTYPE)
    for r, (kf2, nb) in enumerate(nrec):
        narr[r] = (kf2, np.asarray(nb["F12"], np.float32).reshape(-1), nb["skip"], nb["first_obs"])
    nj = len(jobs)
    max_nbors = max(nn for _, _, nn in jrec)
    n1s = [len(c["desc"]) for c, _ in jobs]
    stride = max(max(n1s), 1)
    pstride = stride if point_stride is None else point_stride
    g_n = Guarded(torch, dev, 4 * nj)
    g_p = Guarded(torch, dev, 80 * nj * pstride)
    g_q = Guarded(torch, dev, 16 * nj * pstride)
    g_s = Guarded(torch, dev, nj * max_nbors * stride)
    sb = K.create_new_map_points_scratch_bytes(nj, max_nbors)
    g_x = Guarded(torch, dev, sb)
    cam = all_kfs[0]["cam"]
    K.create_new_map_points_device(up(kfs), up(kst), up(jarr), nj, up(narr), max_nbors, cam,
                                   K.levels(), check_ori, g_n.ptr, g_p.ptr, g_q.ptr, pstride,
                                   g_s.ptr, stride, g_x.ptr, sb,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g_x.get()
    n_new = g_n.get(np.int32)
    pts = g_p.get().reshape(nj, pstride * 80)
    nws = g_q.get().reshape(nj, pstride * 16)
    sts = g_s.get(np.int8).reshape(nj, max_nbors, stride)
    out = []
    for j in range(nj):
        n = max(int(n_new[j]), 0)
        nn = jrec[j][2]
        rows = sts[j, :nn, :n1s[j]]
        tail = [pts[j, 80 * n:], nws[j, 16 * n:], sts[j, :nn, n1s[j]:], sts[j, nn:]]
        out.append(dict(n_new=int(n_new[j]), points=pts[j, :80 * n].copy().view(K.FUSE_POINT_DTYPE),
                        news=nws[j, :16 * n].copy().view(K.NEW_POINT_DTYPE), status=rows,
                        has_mp1=mps[j].get(), d_points=g_p.ptr + 80 * j * pstride,
                        tail_clean=all((t.view(np.uint8) == 0xA5).all() for t in tail)))
    return out, (keep, mps, g_n, g_p, g_q, g_s, g_x, kfs)


def assert_same(got, ref, tail=True):
    assert got["n_new"] == ref["n_new"]
    if ref["n_new"] < 0:
        return
    for f in R.FUSE_POINT_DTYPE.names:
        np.testing.assert_array_equal(got["points"][f], ref["points"][f], err_msg=f)
    for f in R.NEW_POINT_DTYPE.names:
        np.testing.assert_array_equal(got["news"][f], ref["news"][f], err_msg=f)
    np.testing.assert_array_equal(got["status"], ref["status"])
    np.testing.assert_array_equal(got["has_mp1"], ref["has_mp1"])
    if tail:
        assert got["tail_clean"], "wrote past n_new or past a status row"


@pytest.mark.parametrize("n1", [1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes(K, n1):
    cur, nbors, ref = scene(n1, 100 + n1, 2)
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)
    if n1 >= 63:
        assert ref["n_new"] > n1 // 4


def test_feature_limit(K):
    """n1 = SLAMGPU_KF_MAX_FEATURES runs; one more makes the search report -1 and n_new = -1."""
    cur, nbors, ref = scene(4096, 7, 1, n2=600)
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)
    assert ref["n_new"] > 100
    cur, nbors, ref = scene(4097, 7, 1, n2=600)
    assert ref["n_new"] == -1
    got, _ = run_device(K, [(cur, nbors)])
    assert got[0]["n_new"] == -1
    np.testing.assert_array_equal(got[0]["has_mp1"], cur["mp"])


def test_no_matches(K):
    """Every keypoint of the current keyframe already has a map point: no match, no point."""
    cur, nbors, ref = scene(200, 11, 2, mp_frac=1.0)
    assert ref["n_new"] == 0 and not ref["status"].any()
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)


@pytest.mark.parametrize("n_nbors,skips", [(1, ()), (2, ()), (3, ()), (3, (1,))])
def test_neighbours(K, n_nbors, skips):
    cur, nbors, ref = scene(300, 21, n_nbors, skips=skips)
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)
    assert sorted(set(ref["news"]["neighbour"])) == [k for k in range(n_nbors) if k not in skips]
    assert (np.diff(ref["news"]["neighbour"]) >= 0).all()
    for k in range(n_nbors):
        assert (np.diff(ref["news"]["idx1"][ref["news"]["neighbour"] == k]) > 0).all()


def test_chain_dependency(K):
    """A keypoint accepted against the first neighbour is gone from the second search; one that
    was matched and rejected may be matched again."""
    cur, nbors, ref = scene(300, 31, 2)
    m0, m1 = ref["matches"]
    acc0 = ref["status"][0] > 0
    rej0 = ref["status"][0] < 0
    assert acc0.sum() > 50 and (m1[acc0] < 0).all()
    assert (m1[rej0] >= 0).any()
    # without the has_mp update the second search would have matched accepted keypoints again
    free = R.newpoints_chain(cur, [nbors[1]], SC, S2)["matches"][0]
    assert (free[acc0] >= 0).any()
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)


def test_three_jobs_equal_single_runs(K):
    scenes = [scene(300, 21, 3, skips=(1,)), scene(65, 165, 2), scene(500, 41, 1, kind="stereo")]
    got, _ = run_device(K, [(c, n) for c, n, _ in scenes])
    for g, (cur, nbors, ref) in zip(got, scenes):
        assert_same(g, ref)
        single, _ = run_device(K, [(cur, nbors)])
        assert_same(single[0], ref)
        for f in ("points", "news", "status", "has_mp1"):
            assert g[f].tobytes() == single[0][f].tobytes()


def test_sources_and_statuses(K):
    """A mono-only, a stereo-only and a mixed keyframe: all three sources and every test of
    :372-471 that a well-formed keyframe pair can fail occur. x3D(3) == 0, a zero distance, a
    stereo keypoint without depth and a malformed match need constructed keyframes: their device
    parity is test_constructed_rejections."""
    seen = set()
    for kind, seed in (("mono", 51), ("stereo", 52), ("mixed", 53)):
        cur, nbors, ref = scene(600, seed, 3, kind=kind)
        got, _ = run_device(K, [(cur, nbors)])
        assert_same(got[0], ref)
        seen |= set(got[0]["status"].reshape(-1).tolist())
        if kind == "mono":
            assert set(ref["news"]["source"]) == {R.DLT}
    assert {R.DLT, R.STEREO1, R.STEREO2} <= seen
    assert {R.LOW_PARALLAX, R.BEHIND1, R.BEHIND2, R.REPROJ1_STEREO, R.REPROJ1_MONO,
            R.REPROJ2_STEREO, R.REPROJ2_MONO, R.SCALE} <= seen, sorted(seen)


def test_constructed_rejections(K):
    """The rejections no natural scene reaches, through the device path: a stereo keypoint whose
    depth is not positive (NO_DEPTH), NaN poses, x3D(3) == 0 (W_ZERO: rotation blocks with a zero
    third column) and a neighbour centre equal to the point in every bit (DIST_ZERO)."""
    cur, nbors, _ = scene(200, 61, 1, kind="stereo")
    cur = dict(cur, depth=np.where(np.arange(200) % 3 == 0, np.float32(-1.0), cur["depth"]))
    ref = R.newpoints_chain(cur, nbors, SC, S2)
    assert (ref["status"] == R.NO_DEPTH).any()
    got, _ = run_device(K, [(cur, nbors)])
    assert_same(got[0], ref)
    T = cur["T"].copy()
    T[1, 3] = np.nan
    bad = dict(cur, T=T)
    ref = R.newpoints_chain(bad, nbors, SC, S2)
    got, _ = run_device(K, [(bad, nbors)])
    assert_same(got[0], ref)
    # one keypoint each; the epipolar line of F12 is the row of the neighbour's keypoint
    k1, k2 = NS.degenerate_pose_pair()
    F = np.zeros(9, np.float32)
    F[7], F[8] = 1.0, -k2["kps"]["y"][0]
    w_zero = (k1, [dict(kf=k2, F12=F, skip=0, first_obs=0)])
    k1, k2 = NS.wide_pair()
    xyz = R.pair_one(k1, k2, 0, 0, SC, S2)[1]["xyz"]
    nb = dict(kf=NS.with_(k2, Ow=xyz), F12=NS.fundamental(k1["T"], k2["T"]), skip=0, first_obs=1)
    refs = [R.newpoints_chain(c, n, SC, S2) for c, n in (w_zero, (k1, [nb]))]
    assert [int(r["status"][0, 0]) for r in refs] == [R.W_ZERO, R.DIST_ZERO]
    for job, r in zip((w_zero, (k1, [nb])), refs):  # one call each: the cameras differ
        got, _ = run_device(K, [job])
        assert_same(got[0], r)


def test_point_capacity(K):
    """point_stride smaller than the number of new points: n_new = -1, nothing past the rows."""
    cur, nbors, ref = scene(300, 21, 1)
    assert ref["n_new"] > 40
    got, _ = run_device(K, [(cur, nbors)], point_stride=40)
    assert got[0]["n_new"] == -1


def test_synchronous_call_equals_device(K):
    from slam_framework_amd.bow import FeatureVector
    cur, nbors, ref = scene(300, 21, 3, skips=(1,))

    def host(k):
        return (K.host_kf(k["kps"], k["desc"], k["ur"], k["T"], k["mp"], FeatureVector(*k["fv"])),
                K.host_kf_stereo(k["depth"], k["cam"], k["mb"], k.get("raw")))
    a, a_st = host(cur)
    a[0].Ow[:] = [float(x) for x in cur["Ow"]]
    hn = []
    for nb in nbors:
        b, b_st = host(nb["kf"])
        b[0].Ow[:] = [float(x) for x in nb["kf"]["Ow"]]
        hn.append((b, b_st, nb["F12"], nb["skip"], nb["first_obs"]))
    n_new, pts, news, status, has_mp1 = K.create_new_map_points(a, a_st, hn, cur["cam"], K.levels())
    assert_same(dict(n_new=n_new, points=pts, news=news, status=status, has_mp1=has_mp1), ref,
                tail=False)
    np.testing.assert_array_equal(status[1], 0)


def test_list_feeds_fuse_device(K):
    """The compacted slamgpu_fuse_point list handed to slamgpu_fuse_device as it lies in device
    memory gives what the same points packed on the host give."""
    import torch
    dev = torch.device("cuda", 0)
    cur, nbors, ref = scene(300, 21, 2)
    got, hold = run_device(K, [(cur, nbors)])
    n = got[0]["n_new"]
    assert n == ref["n_new"] > 50
    d_kfs = torch.from_numpy(hold[-1].view(np.uint8).copy()).to(dev)
    pkf = torch.full((n,), 2, dtype=torch.int32, device=dev)  # fuse into the second neighbour
    grid, lv = K.kf_grid(1241, 376), K.levels()
    res = []
    packed = torch.from_numpy(ref["points"].view(np.uint8).copy()).to(dev)
    for d_pts in (got[0]["d_points"], packed):
        bi = torch.full((n,), -7, dtype=torch.int32, device=dev)
        bd = torch.full((n,), -7, dtype=torch.int32, device=dev)
        K.fuse_device(d_kfs, d_pts, pkf, n, 3.0, cur["cam"], lv, grid, bi, bd,
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res.append((bi.cpu().numpy(), bd.cpu().numpy()))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert (res[0][0] >= 0).sum() > 20
