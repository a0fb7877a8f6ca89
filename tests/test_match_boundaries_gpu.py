"""The constructed boundary cases of tests/boundary_scenario.py on the device matchers
(kfmatch.hip, loopmatch.hip, the search_cand / search_resolve kernels of orb_search.hip): the
device call's whole output arrays and counts equal the CPU restatement's, which
tests/test_match_boundaries.py holds to the expectations written down from orb_matcher.cpp. Every
case runs through the single call of its entry point, and once through the batched device form of
each of the eight entry points with all its cases in one launch (one launch per window factor,
check_ori setting or nnratio where that is a launch parameter): the batch neighbours are then
boundary cases too. SearchByBoW's cases run through its single call only."""
import numpy as np
import pytest

import boundary_scenario as BS
import test_match_boundaries as TB

pytestmark = pytest.mark.gpu

KF_CASES = BS.kf_cases()
GUARD = 64


@pytest.fixture(scope="module")
def refs(oracle):
    import loopmatch_ref
    import relocmatch_ref
    loopmatch_ref.lib()
    relocmatch_ref.lib()
    return dict(oracle=oracle, loop=loopmatch_ref, reloc=relocmatch_ref,
                grid=oracle.grid_geom(BS.W, BS.H))


@pytest.fixture(scope="module")
def K(gpu_lib):
    from slam_framework_amd import kfmatch
    return kfmatch


def _fv(k):
    from slam_framework_amd.bow import FeatureVector
    return FeatureVector(*k["fv"])


def _tri_kfs(K, i):
    a = K.host_kf(i["k1"]["kps"], i["k1"]["desc"], i["k1"]["ur"], i["T1"], i["k1"]["mp"],
                  _fv(i["k1"]))
    b = K.host_kf(i["k2"]["kps"], i["k2"]["desc"], i["k2"]["ur"], i["T2"], i["k2"]["mp"],
                  _fv(i["k2"]))
    return a, b


def dev_outputs(K, c):
    """The device's outputs of one keyframe-matcher case through the synchronous call."""
    i, lv, grid = c.inp, K.levels(), K.kf_grid(BS.W, BS.H)
    if c.entry == "tri":
        a, b = _tri_kfs(K, i)
        nm, m = K.search_for_triangulation(a, b, i["F"], BS.CAM, lv, i["only_stereo"],
                                           i["check_ori"])
        return dict(n=nm, match12=m)
    if c.entry == "bow":
        from slam_framework_amd import bow
        a, b = i["k1"], i["k2"]
        valid = np.ones(len(b["desc"]), np.uint8) if i["kf_kf"] else None
        nm, m = bow.search_by_bow(a["desc"], a["kps"], None, _fv(a), b["desc"], b["kps"], _fv(b),
                                  b_valid=valid, kf_kf=i["kf_kf"], nnratio=i["nnratio"],
                                  check_ori=i["check_ori"])
        return dict(n=nm, match12=m)
    kf = i.get("kf")
    if c.entry == "fuse":
        h = K.host_kf(kf["kps"], kf["desc"], kf["ur"], BS.T_ID)
        nf, bi, bd = K.fuse(h, i["pts"], i["th"], BS.CAM, lv, grid)
        return dict(n=nf, best_idx=bi, best_dist=bd)
    if c.entry == "fuse_sim3":
        h = K.host_kf_pose(kf["kps"], kf["desc"], BS.I3, BS.Z3, BS.Z3)
        nf, bi, bd = K.fuse_sim3(h, i["pts"], i["th"], BS.CAM, lv, grid)
        return dict(n=nf, best_idx=bi, best_dist=bd)
    if c.entry == "sbp_sim3":
        h = K.host_kf_pose(kf["kps"], kf["desc"], BS.I3, BS.Z3, BS.Z3)
        nm, kpp, pkp = K.search_by_projection_sim3(h, i["pts"], i["matched_in"], i["th"], BS.CAM,
                                                   lv, grid)
        return dict(n=nm, kp_point=kpp, point_kp=pkp)
    h1 = K.host_kf_pose(i["k1"]["kps"], i["k1"]["desc"], BS.I3, BS.Z3, BS.Z3)
    h2 = K.host_kf_pose(i["k2"]["kps"], i["k2"]["desc"], BS.I3, BS.Z3, BS.Z3)
    nf, m, v1, v2 = K.search_by_sim3(h1, h2, i["mp1"], i["mp2"], i["a1"], i["a2"],
                                     (BS.I3, BS.Z3, BS.I3, BS.Z3), i["th"], BS.CAM, lv, grid)
    return dict(n=nf, match12=m, vn1=v1, vn2=v2)


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("c", KF_CASES, ids=[c.id for c in KF_CASES])
def test_keyframe_matcher_single_call(K, refs, c):
    got = dev_outputs(K, c)
    same(got, TB.ref_outputs(refs, c), f"{c.id} ({c.cite})")
    TB.check_case(c, got)


# ---- the batched device forms -------------------------------------------------------------------
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

    def take(self, t, n):
        self.torch.cuda.synchronize()
        a = t.cpu().numpy()
        assert (a[n:] == -9).all(), "wrote past the outputs"
        return a[:n]

    def kf_record(self, K, rec, k, T=None, tri=False):
        rec["kps"], rec["desc"] = self.up(k["kps"]).data_ptr(), self.up(k["desc"]).data_ptr()
        rec["n"] = len(k["desc"])
        T = BS.T_ID if T is None else T
        rec["Rcw"], rec["tcw"] = T[:3, :3].reshape(-1), T[:3, 3]
        rec["Ow"] = K.camera_center(T)
        if "ur" in k:
            rec["u_right"] = self.up(k["ur"]).data_ptr()
        if tri:
            rec["has_mp"] = self.up(k["mp"]).data_ptr()
            rec["nodes"] = self.up(k["fv"][0].astype(np.uint32)).data_ptr()
            rec["node_start"] = self.up(k["fv"][1].astype(np.int32)).data_ptr()
            rec["node_feats"] = self.up(k["fv"][2].astype(np.uint32)).data_ptr()
            rec["n_nodes"] = len(k["fv"][0])

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream


def _of(entry):
    return [c for c in KF_CASES if c.entry == entry]


def _groups(cases, key):
    out = {}
    for c in cases:
        out.setdefault(key(c), []).append(c)
    return list(out.values())


def test_batched_search_for_triangulation(K, refs):
    """All SearchForTriangulation cases as pairs of one launch per check_ori setting."""
    for cases in _groups(_of("tri"), lambda c: c.inp["check_ori"]):
        D = Dev()
        kfs = np.zeros(2 * len(cases), K.KF_DTYPE)
        pairs = np.zeros(len(cases), K.TRI_PAIR_DTYPE)
        for p, c in enumerate(cases):
            i = c.inp
            D.kf_record(K, kfs[2 * p], i["k1"], i["T1"], tri=True)
            D.kf_record(K, kfs[2 * p + 1], i["k2"], i["T2"], tri=True)
            pairs[p] = (2 * p, 2 * p + 1, np.asarray(i["F"], np.float32).reshape(-1),
                        int(i["only_stereo"]))
        cap = 64
        d_m, d_nm = D.out(len(cases) * cap), D.out(len(cases))
        K.search_for_triangulation_device(D.up(kfs), D.up(pairs), len(cases), BS.CAM, K.levels(),
                                          cases[0].inp["check_ori"], d_m, cap, d_nm, D.stream)
        m, nm = D.take(d_m, len(cases) * cap).reshape(-1, cap), D.take(d_nm, len(cases))
        for p, c in enumerate(cases):
            n1 = len(c.inp["k1"]["desc"])
            got = dict(n=int(nm[p]), match12=m[p, :n1])
            same(got, TB.ref_outputs(refs, c), c.id)
            TB.check_case(c, got)
            assert (m[p, n1:] == -9).all()


def test_batched_fuse(K, refs):
    """All Fuse cases of one window factor in one launch (d_point_kf names each point's keyframe)."""
    for cases in _groups(_of("fuse"), lambda c: c.inp["th"]):
        D = Dev()
        kfs = np.zeros(len(cases), K.KF_DTYPE)
        for p, c in enumerate(cases):
            D.kf_record(K, kfs[p], c.inp["kf"])
        pts = np.concatenate([c.inp["pts"] for c in cases])
        pkf = np.concatenate([np.full(len(c.inp["pts"]), p, np.int32)
                              for p, c in enumerate(cases)])
        d_bi, d_bd = D.out(len(pts)), D.out(len(pts))
        K.fuse_device(D.up(kfs), D.up(pts), D.up(pkf), len(pts), cases[0].inp["th"], BS.CAM,
                      K.levels(), K.kf_grid(BS.W, BS.H), d_bi, d_bd, D.stream)
        bi, bd = D.take(d_bi, len(pts)), D.take(d_bd, len(pts))
        o = 0
        for c in cases:
            m = len(c.inp["pts"])
            want = TB.ref_outputs(refs, c)
            got = dict(n=int((bi[o:o + m] >= 0).sum()), best_idx=bi[o:o + m], best_dist=bd[o:o + m])
            same(got, want, c.id)
            TB.check_case(c, got)
            o += m


def test_batched_fuse_sim3(K, refs):
    """All Fuse(pKF, Scw) cases of one window factor in one launch: every keyframe against the
    concatenated points of all cases (a case's own points are its slice of its keyframe's row)."""
    sc, _, _, lsf = TB.levels_arrays()
    for cases in _groups(_of("fuse_sim3"), lambda c: c.inp["th"]):
        D = Dev()
        kfs = np.zeros(len(cases), K.KF_DTYPE)
        for p, c in enumerate(cases):
            D.kf_record(K, kfs[p], c.inp["kf"])
        pts = np.concatenate([c.inp["pts"] for c in cases])
        n, th = len(pts), cases[0].inp["th"]
        d_bi, d_bd = D.out(len(cases) * n), D.out(len(cases) * n)
        K.fuse_sim3_device(D.up(kfs), len(cases), D.up(pts), n, None, th, BS.CAM, K.levels(),
                           K.kf_grid(BS.W, BS.H), d_bi, d_bd, D.stream)
        bi = D.take(d_bi, len(cases) * n).reshape(-1, n)
        bd = D.take(d_bd, len(cases) * n).reshape(-1, n)
        o = 0
        for p, c in enumerate(cases):
            _, bi_o, bd_o = refs["loop"].fuse_sim3(c.inp["kf"], refs["grid"], BS.I3, BS.Z3, BS.Z3,
                                                   BS.CAM, sc, lsf, pts, th)
            np.testing.assert_array_equal(bi[p], bi_o, err_msg=c.id)
            np.testing.assert_array_equal(bd[p], bd_o, err_msg=c.id)
            m = len(c.inp["pts"])
            TB.check_case(c, dict(best_idx=bi[p, o:o + m], best_dist=bd[p, o:o + m]))
            o += m


def test_batched_search_by_projection_sim3(K, refs):
    """All SearchByProjection(pKF, Scw) cases of one window factor as jobs of one launch."""
    for cases in _groups(_of("sbp_sim3"), lambda c: c.inp["th"]):
        D = Dev()
        kfs = np.zeros(len(cases), K.KF_DTYPE)
        jobs = np.zeros(len(cases), K.SBP_JOB_DTYPE)
        pb = kb = 0
        for p, c in enumerate(cases):
            D.kf_record(K, kfs[p], c.inp["kf"])
            jobs[p] = (p, pb, len(c.inp["pts"]), kb)
            pb += len(c.inp["pts"])
            kb += BS.N_KF
        pts = np.concatenate([c.inp["pts"] for c in cases])
        mi = np.concatenate([c.inp["matched_in"] for c in cases])
        sb = K.search_by_projection_sim3_scratch_bytes(len(pts))
        d_scr = D.torch.zeros(sb, dtype=D.torch.uint8, device=D.dev)
        d_kpp, d_pkp, d_nm = D.out(kb), D.out(len(pts)), D.out(len(cases))
        K.search_by_projection_sim3_device(
            D.up(kfs), D.up(pts), len(pts), D.up(jobs), len(cases),
            max(len(c.inp["pts"]) for c in cases), D.up(mi), kb, cases[0].inp["th"], BS.CAM,
            K.levels(), K.kf_grid(BS.W, BS.H), d_kpp, d_pkp, d_nm, d_scr, sb, D.stream)
        kpp, pkp, nm = D.take(d_kpp, kb), D.take(d_pkp, len(pts)), D.take(d_nm, len(cases))
        for p, c in enumerate(cases):
            j = jobs[p]
            got = dict(n=int(nm[p]), kp_point=kpp[j["kp_begin"]:j["kp_begin"] + BS.N_KF],
                       point_kp=pkp[j["pt_begin"]:j["pt_begin"] + j["n_pts"]])
            same(got, TB.ref_outputs(refs, c), c.id)
            TB.check_case(c, got)


def test_batched_search_by_sim3(K, refs):
    """All SearchBySim3 cases of one window factor as pairs of one launch."""
    for cases in _groups(_of("sim3"), lambda c: c.inp["th"]):
        D = Dev()
        kfs = np.zeros(2 * len(cases), K.KF_DTYPE)
        pairs = np.zeros(len(cases), K.SIM3_PAIR_DTYPE)
        stride = BS.N_KF + 6
        a1 = np.zeros((len(cases), stride), np.uint8)
        a2 = np.zeros((len(cases), stride), np.uint8)
        mps = []
        for p, c in enumerate(cases):
            i = c.inp
            D.kf_record(K, kfs[2 * p], i["k1"])
            D.kf_record(K, kfs[2 * p + 1], i["k2"])
            pairs[p] = (2 * p, 2 * p + 1, 2 * p * BS.N_KF, (2 * p + 1) * BS.N_KF,
                        BS.I3.reshape(-1), BS.Z3, BS.I3.reshape(-1), BS.Z3)
            a1[p, :BS.N_KF], a2[p, :BS.N_KF] = i["a1"], i["a2"]
            mps += [i["mp1"], i["mp2"]]
        mp = np.concatenate(mps)
        n = len(cases) * stride
        d_m, d_v1, d_v2, d_nf = D.out(n), D.out(n), D.out(n), D.out(len(cases))
        K.search_by_sim3_device(D.up(kfs), D.up(mp), len(mp), D.up(pairs), len(cases), D.up(a1),
                                D.up(a2), stride, cases[0].inp["th"], BS.CAM, K.levels(),
                                K.kf_grid(BS.W, BS.H), d_m, d_v1, d_v2, d_nf, D.stream)
        m, v1, v2 = (D.take(t, n).reshape(-1, stride) for t in (d_m, d_v1, d_v2))
        nf = D.take(d_nf, len(cases))
        for p, c in enumerate(cases):
            got = dict(n=int(nf[p]), match12=m[p, :BS.N_KF], vn1=v1[p, :BS.N_KF],
                       vn2=v2[p, :BS.N_KF])
            same(got, TB.ref_outputs(refs, c), c.id)
            TB.check_case(c, got)
            assert (m[p, BS.N_KF:] == -9).all()


# ---- the frame matchers -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(refs, gpu_lib):
    """The frame of the cases in a one-frame context, its keypoints asserted equal to the
    oracle's."""
    F = TB.frame(refs["oracle"])
    ctx = gpu_lib.Context(BS.FW, BS.FH, *BS.FRAME_ORB)
    ctx.frame_stereo(F["L"], F["R"], BS.FCAM)
    kl, dl = ctx.keypoints(0)
    assert kl.tobytes() == F["kl"].tobytes() and (dl == F["dl"]).all()
    ur, _ = ctx.stereo(0)
    assert ur.tobytes() == F["ur"].tobytes()
    assert BS.F2F_QUERY_DTYPE == gpu_lib.F2F_QUERY_DTYPE and BS.F2F_POSE_DTYPE == gpu_lib.F2F_POSE_DTYPE
    assert BS.MPS_QUERY_DTYPE == gpu_lib.MPS_QUERY_DTYPE
    assert BS.RELOC_QUERY_DTYPE == gpu_lib.RELOC_QUERY_DTYPE
    assert BS.RELOC_POSE_DTYPE == gpu_lib.RELOC_POSE_DTYPE
    assert BS.families(F["cases"]) == BS.listed(BS.FRAME_FAMILIES)      # no case is left out
    return F, ctx


def dev_frame_outputs(ctx, c):
    i = c.inp
    mp = i["mp0"].copy()
    blk = (mp >= 0).astype(np.uint8)
    if c.entry == "f2f":
        nm = ctx.search_by_projection_frame(0, i["q"], i["pose"], mp, blk)
    elif c.entry == "mps":
        nm = ctx.search_by_projection_mps(0, i["q"], i["nnratio"], int(i["th"]), mp, blk)
    else:
        nm = ctx.search_by_projection_reloc(0, i["q"], i["pose"], mp, blk)
    return dict(n=nm, map_point=mp)


@pytest.mark.parametrize("entry,family", sorted(BS.listed(BS.FRAME_FAMILIES)))
def test_frame_matcher_single_call(world, refs, entry, family):
    F, ctx = world
    cases = [c for c in F["cases"] if (c.entry, c.family) == (entry, family)]
    assert cases
    for c in cases:
        got = dev_frame_outputs(ctx, c)
        same(got, TB.ref_frame_outputs(refs, F, c), f"{c.id} ({c.cite})")
        TB.check_case(c, got)


@pytest.mark.parametrize("entry", ["f2f", "mps", "reloc"])
def test_batched_frame_matchers(world, refs, gpu_lib, entry):
    """All cases of the entry point in one launch of its _device form: one frame of the context
    per case (the same image in every frame), one query list per frame and, for the frame-to-frame
    and relocalisation searches, one pose per frame. The local-map form takes nnratio and th per
    launch: one launch per (nnratio, th) among its cases."""
    import ctypes as C
    import torch
    F, _ = world
    dev = torch.device("cuda", 0)
    all_cases = [c for c in F["cases"] if c.entry == entry]
    key = (lambda c: (c.inp["nnratio"], int(c.inp["th"]))) if entry == "mps" else (lambda c: 0)
    groups = _groups(all_cases, key)
    assert sum(len(g) for g in groups) == len(all_cases)
    ctx = gpu_lib.Context(BS.FW, BS.FH, *BS.FRAME_ORB, max_frames=max(len(g) for g in groups))
    n, kc = len(F["kl"]), ctx.kp_cap
    up = lambda a: torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    for cases in groups:
        nf = len(cases)
        d_l = torch.from_numpy(np.repeat(F["L"][None], nf, 0).copy()).to(dev)
        d_r = torch.from_numpy(np.repeat(F["R"][None], nf, 0).copy()).to(dev)
        ctx.frontend_device(d_l, d_r, BS.FH * BS.FW, BS.FW, nf, BS.FCAM)
        ctx.sync()
        for f in (0, nf - 1):
            assert ctx.keypoints(2 * f)[0].tobytes() == F["kl"].tobytes()
        q = np.concatenate([c.inp["q"] for c in cases])
        q_count = np.array([len(c.inp["q"]) for c in cases], np.int32)
        q_start = (np.cumsum(q_count) - q_count).astype(np.int32)
        mp_h = np.full((nf, kc), -1, np.int32)
        for f, c in enumerate(cases):
            mp_h[f, :n] = c.inp["mp0"]
        blk_h = (mp_h >= 0).astype(np.uint8)
        d_q = up(q)
        d_qs, d_qc = torch.from_numpy(q_start).to(dev), torch.from_numpy(q_count).to(dev)
        d_mp, d_blk = torch.from_numpy(mp_h).to(dev), torch.from_numpy(blk_h).to(dev)
        d_nm = torch.full((nf + 4,), -9, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        if entry == "mps":
            P = gpu_lib._ptr
            ctx.check(gpu_lib.lib().slamgpu_search_by_projection_mps_device(
                ctx.h, P(d_q), len(q), P(d_qs), P(d_qc), int(q_count.max()),
                float(cases[0].inp["nnratio"]), int(cases[0].inp["th"]), P(d_mp), P(d_blk), kc,
                P(d_nm), nf, C.c_void_p(st)))
        else:
            d_p = up(np.concatenate([c.inp["pose"] for c in cases]))
            call = ctx.search_by_projection_frame_device if entry == "f2f" else \
                ctx.search_by_projection_reloc_device
            call(d_q, len(q), d_qs, d_qc, int(q_count.max()), d_p, d_mp, d_blk, kc, d_nm, nf, st)
        torch.cuda.synchronize()
        ctx.sync()
        mp_g, nm_g = d_mp.cpu().numpy(), d_nm.cpu().numpy()
        assert (nm_g[nf:] == -9).all()
        for f, c in enumerate(cases):
            got = dict(n=int(nm_g[f]), map_point=mp_g[f, :n])
            same(got, TB.ref_frame_outputs(refs, F, c), c.id)
            TB.check_case(c, got)
            assert (mp_g[f, n:] == -1).all()
