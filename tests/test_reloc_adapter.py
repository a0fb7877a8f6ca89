"""The relocalisation chain on the device, Tracker::Relocalization's refinement of one candidate
(tracker.cpp:924-975): relocalization_refine of include/slamgpu_adapters.hpp driven from C++
(tests/reloc_adapter_check.cpp) on the frame the context holds, starting from a PnP inlier set.
The test follows the steps the program recorded: every search step is handed to the CPU
restatement (tests/relocmatch_ref.c) with the pose that step received and must agree bit for bit;
every PoseOptimization step is held to the oracle's at the same input by tests/tolerance.py
(outlier flags and the inlier count identical), as test_pose_gpu.py does; and the order of the
steps must be the tracker's for the counts the steps returned.

The scenario (model() below, on the CPU): frame 1 against keyframe 0 with 58 map points, 9 of
them displaced by about 6 px so that the (10, 100) search finds them and PoseOptimization rejects
them; 34 PnP inliers at a perturbed pose. Steps on the CPU model: PoseOptimization (nGood 32),
search (10, 100) (24 more), PoseOptimization (49), search (3, 64) (2 more), PoseOptimization
(49)."""
import os
import subprocess

import numpy as np
import pytest

import reloc_scenario as RS
from slam_framework_amd import slamgpu as G
from slam_framework_amd import synthetic as S
from tolerance import assert_close

CAM = S.KITTI_CAM
W, H = S.KITTI_COLS, S.KITTI_ROWS
N_POINTS, N_DISPLACED, N_INIT = 58, 9, 34


def scenario(oracle, ref):
    """Keyframe 0's map point table (index = keyframe keypoint), the frame's initial slots (the
    PnP inliers) and sFound, the start pose."""
    t, L, R, fr = RS.frames(oracle)
    sc = RS.scale_table(t)
    kf, f = fr[0], fr[1]
    q = RS.kf_queries(kf, 0, sc)
    grid = oracle.grid_geom(W, H)
    true_pose = RS.pose(1, 3.0, 64, 0, dw=(0, 0, 0), dt=(0, 0, 0))
    n = len(f["kl"])
    _, mp, qk, _, _ = ref.search_by_projection_reloc(f["kl"], f["dl"], grid, CAM, sc,
                                                     RS.log_scale_factor(), q, true_pose,
                                                     np.full(n, -1, np.int32))
    good = np.nonzero(qk >= 0)[0]                       # keyframe points with a (3, 64) match
    rng = np.random.default_rng(12)
    keep = np.sort(rng.choice(good, N_POINTS, replace=False))
    q["skip"] = 1
    q["skip"][keep] = 0
    init = keep[:N_INIT]
    init_mp = np.full(n, -1, np.int32)
    init_mp[qk[init]] = init
    rest = keep[N_INIT:]
    moved = rest[:N_DISPLACED]
    q["xyz"][moved] += (q["xyz"][moved, 2:3] * np.float32(6.0 / CAM[0]) *
                        np.array([1.0, -0.4, 0.0], np.float32))
    T0 = np.eye(4, dtype=np.float32)
    p0 = RS.pose(1, 10.0, 100, 1)
    T0[:3, :3], T0[:3, 3] = p0["Rcw"][0].reshape(3, 3), p0["tcw"][0]
    return dict(t=t, L=L, R=R, kf=kf, f=f, q=q, sc=sc, grid=grid, init_mp=init_mp,
                found=np.sort(init).astype(np.int32), T0=T0, isig=S.level_inv_sigma2())


def edges_of(f, q, mp):
    idx = np.nonzero(mp >= 0)[0]
    e = np.zeros(len(idx), G.POSE_EDGE_DTYPE)
    e["xw"] = q["xyz"][mp[idx]]
    e["u"], e["v"], e["ur"] = f["kl"]["x"][idx], f["kl"]["y"][idx], f["ur"][idx]
    e["octave"] = f["kl"]["octave"][idx]
    return e, idx


def search_queries(q, found):
    q2 = q.copy()
    q2["skip"][np.asarray(found, np.int64)] = 1
    return q2


def model(oracle, ref, sc):
    """tracker.cpp:924-975 on the CPU (oracle PoseOptimization + the restatement): the list of
    (kind, result) steps and nGood."""
    f, q = sc["f"], sc["q"]
    mp, T, found = sc["init_mp"].copy(), sc["T0"].copy(), list(sc["found"])
    steps = []

    def popt():
        nonlocal T
        e, idx = edges_of(f, q, mp)
        r, T, out, _ = oracle.pose_optimization(CAM, sc["isig"], e, T)
        steps.append(("pose", r))
        return r, idx[out]

    def search(th, od):
        nonlocal mp
        pose = G.reloc_pose(T, th, od, 1)
        nm, mp, _, _, _ = ref.search_by_projection_reloc(f["kl"], f["dl"], sc["grid"], CAM, sc["sc"],
                                                         RS.log_scale_factor(),
                                                         search_queries(q, found), pose, mp)
        steps.append(("search", nm))
        return nm
    n_good, bad = popt()
    if n_good < 10:
        return steps, n_good
    mp[bad] = -1
    if n_good < 50:
        nadd = search(10.0, 100)
        if nadd + n_good >= 50:
            n_good, bad = popt()
            if 30 < n_good < 50:
                found = [int(m) for m in mp[mp >= 0]]
                nadd = search(3.0, 64)
                if n_good + nadd >= 50:
                    n_good, bad = popt()
                    mp[bad] = -1
    return steps, n_good


def expected_kinds(results):
    """The tracker's control flow replayed on the results the steps returned."""
    kinds = ["pose"]
    n_good = results[0]
    if n_good < 10 or n_good >= 50:
        return kinds
    kinds.append("search")
    if results[1] + n_good >= 50:
        kinds.append("pose")
        n_good = results[2]
        if 30 < n_good < 50:
            kinds.append("search")
            if n_good + results[3] >= 50:
                kinds.append("pose")
    return kinds


def test_scenario_reaches_both_searches(oracle):
    """CPU: the scenario drives the chain through both search stages (the device run is then
    followed step by step, whatever it does)."""
    import relocmatch_ref as ref
    steps, n_good = model(oracle, ref, scenario(oracle, ref))
    kinds = [k for k, _ in steps]
    assert kinds == ["pose", "search", "pose", "search", "pose"], steps
    assert [r for _, r in steps] == [32, 24, 49, 2, 49] and n_good == 49


@pytest.mark.gpu
def test_relocalization_refine_follows_the_restatement(oracle, gpu_lib, tmp_path):
    import relocmatch_ref as ref
    from slam_framework_amd import build
    exe = build.build_reloc_adapter_check()
    sc = scenario(oracle, ref)
    f, q, kf = sc["f"], sc["q"], sc["kf"]
    n, nk = len(f["kl"]), len(kf["kl"])
    d = str(tmp_path)
    for name, a in (("left.u8", sc["L"][1]), ("right.u8", sc["R"][1]),
                    ("kf_kps.bin", np.ascontiguousarray(kf["kl"])),
                    ("queries.bin", np.ascontiguousarray(q)),
                    ("init_mp.i32", sc["init_mp"]), ("found.i32", sc["found"]),
                    ("Tcw0.f32", sc["T0"]), ("inv_sigma2.f32", sc["isig"].astype(np.float32))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    r = subprocess.run([exe, d, str(W), str(H), str(nk)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    head = r.stdout.split()
    assert head[0] == "nkps" and int(head[1]) == n, r.stdout
    n_good_dev, n_steps = int(head[3]), int(head[5])
    rec = np.dtype([("kind", "<i4"), ("result", "<i4"), ("Tcw_in", "<f4", (16,)),
                    ("Tcw_out", "<f4", (16,)), ("pose", G.RELOC_POSE_DTYPE), ("n_found", "<i4"),
                    ("found", "<i4", (nk,)), ("mp_in", "<i4", (n,)), ("mp_out", "<i4", (n,)),
                    ("outlier", "u1", (n,))])
    tr = np.fromfile(os.path.join(d, "trace.bin"), rec)
    assert len(tr) == n_steps
    kinds = ["pose" if s["kind"] == 0 else "search" for s in tr]
    assert kinds == expected_kinds([int(s["result"]) for s in tr])
    assert kinds[:4] == ["pose", "search", "pose", "search"]
    mp, found, T = sc["init_mp"].copy(), list(sc["found"]), sc["T0"].copy()
    outlier = np.zeros(n, np.uint8)
    n_good = 0
    for k, s in enumerate(tr):
        np.testing.assert_array_equal(s["mp_in"], mp)
        assert s["Tcw_in"].tobytes() == T.tobytes()
        if s["kind"] == 0:
            e, idx = edges_of(f, q, mp)
            r_o, T_o, out_o, _ = oracle.pose_optimization(CAM, sc["isig"], e, T)
            assert int(s["result"]) == r_o
            outlier[idx] = out_o
            np.testing.assert_array_equal(s["outlier"], outlier)
            assert_close(s["Tcw_out"].reshape(4, 4), T_o, T, f"step {k} pose")
            np.testing.assert_array_equal(s["mp_out"], mp)
            T = s["Tcw_out"].reshape(4, 4).copy()          # follow the device's pose
            n_good = r_o
            if k == 0 or k == 4:
                mp[outlier != 0] = -1                       # :930-934, :966-970
        else:
            if k == 3:
                found = [int(m) for m in mp[mp >= 0]]       # :950-955
            assert sorted(s["found"][:s["n_found"]]) == sorted(found)
            th, od = (10.0, 100) if k == 1 else (3.0, 64)
            pose = s["pose"].reshape(1)
            assert (float(pose["th"][0]), int(pose["orb_dist"][0]), int(pose["check_ori"][0])) == \
                (th, od, 1)
            assert pose["Rcw"][0].tobytes() == T[:3, :3].tobytes()
            assert pose["tcw"][0].tobytes() == T[:3, 3].tobytes()
            assert pose["Ow"][0].tobytes() == G.reloc_pose(T, th, od, 1)["Ow"][0].tobytes()
            nm, mp_r, _, _, _ = ref.search_by_projection_reloc(
                f["kl"], f["dl"], sc["grid"], CAM, sc["sc"], RS.log_scale_factor(),
                search_queries(q, found), pose, mp)
            assert int(s["result"]) == nm
            np.testing.assert_array_equal(s["mp_out"], mp_r)
            assert s["Tcw_out"].tobytes() == T.tobytes()
            mp = mp_r
    assert n_good_dev == n_good
