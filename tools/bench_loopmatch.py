"""Device time of the LoopCloser's three Sim3 matchers (include/slamgpu_loopmatch.h) on the
kf_scenario keyframes, against the CPU restatement (tests/loopmatch_ref.c, checked against the
device output in the same run) and, for the Fuse batch, against slamgpu_fuse_device on the same
(keyframe, point) products.

  python tools/bench_loopmatch.py [--iters 50] [--warmup 5] [--kfs 30]

Workload (an assumption, not a recorded loop closure): ~4000 map points = one point per feature
of the two keyframes (stereo depth where there is one, 12 m otherwise), distinct descriptors.
  sbp      one SearchByProjection(pKF, Scw, ...) job of all points, th = 10, 20 % of the keypoints
           matched at entry
  fuse     SearchAndFuse-shaped: --kfs keyframes (the two keyframes at poses a fraction of a
           degree apart) x the shared points, th = 4
  sim3     3 SearchBySim3 pairs, th = 7.5
Device times are hipEvent intervals around `iters` back-to-back calls after `warmup` calls,
divided by iters; CPU times are one call of the -O2 restatement on one core. One JSON line each.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1241, 376


def all_points(K, KS, kf, T, default_depth=12.0):
    """One FUSE_POINT record per feature of kf at pose T."""
    fx, fy, cx, cy, _ = KS.CAM
    sc = KS.levels_arrays()[0]
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Ow = KS.center(T).astype(np.float64)
    rec = np.zeros(len(kf["desc"]), K.FUSE_POINT_DTYPE)
    z = np.where(kf["depth"] > 0, kf["depth"], default_depth).astype(np.float64)
    Xc = np.stack([(kf["kps"]["x"] - cx) * z / fx, (kf["kps"]["y"] - cy) * z / fy, z], 1)
    Xw = (Xc - t) @ R
    d = np.linalg.norm(Xw - Ow, axis=1)
    rec["xyz"], rec["normal"] = Xw, (Xw - Ow) / d[:, None]
    rec["max_dist"] = d * sc[kf["kps"]["octave"]]
    rec["min_dist"] = rec["max_dist"] / sc[-1]
    rec["desc"] = kf["desc"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kfs", type=int, default=30)
    a = ap.parse_args()
    import torch
    import kf_scenario as KS
    import loop_scenario as LS
    import loopmatch_ref as ref
    import oracle_lib as O
    from slam_framework_amd import build, kfmatch as K
    if not torch.cuda.is_available():
        raise SystemExit("bench_loopmatch needs the GPU: no device found")
    build.build()
    O.build()
    dev = torch.device("cuda", 0)
    scene, _ = KS.keyframes(O)
    lv, grid, grid_o, lva = K.levels(), K.kf_grid(W, H), O.grid_geom(W, H), KS.levels_arrays()
    T = [KS.pose(0), KS.pose(1)]
    pts = np.concatenate([all_points(K, KS, scene[0], T[0]), all_points(K, KS, scene[1], T[1])])
    n_pts = len(pts)
    keep = []

    def up(x):
        t = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
        keep.append(t)
        return t

    d_arr = [(up(k["kps"]), up(k["desc"]), up(k["ur"])) for k in scene]

    def kf_records(frames):
        rec = np.zeros(len(frames), K.KF_DTYPE)
        for i, (q, R, t, Ow) in enumerate(frames):
            rec[i]["kps"], rec[i]["desc"], rec[i]["u_right"] = (x.data_ptr() for x in d_arr[q])
            rec[i]["n"] = len(scene[q]["desc"])
            rec[i]["Rcw"], rec[i]["tcw"], rec[i]["Ow"] = np.reshape(R, -1), t, Ow
        return rec

    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    cmd = "python tools/bench_loopmatch.py " + " ".join(sys.argv[1:])
    d_pts = up(pts)

    # ---- sbp: one job ------------------------------------------------------------------------
    b1 = K.decompose_scw(LS.scw(T[1], 1.0))
    d_kf = up(kf_records([(1, *b1)]))
    n1 = len(scene[1]["desc"])
    mi = LS.flags(n1, 0.2, 11)
    job = np.zeros(1, K.SBP_JOB_DTYPE)
    job[0] = (0, 0, n_pts, 0)
    sb = K.search_by_projection_sim3_scratch_bytes(n_pts)
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    d_kpp = torch.zeros(n1, dtype=torch.int32, device=dev)
    d_pkp = torch.zeros(n_pts, dtype=torch.int32, device=dev)
    d_nm = torch.zeros(1, dtype=torch.int32, device=dev)
    d_job, d_mi = up(job), up(mi)
    ms = timed(lambda: K.search_by_projection_sim3_device(
        d_kf, d_pts, n_pts, d_job, 1, n_pts, d_mi, n1, 10.0, KS.CAM, lv, grid, d_kpp, d_pkp, d_nm,
        d_scr, sb, st))
    t0 = time.perf_counter()
    nm_o, kpp_o, pkp_o, po = ref.search_by_projection_sim3(scene[1], grid_o, *b1, KS.CAM, lva[0],
                                                           lva[3], pts, mi, 10.0)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    same = bool(int(d_nm.item()) == nm_o and np.array_equal(d_kpp.cpu().numpy(), kpp_o)
                and np.array_equal(d_pkp.cpu().numpy(), pkp_o))
    print(json.dumps({"leg": "sbp", "n_pts": n_pts, "n_kps": n1, "nmatches": nm_o,
                      "points_passing_over_a_claim": int((po > 0).sum()),
                      "device_ms": round(ms, 4), "cpu_restatement_ms": round(cpu_ms, 3),
                      "matches_restatement": same, "cmd": cmd}))

    # ---- fuse: kfs keyframes x shared points --------------------------------------------------
    frames = []
    for q in range(a.kfs):
        Tq = KS.pose(q % 2, (0.002 * q, -0.001 * q, 0.0))
        frames.append((q % 2, *K.decompose_scw(LS.scw(Tq, 1.0 + 0.01 * (q % 5)))))
    d_kfs = up(kf_records(frames))
    d_bi = torch.zeros(a.kfs * n_pts, dtype=torch.int32, device=dev)
    d_bd = torch.zeros(a.kfs * n_pts, dtype=torch.int32, device=dev)
    ms = timed(lambda: K.fuse_sim3_device(d_kfs, a.kfs, d_pts, n_pts, None, 4.0, KS.CAM, lv, grid,
                                          d_bi, d_bd, st))
    bi = d_bi.cpu().numpy().reshape(a.kfs, n_pts)
    bd = d_bd.cpu().numpy().reshape(a.kfs, n_pts)
    t0 = time.perf_counter()
    same, nfused = True, 0
    for q, (f, R, t, Ow) in enumerate(frames):
        nf, bi_o, bd_o = ref.fuse_sim3(scene[f], grid_o, R, t, Ow, KS.CAM, lva[0], lva[3], pts, 4.0)
        same = same and np.array_equal(bi[q], bi_o) and np.array_equal(bd[q], bd_o)
        nfused += nf
    cpu_ms = (time.perf_counter() - t0) * 1e3
    # the plain Fuse of the parent on the same products: the records replicated per keyframe
    d_rep = up(np.tile(pts, a.kfs))
    d_pkf = up(np.repeat(np.arange(a.kfs, dtype=np.int32), n_pts))
    d_bi2, d_bd2 = torch.zeros_like(d_bi), torch.zeros_like(d_bd)
    ms_plain = timed(lambda: K.fuse_device(d_kfs, d_rep, d_pkf, a.kfs * n_pts, 4.0, KS.CAM, lv,
                                           grid, d_bi2, d_bd2, st))
    print(json.dumps({"leg": "fuse", "n_kfs": a.kfs, "n_pts": n_pts, "nfused": nfused,
                      "device_ms": round(ms, 4),
                      "ns_per_kf_point": round(ms * 1e6 / (a.kfs * n_pts), 2),
                      "plain_fuse_device_ms": round(ms_plain, 4),
                      "plain_ns_per_kf_point": round(ms_plain * 1e6 / (a.kfs * n_pts), 2),
                      "cpu_restatement_ms": round(cpu_ms, 3), "matches_restatement": bool(same),
                      "cmd": cmd}))

    # ---- sim3: 3 pairs -----------------------------------------------------------------------
    d_kf2 = up(kf_records([(q, T[q][:3, :3], T[q][:3, 3], K.camera_center(T[q])) for q in (0, 1)]))
    mp = [LS.mp_records(scene[q], T[q]) for q in (0, 1)]
    n = [len(mp[0]), len(mp[1])]
    begin = [0, n[0]]
    plist = [(0, 1, (1.0, 0.0)), (1, 0, (1.0, 0.0)), (0, 1, (1.05, 0.2))]
    stride = max(n)
    pairs = np.zeros(3, K.SIM3_PAIR_DTYPE)
    a1, a2 = np.zeros((3, stride), np.uint8), np.zeros((3, stride), np.uint8)
    sims = []
    for p, (i, j, pert) in enumerate(plist):
        s = K.relative_sim3(*LS.relative_pose(T[i], T[j], *pert))
        sims.append(s)
        pairs[p] = (i, j, begin[i], begin[j], s[0].reshape(-1), s[1], s[2].reshape(-1), s[3])
        a1[p, :n[i]], a2[p, :n[j]] = LS.flags(n[i], 0.15, 60 + p), LS.flags(n[j], 0.15, 70 + p)
    d_m, d_v1, d_v2 = (torch.zeros(3 * stride, dtype=torch.int32, device=dev) for _ in range(3))
    d_nf = torch.zeros(3, dtype=torch.int32, device=dev)
    d_mp, d_pairs, d_a1, d_a2 = up(np.concatenate(mp)), up(pairs), up(a1), up(a2)
    ms = timed(lambda: K.search_by_sim3_device(d_kf2, d_mp, n[0] + n[1], d_pairs, 3, d_a1, d_a2,
                                               stride, 7.5, KS.CAM, lv, grid, d_m, d_v1, d_v2,
                                               d_nf, st))
    m, nf = d_m.cpu().numpy(), d_nf.cpu().numpy()
    t0 = time.perf_counter()
    same, found = True, []
    for p, (i, j, _) in enumerate(plist):
        nf_o, m_o, _, _ = ref.search_by_sim3(scene[i], scene[j], grid_o, T[i], T[j], mp[i], mp[j],
                                             a1[p, :n[i]], a2[p, :n[j]], *sims[p], KS.CAM, lva[0],
                                             lva[3], 7.5)
        same = same and nf[p] == nf_o and np.array_equal(m[p * stride:p * stride + n[i]], m_o)
        found.append(int(nf_o))
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"leg": "sim3", "pairs": 3, "n_features": n, "nfound": found,
                      "device_ms": round(ms, 4), "cpu_restatement_ms": round(cpu_ms, 3),
                      "matches_restatement": bool(same), "cmd": cmd}))


if __name__ == "__main__":
    main()
