"""Device time of the relocalisation matcher, SearchByProjection(CurrentFrame, pKF, sAlreadyFound,
th, ORBdist) (slamgpu_search_by_projection_reloc_device), against its CPU restatement
(tests/relocmatch_ref.c) on one thread, checked against the device output bit for bit in the same
run.

  python tools/bench_relocmatch.py [--iters 200] [--windows 7] [--warmup 20] [--out FILE]

Workload (an ASSUMPTION, not a recorded relocalisation): KITTI-size frames (1241 x 376, 2000
features) of the synthetic three-frame sequence; the candidate keyframe is the frame before, with
a map point on every second keypoint (stereo depth where there is one, 12 m otherwise: about
1000 points), 20 % of the frame's slots occupied at entry, the frame at a perturbed pose, the
rotation check on. Legs:
  single_10_100 / single_3_64   one frame, the tracker's two stages (th, ORBdist)
  batch8_10_100 / batch8_3_64   the same over 8 frames in one call (frames 1, 2, 1, 2, ...)
Device times are hipEvent intervals around `iters` back-to-back calls, per call, one interval per
window; the figure is the median over the windows (min and max beside it). Every timed call is
preceded by the device-to-device reset of its in/out rows (map_point, blocked), which is inside
the interval. CPU times are the median of 5 single calls of the -O2 restatement per frame, summed
over the frames of the leg. Writes profiles/relocmatch_bench.json and prints one JSON line per
leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, PITCH = 1241, 376, 1280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocmatch_bench.json"))
    a = ap.parse_args()
    import torch
    import oracle_lib as O
    import reloc_scenario as RS
    import relocmatch_ref as ref
    from slam_framework_amd import build, slamgpu as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_relocmatch needs the GPU: no device found")
    build.build()
    O.build()
    dev = torch.device("cuda", 0)
    t, L, R, fr = RS.frames(O)
    sc, lsf, grid = RS.scale_table(t), RS.log_scale_factor(), O.grid_geom(W, H)
    B = 8
    cur_of = [1 + f % 2 for f in range(B)]
    hl, hr = np.zeros((B, H, PITCH), np.uint8), np.zeros((B, H, PITCH), np.uint8)
    for f, c in enumerate(cur_of):
        hl[f, :, :W], hr[f, :, :W] = L[c], R[c]
    ctx = G.Context(W, H, max_frames=B)
    kc = ctx.kp_cap
    d_l, d_r = torch.from_numpy(hl).to(dev), torch.from_numpy(hr).to(dev)
    ctx.frontend_device(d_l, d_r, H * PITCH, PITCH, B, RS.CAM)
    ctx.sync()

    def queries(cur):
        kf = dict(fr[cur - 1])
        kf["depth"] = np.where(kf["depth"] > 0, kf["depth"], np.float32(12.0)).astype(np.float32)
        q = RS.kf_queries(kf, cur - 1, sc)
        q["skip"][1::2] = 1
        return q
    qs = [queries(c) for c in cur_of]
    n = [len(fr[c]["kl"]) for c in cur_of]
    mp0 = [RS.occupied(n[f], 0.2, 30 + f) for f in range(B)]
    q_count = np.array([len(q) for q in qs], np.int32)
    q_start = np.concatenate([[0], np.cumsum(q_count)[:-1]]).astype(np.int32)
    qall = np.concatenate(qs)
    mp_h, blk_h = np.full((B, kc), -1, np.int32), np.zeros((B, kc), np.uint8)
    for f in range(B):
        mp_h[f, :n[f]] = mp0[f]
        blk_h[f, :n[f]] = mp0[f] >= 0
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_q, d_qs, d_qc = up(qall), up(q_start), up(q_count)
    d_mp0, d_blk0 = torch.from_numpy(mp_h).to(dev), torch.from_numpy(blk_h).to(dev)
    d_mp, d_blk = d_mp0.clone(), d_blk0.clone()
    d_nm = torch.zeros(B, dtype=torch.int32, device=dev)
    # a stream of its own: a null stream argument would mean the context's stream, which the
    # events and the resets below (issued through torch) are not on
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    cmd = "python tools/bench_relocmatch.py " + " ".join(sys.argv[1:])
    legs = []
    for name, nf, th, od in (("single_10_100", 1, 10.0, 100), ("single_3_64", 1, 3.0, 64),
                             ("batch8_10_100", B, 10.0, 100), ("batch8_3_64", B, 3.0, 64)):
        poses = np.concatenate([RS.pose(cur_of[f], th, od, 1) for f in range(nf)])
        d_p = up(poses)
        total = int(q_start[nf - 1] + q_count[nf - 1])

        def call():
            d_mp[:nf].copy_(d_mp0[:nf])
            d_blk[:nf].copy_(d_blk0[:nf])
            ctx.search_by_projection_reloc_device(d_q, total, d_qs, d_qc, int(q_count[:nf].max()),
                                                  d_p, d_mp, d_blk, kc, d_nm, nf, st)
        per_call = []
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                call()
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                for _ in range(a.iters):
                    call()
                e1.record(stream)
                stream.synchronize()
                per_call.append(e0.elapsed_time(e1) / a.iters)
        ctx.sync()
        mp_g, nm_g = d_mp.cpu().numpy(), d_nm.cpu().numpy()
        same, cpu_ms, nmatches, passed, points = True, 0.0, [], 0, 0
        for f in range(nf):
            c = fr[cur_of[f]]
            runs = []
            for _ in range(5):
                t0 = time.perf_counter()
                nm_o, mp_o, _, po, _ = ref.search_by_projection_reloc(c["kl"], c["dl"], grid, RS.CAM,
                                                                      sc, lsf, qs[f],
                                                                      poses[f:f + 1], mp0[f])
                runs.append((time.perf_counter() - t0) * 1e3)
            cpu_ms += float(np.median(runs))
            same = same and int(nm_g[f]) == nm_o and np.array_equal(mp_g[f, :n[f]], mp_o)
            nmatches.append(int(nm_o))
            passed += int((po > 0).sum())
            points += int((qs[f]["skip"] == 0).sum())
        leg = {"leg": name, "frames": nf, "th": th, "orb_dist": od, "keyframe_points": points,
               "nmatches": nmatches, "queries_passing_over_a_claim": passed,
               "device_ms_median": round(float(np.median(per_call)), 4),
               "device_ms_min": round(min(per_call), 4), "device_ms_max": round(max(per_call), 4),
               "windows": a.windows, "iters_per_window": a.iters,
               "cpu_restatement_ms": round(cpu_ms, 3), "matches_restatement": bool(same),
               "workload": "assumed (synthetic sequence, a point on every second keyframe keypoint)",
               "cmd": cmd}
        print(json.dumps(leg))
        legs.append(leg)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_relocmatch.py", "legs": legs}, f, indent=1)
        f.write("\n")
    if not all(leg["matches_restatement"] for leg in legs):
        raise SystemExit("device output differs from the restatement")


if __name__ == "__main__":
    main()
