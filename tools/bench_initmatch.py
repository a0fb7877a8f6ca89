"""Device time of OrbMatcher::SearchForInitialization (slamgpu_search_for_initialization and its
_device form) against its CPU restatement (tests/initmatch_ref.c) on one thread, checked against
the device output bit for bit in the same run.

  python tools/bench_initmatch.py [--iters 100] [--windows 5] [--warmup 10] [--out FILE]

Workload: the tracker's call on the synthetic sequence (KITTI-size frames, 1241 x 376), F1 = frame
0 with all its keypoints as queries and vbPrevMatched = their positions, F2 = frame 1 made by
slamgpu_frame_mono, windowSize 100, nnratio 0.9, orientation check on; at 2000 and 4000 features.
Per shape:
  host_call_ms      wall time of the synchronous call (staging, both kernels, read-back), median
  device_ms_*       hipEvent interval around `iters` back-to-back _device calls, per call, one
                    interval per window (each call preceded by the device-to-device reset of
                    vbPrevMatched, inside the interval): median, min and max over the windows
  search_cand_ms / init_resolve_ms   the two kernels alone, through slamgpu_timing_* (events
                    around every launch), per call
  cpu_restatement_ms  median of 5 single calls of the -O2 restatement
Writes profiles/initmatch_bench.json and prints one JSON line per shape."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initmatch_bench.json"))
    a = ap.parse_args()
    import torch
    import oracle_lib as O
    import initmatch_ref as ref
    from slam_framework_amd import build, slamgpu as G, synthetic as S
    if not torch.cuda.is_available():
        raise SystemExit("bench_initmatch needs the GPU: no device found")
    build.build()
    O.build()
    dev = torch.device("cuda", 0)
    L, _ = S.sequence(2000, 2)
    grid = O.grid_geom(W, H)
    cmd = "python tools/bench_initmatch.py " + " ".join(sys.argv[1:])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    legs = []
    for nf in (2000, 4000):
        ctx = G.Context(W, H, nfeatures=nf)
        k1, d1 = ctx.extract(L[0])
        ctx.frame_mono(L[1], S.KITTI_CAM)
        k2, d2 = (x.copy() for x in ctx.keypoints(0))
        q = G.init_queries(k1, d1)
        prev0 = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32)
        prm = G.init_search(0.9, 100, 1)
        n1 = len(q)
        # the synchronous call
        host = []
        for i in range(a.warmup + 30):
            p = prev0.copy()
            t0 = time.perf_counter()
            nm_h, m12_h = ctx.search_for_initialization(0, q, prm, p)
            if i >= a.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
        prev_h = p
        # the device form
        d_q, d_p = up(q), up(prm)
        d_qs, d_qc = up(np.zeros(1, np.int32)), up(np.array([n1], np.int32))
        d_prev0 = torch.from_numpy(prev0).to(dev)
        d_prev = d_prev0.clone()
        d_m12 = torch.full((n1,), -7, dtype=torch.int32, device=dev)
        d_nm = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        st = stream.cuda_stream

        def call():
            d_prev.copy_(d_prev0)
            ctx.search_for_initialization_device(d_q, n1, d_qs, d_qc, n1, d_p, d_prev, d_m12, d_nm,
                                                 1, st)
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
            # the two kernels alone
            k_iters = 50
            ctx.timing_start("*", 4 * k_iters)
            for _ in range(k_iters):
                call()
            ctx.timing_stop(st)
        cand_ms, n_cand = ctx.timing_read("search_cand")
        res_ms, n_res = ctx.timing_read("init_resolve")
        ctx.sync()
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = ref.search_for_initialization(k2, d2, grid, q, 0.9, 100, 1, prev0)
            runs.append((time.perf_counter() - t0) * 1e3)
        same = (int(d_nm.cpu()[0]) == r[0] == nm_h and np.array_equal(d_m12.cpu().numpy(), r[1])
                and np.array_equal(m12_h, r[1]) and d_prev.cpu().numpy().tobytes() == r[2].tobytes()
                and prev_h.tobytes() == r[2].tobytes())
        leg = {"nfeatures": nf, "n1": n1, "level0_queries": int((q["octave"] == 0).sum()),
               "n2": len(k2), "window_size": 100, "nnratio": 0.9, "check_ori": 1,
               "nmatches": int(r[0]), **r[4],
               "host_call_ms": round(float(np.median(host)), 4),
               "device_ms_median": round(float(np.median(per_call)), 4),
               "device_ms_min": round(min(per_call), 4), "device_ms_max": round(max(per_call), 4),
               "windows": a.windows, "iters_per_window": a.iters,
               "search_cand_ms": round(cand_ms / max(n_cand, 1), 4),
               "init_resolve_ms": round(res_ms / max(n_res, 1), 4),
               "kernel_launches_timed": [n_cand, n_res],
               "cpu_restatement_ms": round(float(np.median(runs)), 3),
               "matches_restatement": bool(same), "cmd": cmd}
        print(json.dumps(leg))
        legs.append(leg)
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_initmatch.py", "legs": legs}, f, indent=1)
        f.write("\n")
    if not all(leg["matches_restatement"] for leg in legs):
        raise SystemExit("device output differs from the restatement")


if __name__ == "__main__":
    main()
