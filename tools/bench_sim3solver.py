"""Device time of the RANSAC Sim3 solver (include/slamgpu_sim3solver.h) against the CPU restatement
(tests/sim3solver_ref.c, checked bit for bit against the device output in the same run).

  python tools/bench_sim3solver.py [--iters 200] [--warmup 20] [--repeats 5] [--out FILE]

Workload (an ASSUMPTION, not a recorded loop closure: there is no real loop-closure data here):
the tests' synthetic candidate (tests/sim3solver_scenario.py), N = 100 correspondences, the full
300-iteration schedule, min_inliers 20, fixed scale.
  one      one job in one slamgpu_sim3_ransac_device call (both kernels)
  eight    eight such jobs in one call
  sync     slamgpu_sim3_ransac end to end: staging, upload, both kernels, download, synchronise
  cpu      the same schedule through the restatement on one thread at the oracle's CFLAGS. It
           does no cv::Mat allocation per point, so it UNDERSTATES the reference's own cost.
Device times are hipEvent intervals around `iters` back-to-back calls after `warmup` calls,
divided by iters; each figure is the median of `repeats` such windows, with the spread (min, max)
beside it. `sync` and `cpu` are host clocks (the synchronous call ends in a synchronise). One JSON
line each; --out also writes them to a file.
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

N, ITS, MIN_INLIERS = 100, 300, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sim3solver_ref as ref
    import sim3solver_scenario as S
    from slam_framework_amd import build, slamgpu as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_sim3solver needs the GPU: no device found")
    build.build()
    G.lib()
    ref.lib()
    dev = torch.device("cuda", 0)
    cands = [S.candidate(500 + j, N, True) for j in range(8)]
    draws = [S.draws(900 + j, N, ITS) for j in range(8)]
    K, s2 = cands[0]["K"], cands[0]["sigma2"]

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    def batch(nj):
        jobs = np.zeros(nj, G.SIM3_RANSAC_JOB_DTYPE)
        for j in range(nj):
            jobs[j] = (j * N, N, j * 3 * ITS, ITS, MIN_INLIERS, 1)
        d = dict(m=up(np.concatenate([c["matches"] for c in cands[:nj]])),
                 d=up(np.concatenate([x.reshape(-1) for x in draws[:nj]])), j=up(jobs),
                 hyp=torch.zeros(nj * ITS * 64, dtype=torch.uint8, device=dev),
                 bits=torch.zeros(nj * ITS * 2, dtype=torch.int64, device=dev),
                 ev=torch.zeros(nj * ITS, dtype=torch.int32, device=dev),
                 ne=torch.zeros(nj, dtype=torch.int32, device=dev))

        def run():
            G.sim3_ransac_device(K, K, s2, s2, d["m"], nj * N, d["d"], nj * 3 * ITS, d["j"], nj, N,
                                 ITS, d["hyp"], d["bits"], d["ev"], d["ne"],
                                 stream=torch.cuda.current_stream().cuda_stream)
        return run, d

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def device_ms(fn):
        for _ in range(a.warmup):
            fn()
        return sorted(window(fn) for _ in range(a.repeats))

    def host_ms(fn, iters):
        out = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            out.append((time.perf_counter() - t0) * 1e3 / iters)
        return sorted(out)

    cmd = "python tools/bench_sim3solver.py " + " ".join(sys.argv[1:])
    lines = []

    def report(leg, ms, **kw):
        rec = {"bench": "sim3solver", "leg": leg, "ms": round(ms[len(ms) // 2], 5),
               "ms_min": round(ms[0], 5), "ms_max": round(ms[-1], 5), "n": N, "iterations": ITS,
               "workload": "assumed (synthetic candidate)", **kw, "cmd": cmd.strip()}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # the reference of the run: the restatement, also the CPU leg
    want = [ref.ransac(c["matches"], d, ITS, MIN_INLIERS, True, K, K, s2, s2)
            for c, d in zip(cands, draws)]
    run1, d1 = batch(1)
    run8, d8 = batch(8)
    run8()
    torch.cuda.synchronize()
    hyp = d8["hyp"].cpu().numpy().view(G.SIM3_HYP_DTYPE).reshape(8, ITS)
    bits = d8["bits"].cpu().numpy().view(np.uint64).reshape(8, ITS, 2)
    ne = d8["ne"].cpu().numpy()
    for j in range(8):
        wh, wb, we, wne = want[j]
        same = all(np.array_equal(hyp[j][f].view(np.uint32), wh[f].view(np.uint32))
                   for f in ("R12", "t12", "s12", "n_inliers"))
        if not (same and np.array_equal(bits[j], wb) and ne[j] == wne):
            raise SystemExit(f"job {j}: the device differs from the restatement")
    events = [int(x) for x in ne]

    one = device_ms(run1)
    eight = device_ms(run8)
    report("one", one, jobs=1, events=events[:1])
    report("eight", eight, jobs=8, events=events, ms_per_job=round(eight[len(eight) // 2] / 8, 5))
    m0, dr0 = cands[0]["matches"], draws[0]
    G.sim3_ransac(m0, dr0, ITS, MIN_INLIERS, True, K, K, s2, s2)
    report("sync", host_ms(lambda: G.sim3_ransac(m0, dr0, ITS, MIN_INLIERS, True, K, K, s2, s2),
                           max(a.iters // 4, 1)), jobs=1, clock="host")
    report("cpu", host_ms(lambda: ref.ransac(m0, dr0, ITS, MIN_INLIERS, True, K, K, s2, s2), 5),
           jobs=1, clock="host", note="restatement, one thread, oracle CFLAGS; no cv::Mat "
           "allocation per point: understates the reference's own cost")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
