"""Device time of the RANSAC EPnP solver (include/slamgpu_pnpsolver.h) against the CPU restatement
(tests/pnpsolver_ref.c, checked bit for bit against the device output in the same run).

  python tools/bench_pnpsolver.py [--iters 50] [--warmup 5] [--repeats 5] [--out FILE]

Workloads (ASSUMPTIONS, not a recorded relocalisation: there is no real lost-tracking data here),
on the tests' synthetic scenes (tests/pnpsolver_model.py, 0.5 px noise, 40 % outliers):
  reloc    5 candidates x 60 correspondences x 35 iterations, min_inliers 30: what the tracker's
           SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) gives at N = 60
  large    N = 500 x 300 iterations, min_inliers 20
Legs, per workload:
  one      one job in one slamgpu_pnp_ransac_device call (all three kernels)
  batch    five such jobs in one call
  sync     slamgpu_pnp_ransac end to end: staging, upload, the kernels, download, synchronise
  cpu      the same schedule through the restatement on one thread at the oracle's CFLAGS. It
           has no OpenCV allocation per solve, so it UNDERSTATES the reference's own cost.
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

WORKLOADS = {"reloc": (60, 35, 30), "large": (500, 300, 20)}  # N, iterations, min_inliers
JOBS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pnpsolver_model as M
    import pnpsolver_ref as ref
    from slam_framework_amd import build, slamgpu as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_pnpsolver needs the GPU: no device found")
    build.build()
    G.lib()
    ref.lib()
    dev = torch.device("cuda", 0)
    K, s2, th2 = M.K, M.SIGMA2, M.TH2

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

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

    # the arguments that shape the measurement; where the lines are written is not one of them
    cmd = (f"python tools/bench_pnpsolver.py --iters {a.iters} --warmup {a.warmup} "
           f"--repeats {a.repeats}")
    lines = []

    for name, (N, ITS, MIN_INLIERS) in WORKLOADS.items():
        words = (N + 63) // 64
        cands = [M.scene(500 + j, N, 0.5, 0.4)[0] for j in range(JOBS)]
        draws = [M.draws_for(900 + j, N, ITS) for j in range(JOBS)]

        def report(leg, ms, **kw):
            rec = {"bench": "pnpsolver", "workload": name, "leg": leg,
                   "ms": round(ms[len(ms) // 2], 5), "ms_min": round(ms[0], 5),
                   "ms_max": round(ms[-1], 5), "n": N, "iterations": ITS,
                   "assumed": "synthetic scenes, no recorded relocalisation", **kw,
                   "cmd": cmd.strip()}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)

        def batch(nj):
            jobs = np.zeros(nj, G.PNP_JOB_DTYPE)
            for j in range(nj):
                jobs[j] = (j * N, N, j * 4 * ITS, ITS, MIN_INLIERS, 0)
            d = dict(m=up(np.concatenate(cands[:nj])),
                     d=up(np.concatenate([x.reshape(-1) for x in draws[:nj]])), j=up(jobs),
                     hyp=torch.zeros(nj * ITS * 64, dtype=torch.uint8, device=dev),
                     bits=torch.zeros(nj * ITS * words, dtype=torch.int64, device=dev),
                     ref=torch.zeros(nj * ITS * 64, dtype=torch.uint8, device=dev),
                     rbits=torch.zeros(nj * ITS * words, dtype=torch.int64, device=dev),
                     ev=torch.zeros(nj * ITS, dtype=torch.int32, device=dev),
                     ne=torch.zeros(nj, dtype=torch.int32, device=dev))

            def run():
                G.pnp_ransac_device(K, s2, th2, d["m"], nj * N, d["d"], nj * 4 * ITS, d["j"], nj, N,
                                    ITS, d["hyp"], d["bits"], d["ref"], d["rbits"], d["ev"],
                                    d["ne"], stream=torch.cuda.current_stream().cuda_stream)
            return run, d

        # the reference of the run: the restatement, also the CPU leg
        want = [ref.ransac(c, d, ITS, MIN_INLIERS, K, s2, th2) for c, d in zip(cands, draws)]
        run1, _ = batch(1)
        runb, db = batch(JOBS)
        runb()
        torch.cuda.synchronize()
        hyp = db["hyp"].cpu().numpy().view(G.PNP_HYP_DTYPE).reshape(JOBS, ITS)
        refined = db["ref"].cpu().numpy().view(G.PNP_HYP_DTYPE).reshape(JOBS, ITS)
        bits = db["bits"].cpu().numpy().view(np.uint64).reshape(JOBS, ITS, words)
        ne = db["ne"].cpu().numpy()
        for j in range(JOBS):
            wh, wb, wr, _, _, wne = want[j]
            same = all(np.array_equal(g[f].view(np.uint32), w[f].view(np.uint32))
                       for g, w in ((hyp[j], wh), (refined[j], wr))
                       for f in ("Rcw", "tcw", "n_inliers", "best"))
            if not (same and np.array_equal(bits[j], wb) and ne[j] == wne):
                raise SystemExit(f"{name} job {j}: the device differs from the restatement")
        events = [int(x) for x in ne]
        refines = [int(len(np.unique(w[0]["best"][w[0]["best"] >= 0]))) for w in want]

        one = device_ms(run1)
        many = device_ms(runb)
        report("one", one, jobs=1, events=events[:1], refines=refines[:1])
        report("batch", many, jobs=JOBS, events=events, refines=refines,
               ms_per_job=round(many[len(many) // 2] / JOBS, 5))
        m0, dr0 = cands[0], draws[0]
        G.pnp_ransac(m0, dr0, ITS, MIN_INLIERS, K, s2, th2)
        report("sync", host_ms(lambda: G.pnp_ransac(m0, dr0, ITS, MIN_INLIERS, K, s2, th2),
                               max(a.iters // 4, 1)), jobs=1, clock="host")
        report("cpu", host_ms(lambda: ref.ransac(m0, dr0, ITS, MIN_INLIERS, K, s2, th2), 3),
               jobs=1, clock="host", note="restatement, one thread, oracle CFLAGS; no OpenCV "
               "allocation per solve: understates the reference's own cost")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
