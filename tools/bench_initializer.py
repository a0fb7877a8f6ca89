"""Device time of the monocular Initializer (include/slamgpu_initializer.h) against the CPU
restatement (tests/initializer_ref.c, checked bit for bit against the device output in the same
run).

  python tools/bench_initializer.py [--iters 50] [--warmup 5] [--repeats 5] [--out FILE]

Workloads (ASSUMPTIONS, not a recorded monocular start: there is no real sequence here), on the
tests' general scene (tests/initializer_scenario.py, 0.5 px noise, 20 % wrong matches), the
tracker's call of 200 iterations:
  n300     N = 300 matches
  n2000    N = 2000 matches
Legs, per workload:
  device   one job in one slamgpu_init_ransac_device call (all four kernels)
  sync     slamgpu_init_ransac end to end: staging, upload, the kernels, download, synchronise
  cpu      the same job through the restatement on one thread at the oracle's CFLAGS. It has no
           OpenCV allocation per hypothesis and runs H and F one after the other where the
           reference uses two threads.
Device times are hipEvent intervals around `iters` back-to-back calls after `warmup` calls,
divided by iters; each figure is the median of `repeats` such windows, with the spread (min, max)
beside it. `sync` and `cpu` are host clocks. One JSON line each; --out also writes them to a file.
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

WORKLOADS = {"n300": 300, "n2000": 2000}
ITS = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import initializer_ref as ref
    import initializer_scenario as S
    from slam_framework_amd import build, slamgpu as G
    if not torch.cuda.is_available():
        raise SystemExit("bench_initializer needs the GPU: no device found")
    build.build()
    G.lib()
    ref.lib()
    dev = torch.device("cuda", 0)

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

    cmd = (f"python tools/bench_initializer.py --iters {a.iters} --warmup {a.warmup} "
           f"--repeats {a.repeats}")
    lines = []
    for name, N in WORKLOADS.items():
        s = S.make("general", n=N, noise=0.5, extra1=N // 5, extra2=N // 6)
        draws = S.draws(N, ITS, seed=11)
        words = (s.n1 + 63) // 64
        want = ref.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, draws, ITS)

        def report(leg, ms, **kw):
            rec = {"bench": "initializer", "workload": name, "leg": leg,
                   "ms": round(ms[len(ms) // 2], 5), "ms_min": round(ms[0], 5),
                   "ms_max": round(ms[-1], 5), "n": N, "n1": s.n1, "n2": s.n2, "iterations": ITS,
                   "assumed": "synthetic scene, no recorded monocular start", **kw,
                   "cmd": cmd.strip()}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)

        job = np.zeros(1, G.INIT_JOB_DTYPE)
        job[0] = (0, s.n1, 0, s.n2, 0, ITS, s.K, s.sigma, 0)
        d = dict(k1=up(s.keys1), m=up(s.matches12), k2=up(s.keys2), d=up(draws), j=up(job))
        sizes = (2 * ITS * 48, 2 * ITS * words * 8, 80, s.n1 * 8, 8 * 64, 8 * words * 8,
                 8 * s.n1 * 12)
        outs = [torch.zeros(b, dtype=torch.uint8, device=dev) for b in sizes]

        def run():
            G.init_ransac_device(d["k1"], d["m"], s.n1, d["k2"], s.n2, d["d"], 8 * ITS, d["j"], 1,
                                 s.n1, ITS, *outs, stream=torch.cuda.current_stream().cuda_stream)

        run()
        torch.cuda.synchronize()
        for o, w, label in zip(outs, want.arrays(), ("hyp", "bits", "result", "pairs", "motion",
                                                     "good_bits", "p3d")):
            g = o.cpu().numpy()
            wu = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
            nm = int(want.result["n_motions"][0])
            if label in ("motion", "good_bits", "p3d"):  # rows of the motions that exist
                g, wu = g[:len(g) // 8 * nm], wu[:len(wu) // 8 * nm]
            if label == "pairs":
                g, wu = g[:8 * N], wu[:8 * N]
            if not np.array_equal(g, wu):  # no NaN in this scene: bytes compare
                raise SystemExit(f"{name}: {label} differs from the restatement")
        r = want.result[0]
        info = dict(model=int(r["model"]), n_motions=int(r["n_motions"]),
                    n_good=[int(x) for x in want.motion["n_good"][:int(r["n_motions"])]])
        report("device", device_ms(run), **info)
        args = (s.keys1, s.keys2, s.matches12, s.K, s.sigma, draws, ITS)
        G.init_ransac(*args)
        report("sync", host_ms(lambda: G.init_ransac(*args), max(a.iters // 4, 1)), clock="host")
        report("cpu", host_ms(lambda: ref.ransac(*args), 3), clock="host",
               note="restatement, one thread, oracle CFLAGS; H then F, no OpenCV allocation")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
