"""The sweep count of the monocular Initializer's one-sided Jacobi SVD, searched on
the CPU with the restatement tests/initializer_ref.c: the smallest count after which one more
sweep changes no bit of what the Initializer takes from a decomposition -- vt.row(8) of the 16 x 9
and 8 x 9 systems, w / u / vt of the 3 x 3 ones, vt.row(3) of the 4 x 4 one, each rounded to float
as the reference's CV_32F Mats hold them -- over the test scenes (tests/initializer_scenario.py:
every 8-point sample of the schedule for H and F, the motions of both models and the
triangulation of every match under every motion) plus random matrices of each of the four shapes.
The solver uses that count plus two.

  python tools/init_jacobi_sweeps.py [--random 10000] [--its 200] [--max-sweeps 16]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random", type=int, default=10000)
    ap.add_argument("--its", type=int, default=200)
    ap.add_argument("--max-sweeps", type=int, default=16)
    a = ap.parse_args()
    import initializer_ref as R
    import initializer_scenario as S
    rng = np.random.default_rng(1)
    samples, decomps, tris, mats = [], [], [], []
    for kind in ("general", "planar", "rotation"):
        for noise in (0.0, 0.5):
            s = S.make(kind, noise=noise)
            o = R.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, S.draws(s.n, a.its), a.its)
            pairs = o.pairs[:s.n]
            nm = o.result["norm"][0]
            p1 = (s.keys1[pairs[:, 0]] - nm[0:2]) * nm[2:4]
            p2 = (s.keys2[pairs[:, 1]] - nm[4:6]) * nm[6:8]
            for d in S.draws(s.n, a.its):
                idx = R.resolve(s.n, d)
                samples.append((p1[idx].astype(np.float32), p2[idx].astype(np.float32)))
            Km = np.array([[s.K[0], 0, s.K[2]], [0, s.K[1], s.K[3]], [0, 0, 1]], np.float32)
            P1 = np.hstack([Km, np.zeros((3, 1), np.float32)])
            for model in (0, 1):
                b = o.result["best"][0][model]
                if b < 0:
                    continue
                M = o.hyp["M"][model, b]
                decomps.append((M, s.K, model))
                for mo in R.motions(M, s.K, model):
                    Rt = np.hstack([mo["R"].reshape(3, 3), mo["t"].reshape(3, 1)])
                    P2 = (Km.astype(np.float64) @ Rt).astype(np.float32)
                    for i1, i2 in pairs[::4]:
                        tris.append((s.keys1[i1], s.keys2[i2], P1, P2))
    for _ in range(a.random):
        for shape in ((16, 9), (8, 9), (3, 3), (4, 4)):
            mats.append((rng.normal(0, 1, shape) * 10 ** rng.uniform(-3, 3)).astype(np.float32))
    print(f"{len(samples)} samples, {len(decomps)} decompositions, {len(tris)} triangulations, "
          f"{len(mats)} random matrices")

    def run(sw):
        out = []
        for p1, p2 in samples:
            out.append(np.concatenate([R.compute_h21(p1, p2, sw).ravel(),
                                       R.compute_f21(p1, p2, sw).ravel()]))
        for M, K, model in decomps:
            mo = R.motions(M, K, model, sw)
            out.append(np.concatenate([mo["R"].ravel(), mo["t"].ravel()]))
        for t in tris:
            out.append(R.triangulate(*t, sweeps=sw))
        for A in mats:
            if A.shape == (3, 3):
                out.append(np.concatenate([x.ravel() for x in R.svd3(A, sw)]))
            else:
                out.append(R.svd(A, sw)[1][-1].astype(np.float32))
        return out

    prev, settled = run(1), None
    for sw in range(2, a.max_sweeps + 1):
        cur = run(sw)
        changed = sum(not np.array_equal(p, q, equal_nan=True) for p, q in zip(prev, cur))
        print(f"sweeps {sw - 1} -> {sw}: {changed} results changed")
        if changed == 0 and settled is None:
            settled = sw - 1
        elif changed:
            settled = None
        prev = cur
    print(f"settled after {settled} sweeps; the solver uses {R.jacobi_sweeps()}")


if __name__ == "__main__":
    main()
