"""The sweep count of CreateNewMapPoints' 4 x 4 one-sided Jacobi (DESIGN.md "CreateNewMapPoints"),
searched on the CPU with the restatement tests/newpoints_ref.c: the smallest count after which one
more sweep changes no bit of vt.row(3) rounded to float, as the reference's CV_32F Mat holds it,
over every matched pair of the test scenes (tests/newpoints_scenario.py: mono, stereo and mixed,
three neighbours) with the cameras 0 m, 100 m and 1000 m from the world origin -- the matrices
hold world-frame poses, and the translation column grows with the distance. The kernel uses that
count plus two.

  python tools/newpoints_jacobi_sweeps.py [--n 600] [--max-sweeps 16]
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
    ap.add_argument("--n", type=int, default=600)
    ap.add_argument("--max-sweeps", type=int, default=16)
    a = ap.parse_args()
    import newpoints_ref as R
    import newpoints_scenario as NS
    sc, s2 = NS.levels_arrays()
    print("| distance from the origin | pairs | settled after | changes per extra sweep (1->2, 2->3, ...) |")
    print("|---|---|---|---|")
    worst = 0
    for dist in (0.0, 100.0, 1000.0):
        d = dist / np.sqrt(3.0)
        pairs = []
        for kind, seed in (("mono", 51), ("stereo", 52), ("mixed", 53)):
            cur, nbors = NS.scene(a.n, seed, 3, kind, origin=(d, -d, d))
            out = R.newpoints_chain(cur, nbors, sc, s2)
            for nb, m in zip(nbors, out["matches"]):
                pairs += [(cur, nb["kf"], i, int(j)) for i, j in enumerate(m) if j >= 0]

        def run(sw):
            return [R.dlt(k1, k2, i, j, sw)[1].astype(np.float32) for k1, k2, i, j in pairs]

        prev, settled, changes = run(1), None, []
        for sw in range(2, a.max_sweeps + 1):
            cur_out = run(sw)
            changed = sum(not np.array_equal(p, q, equal_nan=True) for p, q in zip(prev, cur_out))
            changes.append(changed)
            if changed == 0 and settled is None:
                settled = sw - 1
            elif changed:
                settled = None
            prev = cur_out
        worst = max(worst, settled if settled is not None else a.max_sweeps + 1)
        print(f"| {dist:g} m | {len(pairs)} | {settled} | {' '.join(map(str, changes))} |")
    print(f"settled after {worst} sweeps at the latest; the kernel uses {R.jacobi_sweeps()}")


if __name__ == "__main__":
    main()
