"""The sweep count of the RANSAC EPnP solver's one-sided Jacobi SVD, searched on the
CPU with the restatement tests/pnpsolver_ref.c: the smallest count after which one more sweep
changes no bit of the pose, the eigenvalues or the eigenvectors of any EPnP solve over the test
scenes (tests/pnpsolver_model.py: four-point samples and whole sets of 5 .. 100 correspondences,
with and without noise) plus random matrices of every shape the solver decomposes. The solver uses
that count plus two.

  python tools/pnp_jacobi_sweeps.py [--scenes 40] [--random 2000] [--max-sweeps 16]
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
    ap.add_argument("--scenes", type=int, default=40)
    ap.add_argument("--random", type=int, default=2000)
    ap.add_argument("--max-sweeps", type=int, default=16)
    a = ap.parse_args()
    import pnpsolver_model as M
    import pnpsolver_ref as R
    rng = np.random.default_rng(1)
    solves, mats = [], []
    for seed in range(a.scenes):
        for n in (4, 5, 6, 8, 20, 100):
            for noise in (0.0, 0.7):
                m, _, _ = M.scene(1000 * n + seed, n, noise)
                solves.append((m, np.arange(n)))
        m, _, _ = M.scene(seed, 60, 0.7, 0.3)
        for d in M.draws_for(seed, 60, 10):
            solves.append((m, np.array(M.resolve(60, d))))
    for _ in range(a.random):
        for shape in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
            A = rng.normal(0, 1, shape) * 10 ** rng.uniform(-3, 3)
            mats.append(A @ A.T if shape == (12, 12) else A)
    print(f"{len(solves)} EPnP solves, {len(mats)} random matrices")

    def run(s):
        out = []
        for m, sel in solves:
            Rm, t, st = R.epnp(m, sel, M.K, sweeps=s)
            out.append(np.concatenate([Rm.ravel(), t, st["d"], st["ut"].ravel()]))
        for A in mats:
            out.append(np.concatenate([x.ravel() for x in R.svd(A, s)]))
        return out

    prev, settled = run(1), None
    for s in range(2, a.max_sweeps + 1):
        cur = run(s)
        changed = sum(not np.array_equal(p, q, equal_nan=True) for p, q in zip(prev, cur))
        print(f"sweeps {s - 1} -> {s}: {changed} results changed")
        if changed == 0 and settled is None:
            settled = s - 1
        elif changed:
            settled = None
        prev = cur
    print(f"settled after {settled} sweeps; the solver uses {R.jacobi_sweeps()}")


if __name__ == "__main__":
    main()
