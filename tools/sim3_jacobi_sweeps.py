"""The Jacobi sweep count of the RANSAC Sim3 solver's FP64 eigen-solve, searched on
the CPU with the restatement tests/sim3solver_ref.c: the smallest count after which one more sweep
changes no eigenvector component, over the N matrices of the test scenarios (300 hypotheses each)
plus 10^5 random symmetric 4x4 float matrices. The solver uses that count plus two.

  python tools/sim3_jacobi_sweeps.py [--random 100000] [--max-sweeps 15]
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
    ap.add_argument("--random", type=int, default=100000)
    ap.add_argument("--max-sweeps", type=int, default=15)
    a = ap.parse_args()
    import sim3solver_ref as R
    import sim3solver_scenario as S
    rng = np.random.default_rng(1)
    mats = []
    for _ in range(a.random):
        A = rng.normal(0, 1, (4, 4)) * 10 ** rng.uniform(-3, 3)
        mats.append((A + A.T).astype(np.float32))
    for n, fs in S.SCENARIOS:
        c = S.candidate(100 + n, n, fs)
        d = S.draws(7, n, 300)
        for k in range(300):
            _, _, N = R.hypothesis(c["matches"], R.resolve(n, d[k]), fs, c["K"], c["K"],
                                   c["sigma2"], c["sigma2"])
            mats.append(N.copy())
    print(f"{len(mats)} matrices ({a.random} random)")
    prev = [R.eigvec(A, 1) for A in mats]
    settled = None
    for s in range(2, a.max_sweeps + 1):
        cur = [R.eigvec(A, s) for A in mats]
        changed = sum(not np.array_equal(p, q, equal_nan=True) for p, q in zip(prev, cur))
        print(f"sweeps {s - 1} -> {s}: {changed} eigenvectors changed")
        if changed == 0 and settled is None:
            settled = s - 1
        elif changed:
            settled = None
        prev = cur
    print(f"settled after {settled} sweeps; the solver uses {R.jacobi_sweeps()}")


if __name__ == "__main__":
    main()
