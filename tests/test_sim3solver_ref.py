"""tests/sim3solver_ref.c (the CPU restatement of the RANSAC Sim3 solver the device is compared
against bit for bit) pinned against a pure-numpy model -- np.linalg.eigh Horn, float64 projection
-- and a straightforward Python port of Sim3Solver::iterate. No GPU."""
import functools
import itertools

import numpy as np
import pytest

import sim3solver_ref as R
import sim3solver_scenario as S

MIN_INLIERS = 20


@functools.lru_cache(maxsize=None)
def scenario(n, fix_scale):
    c = S.candidate(100 + n, n, fix_scale)
    n_its = S.ransac_iterations(n, 0.99, MIN_INLIERS, 300)
    d = S.draws(7 + n, n, n_its)
    hyp, bits, events, ne = R.ransac(c["matches"], d, n_its, MIN_INLIERS, fix_scale, c["K"],
                                     c["K"], c["sigma2"], c["sigma2"])
    assert ne >= 0
    for a in (hyp, bits, events, d):
        a.setflags(write=False)
    return c, d, n_its, hyp, bits, events[:ne]


# ---- the numpy model -----------------------------------------------------------------------

def quat_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def numpy_hypothesis(m, idx, fix_scale, K, sig2):
    """Horn 1987 with np.linalg.eigh, everything after N in float64. N itself is formed as the
    contract forms it -- centroids, relative coordinates, M and the ten entries in float32 --
    because the eigenvector the contract defines is that of the FLOAT-ROUNDED N: with N formed in
    float64 instead, hypotheses whose eigenvalue gap lies between 1e-3 and 6e-2 of the largest
    differ from it by up to 2.0e-5 in R and 8.2e-5 in t (1 and 6 of the 146 well-conditioned
    hypotheses at N = 64; the float rounding of N, about 1e-7 relative, over the gap, times the
    20-40 m lever arm of the sample's centroid), while a float64 eigh of the restatement's own N
    agrees with its Jacobi to 3e-8. Returns (R, t, s, well_conditioned, err1, err2, thr1, thr2)."""
    f32 = np.float32
    P1 = m["x1c"][idx].astype(f32).T
    P2 = m["x2c"][idx].astype(f32).T
    third = f32(1.0 / 3.0)
    O1 = (((P1[:, 0] + P1[:, 1]) + P1[:, 2]) * third).reshape(3, 1)
    O2 = (((P2[:, 0] + P2[:, 1]) + P2[:, 2]) * third).reshape(3, 1)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            M[i, j] = (Pr2[i, 0] * Pr1[j, 0] + Pr2[i, 1] * Pr1[j, 1]) + Pr2[i, 2] * Pr1[j, 2]
    N = np.array([
        [M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
        [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
        [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
        [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]], f32).astype(np.float64)
    N = N + np.triu(N, 1).T
    O1, O2, Pr1, Pr2 = (a.astype(np.float64) for a in (O1, O2, Pr1, Pr2))
    w, v = np.linalg.eigh(N)
    well = (w[-1] - w[-2]) > 1e-3 * abs(w[-1])
    Rm = quat_R(v[:, -1])
    P3 = Rm @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    t = (O1 - s * Rm @ O2).reshape(3)
    fx, fy, cx, cy = [float(k) for k in K]

    def img(X):
        return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)

    X1 = m["x1c"].astype(np.float64)
    X2 = m["x2c"].astype(np.float64)
    with np.errstate(all="ignore"):
        e1 = ((img(X1) - img(s * X2 @ Rm.T + t)) ** 2).sum(1)
        e2 = ((img((X1 - t) @ Rm / s) - img(X2)) ** 2).sum(1)
    thr = np.floor(9.210 * sig2.astype(np.float64))
    return Rm, t, s, well, e1, e2, thr[m["octave1"]], thr[m["octave2"]]


@pytest.mark.parametrize("n,fix_scale", S.SCENARIOS)
def test_restatement_matches_numpy_model(n, fix_scale):
    c, d, n_its, hyp, bits, events = scenario(n, fix_scale)
    m = c["matches"]
    inl = R.unpack_bits(bits, n)
    tests = excluded = compared = 0
    for k in range(n_its):
        idx = R.resolve(n, d[k])
        Rm, t, s, well, e1, e2, t1, t2 = numpy_hypothesis(m, idx, fix_scale, c["K"], c["sigma2"])
        near = (np.abs(e1 - t1) <= 1e-3 * t1), (np.abs(e2 - t2) <= 1e-3 * t2)
        if well:
            compared += 1
            assert np.abs(hyp["R12"][k].reshape(3, 3) - Rm).max() <= 1e-5, k
            assert np.all(np.abs(hyp["t12"][k] - t) <= 1e-5 * np.maximum(np.abs(t), 1)), k
            assert abs(hyp["s12"][k] - s) <= 1e-5 * max(abs(s), 1), k
            ex = near[0] | near[1]
            tests += 2 * n
            excluded += int(near[0].sum() + near[1].sum())
            model = (e1 < t1) & (e2 < t2)
            assert np.array_equal(inl[k][~ex], model[~ex]), k
            assert abs(int(hyp["n_inliers"][k]) - int(model.sum())) <= int(ex.sum()), k
        assert int(hyp["n_inliers"][k]) == int(inl[k].sum())
    assert compared >= 0.9 * n_its
    print(f"n={n} fix_scale={fix_scale}: its={n_its} compared={compared} excluded={excluded}/"
          f"{tests} events={list(events)} best={int(hyp['n_inliers'].max())}")
    assert excluded <= 1e-3 * tests


def test_scenarios_exercise_the_event_path():
    """The recipe gives candidates RANSAC accepts (events) where the schedule is long, the
    35-iteration schedule at N = 40 (:135) and the one-iteration path at N = 20."""
    for n, fs in S.SCENARIOS:
        c, d, n_its, hyp, bits, events = scenario(n, fs)
        if n == MIN_INLIERS:
            assert n_its == 1 and len(events) == 0
        elif n == 40:
            assert n_its == 35
        else:
            assert len(events) >= 2 and hyp["n_inliers"].max() > MIN_INLIERS
        assert not c["mismatched"].all() and c["mismatched"].sum() == round(S.MISMATCH * n)


# ---- swap-and-pop ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 5])
def test_swap_and_pop(n):
    for r in itertools.product(range(n), range(n - 1), range(n - 2)):
        avail = list(range(n))
        want = []
        for x in r:
            want.append(avail[x])
            avail[x] = avail[-1]
            avail.pop()
        assert list(R.resolve(n, r)) == want, r
    assert R.resolve(n, (n, 0, 0)) is None and R.resolve(n, (0, n - 1, 0)) is None
    assert R.resolve(n, (0, 0, n - 2)) is None and R.resolve(n, (-1, 0, 0)) is None
    assert R.resolve(2, (0, 0, 0)) is None


# ---- the state machine ------------------------------------------------------------------------

class PortedSolver:
    """sim3solver.cpp:142-217 over the per-hypothesis results, walked one by one."""

    def __init__(self, n, n_its, min_inliers, hyp, inl):
        self.N, self.max_its, self.min_inliers = n, n_its, min_inliers
        self.hyp, self.inl = hyp, inl
        self.iterations = 0
        self.best_inliers = 0
        self.best = None

    def iterate(self, n_iterations):
        vb = np.zeros(self.N, bool)
        if self.N < self.min_inliers:
            return -1, True, vb, 0
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            self.iterations += 1
            k = self.iterations - 1
            ni = int(self.hyp["n_inliers"][k])
            if ni >= self.best_inliers:
                self.best_inliers = ni
                self.best = k
                if ni > self.min_inliers:
                    return k, False, self.inl[k].copy(), ni
        return -1, self.iterations >= self.max_its, vb, 0

    def find(self):
        k, _, vb, ni = self.iterate(self.max_its)
        return k, vb, ni


def same_best(ref, port, hyp):
    b = ref.best()
    if port.best is None:
        return b is None
    h = hyp[port.best]
    return b is not None and np.array_equal(b[0].reshape(-1), h["R12"]) and \
        np.array_equal(b[1], h["t12"]) and b[2] == float(h["s12"])


def solvers(n, fix_scale, min_inliers=MIN_INLIERS):
    c, d, n_its, hyp, bits, events = scenario(n, fix_scale)
    ref = R.Solver(c["matches"], d, n_its, min_inliers, fix_scale, c["K"], c["K"], c["sigma2"],
                   c["sigma2"])
    return ref, PortedSolver(n, n_its, min_inliers, hyp, R.unpack_bits(bits, n)), hyp, n_its


@pytest.mark.parametrize("n,fix_scale", S.SCENARIOS)
def test_iterate_five_to_exhaustion(n, fix_scale):
    ref, port, hyp, n_its = solvers(n, fix_scale)
    assert same_best(ref, port, hyp)
    for _ in range(n_its + 2):
        a, b = ref.iterate(5), port.iterate(5)
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2])
        assert same_best(ref, port, hyp)
        if a[1]:
            break
    assert a[1] and port.iterations == n_its
    a, b = ref.iterate(5), port.iterate(5)  # past the end: nothing more, best retained
    assert a[0] == b[0] == -1 and a[1] and b[1] and same_best(ref, port, hyp)


@pytest.mark.parametrize("n,fix_scale", S.SCENARIOS)
def test_find_then_iterate_again(n, fix_scale):
    ref, port, hyp, n_its = solvers(n, fix_scale)
    a, b = ref.find(), port.find()
    assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
    assert same_best(ref, port, hyp)
    a, b = ref.iterate(n_its), port.iterate(n_its)  # the best of before is retained
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2])
    assert same_best(ref, port, hyp)


def test_too_few_correspondences_returns_at_once():
    ref, port, hyp, n_its = solvers(20, True, min_inliers=21)
    a, b = ref.iterate(5), port.iterate(5)
    assert a[0] == b[0] == -1 and a[1] and b[1] and a[3] == 0 and not a[2].any()
    assert ref.best() is None


def test_scatter_through_indices1():
    c, d, n_its, hyp, bits, events = scenario(64, True)
    idx1 = np.arange(64) * 3 + 1
    ref = R.Solver(c["matches"], d, n_its, MIN_INLIERS, True, c["K"], c["K"], c["sigma2"],
                   c["sigma2"], indices1=idx1, n1=200)
    k, vb, ni = ref.find()
    assert k == events[0] and vb.shape == (200,) and vb.sum() == ni
    assert np.array_equal(np.flatnonzero(vb), idx1[R.unpack_bits(bits[k], 64)])


# ---- thresholds -------------------------------------------------------------------------------

def test_thresholds_are_truncated():
    s2 = S.sigma2(1.2, 8)
    got = [R.threshold(x) for x in s2]
    assert got[:4] == [9.0, 13.0, 19.0, 27.0]
    assert got == [float(int(9.210 * float(x))) for x in s2]


def test_jacobi_sweep_count_has_converged():
    """One more sweep than the restatement uses changes no eigenvector component on the
    scenarios' N matrices (DESIGN.md records the search over 10^5 random matrices)."""
    sw = R.jacobi_sweeps()
    for n, fs in S.SCENARIOS[:3]:
        c, d, n_its, hyp, bits, events = scenario(n, fs)
        for k in range(0, n_its, 7):
            _, _, N = R.hypothesis(c["matches"], R.resolve(n, d[k]), fs, c["K"], c["K"],
                                   c["sigma2"], c["sigma2"])
            assert np.array_equal(R.eigvec(N, sw - 2), R.eigvec(N, sw + 1))
