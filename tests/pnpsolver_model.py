"""numpy side of the RANSAC EPnP tests: synthetic relocalisation scenes, an EPnP model for the
stages after the eigen-solve, direct restatements of the small host pieces, and a Python port of
PnPsolver::iterate / find / Refine (src/solvers/pnp_solver.cpp:112-258)."""
import math

import numpy as np

import pnpsolver_ref as ref

K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
SIGMA2 = np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32))
TH2 = 5.991


def rot(rng, max_angle=0.6):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def scene(seed, n, noise=0.0, outliers=0.0):
    """n correspondences seen from a random pose: (matches, Rcw, tcw). Points 4 .. 20 m ahead."""
    rng = np.random.default_rng(seed)
    R, t = rot(rng), rng.uniform(-1, 1, 3)
    pc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], 1)
    pw = (pc - t) @ R  # R^T (pc - t)
    m = np.zeros(n, ref.MATCH_DTYPE)
    m["xw"] = pw.astype(np.float32)
    m["u"] = K[0] * pc[:, 0] / pc[:, 2] + K[2] + rng.normal(0, 1, n) * noise
    m["v"] = K[1] * pc[:, 1] / pc[:, 2] + K[3] + rng.normal(0, 1, n) * noise
    m["octave"] = rng.integers(0, 8, n)
    bad = rng.random(n) < outliers
    m["u"][bad] += rng.uniform(30, 200, bad.sum())
    m["v"][bad] -= rng.uniform(30, 200, bad.sum())
    return m, R, t


def draws_for(seed, n, n_its):
    rng = np.random.default_rng(seed)
    d = np.zeros((n_its, 4), np.int32)
    for i in range(4):
        d[:, i] = rng.integers(0, n - i, n_its)
    return d


# The single jobs of the GPU tests: n -> (scene seed, pixel noise, outlier share, draw seed, n_its,
# min_inliers). The seeds were searched on the CPU restatement so that 5, 63, 64, 65, 257 and 4096
# have at least one event, 64, 65 and 257 at least two distinct bests, and 65 a best whose inlier
# set is all 65 correspondences (the tests assert this on the restatement's output).
JOBS = {
    4: (7004, 0.0, 0.0, None, 24, 4),
    5: (7005, 0.0, 0.0, 0, 8, 4),
    10: (7010, 0.0, 0.0, 0, 35, 10),
    63: (7063, 0.5, 0.3, 0, 35, 10),
    64: (7064, 0.5, 0.3, 0, 35, 10),
    65: (7065, 0.2, 0.0, 0, 35, 10),
    257: (27257, 0.5, 0.4, 2, 300, 20),
    4096: (11096, 0.5, 0.4, 0, 8, 20),
}


def job(n):
    """(matches, draws[n_its][4], n_its, min_inliers) of the single job with n correspondences."""
    seed, noise, out, dseed, n_its, min_inliers = JOBS[n]
    m, _, _ = scene(seed, n, noise, out)
    if dseed is None:  # n = 4: all 24 orders of the one sample
        d = np.array([(a, b, c, 0) for a in range(4) for b in range(3) for c in range(2)], np.int32)
    else:
        d = draws_for(dseed, n, n_its)
    return m, d, n_its, min_inliers


def resolve(n, randi):
    """The swap-and-pop of :144-154 on a real list."""
    avail = list(range(n))
    out = []
    for r in randi:
        if not 0 <= r <= len(avail) - 1:
            return None
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def parameters(N, probability, minInliers, maxIterations, minSet, epsilon):
    """SetRansacParameters (:87-105) in float32 / float64 as the reference's types are."""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)
    n_min = max(n_min, minInliers, minSet)
    if eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        its = 1
    else:
        try:
            its = math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3))
        except (ValueError, ZeroDivisionError):
            its = 0  # NaN or -0.0 in C
        if not 1 <= its <= 2 ** 31 - 1:
            its = -2 ** 31  # what the x86 conversion gives for a value that is no int
    return n_min, max(1, min(its, maxIterations))


def check_inliers(m, R, t, sigma2, th2):
    """CheckInliers (:261-292) with numpy scalars of the reference's types."""
    f32, f64 = np.float32, np.float64
    fu, fv, uc, vc = (f64(k) for k in K)
    R = np.asarray(R, f64).reshape(3, 3)
    out = np.zeros(len(m), bool)
    with np.errstate(all="ignore"):
        for i, c in enumerate(m):
            x, y, z = (f64(v) for v in c["xw"])
            Xc = f32(R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0])
            Yc = f32(R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1])
            invZc = f32(f64(1) / (R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]))
            ue = uc + fu * f64(Xc) * f64(invZc)
            ve = vc + fv * f64(Yc) * f64(invZc)
            dx, dy = f32(f64(c["u"]) - ue), f32(f64(c["v"]) - ve)
            e2 = f32(f32(dx * dx) + f32(dy * dy))
            o = int(c["octave"])
            out[i] = 0 <= o < len(sigma2) and bool(e2 < f32(f32(sigma2[o]) * f32(th2)))
    return out


# ---- EPnP after the eigen-solve ------------------------------------------------------------

def _l_6x10(v):
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[v[i][3 * a:3 * a + 3] - v[i][3 * b:3 * b + 3] for a, b in pairs]
                   for i in range(4)])
    L = np.zeros((6, 10))
    for r in range(6):
        d = lambda i, j: float(dv[i][r] @ dv[j][r])
        L[r] = [d(0, 0), 2 * d(0, 1), d(1, 1), 2 * d(0, 2), 2 * d(1, 2), d(2, 2), 2 * d(0, 3),
                2 * d(1, 3), 2 * d(2, 3), d(3, 3)]
    return L


def _gauss_newton(L, rho, betas):
    b = np.array(betas, float)
    for _ in range(5):
        b0, b1, b2, b3 = b
        A = np.stack([2 * L[:, 0] * b0 + L[:, 1] * b1 + L[:, 3] * b2 + L[:, 6] * b3,
                      L[:, 1] * b0 + 2 * L[:, 2] * b1 + L[:, 4] * b2 + L[:, 7] * b3,
                      L[:, 3] * b0 + L[:, 4] * b1 + 2 * L[:, 5] * b2 + L[:, 8] * b3,
                      L[:, 6] * b0 + L[:, 7] * b1 + L[:, 8] * b2 + 2 * L[:, 9] * b3], 1)
        quad = np.array([b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3,
                         b2 * b3, b3 * b3])
        b = b + np.linalg.lstsq(A, rho - L @ quad, rcond=None)[0]
    return b


def epnp_downstream(m, sel, cws, ut):
    """compute_pose (:430-478) from the control points and the eigenvectors on: barycentrics by
    np.linalg.solve, the betas by lstsq, R and t by np.linalg.svd. Returns (R, t, chosen)."""
    fu, fv, uc, vc = (float(k) for k in K)
    pw = m["xw"][sel].astype(float)
    us = np.stack([m["u"][sel], m["v"][sel]], 1).astype(float)
    cws = np.asarray(cws, float)
    CC = (cws[1:] - cws[0]).T
    a123 = np.linalg.solve(CC, (pw - cws[0]).T).T
    alphas = np.concatenate([1 - a123.sum(1, keepdims=True), a123], 1)
    v = [ut[11 - i] for i in range(4)]
    L = _l_6x10(v)
    rho = np.array([np.sum((cws[a] - cws[b]) ** 2)
                    for a, b in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]])

    def approx(cols):
        return np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]

    cands = []
    b4 = approx([0, 1, 3, 6])
    s = -1 if b4[0] < 0 else 1
    b0 = math.sqrt(s * b4[0])
    cands.append([b0, s * b4[1] / b0, s * b4[2] / b0, s * b4[3] / b0])
    for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
        b = approx(cols)
        if b[0] < 0:
            b0, b1 = math.sqrt(-b[0]), (math.sqrt(-b[2]) if b[2] < 0 else 0.0)
        else:
            b0, b1 = math.sqrt(b[0]), (math.sqrt(b[2]) if b[2] > 0 else 0.0)
        if b[1] < 0:
            b0 = -b0
        cands.append([b0, b1, b[3] / b0 if len(cols) == 5 else 0.0, 0.0])
    best = None
    for which, betas in enumerate(cands, 1):
        betas = _gauss_newton(L, rho, betas)
        ccs = sum(betas[i] * v[i] for i in range(4)).reshape(4, 3)
        pcs = alphas @ ccs
        if pcs[0, 2] < 0:
            pcs = -pcs
        pc0, pw0 = pcs.mean(0), pw.mean(0)
        U, _, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        pc = pw @ R.T + t
        err = np.mean(np.hypot(us[:, 0] - (uc + fu * pc[:, 0] / pc[:, 2]),
                               us[:, 1] - (vc + fv * pc[:, 1] / pc[:, 2])))
        if best is None or err < best[0]:
            best = (err, R, t, which)
    return best[1], best[2], best[3]


def pose_distance(R1, t1, R2, t2):
    """max(|dR|, |dt| / max(1, |t|))."""
    return max(np.max(np.abs(np.asarray(R1) - R2)),
               np.max(np.abs(np.asarray(t1) - t2)) / max(1.0, float(np.linalg.norm(t2))))


# ---- the Python port of iterate / find / Refine ----------------------------------------------

class PyPnPsolver:
    """PnPsolver over gathered correspondences; the arithmetic of one hypothesis (compute_pose,
    CheckInliers) comes from the restatement, the control flow is :112-258 line by line."""

    def __init__(self, matches, draws, min_inliers, max_its, sigma2=SIGMA2, th2=TH2, indices=None,
                 n_kp=None):
        self.m = matches
        self.N = len(matches)
        self.draws = np.asarray(draws, np.int32).reshape(-1, 4)
        self.mRansacMinInliers, self.mRansacMaxIts = min_inliers, max_its
        self.sigma2, self.th2 = sigma2, th2
        self.indices = np.arange(self.N) if indices is None else np.asarray(indices)
        self.n_kp = self.N if n_kp is None else n_kp
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.mvbBestInliers = None
        self.mBestTcw = None
        self.refines = 0

    @staticmethod
    def _T(R, t):
        return (np.asarray(R, np.float64).astype(np.float32).reshape(-1),
                np.asarray(t, np.float64).astype(np.float32))

    def _scatter(self, mask):
        vb = np.zeros(self.n_kp, bool)
        vb[self.indices[mask]] = True
        return vb

    def _refine(self):
        self.refines += 1
        sel = np.flatnonzero(self.mvbBestInliers)
        R, t, _ = ref.epnp(self.m, sel, K)
        self.mvbRefinedInliers, self.mnRefinedInliers = ref.check_inliers(
            self.m, R, t, K, self.sigma2, self.th2)
        if self.mnRefinedInliers > self.mRansacMinInliers:
            self.mRefinedTcw = self._T(R, t)
            return True
        return False

    def iterate(self, nIterations):
        """Returns (Tcw as (R9 f32, t3 f32) or None, bNoMore, vbInliers, nInliers)."""
        empty = np.zeros(self.n_kp, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, empty, 0
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            nCurrentIterations += 1
            k = self.mnIterations
            self.mnIterations += 1
            idx = resolve(self.N, self.draws[k])
            R, t, _ = ref.epnp(self.m, idx, K)
            inl, n = ref.check_inliers(self.m, R, t, K, self.sigma2, self.th2)
            if n >= self.mRansacMinInliers:
                if n > self.mnBestInliers:
                    self.mvbBestInliers, self.mnBestInliers = inl, n
                    self.mBestTcw = self._T(R, t)
                if self._refine():
                    return (self.mRefinedTcw, False, self._scatter(self.mvbRefinedInliers),
                            self.mnRefinedInliers)
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return self.mBestTcw, True, self._scatter(self.mvbBestInliers), self.mnBestInliers
            return None, True, empty, 0
        return None, False, empty, 0

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
