"""Seeded two-view scenes for the monocular Initializer tests: a general 3-D scene, a planar one
and a pure rotation, as undistorted keypoints of two frames with vMatches12 (-1 = unmatched),
pixel noise and a share of wrong matches. Plain numpy, no GPU."""
import numpy as np

K = np.array([600.0, 598.5, 642.3, 357.1], np.float32)  # fx, fy, cx, cy
WIDTH, HEIGHT = 1280.0, 720.0
SIGMA = 1.0


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def project(X, R, t):
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)


class Scene:
    """keys1[n1][2], keys2[n2][2] float32, matches12[n1] int32; the truth: R21, t21, X[n1][3]
    (camera-1 coordinates, NaN for an unmatched or wrongly matched key) and wrong[n1]."""


def make(kind, n=300, noise=0.0, wrong=0.2, seed=0, extra1=40, extra2=25, motion=None,
         plane=None):
    """kind: "general", "planar" or "rotation". n matches among n + extra1 keys of frame 1 and
    n + extra2 keys of frame 2, the matched keys scattered among the unmatched ones."""
    rng = np.random.default_rng([seed, {"general": 1, "planar": 2, "rotation": 3}[kind]])
    R21 = rot([0.2, 1.0, 0.1], 0.12)
    t21 = np.array([-2.4, 0.3, 0.9])
    if motion is not None:
        R21, t21 = rot(motion[0], motion[1]), np.asarray(motion[2], np.float64)
    if kind == "rotation":
        t21 = np.zeros(3)
    m = 0
    X = np.zeros((0, 3))
    while len(X) < n:  # points both cameras see
        c = 4 * n
        u = rng.uniform(20, WIDTH - 20, c)
        v = rng.uniform(20, HEIGHT - 20, c)
        if kind == "planar":
            # the plane n . X = d seen from camera 1, tilted against the optical axis
            nrm, d = (np.array([1.0, 0.1, 0.5]), 6.0) if plane is None else plane
            nrm = np.asarray(nrm, np.float64)
            ray = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones(c)], 1)
            z = d / (ray @ nrm)
        else:
            z = rng.uniform(4.0, 20.0, c)
            ray = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones(c)], 1)
        P = ray * z[:, None]
        p2 = project(P, R21, t21)
        ok = ((P @ R21.T + t21)[:, 2] > 0.5) & (p2[:, 0] > 5) & (p2[:, 0] < WIDTH - 5) & \
             (p2[:, 1] > 5) & (p2[:, 1] < HEIGHT - 5) & (z > 0.5)
        X = np.concatenate([X, P[ok]])[:n]
        m += 1
        assert m < 50
    n1, n2 = n + extra1, n + extra2
    pos1 = np.sort(rng.permutation(n1)[:n])
    pos2 = rng.permutation(n2)[:n]
    keys1 = np.stack([rng.uniform(0, WIDTH, n1), rng.uniform(0, HEIGHT, n1)], 1)
    keys2 = np.stack([rng.uniform(0, WIDTH, n2), rng.uniform(0, HEIGHT, n2)], 1)
    keys1[pos1] = project(X, np.eye(3), np.zeros(3)) + noise * rng.standard_normal((n, 2))
    keys2[pos2] = project(X, R21, t21) + noise * rng.standard_normal((n, 2))
    is_wrong = rng.permutation(n) < int(round(wrong * n))
    keys2[pos2[is_wrong]] = np.stack([rng.uniform(0, WIDTH, is_wrong.sum()),
                                      rng.uniform(0, HEIGHT, is_wrong.sum())], 1)
    s = Scene()
    s.kind, s.n, s.n1, s.n2 = kind, n, n1, n2
    s.keys1, s.keys2 = keys1.astype(np.float32), keys2.astype(np.float32)
    s.matches12 = np.full(n1, -1, np.int32)
    s.matches12[pos1] = pos2
    s.R21, s.t21 = R21, t21
    s.X = np.full((n1, 3), np.nan)
    s.X[pos1[~is_wrong]] = X[~is_wrong]
    s.wrong = np.zeros(n1, bool)
    s.wrong[pos1[is_wrong]] = True
    s.K, s.sigma = K, SIGMA
    return s


class Lcg:
    """A seeded stand-in for DUtils::Random::RandomInt: the tests' draws do not depend on rand()."""

    def __init__(self, seed=1):
        self.s = seed

    def __call__(self, lo, hi):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return lo + (self.s >> 8) % (hi - lo + 1)


def draws(n, n_its, seed=1):
    r = Lcg(seed)
    d = np.zeros((n_its, 8), np.int32)
    for k in range(n_its):
        for j in range(8):
            d[k, j] = r(0, n - 1 - j)
    return d
