"""Synthetic loop candidates for the RANSAC Sim3 solver tests. synthetic.sim3_problem will not do:
its 3D points are exact and its outliers live in pixels the solver never reads.

The recipe: the KITTI camera for both keyframes; points at 3-40 m in view of both; each
camera-frame point is RE-TRIANGULATED from a noisy stereo observation of its own keyframe
(PIXEL_NOISE px on u and v, DISPARITY_NOISE px on the disparity, bf 386.1448), so the 3D
correspondences carry the depth-dependent error a stereo map has; MISMATCH of the pairs are
mismatched by a permutation of their second points; octaves are geometric as in sim3_problem."""
import numpy as np

from slam_framework_amd import synthetic as syn

PIXEL_NOISE = 0.5
DISPARITY_NOISE = 0.35
MISMATCH = 0.3
NLEVELS = 8
SCALE_FACTOR = 1.2
MATCH_DTYPE = np.dtype([("x1c", "<f4", (3,)), ("x2c", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"),
                        ("u2", "<f4"), ("v2", "<f4"), ("octave1", "<i4"), ("octave2", "<i4")])


def sigma2(scale_factor=SCALE_FACTOR, nlevels=NLEVELS):
    """level_sigma_sq as ORBextractor builds it (f32 running product)."""
    s2 = np.ones(nlevels, np.float32)
    sc = np.float32(1.0)
    for i in range(1, nlevels):
        sc = np.float32(sc * np.float32(scale_factor))
        s2[i] = sc * sc
    return s2


def _stereo_noise(rng, X, cam):
    fx, fy, cx, cy, bf = cam
    u = X[:, 0] / X[:, 2] * fx + cx + rng.normal(0, PIXEL_NOISE, len(X))
    v = X[:, 1] / X[:, 2] * fy + cy + rng.normal(0, PIXEL_NOISE, len(X))
    d = bf / X[:, 2] + rng.normal(0, DISPARITY_NOISE, len(X))
    z = bf / d
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)


def candidate(seed, n, fix_scale=True, cam=syn.KITTI_CAM):
    """Returns dict(matches, K, sigma2, R, t, s, mismatched): X1c = s R X2c + t is the truth."""
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else 1.1
    R = syn._rodrigues(rng.normal(0, 0.15, 3))
    t = rng.normal(0, 1.5, 3)
    fx, fy, cx, cy = cam[:4]
    X1 = np.zeros((0, 3))
    X2 = np.zeros((0, 3))
    while len(X1) < n:
        m = 4 * n
        u2 = rng.uniform(0, syn.KITTI_COLS, m)
        v2 = rng.uniform(0, syn.KITTI_ROWS, m)
        z2 = rng.uniform(3.0, 40.0, m)
        b = np.stack([(u2 - cx) / fx * z2, (v2 - cy) / fy * z2, z2], 1)
        a = s * b @ R.T + t
        with np.errstate(divide="ignore", invalid="ignore"):
            u1 = a[:, 0] / a[:, 2] * fx + cx
            v1 = a[:, 1] / a[:, 2] * fy + cy
        keep = (a[:, 2] >= 3.0) & (a[:, 2] <= 40.0 * s + 5) & (u1 >= 0) & (u1 < syn.KITTI_COLS) & \
            (v1 >= 0) & (v1 < syn.KITTI_ROWS)
        X1 = np.concatenate([X1, a[keep]])
        X2 = np.concatenate([X2, b[keep]])
    X1, X2 = X1[:n], X2[:n]
    # keyframe 1 triangulates in its own metric frame; with s != 1 its map is the scaled one
    N1 = _stereo_noise(rng, X1 / s, cam) * s
    N2 = _stereo_noise(rng, X2, cam)
    bad = np.zeros(n, bool)
    k = int(round(MISMATCH * n))
    if k >= 2:
        sel = rng.choice(n, k, replace=False)
        N2[sel] = N2[np.roll(sel, 1)]
        bad[sel] = True
    m = np.zeros(n, MATCH_DTYPE)
    m["x1c"] = N1.astype(np.float32)
    m["x2c"] = N2.astype(np.float32)
    m["u1"] = N1[:, 0] / N1[:, 2] * fx + cx
    m["v1"] = N1[:, 1] / N1[:, 2] * fy + cy
    m["u2"] = N2[:, 0] / N2[:, 2] * fx + cx
    m["v2"] = N2[:, 1] / N2[:, 2] * fy + cy
    m["octave1"] = np.minimum(rng.geometric(0.45, n) - 1, NLEVELS - 1)
    m["octave2"] = np.minimum(rng.geometric(0.45, n) - 1, NLEVELS - 1)
    return {"matches": m, "K": np.asarray(cam[:4], np.float32), "sigma2": sigma2(),
            "R": R, "t": t, "s": s, "mismatched": bad}


def draws(seed, n, n_its):
    """n_its x 3 values as RandomInt(0, size - 1) returns them for sizes n, n - 1, n - 2."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n - i, n_its) for i in range(3)], 1).astype(np.int32)


def ransac_iterations(n, probability=0.99, min_inliers=20, max_its=300):
    """The effective mRansacMaxIts of sim3solver.cpp:127-137 (float epsilon, double log / pow)."""
    if min_inliers == n:
        its = 1.0
    else:
        eps = float(np.float32(np.float32(min_inliers) / np.float32(n)))
        with np.errstate(all="ignore"):
            its = np.ceil(np.log(1 - probability) / np.log(np.float64(1 - eps ** 3)))
    if not np.isfinite(its) or its < 1:
        return 1
    return int(max(1, min(its, max_its)))


# (n, fix_scale) of the scenarios the CPU tests and the sweep-count search run
SCENARIOS = [(100, True), (100, False), (64, True), (257, True), (40, False), (20, True)]
