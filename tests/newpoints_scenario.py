"""Synthetic scenes for CreateNewMapPoints: a current keyframe and up to 3 neighbours that see the
same known 3-D points. Keypoints are the points' projections (optional pixel noise), octaves come
from the depth, a chosen subset is stereo (u_right / depth), descriptors are random 256-bit strings
with a controlled Hamming distance between views, and the FeatureVector is a small fake one (point
p sits in node p % n_nodes in every view). Keyframe dicts are those of newpoints_ref.py."""
import numpy as np

from newpoints_ref import KP_DTYPE

CAM = (718.856, 718.856, 607.1928, 185.2157, 386.1448)  # KITTI 00: fx fy cx cy bf
MB = float(np.float32(CAM[4]) / np.float32(CAM[0]))
NLEVELS = 8


def levels_arrays(scale_factor=1.2, nlevels=NLEVELS):
    sc = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        sc[i] = np.float32(float(sc[i - 1]) * float(np.float32(scale_factor)))
    return sc, (sc * sc).astype(np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(center, angles=(0.0, 0.0, 0.0)):
    """Tcw (f32) and Ow (f32) of a camera at `center` (world) with world-to-camera rotation
    rot(angles)."""
    R = rot(*angles)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R.astype(np.float32)
    T[:3, 3] = (-R @ np.asarray(center, np.float64)).astype(np.float32)
    Rf, tf = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    return T, (-Rf.T @ tf).astype(np.float32)


def fundamental(T1, T2, cam1=CAM, cam2=CAM):
    """LocalMapper::ComputeFundamentalMatrix: F12 = K1^-T [t12]x R12 K2^-1 (float64, stored f32)."""
    K = lambda c: np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]])  # noqa: E731
    R1, t1 = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64)
    R2, t2 = T2[:3, :3].astype(np.float64), T2[:3, 3].astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    return (np.linalg.inv(K(cam1)).T @ tx @ R12 @ np.linalg.inv(K(cam2))).astype(np.float32)


def world_points(n, seed, origin=(0.0, 0.0, 0.0), zmin=4.0, zmax=40.0, far_frac=0.1,
                 near_frac=0.03):
    """n points in front of a camera at `origin` looking down +z; far_frac of them beyond 150 m,
    near_frac closer than 0.25 m (behind a neighbour that has moved forward)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(zmin, zmax, n)
    far = rng.random(n) < far_frac
    z[far] = rng.uniform(150.0, 400.0, int(far.sum()))
    near = rng.random(n) < near_frac
    z[near] = rng.uniform(0.15, 0.25, int(near.sum()))
    u = rng.uniform(60.0, 1180.0, n)
    v = rng.uniform(30.0, 340.0, n)
    X = np.stack([(u - CAM[2]) * z / CAM[0], (v - CAM[3]) * z / CAM[1], z], 1)
    return X + np.asarray(origin, np.float64)


def view(X, T, Ow, desc, rng, stereo, noise=0.0, flips=6, mp_frac=0.0, n_nodes=8, perm=None,
         octave_shift=None, depth_scale=None, cam=CAM, mb=MB, along=None, O_ref=None):
    """A keyframe dict seeing the points X (world) from pose T. stereo: bool [n]; perm: keypoint i
    is point perm[i]; octave_shift / depth_scale: per-point disturbances of the octave and of the
    stereo measurement; along: per-point factor a that moves the keypoint along its epipolar line
    to p_inf + a (p - p_inf), p_inf the image of the point at infinity on the ray from O_ref
    (a = 1 the true place, a < 0 a point behind the cameras, 0 < a < 1 less parallax)."""
    n = len(X)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    R64, t64 = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Xc = (R64 @ X.T).T + t64
    Xc = Xc[perm]
    z = Xc[:, 2]
    u0, v0 = cam[0] * Xc[:, 0] / z + cam[2], cam[1] * Xc[:, 1] / z + cam[3]
    if along is not None:
        D = (R64 @ (X - np.asarray(O_ref, np.float64)).T).T[perm]
        ui, vi = cam[0] * D[:, 0] / D[:, 2] + cam[2], cam[1] * D[:, 1] / D[:, 2] + cam[3]
        a = np.asarray(along, np.float64)[perm]
        u0, v0 = ui + a * (u0 - ui), vi + a * (v0 - vi)
    u = u0 + noise * rng.standard_normal(n)
    v = v0 + noise * rng.standard_normal(n)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"] = u.astype(np.float32), v.astype(np.float32)
    kps["size"], kps["angle"], kps["response"] = 31.0, 0.0, 50.0
    octv = np.clip(np.floor(np.log(np.maximum(np.abs(z), 1e-3) / 4.0) / np.log(1.2)), 0, NLEVELS - 1)
    octv = (NLEVELS - 1 - octv).astype(np.int64)  # near points are seen at coarse levels
    if octave_shift is not None:
        octv = np.clip(octv + np.asarray(octave_shift)[perm], 0, NLEVELS - 1)
    kps["octave"] = octv.astype(np.int32)
    st = np.asarray(stereo, bool)[perm] & (z > 0)
    zs = z * (1.0 if depth_scale is None else np.asarray(depth_scale)[perm])
    ur = np.where(st, u - cam[4] / np.where(st, zs, 1.0), -1.0).astype(np.float32)
    depth = np.where(st, zs, -1.0).astype(np.float32)
    d = desc[perm].copy()
    for i in range(n):
        bits = rng.choice(256, flips, replace=False)
        for b in bits:
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    node_of = perm % n_nodes
    nodes = np.unique(node_of).astype(np.uint32)
    feats = [np.nonzero(node_of == nd)[0] for nd in nodes]
    start = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    fv = (nodes, start, (np.concatenate(feats) if n else np.zeros(0)).astype(np.uint32))
    mp = (rng.random(n) < mp_frac).astype(np.uint8)
    return dict(kps=kps, raw=None, desc=d, ur=ur, depth=depth, mp=mp, fv=fv, T=T, Ow=Ow, cam=cam,
                mb=mb)


NBOR_CENTERS = [(-0.9, 0.05, 0.1), (0.8, -0.1, 0.3), (0.1, 0.6, -0.4)]
NBOR_ANGLES = [(0.01, -0.02, 0.005), (-0.015, 0.02, 0.0), (0.0, 0.01, -0.01)]


def scene(n1, seed, n_nbors=1, kind="mixed", noise=0.3, origin=(0.0, 0.0, 0.0), skips=(),
          first_obs=(0, 1, 0), mp_frac=0.1, disturb=True, n2=None, centers=NBOR_CENTERS,
          n_nodes=8):
    """(cur, nbors) with nbors = [dict(kf, F12, skip, first_obs)]. kind: "mono" (no stereo
    keypoint), "stereo" (all) or "mixed" (each keypoint stereo with probability 1/2, drawn per
    view). disturb: 6 % of the points each get a wrong octave in the neighbours, a wrong stereo
    depth in the current keyframe, a wrong one in the neighbours, a neighbour keypoint mirrored
    through the vanishing point of its ray (triangulates behind the cameras) and one pulled towards
    it (too little parallax for the DLT). n2: the neighbours see only the first n2 points.
    centers: the neighbours' camera centres relative to the current keyframe's (more than three:
    the angles and first_obs repeat). n_nodes: the size of the fake FeatureVector."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, np.float64)
    X = world_points(n1, seed + 1, origin)
    desc = rng.integers(0, 256, (n1, 32), dtype=np.uint8)

    def stereo_mask():
        if kind == "mono":
            return np.zeros(n1, bool)
        if kind == "stereo":
            return np.ones(n1, bool)
        return rng.random(n1) < 0.5

    pick = rng.random((5, n1)) < (0.06 if disturb else 0.0)
    along = np.where(pick[3], -1.0, np.where(pick[4], 0.3, 1.0))
    oshift = np.where(pick[0], 4, 0)
    T1, O1 = pose(origin)
    cur = view(X, T1, O1, desc, rng, stereo_mask(), noise, mp_frac=mp_frac, n_nodes=n_nodes,
               depth_scale=np.where(pick[1], 1.6, 1.0))
    nbors = []
    m = n1 if n2 is None else n2
    for k in range(n_nbors):
        T2, O2 = pose(origin + np.asarray(centers[k], np.float64), NBOR_ANGLES[k % 3])
        perm = rng.permutation(m)
        kf = view(X[:m], T2, O2, desc[:m], rng, stereo_mask()[:m], noise, perm=perm, n_nodes=n_nodes,
                  octave_shift=oshift[:m], depth_scale=np.where(pick[2], 0.6, 1.0)[:m],
                  along=along[:m], O_ref=O1)
        nbors.append(dict(kf=kf, F12=fundamental(T1, T2), skip=int(k in skips),
                          first_obs=int(first_obs[k % len(first_obs)])))
    return cur, nbors


# ---- constructed single-keypoint pairs -----------------------------------------------------------

def one_kf(T, Ow, xy, octave=2, ur=-1.0, depth=-1.0, cam=CAM, mb=MB, desc_byte=0):
    """A keyframe with one keypoint at xy (one FeatureVector node, no map point)."""
    kps = np.zeros(1, KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = xy[0], xy[1], octave
    return dict(kps=kps, raw=None, desc=np.full((1, 32), desc_byte, np.uint8),
                ur=np.array([ur], np.float32), depth=np.array([depth], np.float32),
                mp=np.zeros(1, np.uint8),
                fv=(np.zeros(1, np.uint32), np.array([0, 1], np.int32), np.zeros(1, np.uint32)),
                T=np.asarray(T, np.float32), Ow=np.asarray(Ow, np.float32), cam=cam, mb=mb)


def project(T, X, cam=CAM):
    Xc = T[:3, :3].astype(np.float64) @ np.asarray(X, np.float64) + T[:3, 3].astype(np.float64)
    return cam[0] * Xc[0] / Xc[2] + cam[2], cam[1] * Xc[1] / Xc[2] + cam[3], Xc[2]


def wide_pair(X=(1.0, 0.5, 10.0), st1=False, st2=False, center2=(-0.9, 0.05, 0.1),
              angles2=(0.01, -0.02, 0.005), octave=2):
    """Two cameras 0.9 m apart seeing X exactly: the DLT geometry."""
    T1, O1 = pose((0, 0, 0))
    T2, O2 = pose(center2, angles2)
    u1, v1, z1 = project(T1, X)
    u2, v2, z2 = project(T2, X)
    k1 = one_kf(T1, O1, (u1, v1), octave, u1 - CAM[4] / z1 if st1 else -1.0, z1 if st1 else -1.0)
    k2 = one_kf(T2, O2, (u2, v2), octave, u2 - CAM[4] / z2 if st2 else -1.0, z2 if st2 else -1.0)
    return k1, k2


def with_(k, **kw):
    """A copy of the one-keypoint keyframe k with fields replaced: x, y, octave of the keypoint,
    ur, depth, or any key of the dict."""
    k = dict(k)
    for name, v in kw.items():
        if name in ("x", "y", "octave"):
            k["kps"] = k["kps"].copy()
            k["kps"][name] = v
        elif name in ("ur", "depth"):
            k[name] = np.array([v], np.float32)
        else:
            k[name] = v
    return k


def degenerate_pose_pair():
    """Two `poses` whose rotation blocks have a zero third column (no rotation matrices): column
    2 of the DLT matrix is zero, its null vector is (0, 0, 1, 0) and x3D(3) == 0 exactly (:387)."""
    T1 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0.5, 0, 1], [0, 0, 0, 1]], np.float32)
    T2 = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0.5, 0, 0, 1], [0, 0, 0, 1]], np.float32)
    cam = (100.0, 100.0, 0.0, 0.0, 50.0)
    return (one_kf(T1, (0, 0, 0), (20.0, 10.0), cam=cam, mb=0.5),
            one_kf(T2, (1, 0, 0), (20.0, 10.0), cam=cam, mb=0.5))
