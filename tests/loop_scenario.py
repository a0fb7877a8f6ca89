"""Inputs of the Sim3 matcher tests (SearchBySim3, SearchByProjection / Fuse with Scw) on the
kf_scenario keyframes: similarity poses, per-feature map point records from the stereo depths,
seeded flag vectors, sub-sampled keyframes."""
import numpy as np

import kf_scenario as KS


def scw(T, s):
    """Scw = s * [R | t] of a 4x4 f32 pose: what the loop closer's corrected Sim3 looks like."""
    S = np.eye(4, dtype=np.float32)
    S[:3, :3] = (np.float32(s) * T[:3, :3]).astype(np.float32)
    S[:3, 3] = (np.float32(s) * T[:3, 3]).astype(np.float32)
    return S


def mp_records(kf, T):
    """One FUSE_POINT record per feature of `kf` at pose T, unprojected from its stereo depth;
    skip = 1 where the feature has no depth (no map point)."""
    from slam_framework_amd.kfmatch import FUSE_POINT_DTYPE
    fx, fy, cx, cy, _ = KS.CAM
    sc = KS.levels_arrays()[0]
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Ow = KS.center(T).astype(np.float64)
    n = len(kf["desc"])
    rec = np.zeros(n, FUSE_POINT_DTYPE)
    for i in range(n):
        z = float(kf["depth"][i])
        if not z > 0:
            rec[i]["skip"] = 1
            continue
        kp = kf["kps"][i]
        Xw = R.T @ (np.array([(kp["x"] - cx) * z / fx, (kp["y"] - cy) * z / fy, z]) - t)
        d = float(np.linalg.norm(Xw - Ow))
        rec[i]["xyz"] = Xw
        rec[i]["normal"] = (Xw - Ow) / d
        rec[i]["max_dist"] = d * sc[kp["octave"]]
        rec[i]["min_dist"] = d * sc[kp["octave"]] / sc[-1]
        rec[i]["desc"] = kf["desc"][i]
    return rec


def relative_pose(T1, T2, s=1.0, rot_deg=0.0):
    """(s12, R12, t12) of S12 = T1 * T2^-1, optionally perturbed by a scale and a small rotation
    about the optical axis."""
    R1, t1 = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64)
    R2, t2 = T2[:3, :3].astype(np.float64), T2[:3, 3].astype(np.float64)
    a = np.deg2rad(rot_deg)
    dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    R12 = dR @ R1 @ R2.T
    t12 = t1 - R12 @ t2
    return np.float32(s), R12.astype(np.float32), t12.astype(np.float32)


def flags(n, frac, seed):
    return (np.random.default_rng(seed).random(n) < frac).astype(np.uint8)


def subsample(kf, n, seed=3):
    """`n` of the keyframe's features (ascending index, seeded choice)."""
    idx = np.sort(np.random.default_rng(seed).choice(len(kf["desc"]), n, replace=False))
    return {k: kf[k][idx] for k in ("kps", "desc", "ur", "depth")}
