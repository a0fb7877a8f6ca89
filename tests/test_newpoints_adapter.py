"""compute_fundamental_matrix and create_new_map_points of include/slamgpu_adapters.hpp, driven
from C++ (tests/newpoints_adapter_check.cpp): the fundamental matrix against a float64 numpy
value and against the Python binding bit for bit (no GPU); the baseline skips and the NewPoint
actions in the reference's order against the CPU chain (GPU)."""
import subprocess

import numpy as np
import pytest

import newpoints_ref as R
import newpoints_scenario as NS

SC, S2 = NS.levels_arrays()
NEW_POINT_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("kf1", "<i4"), ("idx1", "<i4"), ("kf2", "<i4"),
                            ("idx2", "<i4"), ("desc", "u1", (32,)), ("normal", "<f4", (3,)),
                            ("min_dist", "<f4"), ("max_dist", "<f4"), ("source", "<i4")])
assert NEW_POINT_DTYPE.itemsize == 84

POSES = [((0, 0, 0), (0, 0, 0), (-0.9, 0.05, 0.1), (0.01, -0.02, 0.005)),
         ((3.0, -1.0, 7.0), (0.02, 0.3, -0.01), (3.6, -1.1, 7.4), (0.0, 0.25, 0.02)),
         ((100.0, 5.0, -300.0), (0.0, 1.2, 0.0), (100.5, 5.0, -299.0), (0.01, 1.25, 0.0)),
         ((-577.4, 577.4, 577.4), (-0.1, -2.0, 0.05), (-578.0, 577.0, 578.4), (-0.1, -2.05, 0.05))]
CAM2 = (707.09, 709.3, 601.9, 183.1, 379.8)

# The largest deviation of F12 from the float64 value of the same float32 poses and cameras over
# POSES, relative to the largest entry of F12, measured with
#   python -m pytest tests/test_newpoints_adapter.py -k fundamental -s
# and the bound: 4 x that (the cases are fixed; the float32 roundings of the five products and
# the two inverses are the only slack).
FMAT_MEASURED = 4.3e-5
FMAT_BOUND = 4 * FMAT_MEASURED


@pytest.fixture(scope="module")
def exe():
    from slam_framework_amd import build
    build.build()
    return build.build_newpoints_adapter_check()


def f64_fundamental(T1, T2, cam1, cam2):
    K = lambda c: np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]], np.float64)  # noqa: E731
    c1, c2 = np.asarray(cam1, np.float32), np.asarray(cam2, np.float32)
    R1, t1 = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64)
    R2, t2 = T2[:3, :3].astype(np.float64), T2[:3, 3].astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    return np.linalg.inv(K(c1).T) @ tx @ R12 @ np.linalg.inv(K(c2))


def test_fundamental_matrix(exe, tmp_path):
    from slam_framework_amd import kfmatch as K
    worst = 0.0
    for c1, a1, c2, a2 in POSES:
        T1, _ = NS.pose(c1, a1)
        T2, _ = NS.pose(c2, a2)
        np.concatenate([T1.reshape(-1), T2.reshape(-1)]).astype(np.float32).tofile(
            tmp_path / "poses.f32")
        np.array(NS.CAM + CAM2, np.float32).tofile(tmp_path / "cams.f32")
        subprocess.run([exe, "fmat", str(tmp_path)], check=True, timeout=60)
        F = np.fromfile(tmp_path / "F12.f32", np.float32).reshape(3, 3)
        assert F.tobytes() == K.compute_fundamental_matrix(T1, T2, NS.CAM, CAM2).tobytes()
        F64 = f64_fundamental(T1, T2, NS.CAM, CAM2)
        worst = max(worst, float(np.abs(F - F64).max() / np.abs(F64).max()))
        # a point and its image in the other view satisfy the epipolar constraint
        X = np.array(c1, np.float64) + np.linalg.inv(T1[:3, :3].astype(np.float64)) @ [0.4, -0.2, 9.0]
        p = []
        for T, cam in ((T1, NS.CAM), (T2, CAM2)):
            Xc = T[:3, :3].astype(np.float64) @ X + T[:3, 3].astype(np.float64)
            p.append(np.array([cam[0] * Xc[0] / Xc[2] + cam[2], cam[1] * Xc[1] / Xc[2] + cam[3], 1]))
        line = F64.T @ p[0]
        assert abs(p[1] @ line) / np.hypot(line[0], line[1]) < 1e-2
    print(f"fundamental matrix: largest relative deviation {worst:.3e}, bound {FMAT_BOUND:.3e}")
    assert worst <= FMAT_BOUND


def write_scene(d, cur, nbors, mono, median):
    kfs = [cur] + [nb["kf"] for nb in nbors]
    n_nb = len(nbors)
    np.array([len(kfs), int(mono), n_nb] + list(range(1, 1 + n_nb)) +
             [nb["first_obs"] for nb in nbors], np.int32).tofile(d / "params.i32")
    np.asarray(median, np.float32).tofile(d / "median.f32")
    for i, k in enumerate(kfs):
        b = str(d / f"kf{i}")
        k["kps"].tofile(b + "_kps.bin")
        k["desc"].tofile(b + "_desc.u8")
        k["ur"].astype(np.float32).tofile(b + "_ur.f32")
        k["depth"].astype(np.float32).tofile(b + "_depth.f32")
        np.where(k["mp"] > 0, 7, -1).astype(np.int32).tofile(b + "_mp.i32")
        k["fv"][0].astype(np.uint32).tofile(b + "_nodes.u32")
        k["fv"][1].astype(np.int32).tofile(b + "_start.i32")
        k["fv"][2].astype(np.uint32).tofile(b + "_feats.u32")
        np.concatenate([np.asarray(k["T"], np.float32).reshape(-1), np.asarray(k["Ow"], np.float32),
                        np.asarray(k["cam"], np.float32), [np.float32(k["mb"])]]).astype(
                            np.float32).tofile(b + "_pose.f32")


@pytest.mark.gpu
@pytest.mark.parametrize("mono", [False, True])
def test_create_new_map_points_actions(exe, tmp_path, mono):
    """Stereo: the second neighbour is 0.3 m away, closer than mb = 0.54 m, and is skipped
    (:300-304). Monocular: the third neighbour's median depth is 200 times its baseline and it is
    skipped (:294-299). The NewPoint actions are the chain's, with F12 from
    compute_fundamental_matrix and OrbMatcher(0.6f, false)'s check_ori = false."""
    from slam_framework_amd import kfmatch as K
    centers = [(-0.9, 0.05, 0.1), (0.3, 0.0, 0.0), (0.1, 0.6, -0.4)]
    cur, nbors = NS.scene(300, 71, 3, "mono" if mono else "mixed", centers=centers)
    base = [float(np.float32(np.sqrt(sum(float(np.float32(a) - np.float32(b)) ** 2 for a, b in
                                         zip(nb["kf"]["Ow"], cur["Ow"]))))) for nb in nbors]
    median = [10.0, 10.0, 200.0 * base[2]]
    skips = [b / m < 0.01 for b, m in zip(base, median)] if mono else [b < NS.MB for b in base]
    assert skips == ([False, False, True] if mono else [False, True, False])
    for nb, s in zip(nbors, skips):
        nb["skip"] = int(s)
        nb["F12"] = K.compute_fundamental_matrix(cur["T"], nb["kf"]["T"], cur["cam"], nb["kf"]["cam"])
    ref = R.newpoints_chain(cur, nbors, SC, S2, check_ori=False)
    assert ref["n_new"] > 100
    write_scene(tmp_path, cur, nbors, mono, median)
    r = subprocess.run([exe, "chain", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["n_new", str(ref["n_new"]), "skipped", "1"]
    pts = np.fromfile(tmp_path / "points.bin", NEW_POINT_DTYPE)
    np.testing.assert_array_equal(np.fromfile(tmp_path / "skipped.u8", np.uint8), skips)
    np.testing.assert_array_equal(np.fromfile(tmp_path / "status.i8", np.int8).reshape(3, -1),
                                  ref["status"])
    for f in ("xyz", "normal", "min_dist", "max_dist", "desc"):
        np.testing.assert_array_equal(pts[f], ref["points"][f], err_msg=f)
    np.testing.assert_array_equal(pts["kf1"], 0)
    np.testing.assert_array_equal(pts["kf2"], 1 + ref["news"]["neighbour"])
    for f in ("idx1", "idx2", "source"):
        np.testing.assert_array_equal(pts[f], ref["news"][f], err_msg=f)
    # the reference's order: neighbour by neighbour, ascending idx1 within one
    assert (np.diff(pts["kf2"]) >= 0).all()
    for k in set(pts["kf2"]):
        assert (np.diff(pts["idx1"][pts["kf2"] == k]) > 0).all()
