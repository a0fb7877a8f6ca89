"""Sim3SolverCore (include/slamgpu_adapters.hpp) driven from C++ on the device
(tests/sim3solver_adapter_check.cpp, srand(1) and the default rand() functor) against the CPU
restatement fed the draws the program printed: the gather of sim3solver.cpp:64-105 with its skip
rules (no map point, a bad one on either side, GetIndexInKeyFrame < 0), the eager draws in the
reference's order, every iterate(5) outcome and the estimate it leaves."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import sim3solver_ref as R
import sim3solver_scenario as S

pytestmark = pytest.mark.gpu

N_KPS = 120
MIN_INLIERS = 20


def pose(rng):
    from slam_framework_amd import synthetic as syn
    T = np.eye(4)
    T[:3, :3] = syn._rodrigues(rng.normal(0, 0.3, 3))
    T[:3, 3] = rng.normal(0, 2.0, 3)
    return T.astype(np.float32)


def gemm_row(T, x):
    """cv::Mat R * X + t in f32: a float dot, then a double add (cv_gemm_row)."""
    T, x = np.asarray(T, np.float32), np.asarray(x, np.float32)
    out = np.zeros(3, np.float32)
    for r in range(3):
        dot = np.float32(np.float32(T[r, 0] * x[0] + T[r, 1] * x[1]) + T[r, 2] * x[2])
        out[r] = np.float32(np.float64(dot) + np.float64(T[r, 3]))
    return out


def make_scenario(seed, fix_scale):
    rng = np.random.default_rng(seed)
    n = 90
    c = S.candidate(seed, n, fix_scale)
    T1, T2 = pose(rng), pose(rng)
    inv1, inv2 = np.linalg.inv(T1.astype(np.float64)), np.linalg.inv(T2.astype(np.float64))
    m = c["matches"]
    xyz = np.zeros((2 * n, 3), np.float32)  # map points 0..n-1 are keyframe 1's, n..2n-1 keyframe 2's
    xyz[:n] = (m["x1c"].astype(np.float64) @ inv1[:3, :3].T + inv1[:3, 3])
    xyz[n:] = (m["x2c"].astype(np.float64) @ inv2[:3, :3].T + inv2[:3, 3])
    slot1 = rng.permutation(N_KPS)[:n]       # the keyframe-1 feature of pair p
    slot2 = rng.permutation(N_KPS)[:n]
    kps = [np.zeros((N_KPS, 3), np.float32) for _ in range(2)]
    for k in range(2):
        kps[k][:, 0] = rng.uniform(0, 1241, N_KPS)
        kps[k][:, 1] = rng.uniform(0, 376, N_KPS)
        kps[k][:, 2] = rng.integers(0, S.NLEVELS, N_KPS)
    kps[0][slot1, 2] = m["octave1"]
    kps[1][slot2, 2] = m["octave2"]
    mp1 = np.full(N_KPS, -1, np.int32)
    mp2 = np.full(N_KPS, -1, np.int32)
    mp1[slot1] = np.arange(n)
    mp2[slot2] = n + np.arange(n)
    matched = np.full(N_KPS, -1, np.int32)
    matched[slot1] = n + np.arange(n)
    bad = np.zeros(2 * n, np.int32)
    obs = [(p, 0, int(slot1[p])) for p in range(n)] + [(n + p, 1, int(slot2[p])) for p in range(n)]
    # the skip rules, on pairs 0..11
    mp1[slot1[0]] = mp1[slot1[1]] = -1              # no map point in keyframe 1 at a matched feature
    bad[2] = bad[3] = 1                             # pMP1 bad
    bad[n + 4] = bad[n + 5] = 1                     # pMP2 bad
    obs = [o for o in obs if o[0] not in (6, 7, n + 8, n + 9)]  # GetIndexInKeyFrame < 0
    # pMP1 observed at ANOTHER keypoint of keyframe 1 than the slot it is matched from: the
    # octave is that keypoint's (:83), the inlier flag goes to the slot (:94)
    other = int(np.setdiff1d(np.arange(N_KPS), slot1)[0])
    obs = [(10, 0, other) if o[0] == 10 else o for o in obs]
    kps[0][other, 2] = (m["octave1"][10] + 3) % S.NLEVELS
    matched[np.setdiff1d(np.arange(N_KPS), slot1)[1]] = n + 11   # matched where kf1 has no point
    return {"Tcw1": T1, "Tcw2": T2, "kps1": kps[0], "kps2": kps[1], "map_points1": mp1,
            "map_points2": mp2, "mp_xyz": xyz, "mp_bad": bad, "mp_obs": np.array(obs, np.int32),
            "matched12": matched, "K": c["K"], "sigma2": c["sigma2"],
            "fix_scale": np.array([int(fix_scale)]), "ransac": np.array([0.99, MIN_INLIERS, 300])}


def gather(sc):
    """sim3solver.cpp:64-105 restated on the scenario's arrays."""
    obs = {}
    for mp, kf, kp in sc["mp_obs"]:
        obs.setdefault((int(mp), int(kf)), int(kp))
    recs, idx1 = [], []
    for i1, m2 in enumerate(sc["matched12"]):
        if m2 < 0:
            continue
        m1 = sc["map_points1"][i1]
        if m1 < 0 or sc["mp_bad"][m1] or sc["mp_bad"][m2]:
            continue
        k1, k2 = obs.get((int(m1), 0), -1), obs.get((int(m2), 1), -1)
        if k1 < 0 or k2 < 0:
            continue
        r = np.zeros(1, R.MATCH_DTYPE)[0]
        r["x1c"] = gemm_row(sc["Tcw1"], sc["mp_xyz"][m1])
        r["x2c"] = gemm_row(sc["Tcw2"], sc["mp_xyz"][m2])
        r["octave1"] = int(sc["kps1"][k1, 2])
        r["octave2"] = int(sc["kps2"][k2, 2])
        recs.append(r)
        idx1.append(i1)
    return np.array(recs, R.MATCH_DTYPE), np.array(idx1)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_adapter_core_follows_the_restatement(gpu_lib, tmp_path, fix_scale):
    from slam_framework_amd import build
    exe = build.build_sim3solver_adapter_check()
    sc = make_scenario(40 + fix_scale, fix_scale)
    path = tmp_path / "scenario.json"
    path.write_text(json.dumps({k: np.asarray(v, np.float64).reshape(-1).tolist()
                                for k, v in sc.items()}))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    matches, idx1 = gather(sc)
    n = len(matches)
    assert n == 90 - 10   # pairs 0..9 are skipped; 10 stays with the other keypoint's octave
    n_its = S.ransac_iterations(n, 0.99, MIN_INLIERS, 300)
    assert lines[0] == f"n {n} n_its {n_its}"
    assert [int(x) for x in lines[1].split()[1:]] == list(idx1)
    draws = np.array([int(x) for x in lines[2].split()[1:]], np.int32)
    # the default functor: DUtils::Random::RandomInt on rand(), seeded as the program seeds it
    libc = C.CDLL(None)
    libc.srand(1)
    want = [gpu_lib.reference_random_int(0, n - 1 - i) for _ in range(n_its) for i in range(3)]
    assert list(draws) == want
    ref = R.Solver(matches, draws, n_its, MIN_INLIERS, fix_scale, sc["K"], sc["K"], sc["sigma2"],
                   sc["sigma2"], indices1=idx1, n1=N_KPS)
    calls = events = 0
    for line in lines[3:]:
        f = line.split()
        assert f[0] == "iterate" and f[5] == "best"
        k, no_more, vb, ni = ref.iterate(5)
        assert (int(f[1]), bool(int(f[2])), int(f[3])) == (k, no_more, ni), calls
        assert f[4] == "".join("1" if b else "0" for b in vb), calls
        b = ref.best()
        assert int(f[6]) == 1
        got = np.array([float(x) for x in f[7:20]], np.float32)
        assert np.array_equal(got[:9], b[0].reshape(-1)) and np.array_equal(got[9:12], b[1])
        assert got[12] == np.float32(b[2])
        calls += 1
        events += k >= 0
    assert no_more and events >= 1 and calls >= n_its // 5
