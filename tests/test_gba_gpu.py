"""Device global BundleAdjustment (Optimizer::BundleAdjustment, optimizer.cpp:33-207, on the
cooperative solver of slam_framework_amd/csrc/ba_coop.hip) against the oracle's FP64 restatement
(oracle/ba_oracle.c oc_global_bundle_adjustment_stop). Same tolerance as the local BA tests
(tests/test_ba_gpu.py): poses and points within 1e-5 x the largest delta + 4 f32 ulps, identical
LM iteration counts. Through the C ABI: slamgpu_global_bundle_adjustment."""
import ctypes

import numpy as np
import pytest

from slam_framework_amd import synthetic as S
from test_ba_gpu import assert_close

pytestmark = pytest.mark.gpu
CAM = S.KITTI_CAM


def gba_problem(seed, n_kf, n_points, **kw):
    """A map for the global BA: keyframe 0 fixed (id 0), every other keyframe optimised."""
    return S.ba_problem(seed, n_local=n_kf, n_fixed=0, n_points=n_points, first_local_fixed=True,
                        **kw)


def run(G, P, n_iterations=10, robust=True, stop=False):
    return G.Optimizer.BundleAdjustment(P["kf_Tcw"], P["kf_mode"], P["points"],
                                        P["point_obs_start"], P["obs"], CAM, P["inv_sigma2"],
                                        n_iterations=n_iterations, robust=robust, stop_flag=stop)


@pytest.mark.parametrize("seed,nkf,npt,robust,iters", [(31, 12, 1500, True, 10),
                                                       (32, 30, 4000, True, 10),
                                                       (33, 30, 4000, False, 20),
                                                       (34, 60, 6000, True, 10)])
def test_global_ba_matches_oracle(oracle, gpu_lib, seed, nkf, npt, robust, iters):
    P = gba_problem(seed, nkf, npt, spacing=0.8, outlier_frac=0.02)
    kf_o, pts_o, its_o = oracle.global_ba(CAM, P, iters, robust)
    kf, pts, its = run(gpu_lib, P, iters, robust)
    assert its == its_o
    assert_close(kf, kf_o, P["kf_Tcw"], "keyframe poses")
    assert_close(pts, pts_o, P["points"], "points")
    assert np.array_equal(kf[0], kf_o[0])  # the fixed keyframe: only the Converter round trip


@pytest.mark.parametrize("mwg,min_kf,seed,nkf,npt", [("1", "0", 37, 30, 4000),
                                                     ("1", "0", 38, 26, 3000),
                                                     ("0", "0", 39, 60, 6000),
                                                     ("1", "40", 40, 30, 4000)])
def test_global_ba_both_profile_factorisations(oracle, gpu_lib, monkeypatch, mwg, min_kf, seed,
                                               nkf, npt):
    """The profile LDLT over the whole grid (factor_profile_grid: block rows owned per
    work-group, one write-through hand-off per block column, replicated diagonal blocks) and
    work-group 0 alone (SLAMGPU_GBA_MWG=0, or below SLAMGPU_GBA_MWG_MIN_KF): both match the
    oracle."""
    monkeypatch.setenv("SLAMGPU_GBA_MWG", mwg)
    monkeypatch.setenv("SLAMGPU_GBA_MWG_MIN_KF", min_kf)
    P = gba_problem(seed, nkf, npt, spacing=0.8, outlier_frac=0.02)
    kf_o, pts_o, its_o = oracle.global_ba(CAM, P, 10, True)
    kf, pts, its = run(gpu_lib, P, 10, True)
    assert its == its_o
    assert_close(kf, kf_o, P["kf_Tcw"], "keyframe poses")
    assert_close(pts, pts_o, P["points"], "points")


def test_global_ba_profile_factorisations_equal_bit_for_bit(gpu_lib, monkeypatch):
    """factor_profile_grid and factor_solve_profile apply the same operations in the same order
    to every element (both are built from csrc/ba_ldlt.h's pieces), so the two runs agree bit for
    bit. 26 keyframes: the smallest window past the LDS solver, where both profile solvers run."""
    P = gba_problem(38, 26, 3000, spacing=0.8, outlier_frac=0.02)
    res = {}
    for mwg in ("1", "0"):
        monkeypatch.setenv("SLAMGPU_GBA_MWG", mwg)
        monkeypatch.setenv("SLAMGPU_GBA_MWG_MIN_KF", "0")
        res[mwg] = run(gpu_lib, P, 10, True)
    assert res["1"][2] == res["0"][2]
    assert np.array_equal(res["1"][0], res["0"][0]), "keyframe poses"
    assert np.array_equal(res["1"][1], res["0"][1]), "points"


def test_global_ba_unobserved_point_kept(oracle, gpu_lib):
    """A point without observations is not optimised (optimizer.cpp:149-152)."""
    P = gba_problem(35, 8, 400)
    st = P["point_obs_start"].copy()
    n3 = st[4] - st[3]  # drop point 3's observations
    P["obs"] = np.concatenate([P["obs"][:st[3]], P["obs"][st[4]:]])
    P["point_obs_start"] = np.concatenate([st[:4], st[4:] - n3]).astype(np.int32)
    kf_o, pts_o, its_o = oracle.global_ba(CAM, P, 10, True)
    kf, pts, its = run(gpu_lib, P)
    assert np.array_equal(pts[3], P["points"][3]) and np.array_equal(pts_o[3], P["points"][3])
    assert_close(pts, pts_o, P["points"], "points")


def test_global_ba_stop_before_start(oracle, gpu_lib):
    """A flag already raised: optimize() runs no iteration; the poses still take the Converter
    round trip of the write-back (optimizer.cpp:163-180), as in the oracle."""
    P = gba_problem(36, 6, 300)
    kf_o, pts_o, its_o = oracle.global_ba(CAM, P, 10, True, stop_after=0)
    kf, pts, its = run(gpu_lib, P, stop=ctypes.c_bool(True))
    assert its == its_o == 0
    assert np.array_equal(kf, kf_o) and np.array_equal(pts, pts_o)


@pytest.mark.parametrize("n_kf", [300, 1500, 2000])  # 2000: z past the back-solve LDS
def test_global_ba_map_scale_loop(oracle, gpu_lib, n_kf):
    """A map-scale global BA after a loop closure (GlobalBundleAdjustemnt passes every keyframe,
    optimizer.cpp:18-31): a closed loop of n_kf keyframes (synthetic.map_problem: ~38 points and
    ~230 observations per keyframe; the last keyframes co-observe the first ones, so the reduced
    camera system is a band plus rows reaching back to the start). The device factorises it in
    block-profile storage; the oracle's profile LDLT is its dense one with the exact zeros
    skipped. Poses and points within the tolerance of every BA test, identical LM counts."""
    P = S.map_problem(40 + n_kf, n_kf)
    kf_o, pts_o, its_o = oracle.global_ba(CAM, P, 10, True)
    kf, pts, its = run(gpu_lib, P, 10, True)
    assert its == its_o
    assert_close(kf, kf_o, P["kf_Tcw"], f"{n_kf}-keyframe loop poses")
    assert_close(pts, pts_o, P["points"], f"{n_kf}-keyframe loop points")


def test_local_ba_runs_beside_a_global_ba(oracle, gpu_lib):
    """The LocalMapper's LocalBundleAdjustment and the LoopCloser's global BA run on their own
    threads in the reference (local_mapper.cpp:53, loop_closer.cpp:77). Their coop solves share
    the device's residency budget (64 + 128 of 256 work-groups) instead of a lock, so a C5
    LocalBA started while a 1500-keyframe global BA is running finishes before it, and both match
    the oracle."""
    import threading
    import time
    G = gpu_lib
    PM = S.map_problem(1540, 1500)
    P5 = S.c5_problem(11)
    kf_m, pts_m, its_m = oracle.global_ba(CAM, PM, 10, True)
    kf_5, pts_5, er_5, its_5 = oracle.local_ba(CAM, P5)
    out, errors, t_end = {}, [], {}

    def gba():
        try:
            out["gba"] = run(G, PM, 10, True)
            t_end["gba"] = time.perf_counter()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    L = G.lib()
    assert L.slamgpu_coop_slots_in_use(0) == 0
    th = threading.Thread(target=gba)
    t0 = time.perf_counter()
    th.start()
    # the LocalBA starts once the global BA holds its residency slots (past its host staging, its
    # kernel launched or about to be): the two solves then overlap on the device
    while L.slamgpu_coop_slots_in_use(0) == 0 and th.is_alive():
        time.sleep(0.0005)
    held = L.slamgpu_coop_slots_in_use(0)
    observed = held > 0  # False: the global BA ended before a poll saw its slots
    t_lba0 = time.perf_counter()
    from test_ba_gpu import run_host
    r5 = run_host(G, P5)
    t_end["lba"] = time.perf_counter()
    th.join(timeout=60)
    assert not errors, errors
    print(f"global BA holds {held} slots; LocalBA started {1e3 * (t_lba0 - t0):.1f} ms after it, "
          f"ran {1e3 * (t_end['lba'] - t_lba0):.1f} ms; the global BA ended at "
          f"{1e3 * (t_end['gba'] - t0):.1f} ms")
    kf, pts, er, its = r5
    assert its == its_5 and np.array_equal(er, er_5)
    assert_close(kf, kf_5, P5["kf_Tcw"], "LocalBA poses beside a global BA")
    kf, pts, its = out["gba"]
    assert its == its_m
    assert_close(kf, kf_m, PM["kf_Tcw"], "global BA poses beside a LocalBA")
    assert_close(pts, pts_m, PM["points"], "global BA points beside a LocalBA")
    # the grid the global BA reserves is the device's co-resident work-group count
    # (optimizer_runtime.cpp coop_grid), not a fixed number: any slot held while the LocalBA
    # starts shows the two solves overlapping
    if not observed:
        pytest.skip("the global BA finished before a poll saw its residency slots: the overlap "
                    "was not observed (a timing window, not a failure)")
    assert t_end["lba"] < t_end["gba"], "the LocalBA waited for the global BA"
