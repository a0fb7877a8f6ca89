"""Pins the OptimizeEssentialGraph restatement (oracle/eg_oracle.c) without the reference binary
(g2o needs Eigen3, absent here): EdgeSim3's numeric Jacobians against an independent coarser
difference, a consistent (noise-free) loop closing exactly onto the truth with the loop keyframe
fixed, a noisy graph ending at a stationary point of its chi2, the scale staying 1 when fixed,
and the map point correction of optimizer.cpp:933-959."""
import numpy as np
import pytest

import oracle_lib as O
from slam_framework_amd import synthetic as S


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()


def _mat(S8):
    return S._sim3_mat(np.asarray(S8))


def test_edge_jacobians():
    Scw, fixed, E, St, _ = S.essential_graph_problem(3, 20, fix_scale=False)
    for k in range(0, len(E), 7):
        i, j, M = int(E[k]["i"]), int(E[k]["j"]), E[k]["Sji"]
        c, e, Ji, Jj = O.sim3_edge_eval(Scw[i], Scw[j], M)
        assert np.isclose(c, e @ e)
        h = 1e-6
        for d in range(7):
            u = np.zeros(7)
            u[d] = h
            for which, J in ((0, Ji), (1, Jj)):
                Sp = [Scw[i].copy(), Scw[j].copy()]
                Sm = [Scw[i].copy(), Scw[j].copy()]
                Sp[which] = O.sim3_mul(O.sim3_exp(u), Sp[which])
                Sm[which] = O.sim3_mul(O.sim3_exp(-u), Sm[which])
                _, ep, _, _ = O.sim3_edge_eval(Sp[0], Sp[1], M)
                _, em, _, _ = O.sim3_edge_eval(Sm[0], Sm[1], M)
                # g2o's 2e-9 differences carry ~1e-16 / 2e-9 x |t| of rounding noise
                np.testing.assert_allclose(J[:, d], (ep - em) / (2 * h), rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_consistent_loop_closes_to_truth(fix_scale):
    Scw, fixed, E, St, _ = S.essential_graph_problem(5, 40, fix_scale=fix_scale, meas_noise=0.0)
    S1, T1, its = O.optimize_essential_graph(Scw, fixed, E, fix_scale=fix_scale)
    assert its > 0
    for k in range(len(St)):
        np.testing.assert_allclose(_mat(S1[k]), _mat(St[k]), atol=2e-6)
    np.testing.assert_array_equal(S1[fixed == 1], Scw[fixed == 1])
    if fix_scale:
        np.testing.assert_array_equal(S1[:, 7], Scw[:, 7])
    # pose recovery [R t/s]
    M = _mat(S1[7])
    np.testing.assert_allclose(T1[7][:3, 3], M[:3, 3] / S1[7][7], rtol=1e-6, atol=1e-5)


def _chi2(Sv, E):
    tot = 0.0
    for e in E:
        c, _, _, _ = O.sim3_edge_eval(Sv[e["i"]], Sv[e["j"]], e["Sji"])
        tot += c
    return tot


def test_noisy_graph_reaches_stationary_point():
    Scw, fixed, E, St, _ = S.essential_graph_problem(6, 30, fix_scale=True, meas_noise=0.002)
    chi0 = _chi2(Scw, E)
    S1, _, its = O.optimize_essential_graph(Scw, fixed, E, fix_scale=True)
    chi1 = _chi2(S1, E)
    assert chi1 < 0.1 * chi0
    # a further tiny move of any free vertex does not lower the chi2 beyond first order
    rng = np.random.default_rng(0)
    for _ in range(5):
        k = int(rng.integers(0, len(S1)))
        if fixed[k]:
            continue
        u = np.concatenate([rng.normal(0, 1e-4, 6), [0.0]])
        Sp = S1.copy()
        Sp[k] = O.sim3_mul(O.sim3_exp(u), S1[k])
        assert _chi2(Sp, E) >= chi1 - 1e-10


def test_reference_graph_runs_and_lowers_chi2():
    """The reference's own measurements (drifted / corrected estimates): the loop error is
    spread over the graph."""
    Scw, fixed, E, _, _ = S.essential_graph_problem(7, 50, fix_scale=True, old_loop=(30, 12))
    chi0 = _chi2(Scw, E)
    S1, _, its = O.optimize_essential_graph(Scw, fixed, E)
    assert _chi2(S1, E) < chi0 and its > 0


def test_large_tight_case_is_a_fixed_point_of_the_oracle():
    """What makes (12, 130, True, None, (100, 30)) the large case of tests/test_eg_gpu.py's tight
    tolerance: a second oracle run started from the first one's result moves nothing, so where
    the LM stop rule ends the run is not in question. Seed 12 is the smallest of seeds 7 .. 26 of
    which that holds at 130 keyframes with the reference's own measurements; the issue-sized
    (7, 200, True, None, (150, 40)) is not such a case."""
    def moved(seed, n, old):
        Scw, fixed, E, _, _ = S.essential_graph_problem(seed, n, fix_scale=True, old_loop=old)
        S1, _, its = O.optimize_essential_graph(Scw, fixed, E, fix_scale=True)
        S2, _, _ = O.optimize_essential_graph(S1, fixed, E, fix_scale=True)
        assert its > 0
        return np.abs(S2 - S1).max()

    assert moved(12, 130, (100, 30)) == 0.0
    assert all(moved(seed, 130, (100, 30)) > 0.0 for seed in range(7, 12))
    assert moved(7, 200, (150, 40)) > 1e-5


def test_correct_points():
    rng = np.random.default_rng(2)
    Sb = np.stack([O.sim3_exp(np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 2, 3),
                                              [rng.normal(0, 0.2)]])) for _ in range(5)])
    Sa = np.stack([O.sim3_exp(np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 2, 3),
                                              [rng.normal(0, 0.2)]])) for _ in range(5)])
    ref = rng.integers(0, 5, 100).astype(np.int32)
    P = rng.normal(0, 10, (100, 3)).astype(np.float32)
    Q = O.correct_points_sim3(Sb, Sa, ref, P)
    for p in range(100):
        M = np.linalg.inv(_mat(Sa[ref[p]])) @ _mat(Sb[ref[p]])
        np.testing.assert_allclose(Q[p], (M @ np.append(P[p].astype(np.float64), 1))[:3],
                                   rtol=1e-5, atol=1e-4)
