"""Pins tests/initmatch_ref.c (the CPU restatement of OrbMatcher::SearchForInitialization,
src/orb_features/orb_matcher.cpp:264-382) on the CPU: against a plain-Python model of the loop
(brute-force window, no cell walk) on the scenario of test_initmatch_gpu.py, and with the
constructed cases of initmatch_scenario.py, whose expected outputs follow from the cited lines.
No GPU. Parity against the reference binary is unpinned (see the header of initmatch_ref.c).

Scenario counts measured with the restatement (F1 = frame 0, 436 level-0 queries of 2004,
nnratio 0.9; test_scenario_counts prints them). windowSize 100, frames 0 -> 1: 184 matches
without and 180 with the orientation check (4 removals), 3 take-overs, 3008 candidates skipped by
rule 4, at most 59 candidates per query; 0 -> 2 with the returned vbPrevMatched: 150 / 139 matches
(11 removals), 3 take-overs. windowSize 30: 185 / 181 matches (2 take-overs, 4 removals), then
143 / 141. At 4000 features (870 level-0 queries): 373 / 358 matches, 12 take-overs, 15 removals,
at most 106 candidates per query."""
import os
import subprocess

import numpy as np
import pytest

import initmatch_scenario as IS


@pytest.fixture(scope="module")
def world(oracle):
    import initmatch_ref
    initmatch_ref.lib()
    t, _, _, fr = IS.frames(oracle)
    grid = oracle.grid_geom(IS.W, IS.H)

    def ref(f2, q, nnratio, window, ori, prev):
        return initmatch_ref.search_for_initialization(f2["kl"], f2["dl"], grid, q, nnratio,
                                                       window, ori, prev)

    def both(f2, q, nnratio, window, ori, prev):
        a = ref(f2, q, nnratio, window, ori, prev)
        b = IS.py_search(f2["kl"], f2["dl"], q, nnratio, window, ori, prev)
        assert a[0] == b[0] and a[4] == b[4], (a[0], b[0], a[4], b[4])
        np.testing.assert_array_equal(a[1], b[1])
        assert a[2].tobytes() == b[2].tobytes()
        np.testing.assert_array_equal(a[3], b[3])
        return a
    return fr, ref, both


@pytest.mark.parametrize("window", [100, 30])
@pytest.mark.parametrize("check_ori", [0, 1])
def test_scenario_matches_python(world, window, check_ori):
    """Frames 0 -> 1, then 0 -> 2 with the vbPrevMatched the first call returned."""
    fr, ref, both = world
    q, prev0 = IS.f1_queries(fr[0])
    nm, m12, prev1, ak, cnt = both(fr[1], q, 0.9, window, check_ori, prev0)
    print(f"0->1 window {window} ori {check_ori}: nmatches {nm} {cnt}")
    assert nm == int((m12 >= 0).sum())
    assert (m12[q["octave"] > 0] == -1).all()
    held = m12 >= 0
    assert (prev1[~held] == prev0[~held]).all()
    np.testing.assert_array_equal(prev1[held, 0], fr[1]["kl"]["x"][m12[held]])
    assert len(set(m12[held])) == int(held.sum())                 # one query per keypoint
    if window == 100:
        assert nm >= 100                                          # tracker.cpp:331
        assert cnt["takeovers"] >= 1 and cnt["skipped"] >= 1
        assert cnt["removed"] >= 1 if check_ori else cnt["removed"] == 0
    nm2, m12b, prev2, _, cnt2 = both(fr[2], q, 0.9, window, check_ori, prev1)
    print(f"0->2 window {window} ori {check_ori}: nmatches {nm2} {cnt2}")
    assert nm2 == int((m12b >= 0).sum())


def test_constructed_cases(world):
    fr, ref, both = world
    f2 = fr[1]
    cs = IS.cases(f2["kl"], f2["dl"])
    assert len(cs) == 13
    for c in cs:
        nm, m12, prev, ak, cnt = both(f2, c.queries, c.nnratio, c.window, c.check_ori, c.prev0)
        c.check(f2["kl"], nm, m12, prev, cnt)
    by = {c.name: c for c in cs}
    # a ratio above 1 and below: the same tie, two outcomes
    assert (by["ratio_0.9"].want12[2] == -1) and by["ratio_1.5_tie_goes_to_the_first"].want12[0] >= 0
    # the rescan case keeps more candidates than the device scan does
    c = by["kept_candidates_all_held"]
    assert len(c.queries) == 7 and c.want12[6] not in c.want12[:6]


def test_accept_keypoint_is_kept_after_a_take_over(world):
    """accept_kp (the restatement's diagnostic) is the keypoint at accept time, whatever happens
    to the match later."""
    fr, ref, both = world
    f2 = fr[1]
    c = {x.name: x for x in IS.cases(f2["kl"], f2["dl"])}["take_over"]
    nm, m12, prev, ak, cnt = ref(f2, c.queries, c.nnratio, c.window, c.check_ori, c.prev0)
    assert list(m12) == [-1, ak[1]] and ak[0] == ak[1] >= 0


def test_empty_inputs(world, oracle):
    """n1 = 0; an F2 without a level-0 keypoint; an F2 without keypoints."""
    fr, ref, both = world
    q, prev0 = IS.f1_queries(fr[0])
    nm, m12, prev, ak, cnt = both(fr[1], q[:0], 0.9, 100, 1, prev0[:0])
    assert nm == 0 and len(m12) == 0
    up = fr[1]["kl"]["octave"] > 0
    f2 = dict(kl=fr[1]["kl"][up], dl=fr[1]["dl"][up])
    nm, m12, prev, ak, cnt = both(f2, q, 0.9, 100, 1, prev0)
    assert nm == 0 and (m12 == -1).all() and prev.tobytes() == prev0.tobytes()
    f2 = dict(kl=fr[1]["kl"][:0], dl=fr[1]["dl"][:0])
    nm, m12, prev, ak, cnt = both(f2, q, 0.9, 100, 0, prev0)
    assert nm == 0 and (m12 == -1).all() and prev.tobytes() == prev0.tobytes()


def test_scenario_counts(world, oracle):
    """The counts the docstrings quote, at 2000 and 4000 features (restatement only)."""
    import initmatch_ref
    grid = oracle.grid_geom(IS.W, IS.H)
    for nf in (2000, 4000):
        _, _, _, fr = IS.frames(oracle, nf)
        q, prev0 = IS.f1_queries(fr[0])
        for ori in (0, 1):
            nm, m12, prev1, _, cnt = initmatch_ref.search_for_initialization(
                fr[1]["kl"], fr[1]["dl"], grid, q, 0.9, 100, ori, prev0)
            print(f"nfeatures {nf} level-0 queries {int((q['octave'] == 0).sum())} ori {ori}: "
                  f"nmatches {nm} {cnt}")
            assert nm >= 100 and nm == int((m12 >= 0).sum())


def test_restatement_is_clean_under_the_sanitizers(tmp_path):
    """initmatch_ref.c with its own main (INITMATCH_REF_MAIN) and the oracle sources it calls,
    built with the address and undefined-behaviour sanitizers and run as a program; the runtimes
    are linked statically, so it runs as it is whatever else is preloaded."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "initmatch_sanitizer_check")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-Wno-unused-parameter", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-DINITMATCH_REF_MAIN", os.path.join(root, "tests", "initmatch_ref.c"),
                    os.path.join(root, "oracle", "matcher_oracle.c"),
                    os.path.join(root, "oracle", "cv_semantics.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 4, r.stdout + r.stderr
    assert not r.stderr.strip(), r.stderr
    assert "take-overs 0" not in r.stdout and "removed 0" not in r.stdout.splitlines()[1]
