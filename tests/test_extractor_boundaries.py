"""ORBextractor's comparisons, decided on the CPU: extractor_ref.py, a numpy
restatement of orb_extractor.cpp:18-88, 351-411, 422-794, 985-1075 that shares nothing with
oracle/ or csrc/, against the oracle byte for byte (every pyramid level, the FAST candidates and
the octree output of every level, keypoints, descriptors) on the constructed images of
extractor_boundary_scenario.py and on synthetic.image(1000..1004); every case's precondition; and
the kill matrix: for every rule of extractor_ref.RULES, the restatement with that one comparison
replaced by its nearest wrong variant changes the keypoints or descriptors of a constructed case
designated for it (run with -s: the matrix is printed, every case a rule changes). There are no
tolerances: every comparison is of bytes.

The rules that no input reaches (extractor_ref.UNREACHABLE) get no case but an assertion of the
argument over every case and seed:
  cell_skip    a skipped cell is at most 6 wide or 3 high: FAST has no pixel to test in it
  resize_right_edge   for scale factors above 1 no destination column maps past the last source
      column but one: xmax == dw on every level
The blur's scalar tail (the last w % 4 columns, rounded half up) and its mirrored border are NOT
among them: the pattern's corner points (+-13, +-13) lie 18.4 pixels out, a keypoint lies 19 to
w - 20, so a sample reads columns 1 to w - 2 (asserted below as the bound); the case blur_border
decides both."""
import numpy as np
import pytest

import extractor_boundary_scenario as B
import extractor_ref as R

SEEDS = (1000, 1001, 1002, 1003, 1004)
KITTI = (2000, 1.2, 8, 20, 7)

_eval = {}


def evaluate(oracle, name):
    """Image, the oracle's levels / candidates / octree output / keypoints / descriptors and the
    restatement's keypoints, descriptors and trace: computed once, never changed."""
    if name not in _eval:
        if name in B.CASES:
            img, orb = B.CASES[name].image(), B.CASES[name].orb
        else:
            from slam_framework_amd import synthetic
            img, orb = synthetic.image(int(name)), KITTI
        t = oracle.tables(*orb)
        k, d, pyr = oracle.extract(t, img, with_pyramid=True)
        e = dict(img=img, orb=orb, t=t, k=k, d=d, levels=[], cand=[], octo=[])
        for l in range(t.nlevels):
            e["levels"].append(pyr.level(l))
            e["cand"].append(oracle.level_candidates(t, pyr, l))
            e["octo"].append(oracle.distribute_octree(t, pyr, l, e["cand"][-1]))
        e["rk"], e["rd"], e["trace"] = R.extract(orb, img)
        _eval[name] = e
    return _eval[name]


ALL = list(B.CASES) + [str(s) for s in SEEDS]


@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_oracle(oracle, name):
    e = evaluate(oracle, name)
    tr = e["trace"]
    assert [int(b) for b in e["t"].features_per_level[:e["t"].nlevels]] == tr["tables"].budget
    assert list(e["t"].umax[:16]) == tr["tables"].umax
    for l, lv in enumerate(e["levels"]):
        assert lv.tobytes() == tr["pyramid"][l].tobytes(), f"level {l}"
        K = tr["levels"][l]["candidates"]
        mine = np.array([c[:3] for c in K], np.float32).reshape(-1, 3)
        theirs = np.stack([e["cand"][l][f] for f in ("x", "y", "response")], 1)
        assert mine.tobytes() == theirs.tobytes(), f"FAST candidates of level {l}"
        kept = np.array([K[i][:3] for i in tr["levels"][l]["kept"]], np.float32).reshape(-1, 3)
        theirs = np.stack([e["octo"][l][f] for f in ("x", "y", "response")], 1)
        assert kept.tobytes() == theirs.tobytes(), f"octree output of level {l}"
    assert e["rk"].tobytes() == e["k"].tobytes(), "keypoints"
    assert e["rd"].tobytes() == e["d"].tobytes(), "descriptors"


def test_primitives_equal_oracle(oracle):
    """sincosf over [0, 2 pi) and fastAtan2 over small moments, sampled; both kept exact."""
    L = oracle.lib()
    rng = np.random.default_rng(1)
    for x in rng.uniform(0, 2 * np.pi, 2000).astype(np.float32):
        s, c = R.sincosf(x)
        assert s.tobytes() == np.float32(L.oc_sinf(float(x))).tobytes(), x
        assert c.tobytes() == np.float32(L.oc_cosf(float(x))).tobytes(), x
    for y, x in rng.integers(-400, 401, (2000, 2)):
        assert R.fast_atan2(y, x).tobytes() == \
            np.float32(L.oc_fast_atan2(float(y), float(x))).tobytes(), (y, x)


@pytest.mark.parametrize("name", list(B.CASES))
def test_precondition(oracle, name):
    e = evaluate(oracle, name)
    for check in B.CASES[name].expect:
        check(B.CASES[name], e["rk"], e["rd"], e["trace"])


def designated(rule):
    return [c.name for c in B.CASES.values() if rule in c.rules]


# the ten rules the random-image suite left undecided, by their names here
TABLE_ROWS = ("atan_branch", "atan_sign_x", "atan_sign_y", "desc_fma", "oct_expand_threshold",
              "oct_outer_finish", "nini_round", "blur_tail", "cell_skip", "resize_right_edge")


def test_rule_list_is_whole():
    for rule in TABLE_ROWS:
        assert rule in R.RULES
    for rule in R.RULES:
        assert bool(designated(rule)) != (rule in R.UNREACHABLE), rule
    for c in B.CASES.values():
        assert c.rules and all(r in R.RULES for r in c.rules), c.name


@pytest.mark.parametrize("rule", [r for r in R.RULES if r not in R.UNREACHABLE])
def test_kill_matrix(oracle, rule):
    """The wrong variant changes keypoints or descriptors on every case designated for the rule;
    the other constructed cases it changes are listed with them."""
    killed = []
    for name, c in B.CASES.items():
        e = evaluate(oracle, name)
        k, d, _ = R.extract(c.orb, e["img"], rule=rule)
        if k.tobytes() != e["rk"].tobytes() or d.tobytes() != e["rd"].tobytes():
            killed.append(name)
    where, right, wrong = R.RULES[rule]
    print(f"\n{rule} ({where}: {right} | {wrong}): {' '.join(killed)}")
    for name in designated(rule):
        assert name in killed, f"{rule} survives {name}"


@pytest.mark.parametrize("name", ALL)
def test_unreachable_rules(oracle, name):
    e = evaluate(oracle, name)
    tr = e["trace"]
    assert (R.PATTERN ** 2).sum(1).max() == 2 * 13 * 13  # 18.4 pixels: a sample reaches 18
    for t in tr["kp"]:
        w, h = tr["levels"][t["level"]]["w"], tr["levels"][t["level"]]["h"]
        assert t["reach"] <= 18
        assert 19 <= t["lx"] <= w - 20 and 19 <= t["ly"] <= h - 20, t
    for l, lv in enumerate(tr["levels"]):
        for cw, ch in lv["skipped_cells"]:
            assert (cw is None or cw <= 6) and (ch is None or ch <= 3), (l, cw, ch)
        if l:
            assert lv["xmax"] == lv["dw"], (l, lv["xmax"], lv["dw"])
    for rule in R.UNREACHABLE:  # and so the wrong variants change nothing
        k, d, _ = R.extract(e["orb"], e["img"], rule=rule)
        assert k.tobytes() == e["rk"].tobytes() and d.tobytes() == e["rd"].tobytes(), rule
