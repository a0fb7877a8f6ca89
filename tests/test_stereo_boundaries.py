"""ComputeStereoMatches' comparisons, decided on the CPU: stereo_ref.py, a
plain restatement of frame.cpp:406-577 that shares nothing with oracle/ or csrc/, against
oc_stereo_match byte for byte, on the constructed pairs of stereo_boundary_scenario.py and on the
six image pairs of test_stereo_sad_gpu.py; every case's precondition; and the kill matrix: for
every rule of stereo_ref.RULES, the restatement with that one comparison replaced by its nearest
wrong variant changes u_right or depth at the keypoints designated for the rule. There are no
tolerances: every comparison is of bytes.

The reference's branches that no input reaches get no case but an assertion over every trace:
  maxU < 0 (:459) and iniu < 0 || endu >= cols (:513): keypoints lie at least 19 level pixels
      inside every level and maxU = uL >= 19; the window reaches 10 pixels from the keypoint.
  the kernel's extra ROI guard (stereo_match.hip, the line after endu): the same margin.
  deltaR < -1 || deltaR > 1 (:544): dist2 is the strict first minimum and the offsets beside
      it exist, so the denominator 2 ((d1 - d2) + (d3 - d2)) is positive and |d1 - d3| is at most
      half of it: |deltaR| <= 0.5, never NaN."""
import numpy as np
import pytest

import stereo_boundary_scenario as B
import stereo_ref as R
import test_stereo_sad_gpu as SAD

IMAGE_CASES = SAD.CASES  # pair, rolled, flipped, constant, noise, half: at 640 columns

_eval = {}


def evaluate(oracle, name):
    """Keypoints, descriptors and levels of both images from the oracle, the oracle's and the
    restatement's u_right / depth and the restatement's trace: computed once, never changed."""
    if name not in _eval:
        t = oracle.tables(*B.ORB)
        if name in B.CASES:
            left, right = B.CASES[name].images()
            fx, bf = B.CASES[name].camera
        else:
            left, right = SAD.images(640)[name]
            cam = SAD.camera(640)
            fx, bf = cam[0], cam[4]
        kl, dl, pl = oracle.extract(t, left, with_pyramid=True)
        kr, dr, pr = oracle.extract(t, right, with_pyramid=True)
        nlev = t.nlevels
        e = dict(t=t, left=left, right=right, fx=fx, bf=bf, kl=kl, dl=dl, kr=kr, dr=dr,
                 levels_l=[pl.level(l) for l in range(nlev)],
                 levels_r=[pr.level(l) for l in range(nlev)],
                 scale=list(t.scale)[:nlev], inv_scale=list(t.inv_scale)[:nlev])
        e["ur"], e["depth"], _ = oracle.stereo(t, kl, dl, kr, dr, pl, pr, fx, bf)
        e["ref_ur"], e["ref_depth"], e["trace"] = restate(e)
        _eval[name] = e
    return _eval[name]


def restate(e, rule=None):
    return R.stereo_matches(e["kl"], e["dl"], e["kr"], e["dr"], e["levels_l"], e["levels_r"],
                            e["scale"], e["inv_scale"], e["fx"], e["bf"], rule=rule)


@pytest.mark.parametrize("name", list(B.CASES) + list(IMAGE_CASES))
def test_restatement_equals_oracle(oracle, name):
    e = evaluate(oracle, name)
    assert e["ref_ur"].tobytes() == e["ur"].tobytes(), "u_right"
    assert e["ref_depth"].tobytes() == e["depth"].tobytes(), "depth"


@pytest.mark.parametrize("name", list(B.CASES))
def test_precondition(oracle, name):
    e = evaluate(oracle, name)
    B.check(B.CASES[name], e["kl"], e["dl"], e["kr"], e["dr"], e["ref_ur"], e["ref_depth"],
            e["trace"], e["scale"], e["inv_scale"])


def designated(rule):
    return [(c.name, s) for c in B.CASES.values() for s in c.sites if rule in s.rules]


def test_rule_list_is_whole():
    """The 21 rules of the survey less the differently rounded factor (no mutant of its own: the
    exact-integer thDist cases with a SAD equal to it stand for it), plus the band radius from the
    left keypoint's octave and uR0 scaled by the right keypoint's octave."""
    assert len(R.RULES) == 22
    for rule in R.RULES:
        assert designated(rule), f"no constructed case is designated for {rule}"
    for case, site in (("median10", "s21"), ("median10", "s20"), ("median40", "s84"),
                       ("median40", "s83")):
        assert B.CASES[case].site(site).expect["thDist"] == float(
            np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(
                B.CASES[case].site(site).expect["median"]))


@pytest.mark.parametrize("rule", list(R.RULES))
def test_kill_matrix(oracle, rule):
    """expected != alt at every keypoint designated for the rule, on constructed cases only."""
    for name, site in designated(rule):
        e = evaluate(oracle, name)
        iL = B.index_of(e["kl"], site.x, site.y, site.octave)
        ur, depth, _ = restate(e, rule)
        assert (ur[iL].tobytes(), depth[iL].tobytes()) != \
            (e["ref_ur"][iL].tobytes(), e["ref_depth"][iL].tobytes()), \
            f"{rule} survives {name}/{site.name}"


@pytest.mark.parametrize("name", list(B.CASES) + list(IMAGE_CASES))
def test_unreachable_branches(oracle, name):
    e = evaluate(oracle, name)
    for iL in range(len(e["kl"])):
        tr = e["trace"][iL]
        assert tr["stage"] not in ("maxU_negative", "window_outside", "deltaR_rejected"), (iL, tr)
        if "maxU" in tr:
            assert tr["maxU"] >= 19, (iL, tr["maxU"])
        if "iniu" in tr:
            assert tr["iniu"] >= 0 and tr["endu"] < tr["cols"] and tr["roi_ok"], (iL, tr)
        if "deltaR" in tr:
            assert np.isfinite(tr["deltaR"]) and abs(tr["deltaR"]) <= np.float32(0.5), (iL, tr)
