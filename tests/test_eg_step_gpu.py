"""One linear step of OptimizeEssentialGraph (eg_products, eg_assemble and both variants of
eg_factor_solve_kernel, slam_framework_amd/csrc/eg_kernels.hip) and the small kernels around it,
run alone by tests/eg_step_check on the graphs of tests/eg_step_spec.py: the layer under the
Levenberg-Marquardt runs of test_eg_gpu.py, which forgive a wrong H or x as long as b is right.

contrib, H and b are compared for equality with an integer computation (the inputs are dyadic
rationals); x and the scale term with the 50-digit values of tests/golden/eg_step.npz within the
fixture's bounds (16 x the error of a plain float64 LDLT, floor 2^-52), never bounds taken from
the device's output.

One child process per group of classes. After a child fails or times out no further child is
started: the remaining tests of the module fail without touching the GPU.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import device_math_spec as DS
import eg_step_spec as ES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "eg_step_check")
GRAPHS = ES.graphs()
BY_NAME = {g["name"]: g for g in GRAPHS}
_results = {}
_dead = []  # the reason no further child may start
_expected = {}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "eg_step.npz")))


def group_records(group):
    """(keys, kinds, records) of one child: every graph of the group's classes with fix_scale 0
    and 1; the small group also carries the chi2 sums and the update / finish problem."""
    keys, kinds, recs = [], [], []
    for g in GRAPHS:
        if g["cls"] in ES.GROUPS[group]:
            for fs in (0, 1):
                keys.append((g["name"], fs))
                kinds.append(ES.REC_STEP)
                recs.append(ES.step_record(g, fs))
    if group == "small":
        for n in ES.CHI2_SIZES:
            keys.append(("chi2", n))
            kinds.append(ES.REC_CHI2)
            recs.append(ES.chi2_record(ES.chi2_values(n)))
        P = ES.update_problem()
        for fs in (0, 1):
            keys.append(("update", fs))
            kinds.append(ES.REC_UPDATE)
            recs.append(ES.update_record(P, fs))
    return keys, kinds, recs


def run_group(group, tmp):
    if group in _results:
        return _results[group]
    if _dead:
        pytest.fail(f"not run: {_dead[0]}")
    assert os.path.exists(EXE), "tests/eg_step_check is not built (slam_framework_amd.build)"
    keys, kinds, recs = group_records(group)
    fin, fout = os.path.join(tmp, group + ".in"), os.path.join(tmp, group + ".out")
    ES.write_case_file(fin, recs)
    try:
        p = subprocess.run([EXE, fin, fout], timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _dead.append(f"eg_step_check timed out on group {group}")
        pytest.fail(_dead[0])
    if p.returncode != 0:
        _dead.append(f"eg_step_check exited {p.returncode} on group {group}: {p.stderr[-500:]}")
        pytest.fail(_dead[0])
    _results[group] = dict(zip(keys, ES.read_result_file(fout, kinds)))
    os.remove(fin)
    os.remove(fout)
    return _results[group]


def group_of(cls):
    return next(g for g, cl in ES.GROUPS.items() if cls in cl)


def expected(g):
    """The integer reference of one graph, computed once and left unchanged."""
    if g["name"] not in _expected:
        st = ES.structure(g)
        _expected[g["name"]] = (st, ES.expected_contrib(g), *ES.expected_system(g, st))
        for a in _expected[g["name"]][1:]:
            a.setflags(write=False)
    return _expected[g["name"]]


@pytest.mark.parametrize("name", [g["name"] for g in GRAPHS])
def test_linear_step(name, fx, tmp_path_factory):
    g = BY_NAME[name]
    res = run_group(group_of(g["cls"]), str(tmp_path_factory.getbasetemp()))
    st, contrib, H, b = expected(g)
    F = st["F"]
    staged_expected = not ES.EXPECT[name][4]
    failure = g["cls"] == "failure"
    if not failure:
        c = list(fx["classes"]).index(g["cls"])
        bound_x, bound_s = float(fx["bound_x"][c]), float(fx["bound_scale"][c])
    for fs in (0, 1):
        r = res[(name, fs)]
        assert (r["F"], r["n_blocks"]) == (F, st["n_blocks"])
        # products and assembly: exact, and storage nothing writes still holds its pattern
        assert ES.same_bits_or_value(r["contrib"], contrib), \
            f"{name}: contrib differs at {np.argwhere(~((r['contrib'] == contrib) | np.isnan(contrib)))[:5]}"
        assert np.array_equal(r["H"], H), \
            f"{name}: H differs at blocks {np.flatnonzero((r['H'] != H).any(1))[:8]}"
        assert np.array_equal(r["b"], b), f"{name}: b differs at {np.flatnonzero(r['b'] != b)[:8]}"
        # which variant the launcher takes
        assert r["staged"] == int(staged_expected), \
            f"{name}: launcher chose staged = {r['staged']} for {ES.meta_bytes(st)} structure bytes"
        assert r["meta_bytes"] == (ES.meta_bytes(st) if staged_expected else 0)
        for l, lam in enumerate(g["lambdas"]):
            runs = r["solves"][l]
            assert sorted(runs) == sorted(["launcher", "global"] + ["staged"] * staged_expected)
            if failure:  # the isolated vertex's pivot is 0: x keeps the sentinel in every bit
                for way, o in runs.items():
                    assert o["ok"] == 0.0, f"{name}/{way}: ok = {o['ok']}"
                    assert (o["x"].view(np.uint64) ==
                            np.float64(ES.SENTINEL).view(np.uint64)).all(), f"{name}/{way}: x written"
                continue
            x_ref = fx[f"{name}/x_ref/{l}"].copy()
            if fs:
                x_ref[6::7] = 0.0
            s_ref = float(fx[f"{name}/scale/{l}"][fs])
            s_abs = float(fx[f"{name}/scale_abs/{l}"][fs])
            for way, o in runs.items():
                e_x = np.abs(o["x"] - x_ref).max() / np.abs(x_ref).max()
                e_s = abs(o["scale"] - s_ref) / s_abs
                print(f"{name} fix_scale {fs} lambda {lam:g} {way}: x error {e_x:.3g} (bound "
                      f"{bound_x:.3g}), scale error {e_s:.3g} (bound {bound_s:.3g})")
                assert o["ok"] == 1.0, f"{name}/{way}: ok = {o['ok']}"
                assert np.isfinite(o["x"]).all() and e_x <= bound_x, \
                    f"{name}/{way} lambda {lam:g}: x error {e_x:.3g} > {bound_x:.3g}, worst at " \
                    f"{int(np.abs(o['x'] - x_ref).argmax())}"
                assert e_s <= bound_s, f"{name}/{way} lambda {lam:g}: scale error {e_s:.3g}"
                if fs:
                    assert (o["x"][6::7].view(np.uint64) == 0).all(), f"{name}/{way}: scale rows"
            for way in runs:
                assert runs[way]["x"].tobytes() == runs["launcher"]["x"].tobytes(), \
                    f"{name} lambda {lam:g}: {way} and the launcher differ at " \
                    f"{np.flatnonzero(runs[way]['x'] != runs['launcher']['x'])[:8]}"


@pytest.mark.parametrize("n", ES.CHI2_SIZES)
def test_chi2_sum(n, tmp_path_factory):
    got = run_group("small", str(tmp_path_factory.getbasetemp()))[("chi2", n)]["sum"]
    v = ES.chi2_values(n)
    want = ES.chi2_sum_restated(v)
    exact = math.fsum(v)
    print(f"chi2 sum n = {n}: {got!r}, restated {want!r}, fsum {exact!r}")
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
    assert abs(got - exact) <= n * 2.0 ** -53 * math.fsum(np.abs(v))


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_update(fix_scale, fx, tmp_path_factory):
    """eg_update is sim3_exp then sim3_mul (the composition eg_oplus_axis is): its error may be
    the sum of the two bounds of tests/golden/device_math.npz, measured as eg_oplus_axis's."""
    r = run_group("small", str(tmp_path_factory.getbasetemp()))[("update", fix_scale)]
    P = ES.update_problem()
    dm = np.load(os.path.join(HERE, "golden", "device_math.npz"))
    bound = float(dm["sim3_exp/bound"][list(dm["sim3_exp/classes"]).index("generic")] +
                  dm["sim3_mul/bound"][list(dm["sim3_mul/classes"]).index("generic")])
    free = P["fixed"] == 0
    err = DS.case_errors("eg_oplus_axis", DS.comparable("eg_oplus_axis", r["S"]),
                         fx["update/ref"][fix_scale])
    print(f"eg_update fix_scale {fix_scale}: worst error {err[free].max():.3g} (bound {bound:.3g})")
    assert (err[free] <= bound).all(), f"vertex {int(err.argmax())}: {err.max():.3g}"
    assert r["S"][~free].tobytes() == P["S"][~free].tobytes(), "a fixed vertex moved"
    if fix_scale:
        assert (r["S"][:, 7] == P["S"][:, 7]).all()


def test_finish(fx, tmp_path_factory):
    res = run_group("small", str(tmp_path_factory.getbasetemp()))
    for fs in (0, 1):  # eg_finish does not depend on fix_scale
        r = res[("update", fs)]
        for what, got, want in (("Tcw", r["Tcw"], fx["finish/Tcw"]),
                                ("points", r["points"], fx["finish/points"])):
            got = got.astype(np.float32)
            assert got.shape == want.shape
            off = np.abs(got.astype(np.float64) - want.astype(np.float64))
            miss = got != want
            print(f"eg_finish {what}: {int(miss.sum())} of {miss.size} floats differ from the "
                  f"correctly rounded value")
            assert (off <= np.spacing(np.abs(want)).astype(np.float64)).all(), \
                f"{what}: more than 1 ulp at {np.argwhere(off > np.spacing(np.abs(want)))[:5]}"
            assert miss.sum() <= 0.01 * miss.size
        assert (r["Tcw"][:, 12:] == [0.0, 0.0, 0.0, 1.0]).all()
