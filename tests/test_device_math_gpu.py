"""The optimizers' device helpers against the 50-digit fixture (tests/golden/device_math.npz): the
layer under the Levenberg-Marquardt runs the other optimizer tests compare. tests/device_math_check
runs each helper one case per thread; one child process per operation group. Bounds come from
the fixture (16 x the float64 baseline's own error, or the fixed 2 ulps / exact rules), never
from the device's output.

After a child fails or times out no further child is started: the remaining tests of the module
fail without touching the GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import device_math_spec as DS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "device_math_check")
_results = {}
_dead = []  # the reason no further child may start


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "device_math.npz")))


def run_group(group, fx, tmp):
    if group in _results:
        return _results[group]
    if _dead:
        pytest.fail(f"not run: {_dead[0]}")
    assert os.path.exists(EXE), "tests/device_math_check is not built (slam_framework_amd.build)"
    ops = DS.GROUPS[group]
    fin, fout = os.path.join(tmp, group + ".in"), os.path.join(tmp, group + ".out")
    DS.write_case_file(fin, ops, fx)
    try:
        p = subprocess.run([EXE, fin, fout], timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _dead.append(f"device_math_check timed out on group {group}")
        pytest.fail(_dead[0])
    if p.returncode != 0:
        _dead.append(f"device_math_check exited {p.returncode} on group {group}: "
                     f"{p.stderr[-500:]}")
        pytest.fail(_dead[0])
    _results[group] = DS.read_result_file(fout, ops, fx)
    return _results[group]


def group_of(op):
    return next(g for g, ops in DS.GROUPS.items() if op in ops)


def check_classes(op, fx, out):
    """Every class of `op` against its bound; returns the comparable output."""
    cmpb = DS.comparable(op, out)
    err = DS.case_errors(op, cmpb, fx[op + "/ref"], fx.get(op + "/ref_lo"), fx[op + "/alt"])
    cls, classes = fx[op + "/cls"], list(fx[op + "/classes"])
    bad = []
    for c, name in enumerate(classes):
        idx = np.flatnonzero(cls == c)
        i = int(idx[np.argmax(err[idx])])
        bound = float(fx[op + "/bound"][c])
        line = (f"{op}/{name}: worst error {err[i]:.3g} (bound {bound:.3g}, E_cpu "
                f"{float(fx[op + '/ecpu'][c]):.3g}) at case {i}")
        print(line)
        if not err[i] <= bound:
            bad.append(f"{line}\n  inputs {fx[op + '/in'][i].tolist()}\n  output {out[i].tolist()}"
                       f"\n  expected {fx[op + '/ref'][i].tolist()}")
    assert not bad, "\n".join(bad)
    return cmpb


@pytest.mark.parametrize("op", [o for g in DS.GROUPS.values() for o in g])
def test_operation(op, fx, tmp_path_factory):
    out = run_group(group_of(op), fx, str(tmp_path_factory.getbasetemp()))[op]
    inp, ref = fx[op + "/in"], fx[op + "/ref"]
    check_classes(op, fx, out)

    if op in DS.EXACT_WHERE_REF:  # zero components, zero reciprocals, the untouched x
        sl, values = DS.EXACT_WHERE_REF[op]
        for v in values:
            m = ref[:, sl] == v
            assert (out[:, sl][m] == v).all(), \
                f"{op}: not exactly {v} at cases {np.flatnonzero((m & (out[:, sl] != v)).any(1))}"

    if op in ("huber", "huber_sim3"):
        # at and below the corner nothing is computed: rho = e and rho' = 1 bit for bit. (At
        # e = delta^2 itself the other branch gives the same bits, since sqrt(fl(d * d)) = d in
        # binary floating point: `e > d2` and `e >= d2` cannot be told apart from outside.)
        e, d2 = inp[:, 0], inp[:, 1] * inp[:, 1]
        m = e <= d2
        assert m.sum() >= 6
        want = np.stack([e, e, e, np.ones_like(e)] if op == "huber" else [e, np.ones_like(e)], 1)
        assert (out[m] == want[m]).all(), f"{op}: rho / rho' not exact at e <= delta^2: {out[m]}"

    if op == "left_update":
        for names in (("pose_R", "pose_t"), ("se3_R", "se3_t")):  # each implementation's own error
            e = DS.case_errors(op, DS.comparable(op, out), ref, None, fx[op + "/alt"], only=names)
            for c, name in enumerate(fx[op + "/classes"]):
                worst = e[fx[op + "/cls"] == c].max()
                print(f"left_update/{name} {names[0][:-2]}: worst error {worst:.3g}")
        # both implementations: w >= 0, unit norm within 4 ulps; and they agree with each other
        # within the sum of their bounds (cases that may take either branch excepted)
        for name, q in (("pose_left_update", out[:, 0:4]), ("se3_left_update", out[:, 7:11])):
            assert (q[:, 3] >= 0).all(), f"{name}: w < 0 at cases {np.flatnonzero(q[:, 3] < 0)}"
            n = np.sqrt((q.astype(np.longdouble) ** 2).sum(1)).astype(np.float64)
            worst = np.abs(n - 1.0).max() / DS.EPS52
            assert worst <= 4.0, \
                f"{name}: |q| off 1 by {worst:.2f} ulps at case {np.abs(n - 1).argmax()}"
        c = DS.comparable(op, out)
        either = ~np.isnan(fx[op + "/alt"]).any(1)
        for lo, hi in ((0, 9), (9, 12)):
            a, b = c[:, lo:hi], c[:, 12 + lo:12 + hi]
            scale = np.maximum(np.abs(ref[:, lo:hi]).max(1), 1.0)
            d = np.abs(a - b).max(1) / scale
            lim = 2.0 * fx[op + "/bound"][fx[op + "/cls"]]
            i = int(np.argmax(np.where(either, 0.0, d / lim)))
            assert (d <= lim)[~either].all(), (f"pose_left_update and se3_left_update differ by "
                                               f"{d[i]:.3g} at case {i}: {inp[i].tolist()}")

    if op == "eval_edge":
        # "x * (1 / z) plus one residual step is the correctly rounded quotient but for rare
        # ties": in the quotient class e = -(x / z, y / z) of the inputs' t. Rare is taken as at
        # most 1 % of the 512 quotients, and a miss as the neighbouring double
        m = fx[op + "/cls"] == list(fx[op + "/classes"]).index("quotient")
        t = inp[m, 16:19]
        want = -(t[:, :2] / t[:, 2:3])
        got = out[m, 1:3]
        miss = got != want
        assert miss.sum() <= 0.01 * miss.size, \
            f"eval_edge: {miss.sum()} of {miss.size} quotients not correctly rounded"
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
        print(f"eval_edge/quotient: {int(miss.sum())} of {miss.size} differ from IEEE division")

    if op == "factor_diag_block":
        # only block 1's strict lower triangle of the factor storage may change
        touched = np.zeros(78, bool)
        for r in range(1, 6):
            for k in range(r):
                touched[(6 + r) * (7 + r) // 2 + 6 + k] = True
        assert (out[:, 1:79][:, ~touched] == inp[:, :78][:, ~touched]).all(), \
            "factor_diag_block wrote outside its block's strict lower triangle"
        assert (out[:, 79:85] == inp[:, 78:84]).all(), "factor_diag_block touched block 0's rhs"
