"""The committed high-precision fixture of the optimizers' device math
(tests/golden/device_math.npz, generator tests/golden/make_device_math.py) and what can be said
about it without a GPU: its contents, that the generator reproduces it, that the oracle's exported
Sim3 / SE3 primitives meet the recorded float64 error against it (the first pin of
oracle/sim3_oracle.h and se3_oracle.h that does not come from the same hands' restatement), and
that the device harness builds."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import device_math_spec as DS
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "device_math.npz")
GEN = os.path.join(HERE, "golden", "make_device_math.py")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(NPZ))


def test_fixture_is_small():
    assert os.path.getsize(NPZ) < 1_000_000


@pytest.mark.parametrize("op", sorted(DS.OPS))
def test_fixture_has_every_class(fx, op):
    s = DS.OPS[op]
    inp, ref, alt, cls = fx[op + "/in"], fx[op + "/ref"], fx[op + "/alt"], fx[op + "/cls"]
    classes = list(fx[op + "/classes"])
    wc = max(g[1].stop for g in s["groups"])
    assert inp.shape == (len(cls), s["win"]) and ref.shape == (len(cls), wc) == alt.shape
    assert np.isfinite(inp).all() and np.isfinite(ref).all()
    for c, k in DS.MIN_CASES[op].items():
        assert c in classes, f"{op}: class {c} is missing"
        assert (cls == classes.index(c)).sum() >= k, f"{op}/{c}: fewer than {k} cases"
    ecpu, bound = fx[op + "/ecpu"], fx[op + "/bound"]
    assert len(ecpu) == len(bound) == len(classes)
    if any(g[2] == DS.ULP for g in s["groups"]):
        assert (bound == 2.0).all() and (op + "/ref_lo") in fx
    else:  # never from the device's output: a function of the float64 baseline's error alone
        assert (bound == DS.MARGIN * np.maximum(ecpu, DS.EPS52)).all()
    for c in DS.CAPPED.get(op, []):
        assert ecpu[classes.index(c)] <= DS.CAP, f"{op}/{c}: E_cpu past the cap"
    assert (~np.isnan(alt).any(1)).mean() <= DS.ALT_SHARE


def test_every_operation_is_in_one_group():
    ops = [o for g in DS.GROUPS.values() for o in g]
    assert sorted(ops) == sorted(DS.OPS)


def test_generator_reproduces_fixture(fx):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_device_math", GEN)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()
    assert sorted(new) == sorted(fx)
    for k in sorted(fx):
        a, b = fx[k], np.asarray(new[k])
        if k.endswith("/ecpu") or k.endswith("/bound"):
            # the float64 baseline goes through this machine's libm (sin, cos, acos, exp, log),
            # whose last bit may differ between processors; inputs and 50-digit values may not
            assert a.shape == b.shape and (b <= 4.0 * np.maximum(a, DS.EPS52)).all() and \
                (a <= 4.0 * np.maximum(b, DS.EPS52)).all(), k
        else:
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k


ORACLE_OPS = ["left_update", "sim3_exp", "sim3_log", "sim3_mul", "sim3_inverse", "eg_edge_error",
              "eg_oplus_axis"]


@pytest.mark.parametrize("op", ORACLE_OPS)
def test_oracle_primitives_meet_ecpu(fx, op):
    """oc_sim3_exp / log / mul / inverse and oc_se3_exp against the 50-digit statement of g2o's
    formulas. The allowance over the recorded E_cpu (a factor 4, floor 2^-52; the device gets 16)
    covers a libm whose last bit differs from the generating machine's; a transcription error
    is orders larger."""
    O.build()
    base = DS.oracle_baseline(op, fx[op + "/in"])
    err = DS.case_errors(op, base, fx[op + "/ref"], None, fx[op + "/alt"])
    cls, classes = fx[op + "/cls"], list(fx[op + "/classes"])
    for c, name in enumerate(classes):
        e = err[cls == c]
        lim = 4.0 * max(fx[op + "/ecpu"][c], DS.EPS52)
        i = int(np.flatnonzero(cls == c)[e.argmax()])
        assert e.max() <= lim, (f"{op}/{name}: oracle error {e.max():.3g} > {lim:.3g} at case "
                                f"{i}, inputs {fx[op + '/in'][i].tolist()}")


def test_harness_builds():
    sys.path.insert(0, os.path.dirname(HERE))
    from slam_framework_amd import build as B

    B.build()
    exe = B.build_device_math_check()
    assert os.path.exists(exe) and os.access(exe, os.X_OK)
    assert os.path.getmtime(exe) >= max(os.path.getmtime(s) for s in B.DEVICE_MATH_SRCS)


def test_harness_rejects_malformed_case_files(fx, tmp_path):
    """Every count and size is checked against the file length before anything touches the GPU:
    a malformed case file ends the program with an error and no output, on a machine without
    one too."""
    import struct
    import subprocess

    sys.path.insert(0, os.path.dirname(HERE))
    from slam_framework_amd import build as B

    B.build()
    exe = B.build_device_math_check()
    good = tmp_path / "good.in"
    DS.write_case_file(str(good), ["rcp_nr"], fx)
    b = good.read_bytes()
    q = lambda v: struct.pack("<Q", v)  # noqa: E731
    bad = {"truncated record": b[:-8], "bad magic": q(0) + b[8:], "trailing bytes": b + q(0),
           "case width": b[:32] + q(2) + b[40:], "too many cases": b[:24] + q(1 << 40) + b[32:],
           "unknown operation": b[:16] + q(999) + b[24:],
           "truncated record header": b[:8] + q(2) + b[16:], "case file length": b[:15]}
    for what, data in bad.items():
        fin, fout = tmp_path / "bad.in", tmp_path / "bad.out"
        fin.write_bytes(data)
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and what in p.stderr and not fout.exists(), (what, p.stderr)
