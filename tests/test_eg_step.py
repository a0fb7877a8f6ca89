"""The fixture of the essential graph's linear step (tests/golden/eg_step.npz, generator
tests/golden/make_eg_step.py, cases tests/eg_step_spec.py) and what can be said about it without
a GPU: its contents, that the generator reproduces it, that tests/eg_step_check builds and
refuses malformed files, that the structure builder the runtime ships (csrc/eg_structure.h,
through the harness's --structure mode) equals the numpy restatement, and that every graph
reaches the path of eg_factor_solve_kernel it was built for."""
import importlib.util
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import device_math_spec as DS
import eg_step_spec as ES

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "eg_step.npz")
GEN = os.path.join(HERE, "golden", "make_eg_step.py")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(NPZ))


@pytest.fixture(scope="module")
def exe():
    sys.path.insert(0, os.path.dirname(HERE))
    from slam_framework_amd import build as B

    B.build()
    return B.build_eg_step_check()


@pytest.fixture(scope="module")
def graphs():
    return ES.graphs()


def test_fixture_is_small():
    assert os.path.getsize(NPZ) < 1_000_000


def test_fixture_has_every_class(fx, graphs):
    solved = [c for c in ES.CLASSES if c != "failure"]
    assert list(fx["classes"]) == solved
    assert sorted({g["cls"] for g in graphs}) == sorted(ES.CLASSES)
    assert sorted(g["name"] for g in graphs) == sorted(ES.EXPECT)
    for k in ("ecpu_x", "ecpu_scale", "bound_x", "bound_scale"):
        assert fx[k].shape == (len(solved),)
    # never from the device's output: a function of the float64 baseline's error alone
    assert (fx["bound_x"] == DS.MARGIN * np.maximum(fx["ecpu_x"], DS.EPS52)).all()
    assert (fx["bound_scale"] == DS.MARGIN * np.maximum(fx["ecpu_scale"], DS.EPS52)).all()
    assert (fx["ecpu_x"] <= DS.CAP).all()
    for g in graphs:
        assert str(fx[g["name"] + "/sha256"]) == ES.inputs_sha256(g), g["name"]
        assert fx[g["name"] + "/lambdas"].tolist() == list(g["lambdas"])
        F = int((g["fixed"] == 0).sum())
        for l in range(len(g["lambdas"]) if g["cls"] != "failure" else 0):
            x = fx[f"{g['name']}/x_ref/{l}"]
            assert x.shape == (7 * F,) and np.isfinite(x).all()
            assert fx[f"{g['name']}/scale/{l}"].shape == (2,)
    assert not any(k.startswith("failure/x_ref") for k in fx)


def test_every_class_has_its_parameters(graphs):
    """fix_scale 0 and 1 come from the GPU test; the lambdas are the graphs'."""
    for g in graphs:
        want = [0.0] if g["cls"] == "failure" else \
            [1e-16, 0.5, 0.0] if g["cls"] in ("chain", "panel") else [1e-16, 0.5]
        assert list(g["lambdas"]) == want, g["name"]
    assert sorted(c for cl in ES.GROUPS.values() for c in cl) == sorted(ES.CLASSES)


def test_inputs_are_exact(graphs):
    """|N| <= 8, err in eighths, both edge orientations, and an anchor in every graph."""
    for g in graphs:
        J8, e8 = ES.inputs(g)
        N = np.abs(J8) - 24 * np.eye(7, dtype=np.int64)
        assert np.abs(N).max() <= 8 and np.abs(e8).max() <= 8
        assert (J8[:, 0].diagonal(axis1=1, axis2=2) > 0).all()
        assert (J8[:, 1].diagonal(axis1=1, axis2=2) < 0).all()
        fx_end = g["fixed"][g["edges"]] != 0
        assert (fx_end.sum(1) == 1).any(), g["name"]
        if len(g["edges"]) > 8:
            d = g["edges"][:, 0] < g["edges"][:, 1]
            assert d.any() and (~d).any(), g["name"]
        A, _ = ES.dense_system(g)
        assert np.abs(A).max() < 2 ** 40


def test_generator_reproduces_fixture(fx):
    spec = importlib.util.spec_from_file_location("make_eg_step", GEN)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()
    assert sorted(new) == sorted(fx)
    for k in sorted(fx):
        a, b = fx[k], np.asarray(new[k])
        if k.startswith("ecpu") or k.startswith("bound"):
            # the float64 baseline's sums go through this machine's BLAS, whose order may differ
            # between processors; inputs and 50-digit values may not
            assert a.shape == b.shape and (b <= 4.0 * np.maximum(a, DS.EPS52)).all() and \
                (a <= 4.0 * np.maximum(b, DS.EPS52)).all(), k
        else:
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_harness_builds(exe):
    sys.path.insert(0, os.path.dirname(HERE))
    from slam_framework_amd import build as B

    assert os.path.exists(exe) and os.access(exe, os.X_OK)
    assert os.path.getmtime(exe) >= os.path.getmtime(B.EG_STEP_SRC)


def test_structure_matches_restatement_and_table(exe, graphs, tmp_path):
    """--structure never initialises HIP: the shipped builder's arrays for every graph equal the
    numpy restatement, and the fixed table shows what each graph reaches: the largest extent
    against kPanStage = 96, the extent entries, the columns without look-ahead, the structure's
    bytes against the 100 KiB of the staged variant."""
    fin, fout = tmp_path / "all.in", tmp_path / "all.st"
    ES.write_case_file(str(fin), [ES.step_record(g, 0) for g in graphs] +
                       [ES.chi2_record(ES.chi2_values(3))])
    p = subprocess.run([exe, "--structure", str(fin), str(fout)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    got = ES.read_structure_file(str(fout), len(graphs))
    for g, st in zip(graphs, got):
        mine = ES.structure(g)
        assert (st["F"], st["n_blocks"]) == (mine["F"], mine["n_blocks"]), g["name"]
        for k in ES.STRUCT_ARRAYS:
            assert np.array_equal(st[k], mine[k]), (g["name"], k)
        ne = np.diff(st["ext_ptr"])
        reached = (st["F"], int(ne.max()), len(st["ext_rows"]), ES.nxt_in_false(st),
                   ES.meta_bytes(st) > ES.META_LIMIT)
        assert reached == ES.EXPECT[g["name"]], (g["name"], reached)
    by = {g["name"]: ES.EXPECT[g["name"]] for g in graphs}
    assert by["panel97"][1] == 96 and by["panel98"][1] == 97 and by["panel_nola"][1] == 97
    assert by["panel98"][1] * (by["panel98"][1] + 1) // 2 == 4753


def test_harness_rejects_malformed_case_files(exe, graphs, tmp_path):
    """Every count, size and index is checked against the file length before anything touches
    the GPU: a malformed case file ends the program with status 1, a message naming the fault
    and no output file, on a machine without a GPU too."""
    g = next(x for x in graphs if x["name"] == "tiny2")
    good = tmp_path / "good.in"
    ES.write_case_file(str(good), [ES.step_record(g, 1)])
    b = good.read_bytes()
    q = lambda v: struct.pack("<Q", v)  # noqa: E731
    w = lambda i, v: b[:8 * i] + q(v) + b[8 * i + 8:]  # noqa: E731
    P = ES.update_problem()
    upd = struct.pack("<QQ", ES.MAGIC, 1) + ES.update_record(P, 0)
    # words: 0 magic, 1 records, 2 kind, 3 n_kf, 4 n_edges, 5 fix_scale, 6 n_lambda, 7.. fixed[3],
    # 10.. edges
    bad = {"truncated record": b[:-8], "bad magic": w(0, 0), "trailing bytes": b + q(0),
           "too many records": w(1, 1 << 20), "unknown record kind": w(2, 9),
           "too many keyframes or edges": w(4, 1 << 40), "fix_scale flag": w(5, 2),
           "too many lambdas": w(6, 9), "fixed flag": w(7, 2), "edge index": w(10, 3),
           "truncated record header": w(1, 2), "case file length": b[:15],
           "point reference": upd[:-8] + q(len(P["S"])),
           "too many chi2 values": struct.pack("<QQQQ", ES.MAGIC, 1, ES.REC_CHI2, 1 << 30)}
    for mode in ([], ["--structure"]):
        for what, data in bad.items():
            fin, fout = tmp_path / "bad.in", tmp_path / "bad.out"
            fin.write_bytes(data)
            p = subprocess.run([exe, *mode, str(fin), str(fout)], capture_output=True, text=True,
                               timeout=60)
            assert p.returncode == 1 and what in p.stderr and not fout.exists(), (what, p.stderr)


def test_integer_reference_is_consistent(graphs):
    """The two integer statements agree: summing expected_contrib over the targets' items gives
    the profile blocks cut from the dense sum over edges."""
    for g in graphs:
        if g["name"] == "meta":
            continue
        st = ES.structure(g)
        c = ES.expected_contrib(g)
        H, b = ES.expected_system(g, st)
        H2, b2 = np.zeros_like(H), np.zeros_like(b)
        for t in range(len(st["tgt_block"])):
            for item in st["tgt_items"][st["tgt_ptr"][t]:st["tgt_ptr"][t + 1]]:
                k, kind = item >> 2, item & 3
                blk = c[k, [0, 49, 98, 98][kind]:][:49]
                H2[st["tgt_block"][t]] += blk.reshape(7, 7).T.ravel() if kind == 3 else blk
                if st["tgt_vertex"][t] >= 0:
                    f = st["tgt_vertex"][t]
                    b2[7 * f:7 * f + 7] += c[k, 147 + 7 * kind:154 + 7 * kind]
        assert np.array_equal(H, H2) and np.array_equal(b, b2), g["name"]
