"""The keyframe database and TemplatedVocabulary::score on the device (include/slamgpu_kfdb.h,
slamgpu_bow_score) against tests/kfdb_ref.c, byte for byte, on every scenario of
kfdb_scenario.py: the score's doubles, both detect calls' candidate lists, counts and min_score,
and the diagnostic common-word counts and scores; the host form against the *_device form;
set_bow_device fed from slamgpu_bow_transform_device; a history of mixed calls on one stream with
no synchronisation in between; the error paths."""
import numpy as np
import pytest

import kfdb_ref
import kfdb_scenario as KS
from slam_framework_amd import synthetic as S

pytestmark = pytest.mark.gpu

SCENARIOS = KS.all_scenarios()
IDS = [s["name"] for s in SCENARIOS]
EINVAL = "slamgpu error -1:"


@pytest.fixture(scope="module")
def B(gpu_lib):
    from slam_framework_amd import bow
    return bow


@pytest.fixture(scope="module")
def torch_dev(gpu_lib):
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def voc_arrays():
    return S.vocabulary(5, k=5, L=3)


@pytest.fixture(scope="module")
def voc(B, voc_arrays):
    return B.ORBVocabulary.from_arrays(voc_arrays)


def new_db(B, max_words=KS.MAX_WORDS):
    return B.KeyFrameDatabase(KS.MAX_KF, max_words)


class DeviceReplay:
    """A history through the *_device calls: every input is uploaded first, then all calls are
    issued on one stream back to back, and the outputs are read after a single synchronisation."""

    def __init__(self, B, torch_dev):
        self.torch, self.dev = torch_dev
        self.db = new_db(B)

    def _up(self, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        t = self.torch.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype))
        return t.to(self.dev)

    def run(self, ops):
        torch, dev, db = self.torch, self.dev, self.db
        nq = sum(op[0] in ("loop", "reloc") for op in ops)
        n = KS.MAX_KF
        ms = torch.full((max(nq, 1),), -7.0, dtype=torch.float32, device=dev)
        cand = torch.full((max(nq, 1), n), -7, dtype=torch.int32, device=dev)
        cnt = torch.full((max(nq, 1),), -7, dtype=torch.int32, device=dev)
        cw = torch.zeros((max(nq, 1), n), dtype=torch.int32, device=dev)
        sc = torch.zeros((max(nq, 1), n), dtype=torch.float32, device=dev)
        scratch = torch.zeros(db.scratch_bytes(), dtype=torch.uint8, device=dev)
        staged = []
        for op in ops:  # uploads only
            if op[0] in ("set_bow", "reloc"):
                w, v = op[-2], op[-1]
                staged.append((self._up(w, np.uint32), self._up(v, np.float64),
                               self._up([len(w)], np.int32)))
            elif op[0] == "set_covisible":
                staged.append((self._up(op[2], np.int32),))
            elif op[0] == "loop":
                staged.append((self._up(op[2], np.int32), self._up(op[3], np.int32)))
            else:
                staged.append(())
        torch.cuda.synchronize()
        st = torch.cuda.current_stream().cuda_stream
        q = 0
        kinds = []
        for op, t in zip(ops, staged):  # calls only: nothing here waits for the device
            kind = op[0]
            if kind == "set_bow":
                db.set_bow_device(op[1], *t, stream=st)
            elif kind == "set_covisible":
                db.set_covisible_device(op[1], t[0], len(op[2]), stream=st)
            elif kind == "add":
                db.add_device(op[1], stream=st)
            elif kind == "erase":
                db.erase_device(op[1], stream=st)
            elif kind == "clear":
                db.clear_device(stream=st)
            elif kind == "loop":
                db.DetectLoopCandidates_device(op[1], t[0], len(op[2]), t[1], len(op[3]),
                                               ms[q:q + 1], cand[q], cnt[q:q + 1], scratch,
                                               cw[q], sc[q], stream=st)
                kinds.append(kind)
                q += 1
            elif kind == "reloc":
                db.DetectRelocalizationCandidates_device(t[0], t[1], t[2], cand[q], cnt[q:q + 1],
                                                         scratch, cw[q], sc[q], stream=st)
                kinds.append(kind)
                q += 1
        torch.cuda.synchronize()
        ms, cand, cnt, cw, sc = (x.cpu().numpy() for x in (ms, cand, cnt, cw, sc))
        out = []
        for q, kind in enumerate(kinds):
            assert 0 <= cnt[q] <= n
            assert (cand[q, cnt[q]:] == -7).all(), "written past the candidate count"
            out.append((kind, cand[q, :cnt[q]].copy(), ms[q] if kind == "loop" else None,
                        cw[q].copy(), sc[q].copy()))
        return out


@pytest.mark.parametrize("scn", SCENARIOS, ids=IDS)
def test_score_doubles_equal_reference(voc, scn):
    pairs = KS.score_pairs(scn["ops"])
    a = [type("V", (), dict(words=p[0][0], values=p[0][1])) for p in pairs]
    b = [type("V", (), dict(words=p[1][0], values=p[1][1])) for p in pairs]
    got = voc.score_pairs(a, b)
    want = np.array([kfdb_ref.score(*p[0], *p[1]) for p in pairs], np.float64)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, (scn["name"], bad[:5], got[bad[:5]], want[bad[:5]])
    if pairs:
        one = voc.score(a[0], b[0])
        assert np.float64(one).tobytes() == want[0].tobytes()


@pytest.mark.parametrize("scn", SCENARIOS, ids=IDS)
def test_host_form_equals_reference(B, scn):
    db = new_db(B)
    got = KS.replay(db, scn["ops"])
    db.close()
    diff = KS.records_equal(kfdb_ref.records(scn), got)
    assert diff is None, (scn["name"], diff)
    KS.check_expectations(scn, got)


@pytest.mark.parametrize("scn", SCENARIOS, ids=IDS)
def test_device_form_equals_reference(B, torch_dev, scn):
    """Also the history test: the random scenes are about 30 mixed add / erase / set_covisible /
    set_bow / query calls each, issued on one stream without synchronising."""
    r = DeviceReplay(B, torch_dev)
    got = r.run(scn["ops"])
    r.db.close()
    diff = KS.records_equal(kfdb_ref.records(scn), got)
    assert diff is None, (scn["name"], diff)


def test_stale_reloc_score_changes_the_candidates(B):
    out = []
    for before in (True, False):
        db = new_db(B)
        out.append(KS.replay(db, KS.reloc_stale(before)["ops"])[-1][1].tolist())
        db.close()
    assert out == [[KS.X], [KS.A, KS.B]]


def test_diagnostics_are_optional(B):
    scn = KS.same_best()
    db = new_db(B)
    want = kfdb_ref.records(scn)
    for op in scn["ops"]:
        if op[0] == "loop":
            cand, ms = db.DetectLoopCandidates(op[1], op[2], op[3])
            assert cand.tolist() == want[0][1].tolist() and ms.tobytes() == want[0][2].tobytes()
        elif op[0] == "reloc":
            assert db.DetectRelocalizationCandidates(op[1], op[2]).tolist() == want[1][1].tolist()
        else:
            getattr(db, op[0])(*op[1:])
    db.close()


def test_set_bow_device_from_transform_device(B, torch_dev, voc):
    """BowVectors go from slamgpu_bow_transform_device's outputs into the database without a
    round trip; the queries equal those of a database filled through the host path."""
    torch, dev = torch_dev
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    sets = [pool[rng.choice(40, n, replace=False)] for n in (30, 25, 1, 0, 33)]
    cap = 64
    desc = np.zeros((len(sets), cap, 32), np.uint8)
    for s, d in enumerate(sets):
        desc[s, :len(d)] = d
    d_desc = torch.from_numpy(desc).to(dev)
    d_cnt = torch.tensor([len(d) for d in sets], dtype=torch.int32, device=dev)
    out = B.DeviceBowSets(len(sets), cap, dev)
    st = torch.cuda.current_stream().cuda_stream
    voc.transform_device(d_desc, cap, d_cnt, 1, len(sets), 4, out, st)
    ddb, hdb = new_db(B), new_db(B)
    for s, d in enumerate(sets):
        ddb.set_bow_device(s, out.words[s], out.values[s], out.n_words[s:s + 1], stream=st)
        ddb.add_device(s, stream=st)
        bv, _ = voc.transform(d)
        hdb.set_bow(s, bv)
        hdb.add(s)
    torch.cuda.synchronize()
    shared = 0
    for s, d in enumerate(sets):
        bv, _ = voc.transform(d)
        a = ddb.DetectRelocalizationCandidates(bv, diagnostics=True)
        b = hdb.DetectRelocalizationCandidates(bv, diagnostics=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        a = ddb.DetectLoopCandidates(s, [], [(s + 1) % len(sets)], diagnostics=True)
        b = hdb.DetectLoopCandidates(s, [], [(s + 1) % len(sets)], diagnostics=True)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        shared += int((a[2] > 0).sum())
    assert shared > len(sets), "the sets share no word: the comparison is empty"
    ddb.close()
    hdb.close()


def test_error_paths_write_nothing(B, voc_arrays):
    from slam_framework_amd.slamgpu import SlamGpuError
    scn = KS.same_best()
    db = new_db(B)
    small = new_db(B, max_words=8)
    w9, v9 = np.arange(9, dtype=np.uint32), np.full(9, 1.0 / 16)
    for bad in (-1, KS.MAX_KF):
        for call in (lambda: db.set_bow(bad, w9, v9), lambda: db.set_covisible(bad, [0]),
                     lambda: db.add(bad), lambda: db.erase(bad),
                     lambda: db.DetectLoopCandidates(bad, [], [])):
            with pytest.raises(SlamGpuError, match="outside") as e:
                call()
            assert EINVAL in str(e.value)
    with pytest.raises(SlamGpuError, match="max_words") as e:
        small.set_bow(0, w9, v9)
    assert EINVAL in str(e.value)
    with pytest.raises(SlamGpuError, match="no BoW vector"):
        small.add(0)  # the refused set_bow left nothing behind
    with pytest.raises(SlamGpuError, match="outside"):
        db.set_covisible(0, list(range(11)))
    with pytest.raises(SlamGpuError, match="not strictly ascending"):
        db.set_bow(0, [3, 3], [0.5, 0.5])
    with pytest.raises(SlamGpuError, match="no BoW vector"):
        db.add(0)
    # the scenario, with refused calls woven in, still equals the reference
    got = []
    for op in scn["ops"]:
        got += KS.replay(db, [op])
        if op[0] == "add":
            with pytest.raises(SlamGpuError, match="already listed") as e:
                db.add(op[1])
            assert EINVAL in str(e.value)
    assert KS.records_equal(kfdb_ref.records(scn), got) is None
    db.close()
    small.close()
    # a non-L1 vocabulary: score names the scoring it will not compute
    l2 = B.ORBVocabulary.from_arrays(dict(voc_arrays, scoring=B.L2_NORM))
    v = B.BowVector(np.array([1], np.uint32), np.array([1.0]))
    with pytest.raises(SlamGpuError, match="L2_NORM") as e:
        l2.score(v, v)
    assert EINVAL in str(e.value)
    l2.close()
