"""CPU checks of the keyframe database's contract (no GPU): tests/kfdb_ref.c, the literal
restatement of KeyframeDatabase with its inverted file, against a second, flat statement in plain
Python that has no inverted file -- sorted-set intersections, the ordering key (smallest shared
word, add sequence) and sequential sums in numpy scalars. Byte equality on every scenario of
kfdb_scenario.py, whose histories interleave add / erase / re-add / Clear, pins the ordering-key
argument of include/slamgpu_kfdb.h before any kernel runs. Also: kfdb_ref.c under the address and
undefined-behaviour sanitizers as a stand-alone program, and LoopDetectorCore
(include/slamgpu_adapters.hpp) against a Python statement of DetectLoop's group bookkeeping."""
import json
import os
import subprocess

import numpy as np
import pytest

import kfdb_ref
import kfdb_scenario as KS

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def flat_score(w1, v1, w2, v2):
    """L1Scoring::score: the terms of the common words, added one after another in ascending
    word order in float64."""
    _, i1, i2 = np.intersect1d(w1, w2, assume_unique=True, return_indices=True)
    s = np.float64(0)
    for vi, wi in zip(np.asarray(v1, np.float64)[i1], np.asarray(v2, np.float64)[i2]):
        s = s + ((np.abs(vi - wi) - np.abs(vi)) - np.abs(wi))
    return -s / np.float64(2)


def score_terms(w1, v1, w2, v2):
    _, i1, i2 = np.intersect1d(w1, w2, assume_unique=True, return_indices=True)
    vi, wi = np.asarray(v1, np.float64)[i1], np.asarray(v2, np.float64)[i2]
    return (np.abs(vi - wi) - np.abs(vi)) - np.abs(wi)


class FlatDatabase:
    """The database as slamgpu_kfdb.h describes it: per-slot vectors, neighbour lists, add
    sequence numbers and one persistent mRelocScore; a query is set intersections and a key sort."""

    def __init__(self, max_kf):
        self.n = max_kf
        self.bow, self.covis = {}, {}
        self.seq = np.zeros(max_kf, np.int64)
        self.next_seq = 1
        self.reloc_score = np.zeros(max_kf, F32)

    def set_bow(self, kf, words, values):
        self.bow[kf] = (np.asarray(words, np.uint32), np.asarray(values, np.float64))

    def set_covisible(self, kf, ids):
        self.covis[kf] = [int(i) for i in ids]

    def add(self, kf):
        assert self.seq[kf] == 0 and kf in self.bow
        self.seq[kf] = self.next_seq
        self.next_seq += 1

    def erase(self, kf):
        self.seq[kf] = 0

    def clear(self):
        self.seq[:] = 0

    def _query(self, qw, qv, loop, connected, min_score):
        cw = np.full(self.n, -1, np.int32)
        key = {}
        for kf in range(self.n):
            if self.seq[kf] == 0 or kf in connected:
                continue
            common = np.intersect1d(qw, self.bow[kf][0], assume_unique=True)
            cw[kf] = len(common)
            if len(common):
                key[kf] = (int(common[0]), int(self.seq[kf]))
        max_common = max((int(cw[kf]) for kf in key), default=0)
        min_common = int(F32(max_common) * F32(0.8))
        sc = np.zeros(self.n, F32) if loop else self.reloc_score
        scored = [kf for kf in key if cw[kf] > min_common]
        for kf in scored:
            sc[kf] = F32(flat_score(qw, qv, *self.bow[kf]))
        entries = sorted((kf for kf in scored if not loop or sc[kf] >= min_score), key=key.get)
        best_acc = F32(min_score) if loop else F32(0)
        accs = []
        for kf in entries:
            best_score = acc = sc[kf]
            best = kf
            for nb in self.covis.get(kf, []):
                if not 0 <= nb < self.n:
                    continue
                if cw[nb] > min_common if loop else cw[nb] > 0:
                    acc = F32(acc + sc[nb])
                    if sc[nb] > best_score:
                        best, best_score = nb, sc[nb]
            accs.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(0.75) * best_acc
        out = []
        for acc, best in accs:
            if acc > retain and best not in out:
                out.append(best)
        return np.array(out, np.int32), cw, sc.copy()

    def DetectLoopCandidates(self, kf, connected, covisible, diagnostics=True):
        qw, qv = self.bow[kf]
        ms = F32(1)
        for c in covisible:
            if 0 <= c < self.n:
                s = F32(flat_score(qw, qv, *self.bow[int(c)]))
                ms = s if s < ms else ms
        cand, cw, sc = self._query(qw, qv, True, {int(c) for c in connected}, ms)
        return cand, ms, cw, sc

    def DetectRelocalizationCandidates(self, words, values, diagnostics=True):
        return self._query(np.asarray(words, np.uint32), np.asarray(values, np.float64), False,
                           set(), None)


SCENARIOS = KS.all_scenarios()
ref_records = kfdb_ref.records


@pytest.mark.parametrize("scn", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_flat_statement_equals_literal_restatement(scn):
    ref = ref_records(scn)
    flat = KS.replay(FlatDatabase(KS.MAX_KF), scn["ops"])
    assert KS.records_equal(ref, flat) is None, KS.records_equal(ref, flat)
    KS.check_expectations(scn, ref)


@pytest.mark.parametrize("scn", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_flat_score_equals_lower_bound_walk(scn):
    for (w1, v1), (w2, v2) in KS.score_pairs(scn["ops"]):
        a, b = kfdb_ref.score(w1, v1, w2, v2), flat_score(w1, v1, w2, v2)
        assert a.tobytes() == b.tobytes(), (scn["name"], a, b)


def test_min_common_words_rounding():
    for max_common, want in ((5, 4), (10, 8), (16, 12)):
        assert int(F32(max_common) * F32(0.8)) == want


def test_stale_reloc_score_changes_the_candidates():
    a = ref_records(KS.reloc_stale(True))[-1][1].tolist()
    b = ref_records(KS.reloc_stale(False))[-1][1].tolist()
    assert a == [KS.X] and b == [KS.A, KS.B]


def test_random_scenes_tell_sequential_from_pairwise_sums():
    """The double of a score depends on the order of its additions: on the random scenes numpy's
    pairwise np.sum of the terms differs from the sequential sum for at least one scored pair (with
    100-300 common words), which is why slamgpu_bow_score's double is compared and not only the
    float the database keeps."""
    differ = total = 0
    for scn in SCENARIOS:
        if not scn["name"].startswith("random_"):
            continue
        for (w1, v1), (w2, v2) in KS.score_pairs(scn["ops"]):
            t = score_terms(w1, v1, w2, v2)
            if not 100 <= len(t) <= 300:
                continue
            total += 1
            seq = np.float64(0)
            for x in t:
                seq = seq + x
            differ += int(np.sum(t).tobytes() != seq.tobytes())
    print(f"{differ} of {total} pairs: pairwise sum != sequential sum")
    assert total > 0 and differ >= 1


def test_kfdb_ref_under_sanitizers():
    """tests/kfdb_sanitizer_check.c: kfdb_ref.c with -fsanitize=address,undefined, run as a
    program on empty vectors, a query with no listed keyframe, neighbour ids out of range and
    n_covisible = 0."""
    exe = os.path.join(HERE, "kfdb_sanitizer_check")
    src = [os.path.join(HERE, "kfdb_sanitizer_check.c"), kfdb_ref.SRC]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in src):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-std=c11", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", src[0], "-o", tmp, "-lm"],
                       check=True)
        os.replace(tmp, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kfdb_sanitizer_check ok" in r.stdout


# ---- LoopDetectorCore ---------------------------------------------------------------------------
class PyLoopDetector:
    """LoopCloser::DetectLoop (loop_closer.cpp:194-297) around the database call, as sets of ids."""

    def __init__(self, threshold):
        self.threshold, self.groups, self.last_loop_kf_id = threshold, [], 0

    def too_soon(self, kf_id):
        return kf_id < self.last_loop_kf_id + 10

    def update(self, candidates, connected_of):
        if not candidates:
            self.groups = []
            return []
        enough, current = [], []
        visited = [False] * len(self.groups)
        for c in candidates:
            group = set(connected_of[c]) | {c}
            has_enough = consistent_some = False
            for g, (prev, n_prev) in enumerate(self.groups):
                if group & prev:
                    consistent_some = True
                    n_cur = n_prev + 1
                    if not visited[g]:
                        current.append((group, n_cur))
                        visited[g] = True
                    if n_cur >= self.threshold and not has_enough:
                        enough.append(c)
                        has_enough = True
            if not consistent_some:
                current.append((group, 0))
        self.groups = current
        return enough


def loop_detector_sequence():
    """Nine queries: a group reaches the threshold 3 (queries 0-3 and again 5-8), a query without
    candidates clears the groups (query 4), and three candidates of one query visit the same
    previous group (query 6: only the first extends it, the is_visited rule)."""
    connected_of = {1: [2, 3], 2: [1, 3], 3: [1, 2], 10: [11], 11: [10, 12], 12: [11],
                    20: [21], 21: [20], 30: []}
    queries = [dict(kf=100, cand=[1]), dict(kf=101, cand=[2, 20]), dict(kf=102, cand=[3, 21]),
               dict(kf=103, cand=[1, 30]), dict(kf=104, cand=[]), dict(kf=105, cand=[10]),
               dict(kf=106, cand=[11, 12, 10]), dict(kf=107, cand=[12, 11]),
               dict(kf=108, cand=[10, 1])]
    return connected_of, queries


def test_loop_detector_core_matches_group_logic(tmp_path):
    from slam_framework_amd import build
    exe = build.build_kfdb_adapter_check()
    connected_of, queries = loop_detector_sequence()
    py = PyLoopDetector(3)
    want = []
    for q in queries:
        enough = py.update(q["cand"], connected_of)
        want.append(dict(enough=enough, groups=sorted([sorted(g), n] for g, n in py.groups)))
    # the properties the sequence is built for
    assert any(w["enough"] for w in want), "no group reaches the threshold"
    assert want[4]["groups"] == [] and want[4]["enough"] == []
    assert len(want[6]["groups"]) == 1, "two candidates visiting one group extend it once"
    assert want[3]["enough"] == [1] and want[8]["enough"] == [10]
    lines = [f"{3} {len(connected_of)} {len(queries)}"]
    for k, v in connected_of.items():
        lines.append(" ".join(map(str, [k, len(v)] + v)))
    for q in queries:
        lines.append(" ".join(map(str, [q["kf"], len(q["cand"])] + q["cand"])))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    assert got["queries"] == want
    # the early exit: no query, the caller still adds the keyframe
    assert got["early"] == dict(too_soon_5=True, too_soon_10=False, add=True)
    assert got["gather"] == dict(kf_id=7, connected=[27, 17], covisible=[27])
