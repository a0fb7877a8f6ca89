"""Constructed inputs for the keyframe database (include/slamgpu_kfdb.h), shared by
test_kfdb_ref.py (CPU) and test_kfdb_gpu.py. A scenario is a dict(name, n_vocab, ops); ops is a
history of
  ("set_bow", kf, words u32, values f64)   ("set_covisible", kf, ids)
  ("add", kf)  ("erase", kf)  ("clear",)
  ("loop", kf, connected ids, covisible ids)        DetectLoopCandidates + DetectLoop's min_score
  ("reloc", words, values)                          DetectRelocalizationCandidates
replay(db, ops) runs it on anything with KeyFrameDatabase's method names and returns one record
per query. At most MAX_KF keyframes, word ids below 1024 (8192 where a 4096-word vector needs
them). Values are dyadic where a boundary must be hit exactly; those boundaries are checked here
in exact rational arithmetic (for positive values a common word's term is -2 min(vi, wi), so the
score is the sum of the minima)."""
from fractions import Fraction

import numpy as np

MAX_KF = 48
MAX_WORDS = 4096
QKF = 40   # the loop query's keyframe: has a BoW vector, is not listed
COV = 41   # a covisible keyframe that only sets min_score: not listed


class Ops(list):
    def set_bow(self, kf, words, values):
        w = np.asarray(words, np.uint32)
        v = np.asarray(values, np.float64)
        order = np.argsort(w, kind="stable")
        assert len(np.unique(w)) == len(w) and len(w) == len(v)
        self.append(("set_bow", kf, w[order].copy(), v[order].copy()))

    def set_covisible(self, kf, ids):
        self.append(("set_covisible", kf, np.asarray(ids, np.int32)))

    def add(self, *kfs):
        for kf in kfs:
            self.append(("add", kf))

    def erase(self, kf):
        self.append(("erase", kf))

    def clear(self):
        self.append(("clear",))

    def loop(self, kf, connected=(), covisible=()):
        self.append(("loop", kf, np.asarray(connected, np.int32), np.asarray(covisible, np.int32)))

    def reloc(self, words, values):
        w = np.asarray(words, np.uint32)
        v = np.asarray(values, np.float64)
        order = np.argsort(w, kind="stable")
        self.append(("reloc", w[order].copy(), v[order].copy()))

    def both(self, words, values, connected=(), covisible=()):
        """The same query vector through both variants."""
        self.set_bow(QKF, words, values)
        self.loop(QKF, connected, covisible)
        self.reloc(words, values)


def replay(db, ops):
    """-> [(kind, candidates i32, min_score f32 or None, common words i32[max_kf], scores f32)]."""
    out = []
    for op in ops:
        kind = op[0]
        if kind == "loop":
            cand, ms, cw, sc = db.DetectLoopCandidates(op[1], op[2], op[3], diagnostics=True)
            out.append(("loop", np.asarray(cand, np.int32), np.float32(ms), cw.copy(), sc.copy()))
        elif kind == "reloc":
            cand, cw, sc = db.DetectRelocalizationCandidates(op[1], op[2], diagnostics=True)
            out.append(("reloc", np.asarray(cand, np.int32), None, cw.copy(), sc.copy()))
        else:
            getattr(db, kind)(*op[1:])
    return out


def records_equal(a, b):
    """Byte equality of two replay() results; returns a description of the first difference."""
    if len(a) != len(b):
        return f"{len(a)} queries != {len(b)}"
    for q, (x, y) in enumerate(zip(a, b)):
        if x[0] != y[0]:
            return f"query {q}: kind"
        if x[1].tobytes() != y[1].tobytes():
            return f"query {q} ({x[0]}): candidates {x[1].tolist()} != {y[1].tolist()}"
        if (x[2] is None) != (y[2] is None) or (
                x[2] is not None and x[2].tobytes() != y[2].tobytes()):
            return f"query {q}: min_score {x[2]!r} != {y[2]!r}"
        if x[3].tobytes() != y[3].tobytes():
            return f"query {q} ({x[0]}): common words differ at {np.nonzero(x[3] != y[3])[0].tolist()}"
        if x[4].tobytes() != y[4].tobytes():
            return f"query {q} ({x[0]}): scores differ at {np.nonzero(x[4].view(np.uint32) != y[4].view(np.uint32))[0].tolist()}"
    return None


def score_pairs(ops):
    """Every (query vector, stored vector) pair a history's queries can meet: the inputs of the
    slamgpu_bow_score comparison."""
    bow, pairs = {}, []
    for op in ops:
        if op[0] == "set_bow":
            bow[op[1]] = (op[2], op[3])
        elif op[0] in ("loop", "reloc"):
            q = bow[op[1]] if op[0] == "loop" else (op[1], op[2])
            pairs += [(q, v) for k, v in sorted(bow.items())]
    return pairs


def exact_score(q, v):
    """The score of two positive vectors as a Fraction (dict word -> Fraction)."""
    return sum((min(q[w], v[w]) for w in q if w in v), Fraction(0))


def _min_common(max_common):
    return int(np.float32(max_common) * np.float32(0.8))


S = 1.0 / 16  # the usual dyadic value


def _filler(kf, n=4):
    """n words no query uses, private to the keyframe."""
    return list(range(600 + 8 * kf, 600 + 8 * kf + n))


def _kf(o, kf, words, values=None, covis=None, fill=4):
    words = list(words)
    values = [S] * len(words) if values is None else list(values)
    f = _filler(kf, fill)
    o.set_bow(kf, words + f, values + [S] * len(f))
    if covis is not None:
        o.set_covisible(kf, covis)


def _low_cov(o, word=0):
    """COV shares one word at 2^-10 with the query: min_score = 2^-10."""
    o.set_bow(COV, [word, 599], [2.0 ** -10, 0.5])


def threshold(max_common):
    """words == minCommonWords is not scored, minCommonWords + 1 is
    (keyframe_database.cpp:98,106 / :222,232)."""
    mc = _min_common(max_common)
    assert (max_common, mc) in ((5, 4), (10, 8), (16, 12))
    o = Ops()
    _kf(o, 0, range(max_common))
    _kf(o, 1, range(mc))
    _kf(o, 2, range(mc + 1))
    o.add(0, 1, 2)
    _low_cov(o)
    o.both(list(range(max_common)), [S] * max_common, covisible=[COV])
    return dict(name=f"threshold_{max_common}", ops=o,
                expect={0: dict(words={0: max_common, 1: mc, 2: mc + 1}, zero_score=[1],
                                scored=[0, 2])})


def score_equals_min():
    """mLoopScore == minScore is accepted (:110, >=): COV and keyframe 0 hold the same vector."""
    o = Ops()
    words, values = list(range(8)) + [700, 701], [S] * 8 + [0.25, 0.25]
    o.set_bow(0, words, values)
    o.set_bow(COV, words, values)
    o.add(0)
    o.both(list(range(16)), [S] * 16, covisible=[COV])
    return dict(name="score_equals_min", ops=o, expect={0: dict(cand=[0])})


def retain_boundary():
    """acc == 0.75f * bestAccScore is dropped (:166 / :290, >); one ulp above is kept."""
    q = {w: Fraction(1, 16) for w in range(16)}
    k1 = {w: Fraction(3, 64) for w in range(16)}
    k2 = dict(k1)
    k2[0] = Fraction(3, 64) + Fraction(1, 2 ** 24)
    assert exact_score(q, q) == 1 and exact_score(q, k1) == Fraction(3, 4)
    assert exact_score(q, k2) == Fraction(3, 4) + Fraction(1, 2 ** 24)
    assert np.float32(float(exact_score(q, k2))) == np.nextafter(np.float32(0.75), np.float32(1))
    o = Ops()
    _kf(o, 0, range(16))
    _kf(o, 1, range(16), [3.0 / 64] * 16)
    _kf(o, 2, range(16), [float(k2[w]) for w in range(16)])
    o.add(0, 1, 2)
    _low_cov(o)
    o.both(list(range(16)), [S] * 16, covisible=[COV])
    return dict(name="retain_boundary", ops=o, expect={0: dict(cand=[0, 2]), 1: dict(cand=[0, 2])})


def same_key_word():
    """Same key word: add order decides; erase + re-add of the first flips it."""
    o = Ops()
    _kf(o, 0, range(10), fill=0)
    _kf(o, 1, range(10), fill=0)
    o.add(0, 1)
    _low_cov(o)
    o.both(list(range(10)), [S] * 10, covisible=[COV])
    o.erase(0)
    o.add(0)
    o.both(list(range(10)), [S] * 10, covisible=[COV])
    return dict(name="same_key_word", ops=o,
                expect={0: dict(cand=[0, 1]), 1: dict(cand=[0, 1]), 2: dict(cand=[1, 0]),
                        3: dict(cand=[1, 0])})


def word_order_wins():
    """A smaller key word beats an earlier add."""
    o = Ops()
    _kf(o, 0, range(5, 10))
    _kf(o, 1, range(2, 7))
    o.add(0, 1)
    _low_cov(o)
    o.both(list(range(10)), [S] * 10, covisible=[COV])
    return dict(name="word_order_wins", ops=o, expect={0: dict(cand=[1, 0]), 1: dict(cand=[1, 0])})


def same_best():
    """Two entries with the same pBestKF: listed once, at the first position."""
    o = Ops()
    _kf(o, 1, range(0, 13), covis=[0])
    _kf(o, 3, range(1, 15), covis=[1])
    _kf(o, 0, range(2, 16), covis=[3])
    _kf(o, 2, range(3, 16), covis=[0])
    o.add(0, 1, 2, 3)
    _low_cov(o)
    o.both(list(range(16)), [S] * 16, covisible=[COV])
    return dict(name="same_best", ops=o, expect={0: dict(cand=[0, 3]), 1: dict(cand=[0, 3])})


def low_neighbours_and_connected():
    """Loop: neighbours with words > minCommonWords and a score below minScore are no entries of
    their own but count in accScore (:139-141) -- here they lift bestAccScore until keyframe 0 is
    dropped. (They cannot become pBestKF: bestScore starts at an entry's score >= minScore and is
    replaced only by '>'.) Keyframe 5 equals the query, is connected and is keyframe 0's
    neighbour: never counted, never returned."""
    o = Ops()
    _kf(o, 0, range(14), covis=[5])
    for k in (1, 3, 4):
        _kf(o, k, range(13), [1.0 / 64] * 13)
    _kf(o, 2, range(2, 16), covis=[1, 3, 4])
    _kf(o, 5, range(16), fill=0)
    o.add(0, 1, 2, 3, 4, 5)
    _kf(o, COV, range(10))  # min_score = 10/16
    o.both(list(range(16)), [S] * 16, connected=[5], covisible=[COV])
    return dict(name="low_neighbours_and_connected", ops=o,
                expect={0: dict(cand=[2], words={5: -1})})


X, A, B = 2, 0, 1


def reloc_stale(scored_before):
    """The reloc quirk (:264-272): X shares one word with query 2, is not scored by it, and is a
    neighbour of A; it contributes the mRelocScore query 1 left on it (1.0), or 0.0f in the twin
    in which query 1 never ran."""
    o = Ops()
    o.set_bow(X, [0] + list(range(100, 116)), [2.0 ** -10] + [S] * 16)
    _kf(o, A, range(15), covis=[X])
    _kf(o, B, range(14))
    o.add(A, B, X)
    if scored_before:
        o.reloc(list(range(100, 116)), [S] * 16)
    o.reloc(list(range(16)), [S] * 16)
    last = 1 if scored_before else 0
    return dict(name=f"reloc_stale_{int(scored_before)}", ops=o,
                expect={last: dict(cand=[X] if scored_before else [A, B])})


def _rand_values(rng, n):
    v = rng.random(n) + 0.05
    return v / v.sum()


def lengths():
    """Vector lengths 0, 1, 63, 64, 65 and 4096 on both sides of the search."""
    rng = np.random.default_rng(7)
    o = Ops()
    for kf, n in enumerate((0, 1, 63, 64, 65, 4096)):
        o.set_bow(kf, np.arange(n), _rand_values(rng, n) if n else [])
        o.set_covisible(kf, [(kf + 1) % 6, (kf + 2) % 6])
        o.add(kf)
    o.set_bow(COV, [3, 70], [0.01, 0.99])
    for n in (65, 64, 63, 1, 0):
        o.both(np.arange(n), _rand_values(rng, n) if n else [], covisible=[COV])
    o.reloc(np.arange(4096), _rand_values(rng, 4096))
    o.loop(5, [4], [COV, 3])  # the query keyframe is listed itself
    return dict(name="lengths", n_vocab=8192, ops=o, expect={})


def last_first():
    """The only hit is the last word of one vector and the first of the other."""
    o = Ops()
    o.set_bow(0, list(range(10, 21)), [S] * 11)
    o.set_bow(1, [0, 1], [0.5, 0.5])
    o.add(0, 1)
    _low_cov(o, word=1)
    o.both(list(range(1, 11)), [S] * 10, covisible=[COV])
    return dict(name="last_first", ops=o, expect={0: dict(words={0: 1, 1: 1}, cand=[1, 0])})


def no_common_word():
    o = Ops()
    for kf in range(4):
        _kf(o, kf, range(10 * kf, 10 * kf + 10), covis=[(kf + 1) % 4])
    o.add(0, 1, 2, 3)
    o.both(list(range(500, 510)), [S] * 10)
    return dict(name="no_common_word", ops=o,
                expect={0: dict(cand=[], words={0: 0, 1: 0, 2: 0, 3: 0}), 1: dict(cand=[])})


def all_connected():
    o = Ops()
    for kf in range(4):
        _kf(o, kf, range(10), covis=[(kf + 1) % 4])
    o.add(0, 1, 2, 3)
    o.both(list(range(10)), [S] * 10, connected=[0, 1, 2, 3, 3, -5, 1000])
    return dict(name="all_connected", ops=o, expect={0: dict(cand=[])})


def empty_database():
    o = Ops()
    _kf(o, 0, range(10))  # a BoW vector, never added
    o.both(list(range(10)), [S] * 10, covisible=[0])
    o.add(0)
    o.clear()
    o.both(list(range(10)), [S] * 10, covisible=[])
    return dict(name="empty_database", ops=o,
                expect={k: dict(cand=[]) for k in range(4)})


def odd_neighbours():
    """Neighbour ids that are unlisted, erased, the query keyframe or out of range."""
    o = Ops()
    _kf(o, 0, range(12), covis=[7, 3, QKF, -1, 1000, 1])
    _kf(o, 1, range(11), covis=[0, 0, MAX_KF])
    _kf(o, 3, range(12))
    _kf(o, 7, range(12))
    o.add(0, 1, 3)
    o.erase(3)
    _low_cov(o)
    o.both(list(range(12)), [S] * 12, covisible=[COV, -1, MAX_KF, 7])
    return dict(name="odd_neighbours", ops=o, expect={0: dict(words={3: -1, 7: -1, QKF: -1})})


def random_scene(seed):
    """Non-dyadic values, 100-300 common words per scored pair, a history of adds, erases,
    re-adds, neighbour updates and queries of both kinds."""
    rng = np.random.default_rng(seed)
    n_kf = 36
    o = Ops()
    base = rng.choice(1024, 300, replace=False)
    rest = np.setdiff1d(np.arange(1024), base)

    def near(n_common):
        w = np.concatenate([rng.choice(base, n_common, replace=False),
                            rng.choice(rest, 300 - n_common, replace=False)])
        return w, _rand_values(rng, 300)

    for kf in range(n_kf):
        o.set_bow(kf, *near(int(rng.integers(100, 301))))
        o.set_covisible(kf, rng.choice(n_kf, int(rng.integers(0, 11)), replace=False))
    order = rng.permutation(n_kf)
    o.add(*order[:24].tolist())
    qv = _rand_values(rng, 300)
    o.set_bow(QKF, base, qv)
    o.set_bow(COV, *near(150))
    o.set_bow(COV + 1, *near(220))
    con = rng.choice(n_kf, 5, replace=False)
    o.loop(QKF, con, [COV, COV + 1])
    o.reloc(base, qv)
    for kf in order[:6].tolist():
        o.erase(kf)
    o.add(*order[24:].tolist())
    o.add(*order[:3].tolist())
    o.set_covisible(int(order[30]), order[:10])
    w2, v2 = near(280)
    o.reloc(w2, v2)
    o.loop(QKF, con[:2], [COV + 1])
    o.set_bow(QKF + 3, w2, v2)
    o.loop(QKF + 3, [], [COV, COV + 1, int(order[8])])
    o.clear()
    o.add(*order[10:20].tolist())
    o.reloc(base, qv)
    o.loop(QKF, [], [COV])
    return dict(name=f"random_{seed}", ops=o, expect={})


def all_scenarios():
    return [threshold(5), threshold(10), threshold(16), score_equals_min(), retain_boundary(),
            same_key_word(), word_order_wins(), same_best(), low_neighbours_and_connected(),
            reloc_stale(True), reloc_stale(False), lengths(), last_first(), no_common_word(),
            all_connected(), empty_database(), odd_neighbours(), random_scene(11),
            random_scene(12), random_scene(13)]


def check_expectations(scn, records):
    """The hand-derived part of a scenario's outcome (query index -> what must hold)."""
    for q, e in scn["expect"].items():
        kind, cand, ms, cw, sc = records[q]
        if "cand" in e:
            assert cand.tolist() == e["cand"], (scn["name"], q, cand.tolist(), e["cand"])
        for kf, n in e.get("words", {}).items():
            assert cw[kf] == n, (scn["name"], q, kf, int(cw[kf]), n)
        for kf in e.get("zero_score", []):
            assert sc[kf] == 0, (scn["name"], q, kf)
        for kf in e.get("scored", []):
            assert sc[kf] > 0, (scn["name"], q, kf)
