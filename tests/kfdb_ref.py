"""Builds tests/kfdb_ref.c on demand (gcc, the oracle Makefile's CFLAGS) and wraps it: the literal
CPU restatement of KeyframeDatabase, L1Scoring::score and DetectLoop's min_score that
slamgpu_kfdb_* and slamgpu_bow_score are compared against bit for bit. RefDatabase has the method
names and return shapes of slam_framework_amd.bow.KeyFrameDatabase (diagnostics=True)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "kfdb_ref.c")
LIB = os.path.join(HERE, "libkfdb_ref.so")
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

_lib = None


def cflags():
    text = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS \?= (.*)$", text, re.M).group(1).split()


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *cflags(), "-shared", "-o", tmp, SRC, "-lm"],
                   check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        vp, ip = C.c_void_p, C.c_int
        L.kr_create.argtypes = [ip, ip]
        L.kr_create.restype = vp
        L.kr_destroy.argtypes = [vp]
        L.kr_destroy.restype = None
        L.kr_set_bow.argtypes = [vp, ip, vp, vp, ip]
        L.kr_set_covisible.argtypes = [vp, ip, vp, ip]
        for name in ("kr_add", "kr_erase"):
            getattr(L, name).argtypes = [vp, ip]
            getattr(L, name).restype = None
        L.kr_clear.argtypes = [vp]
        L.kr_clear.restype = None
        L.kr_score.argtypes = [vp, vp, ip, vp, vp, ip]
        L.kr_score.restype = C.c_double
        L.kr_detect_loop.argtypes = [vp, ip, vp, ip, vp, ip, vp, vp, vp, vp]
        L.kr_detect_reloc.argtypes = [vp, vp, vp, ip, vp, vp, vp]
        _lib = L
    return _lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vec(words, values):
    return np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(values, np.float64)


def score(w1, v1, w2, v2):
    """L1Scoring::score as an np.float64."""
    w1, v1 = _vec(w1, v1)
    w2, v2 = _vec(w2, v2)
    return np.float64(lib().kr_score(ptr(w1), ptr(v1), len(w1), ptr(w2), ptr(v2), len(w2)))


class RefDatabase:
    def __init__(self, max_keyframes, n_vocab_words):
        self.max_kf = max_keyframes
        self.h = C.c_void_p(lib().kr_create(max_keyframes, n_vocab_words))

    def close(self):
        if self.h:
            lib().kr_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_bow(self, kf, words, values):
        w, v = _vec(words, values)
        lib().kr_set_bow(self.h, kf, ptr(w), ptr(v), len(w))

    def set_covisible(self, kf, ids):
        a = np.ascontiguousarray(ids, np.int32)
        lib().kr_set_covisible(self.h, kf, ptr(a), len(a))

    def add(self, kf):
        lib().kr_add(self.h, kf)

    def erase(self, kf):
        lib().kr_erase(self.h, kf)

    def clear(self):
        lib().kr_clear(self.h)

    def DetectLoopCandidates(self, kf, connected, covisible, diagnostics=True):
        con = np.ascontiguousarray(connected, np.int32)
        cov = np.ascontiguousarray(covisible, np.int32)
        ms = np.zeros(1, np.float32)
        cand, words = np.zeros(self.max_kf, np.int32), np.zeros(self.max_kf, np.int32)
        scores = np.zeros(self.max_kf, np.float32)
        n = lib().kr_detect_loop(self.h, kf, ptr(con), len(con), ptr(cov), len(cov), ptr(ms),
                                 ptr(cand), ptr(words), ptr(scores))
        return cand[:n].copy(), ms[0], words, scores

    def DetectRelocalizationCandidates(self, words, values, diagnostics=True):
        w, v = _vec(words, values)
        cand, cw = np.zeros(self.max_kf, np.int32), np.zeros(self.max_kf, np.int32)
        scores = np.zeros(self.max_kf, np.float32)
        n = lib().kr_detect_reloc(self.h, ptr(w), ptr(v), len(w), ptr(cand), ptr(cw), ptr(scores))
        return cand[:n].copy(), cw, scores


_records = {}


def records(scn):
    """kfdb_scenario.replay of a scenario on a RefDatabase, computed once per process and shared
    by the tests that compare against it (treat as read-only)."""
    import kfdb_scenario as KS
    if scn["name"] not in _records:
        db = RefDatabase(KS.MAX_KF, scn.get("n_vocab", 1024))
        _records[scn["name"]] = KS.replay(db, scn["ops"])
        db.close()
    return _records[scn["name"]]
