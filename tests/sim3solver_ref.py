"""Builds tests/sim3solver_ref.c on demand (gcc, the oracle Makefile's CFLAGS) and wraps it: the
CPU restatement of the RANSAC Sim3 solver the device path is compared against bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim3solver_ref.c")
LIB = os.path.join(HERE, "libsim3solver_ref.so")  # not "sim3solver_ref.so": import would load it
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

MATCH_DTYPE = np.dtype([("x1c", "<f4", (3,)), ("x2c", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"),
                        ("u2", "<f4"), ("v2", "<f4"), ("octave1", "<i4"), ("octave2", "<i4")])
HYP_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"),
                      ("n_inliers", "<i4"), ("pad", "<i4", (2,))])
assert MATCH_DTYPE.itemsize == 48 and HYP_DTYPE.itemsize == 64

_lib = None


def _cflags():
    text = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS \?= (.*)$", text, re.M).group(1).split()


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *_cflags(), "-shared", "-o", tmp, SRC, "-lm"],
                   check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB)
        vp, ip, fp = C.c_void_p, C.c_int, C.c_float
        L.s3_resolve.argtypes = [ip, vp, vp]
        L.s3_eigvec.argtypes = [vp, ip, vp]
        L.s3_eigvec.restype = None
        L.s3_threshold.argtypes = [fp]
        L.s3_threshold.restype = fp
        L.s3_hypothesis.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, ip, vp]
        L.s3_hypothesis.restype = None
        L.s3_create.argtypes = [vp, ip, vp, vp, vp, vp, ip, ip, vp, ip, ip]
        L.s3_create.restype = vp
        L.s3_destroy.argtypes = [vp]
        L.s3_destroy.restype = None
        L.s3_iterate.argtypes = [vp, ip, vp, vp, vp]
        L.s3_find.argtypes = [vp, vp, vp]
        L.s3_best.argtypes = [vp, vp]
        L.s3_ransac.argtypes = [vp, ip, vp, vp, vp, vp, ip, ip, vp, ip, ip, ip, ip, vp, vp, vp, vp]
        L.s3_ransac.restype = None
        _lib = L
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def jacobi_sweeps():
    return lib().s3_jacobi_sweeps()


def resolve(n, randi):
    """The sample of :166-180 for the three draws, or None when one is out of range."""
    r = np.ascontiguousarray(randi, np.int32)
    idx = np.zeros(3, np.int32)
    return idx if lib().s3_resolve(int(n), ptr(r), ptr(idx)) else None


def eigvec(N, sweeps):
    Nf = _f(N)
    q = np.zeros(4)
    lib().s3_eigvec(ptr(Nf), int(sweeps), ptr(q))
    return q


def threshold(sigma2):
    return float(lib().s3_threshold(float(np.float32(sigma2))))


def unpack_bits(bits, n):
    """uint64 mask words (last axis) -> bool[..., n]."""
    b = np.ascontiguousarray(bits, np.uint64)
    u8 = np.unpackbits(b.view(np.uint8).reshape(*b.shape[:-1], -1), axis=-1, bitorder="little")
    return u8[..., :n].astype(bool)


def hypothesis(matches, idx, fix_scale, K1, K2, sigma2_1, sigma2_2, sweeps=None):
    """One iteration on the sample idx. Returns (hyp record, inlier bool[n], N 4x4 f32)."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(m)
    words = max((n + 63) // 64, 1)
    keep = [_f(K1)[:4].copy(), _f(K2)[:4].copy(), _f(sigma2_1), _f(sigma2_2),
            np.ascontiguousarray(idx, np.int32)]
    h = np.zeros(1, HYP_DTYPE)
    bits = np.zeros(words, np.uint64)
    N = np.zeros(16, np.float32)
    lib().s3_hypothesis(ptr(m), n, ptr(keep[4]), int(bool(fix_scale)), ptr(keep[0]), ptr(keep[1]),
                        ptr(keep[2]), ptr(keep[3]), len(keep[2]),
                        jacobi_sweeps() if sweeps is None else int(sweeps), ptr(h), ptr(bits),
                        words, ptr(N))
    return h[0], unpack_bits(bits, n), N.reshape(4, 4)


def ransac(matches, draws, n_its, min_inliers, fix_scale, K1, K2, sigma2_1, sigma2_2,
           max_its=None, words=None):
    """The whole schedule of one job in the device call's layout. Returns (hyp[max_its],
    bits[max_its][words], events[max_its], n_events); rows the job does not write stay zero."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(m)
    max_its = n_its if max_its is None else max_its
    words = max((n + 63) // 64, 1) if words is None else words
    keep = [_f(K1)[:4].copy(), _f(K2)[:4].copy(), _f(sigma2_1), _f(sigma2_2),
            np.ascontiguousarray(draws, np.int32).reshape(-1)]
    rows = max(max_its, 1)
    hyp = np.zeros(rows, HYP_DTYPE)
    bits = np.zeros((rows, words), np.uint64)
    events = np.zeros(rows, np.int32)
    ne = np.zeros(1, np.int32)
    mm = m if n else np.zeros(1, MATCH_DTYPE)
    lib().s3_ransac(ptr(mm), n, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                    len(keep[2]), int(bool(fix_scale)), ptr(keep[4]), int(n_its), int(max_its),
                    int(min_inliers), words, ptr(hyp), ptr(bits), ptr(events), ptr(ne))
    return hyp, bits, events, int(ne[0])


class Solver:
    """The restatement's sequential solver: iterate / find over the draws given at construction
    (n_its = the effective mRansacMaxIts). indices1 = mvnIndices1, n1 = mN1 for the scatter."""

    def __init__(self, matches, draws, n_its, min_inliers, fix_scale, K1, K2, sigma2_1, sigma2_2,
                 indices1=None, n1=None):
        self.m = np.ascontiguousarray(matches, MATCH_DTYPE)
        self.n = len(self.m)
        self.words = max((self.n + 63) // 64, 1)
        self.indices1 = np.arange(self.n) if indices1 is None else np.asarray(indices1)
        self.n1 = self.n if n1 is None else int(n1)
        self._keep = [_f(K1)[:4].copy(), _f(K2)[:4].copy(), _f(sigma2_1), _f(sigma2_2),
                      np.ascontiguousarray(draws, np.int32).reshape(-1),
                      self.m if self.n else np.zeros(1, MATCH_DTYPE)]
        k = self._keep
        self._s = lib().s3_create(ptr(k[5]), self.n, ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(k[3]),
                                  len(k[2]), int(bool(fix_scale)), ptr(k[4]), int(n_its),
                                  int(min_inliers))

    def __del__(self):
        if getattr(self, "_s", None):
            lib().s3_destroy(self._s)
            self._s = None

    def _scatter(self, bits):
        vb = np.zeros(self.n1, bool)
        vb[self.indices1[unpack_bits(bits, self.n)]] = True
        return vb

    def iterate(self, n_iterations):
        """Returns (k or -1, bNoMore, vbInliers[n1], nInliers)."""
        nm, ni = C.c_int(), C.c_int()
        bits = np.zeros(self.words, np.uint64)
        k = lib().s3_iterate(self._s, int(n_iterations), C.byref(nm), C.byref(ni), ptr(bits))
        assert k >= -1
        return k, bool(nm.value), self._scatter(bits), ni.value

    def find(self):
        """Returns (k or -1, vbInliers[n1], nInliers)."""
        ni = C.c_int()
        bits = np.zeros(self.words, np.uint64)
        k = lib().s3_find(self._s, C.byref(ni), ptr(bits))
        assert k >= -1
        return k, self._scatter(bits), ni.value

    def best(self):
        """(R 3x3, t, s) of GetEstimated*, or None while the reference's are still empty."""
        h = np.zeros(1, HYP_DTYPE)
        if not lib().s3_best(self._s, ptr(h)):
            return None
        return h[0]["R12"].reshape(3, 3).copy(), h[0]["t12"].copy(), float(h[0]["s12"])
