"""Builds tests/pnpsolver_ref.c on demand (gcc, the oracle Makefile's CFLAGS) and wraps it: the
CPU restatement of the RANSAC EPnP solver the device path is compared against bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pnpsolver_ref.c")
LIB = os.path.join(HERE, "libpnpsolver_ref.so")  # not "pnpsolver_ref.so": import would load it
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

MATCH_DTYPE = np.dtype([("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("octave", "<i4")])
HYP_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("n_inliers", "<i4"),
                      ("best", "<i4"), ("pad", "<i4", (2,))])
assert MATCH_DTYPE.itemsize == 24 and HYP_DTYPE.itemsize == 64
N_STAGES = 394

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
        vp, ip, fp, dp = C.c_void_p, C.c_int, C.c_float, C.c_double
        L.pnp_svd.argtypes = [vp, ip, ip, ip, vp, vp, vp]
        L.pnp_svd.restype = None
        L.pnp_svd_solve.argtypes = [vp, ip, ip, vp, ip, vp]
        L.pnp_svd_solve.restype = None
        L.pnp_epnp.argtypes = [vp, vp, ip, vp, ip, vp, vp, vp, vp]
        L.pnp_epnp.restype = None
        L.pnp_threshold.argtypes = [fp, fp]
        L.pnp_threshold.restype = fp
        L.pnp_resolve.argtypes = [ip, vp, vp]
        L.pnp_check_inliers.argtypes = [vp, ip, vp, vp, vp, vp, ip, fp, vp, ip, vp]
        L.pnp_check_inliers.restype = None
        L.pnp_ransac.argtypes = [vp, ip, vp, vp, ip, fp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp]
        L.pnp_ransac.restype = None
        L.pnp_create.argtypes = [vp, ip, vp, vp, ip, fp, vp, ip, ip, ip]
        L.pnp_create.restype = vp
        L.pnp_destroy.argtypes = [vp]
        L.pnp_destroy.restype = None
        L.pnp_iterate.argtypes = [vp, ip, vp, vp, vp, vp]
        L.pnp_find.argtypes = [vp, vp, vp, vp]
        L.pnp_iterations.argtypes = [vp]
        L.pnp_refines.argtypes = [vp]
        L.pnp_parameters.argtypes = [ip, dp, ip, ip, ip, fp, vp, vp]
        L.pnp_parameters.restype = None
        _lib = L
    return _lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def jacobi_sweeps():
    return lib().pnp_jacobi_sweeps()


def qr_zero_returns():
    """How often qr_solve took its zero-column return since the library was loaded."""
    return lib().pnp_qr_zero_returns()


def svd(A, sweeps=None):
    """(d[n] descending, vt[n][n], ut[n][m]) of the m x n matrix A by the contract's routine."""
    A = np.ascontiguousarray(A, np.float64)
    m, n = A.shape
    d, vt, ut = np.zeros(n), np.zeros((n, n)), np.zeros((n, m))
    lib().pnp_svd(ptr(A), m, n, jacobi_sweeps() if sweeps is None else int(sweeps), ptr(d), ptr(vt),
                  ptr(ut))
    return d, vt, ut


def svd_solve(A, b, sweeps=None):
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    m, n = A.shape
    x = np.zeros(n)
    lib().pnp_svd_solve(ptr(A), m, n, ptr(b), jacobi_sweeps() if sweeps is None else int(sweeps),
                        ptr(x))
    return x


def epnp(matches, sel, K, sweeps=None, ut_override=None):
    """compute_pose over matches[sel]. Returns (R 3x3, t, stages dict)."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    s = np.ascontiguousarray(sel, np.int32)
    k = _f(K)[:4].copy()
    R, t, st = np.zeros(9), np.zeros(3), np.zeros(N_STAGES)
    uo = None if ut_override is None else np.ascontiguousarray(ut_override, np.float64)
    lib().pnp_epnp(ptr(m), ptr(s), len(s), ptr(k), jacobi_sweeps() if sweeps is None else int(sweeps),
                   ptr(uo), ptr(R), ptr(t), ptr(st))
    o = np.cumsum([0, 12, 144, 12, 144, 60, 6, 12, 3, 1])
    names = ["cws", "mtm", "d", "ut", "l_6x10", "rho", "betas", "rep_errors", "chosen"]
    shapes = [(4, 3), (12, 12), (12,), (12, 12), (6, 10), (6,), (3, 4), (3,), ()]
    stages = {nm: st[o[i]:o[i + 1]].reshape(sh).copy() for i, (nm, sh) in enumerate(zip(names, shapes))}
    stages["chosen"] = int(stages["chosen"])
    return R.reshape(3, 3), t, stages


def threshold(sigma2, th2):
    return float(lib().pnp_threshold(float(np.float32(sigma2)), float(np.float32(th2))))


def resolve(n, randi):
    """The sample of :144-154 for the four draws, or None when one is out of range."""
    r = np.ascontiguousarray(randi, np.int32)
    idx = np.zeros(4, np.int32)
    return idx if lib().pnp_resolve(int(n), ptr(r), ptr(idx)) else None


def unpack_bits(bits, n):
    """uint64 mask words (last axis) -> bool[..., n]."""
    b = np.ascontiguousarray(bits, np.uint64)
    u8 = np.unpackbits(b.view(np.uint8).reshape(*b.shape[:-1], -1), axis=-1, bitorder="little")
    return u8[..., :n].astype(bool)


def check_inliers(matches, R, t, K, sigma2, th2):
    """CheckInliers with mRi / mti in double. Returns (bool[n], count)."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(m)
    words = max((n + 63) // 64, 1)
    keep = [np.ascontiguousarray(R, np.float64).reshape(-1), np.ascontiguousarray(t, np.float64),
            _f(K)[:4].copy(), _f(sigma2)]
    bits = np.zeros(words, np.uint64)
    cnt = C.c_int()
    lib().pnp_check_inliers(ptr(m), n, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                            len(keep[3]), float(np.float32(th2)), ptr(bits), words, C.byref(cnt))
    return unpack_bits(bits, n), cnt.value


def ransac(matches, draws, n_its, min_inliers, K, sigma2, th2, max_its=None, words=None):
    """The whole schedule of one job in the device call's layout. Returns (hyp[max_its],
    bits[max_its][words], refined[max_its], refined_bits[max_its][words], events[max_its],
    n_events); rows the job does not write stay zero."""
    m = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(m)
    max_its = n_its if max_its is None else max_its
    words = max((n + 63) // 64, 1) if words is None else words
    keep = [_f(K)[:4].copy(), _f(sigma2), np.ascontiguousarray(draws, np.int32).reshape(-1)]
    rows = max(max_its, 1)
    hyp, refined = np.zeros(rows, HYP_DTYPE), np.zeros(rows, HYP_DTYPE)
    bits, rbits = np.zeros((rows, words), np.uint64), np.zeros((rows, words), np.uint64)
    events = np.zeros(rows, np.int32)
    ne = np.zeros(1, np.int32)
    mm = m if n else np.zeros(1, MATCH_DTYPE)
    lib().pnp_ransac(ptr(mm), n, ptr(keep[0]), ptr(keep[1]), len(keep[1]), float(np.float32(th2)),
                     ptr(keep[2]), int(n_its), int(max_its), int(min_inliers), words, ptr(hyp),
                     ptr(bits), ptr(refined), ptr(rbits), ptr(events), ptr(ne))
    return hyp, bits, refined, rbits, events, int(ne[0])


def parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
    """(effective mRansacMinInliers, mRansacMaxIts) of SetRansacParameters (:87-105)."""
    a, b = C.c_int(), C.c_int()
    lib().pnp_parameters(int(N), float(probability), int(minInliers), int(maxIterations),
                         int(minSet), float(np.float32(epsilon)), C.byref(a), C.byref(b))
    return a.value, b.value


class Solver:
    """The restatement's sequential solver: iterate / find over the draws given at construction
    (draws for len(draws) / 4 iterations; max_its = the effective mRansacMaxIts). indices =
    mvKeyPointIndices, n_kp = the frame's keypoint count for the scatter."""

    def __init__(self, matches, draws, min_inliers, max_its, K, sigma2, th2, indices=None,
                 n_kp=None):
        self.m = np.ascontiguousarray(matches, MATCH_DTYPE)
        self.n = len(self.m)
        self.words = max((self.n + 63) // 64, 1)
        self.indices = np.arange(self.n) if indices is None else np.asarray(indices)
        self.n_kp = self.n if n_kp is None else int(n_kp)
        self._keep = [_f(K)[:4].copy(), _f(sigma2),
                      np.ascontiguousarray(draws, np.int32).reshape(-1),
                      self.m if self.n else np.zeros(1, MATCH_DTYPE)]
        k = self._keep
        self._s = lib().pnp_create(ptr(k[3]), self.n, ptr(k[0]), ptr(k[1]), len(k[1]),
                                   float(np.float32(th2)), ptr(k[2]), len(k[2]) // 4,
                                   int(min_inliers), int(max_its))

    def __del__(self):
        if getattr(self, "_s", None):
            lib().pnp_destroy(self._s)
            self._s = None

    def _scatter(self, bits):
        vb = np.zeros(self.n_kp, bool)
        vb[self.indices[unpack_bits(bits, self.n)]] = True
        return vb

    def iterate(self, n_iterations):
        """Returns (hyp record or None, bNoMore, vbInliers[n_kp], nInliers)."""
        nm, ni = C.c_int(), C.c_int()
        bits = np.zeros(self.words, np.uint64)
        T = np.zeros(1, HYP_DTYPE)
        r = lib().pnp_iterate(self._s, int(n_iterations), C.byref(nm), C.byref(ni), ptr(bits),
                              ptr(T))
        assert r >= 0, "the draws ran out"
        return (T[0] if r else None), bool(nm.value), self._scatter(bits), ni.value

    def find(self):
        ni = C.c_int()
        bits = np.zeros(self.words, np.uint64)
        T = np.zeros(1, HYP_DTYPE)
        r = lib().pnp_find(self._s, C.byref(ni), ptr(bits), ptr(T))
        assert r >= 0, "the draws ran out"
        return (T[0] if r else None), self._scatter(bits), ni.value

    @property
    def iterations(self):
        return lib().pnp_iterations(self._s)

    @property
    def refines(self):
        return lib().pnp_refines(self._s)
