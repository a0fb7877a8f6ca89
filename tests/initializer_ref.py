"""Builds tests/initializer_ref.c on demand (gcc, the oracle Makefile's CFLAGS) and wraps it: the
CPU restatement of the monocular Initializer the device path is compared against bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "initializer_ref.c")
LIB = os.path.join(HERE, "libinitializer_ref.so")  # not "initializer_ref.so": import would load it
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

HYP_DTYPE = np.dtype([("M", "<f4", (9,)), ("score", "<f4"), ("pad", "<i4", (2,))])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("best", "<i4", (2,)), ("SH", "<f4"),
                         ("SF", "<f4"), ("RH", "<f4"), ("model", "<i4"), ("n_motions", "<i4"),
                         ("norm", "<f4", (8,)), ("pad", "<i4", (3,))])
MOTION_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("n_good", "<i4"),
                         ("cos_parallax", "<f4"), ("pad", "<i4", (2,))])
assert HYP_DTYPE.itemsize == 48 and RESULT_DTYPE.itemsize == 80 and MOTION_DTYPE.itemsize == 64
MAX_KEYS, MAX_ITS, MAX_MOTIONS = 8192, 512, 8

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
        for name, args, res in [
                ("init_svd", [vp, ip, ip, ip, vp, vp, vp], None),
                ("init_svd3", [vp, ip, vp, vp, vp], None),
                ("init_inv3", [vp, vp], None),
                ("init_det3", [vp], C.c_double),
                ("init_normalize", [vp, ip, vp], None),
                ("init_compute_h21", [vp, vp, ip, vp], None),
                ("init_compute_f21", [vp, vp, ip, vp], None),
                ("init_check_homography", [vp, vp, vp, vp, vp, ip, fp, vp], fp),
                ("init_check_fundamental", [vp, vp, vp, vp, ip, fp, vp], fp),
                ("init_resolve", [ip, vp, vp], ip),
                ("init_triangulate", [vp, vp, vp, vp, ip, vp], None),
                ("init_check_rt", [vp, vp, vp, ip, vp, vp, ip, vp, vp, fp, ip, vp, vp, vp], ip),
                ("init_decompose_e", [vp, ip, vp, vp, vp], None),
                ("init_motions_f", [vp, vp, ip, vp], ip),
                ("init_motions_h", [vp, vp, ip, vp], ip),
                ("init_ransac", [vp, ip, vp, ip, vp, vp, fp, vp, ip, ip, ip, vp, vp, vp, vp, vp, vp,
                                 vp], None),
                ("init_reconstruct", [vp, vp, ip, ip, vp, fp, ip, vp], ip)]:
            getattr(L, name).argtypes = args
            getattr(L, name).restype = res
        _lib = L
    return _lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def _sw(sweeps):
    return jacobi_sweeps() if sweeps is None else int(sweeps)


def jacobi_sweeps():
    return lib().init_jacobi_sweeps()


def svd(A, sweeps=None):
    """(d[n] descending, vt[n][n], ut[n][m]) in double of the float m x n matrix A."""
    A = np.ascontiguousarray(A, np.float32)
    m, n = A.shape
    d, vt, ut = np.zeros(n), np.zeros((n, n)), np.zeros((n, m))
    lib().init_svd(ptr(A), m, n, _sw(sweeps), ptr(d), ptr(vt), ptr(ut))
    return d, vt, ut


def svd3(A, sweeps=None):
    """cv::SVD::compute of a 3 x 3 CV_32F Mat: (w[3], u[3][3], vt[3][3]) as float."""
    A = _f(A)
    w, u, vt = np.zeros(3, np.float32), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    lib().init_svd3(ptr(A), _sw(sweeps), ptr(w), ptr(u), ptr(vt))
    return w, u, vt


def inv3(A):
    A, o = _f(A), np.zeros((3, 3), np.float32)
    lib().init_inv3(ptr(A), ptr(o))
    return o


def normalize(keys):
    """(meanX, meanY, sX, sY) of Normalize over all the keys."""
    k, o = _f(keys), np.zeros(4, np.float32)
    lib().init_normalize(ptr(k), len(k) // 2, ptr(o))
    return o


def compute_h21(p1, p2, sweeps=None):
    a, b, o = _f(p1), _f(p2), np.zeros((3, 3), np.float32)
    lib().init_compute_h21(ptr(a), ptr(b), _sw(sweeps), ptr(o))
    return o


def compute_f21(p1, p2, sweeps=None):
    a, b, o = _f(p1), _f(p2), np.zeros((3, 3), np.float32)
    lib().init_compute_f21(ptr(a), ptr(b), _sw(sweeps), ptr(o))
    return o


def unpack_bits(bits, n):
    """uint64 mask words (last axis) -> bool[..., n]."""
    b = np.ascontiguousarray(bits, np.uint64)
    u8 = np.unpackbits(b.view(np.uint8).reshape(*b.shape[:-1], -1), axis=-1, bitorder="little")
    return u8[..., :n].astype(bool)


def pack_bits(mask):
    m = np.asarray(mask, bool)
    out = np.zeros(max((len(m) + 63) // 64, 1) * 64, np.uint8)
    out[:len(m)] = m
    return np.packbits(out, bitorder="little").view(np.uint64).copy()


def _pairs(pairs):
    return np.ascontiguousarray(pairs, np.int32).reshape(-1)


def check_homography(H21, H12, keys1, keys2, pairs, sigma):
    """(score, bool[n])."""
    p = _pairs(pairs)
    n = len(p) // 2
    bits = np.zeros(max((n + 63) // 64, 1), np.uint64)
    keep = [_f(H21), _f(H12), _f(keys1), _f(keys2)]
    s = lib().init_check_homography(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(p),
                                    n, float(np.float32(sigma)), ptr(bits))
    return np.float32(s), unpack_bits(bits, n)


def check_fundamental(F21, keys1, keys2, pairs, sigma):
    p = _pairs(pairs)
    n = len(p) // 2
    bits = np.zeros(max((n + 63) // 64, 1), np.uint64)
    keep = [_f(F21), _f(keys1), _f(keys2)]
    s = lib().init_check_fundamental(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(p), n,
                                     float(np.float32(sigma)), ptr(bits))
    return np.float32(s), unpack_bits(bits, n)


def resolve(n, randi):
    r, idx = np.ascontiguousarray(randi, np.int32), np.zeros(8, np.int32)
    return idx if lib().init_resolve(int(n), ptr(r), ptr(idx)) else None


def triangulate(kp1, kp2, P1, P2, sweeps=None):
    keep = [_f(kp1), _f(kp2), _f(P1), _f(P2)]
    x = np.zeros(3, np.float32)
    lib().init_triangulate(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), _sw(sweeps),
                           ptr(x))
    return x


def check_rt(R, t, keys1, keys2, pairs, inliers, K, th2, sweeps=None):
    """(nGood, vbGood[n1], P3D[n1][3], the selected cosine)."""
    p = _pairs(pairs)
    n, k1, k2 = len(p) // 2, _f(keys1), _f(keys2)
    n1 = len(k1) // 2
    keep = [_f(R), _f(t), pack_bits(inliers), _f(K)]
    good = np.zeros(max((n1 + 63) // 64, 1), np.uint64)
    p3d, c = np.zeros((n1, 3), np.float32), np.zeros(1, np.float32)
    ng = lib().init_check_rt(ptr(keep[0]), ptr(keep[1]), ptr(k1), n1, ptr(k2), ptr(p), n,
                             ptr(keep[2]), ptr(keep[3]), float(np.float32(th2)), _sw(sweeps),
                             ptr(good), ptr(p3d), ptr(c))
    return ng, unpack_bits(good, n1), p3d, c[0]


def decompose_e(E, sweeps=None):
    E = _f(E)
    R1, R2, t = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    lib().init_decompose_e(ptr(E), _sw(sweeps), ptr(R1), ptr(R2), ptr(t))
    return R1, R2, t


def motions(M, K, model, sweeps=None):
    """The motions of ReconstructH (model 0) or ReconstructF (model 1): MOTION_DTYPE[n]."""
    keep, m = [_f(M), _f(K)], np.zeros(MAX_MOTIONS, MOTION_DTYPE)
    fn = lib().init_motions_h if model == 0 else lib().init_motions_f
    return m[:fn(ptr(keep[0]), ptr(keep[1]), _sw(sweeps), ptr(m))]


class Outputs:
    """One job's arrays in the device call's layout."""

    def __init__(self, max_n1, max_its, fill=0):
        self.max_n1, self.max_its = int(max_n1), int(max_its)
        self.words = (self.max_n1 + 63) // 64

        def z(shape, dt):
            a = np.zeros(shape, dt)
            a.view(np.uint8)[...] = fill
            return a
        self.hyp = z((2, self.max_its), HYP_DTYPE)
        self.bits = z((2, self.max_its, self.words), np.uint64)
        self.result = z(1, RESULT_DTYPE)
        self.pairs = z((self.max_n1, 2), np.int32)
        self.motion = z(MAX_MOTIONS, MOTION_DTYPE)
        self.good_bits = z((MAX_MOTIONS, self.words), np.uint64)
        self.p3d = z((MAX_MOTIONS, self.max_n1, 3), np.float32)

    def arrays(self):
        return [self.hyp, self.bits, self.result, self.pairs, self.motion, self.good_bits,
                self.p3d]


def ransac(keys1, keys2, matches12, K, sigma, draws, n_its, max_n1=None, max_its=None, fill=0):
    """The whole device call of one job: Outputs (rows the job does not write keep `fill`)."""
    k1, k2 = _f(keys1), _f(keys2)
    m = np.ascontiguousarray(matches12, np.int32)
    n1, n2 = len(k1) // 2, len(k2) // 2
    assert len(m) == n1
    o = Outputs(n1 if max_n1 is None else max_n1, n_its if max_its is None else max_its, fill)
    keep = [_f(K), np.ascontiguousarray(draws, np.int32).reshape(-1)]
    lib().init_ransac(ptr(k1), n1, ptr(k2), n2, ptr(m), ptr(keep[0]), float(np.float32(sigma)),
                      ptr(keep[1]), int(n_its), o.max_n1, o.max_its, *[ptr(a) for a in o.arrays()])
    return o


def reconstruct(o, n1, min_parallax=1.0, min_triangulated=50):
    """Initialize's return from the outputs: (ok, R21, t21, vP3D[n1][3], vbTriangulated[n1])."""
    ch = C.c_int()
    ok = lib().init_reconstruct(ptr(o.result), ptr(o.bits), o.max_n1, o.max_its, ptr(o.motion),
                                float(min_parallax), int(min_triangulated), C.byref(ch))
    if not ok:
        return False, None, None, None, None
    i = ch.value
    return (True, o.motion["R"][i].reshape(3, 3).copy(), o.motion["t"][i].copy(),
            o.p3d[i, :n1].copy(), unpack_bits(o.good_bits[i], n1))


def draw_schedule(n, n_its, random_int):
    """The eight RandomInt values per iteration of :62-77."""
    d = np.zeros((n_its, 8), np.int32)
    for k in range(n_its):
        for j in range(8):
            d[k, j] = random_int(0, n - 1 - j)
    return d


def initialize(keys1, keys2, matches12, K, sigma, n_its, random_int):
    """Initializer::Initialize on the restatement. Returns reconstruct()'s tuple and the Outputs."""
    n = int((np.asarray(matches12) >= 0).sum())
    o = ransac(keys1, keys2, matches12, K, sigma, draw_schedule(n, n_its, random_int), n_its)
    return reconstruct(o, len(np.asarray(matches12))), o
