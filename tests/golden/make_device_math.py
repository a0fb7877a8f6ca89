"""Generator of tests/golden/device_math.npz: inputs, 50-digit expected outputs and per-class
bounds for the device helpers that tests/device_math_check runs (layout and error metric:
tests/device_math_spec.py).

    python tests/golden/make_device_math.py [out.npz]

Every formula is stated here in mpmath, from g2o's sim3.h / se3quat.h / se3_ops.hpp and Eigen's
quaternion rules (Quaternion(Matrix3), toRotationMatrix, q * v, PartialPivLU's result), branch
for branch: the reference is what g2o's text computes in exact arithmetic, not the mathematical
exponential (g2o's small-angle branches differ from it by up to 2e-4). Where g2o's formula is
exact the generator asserts agreement with an independent definition to 1e-30 (mp.expm of the
generator matrix, log(exp(u)) = u, matrix products and inverses, an mp linear solve).

Per class it also evaluates a plain float64 statement of the same formulas (the oracle's exported
sim3 / se3 primitives; numpy transcriptions of the unblocked algorithms for the rest), records
its largest error E_cpu, and sets the device bound to 16 * max(E_cpu, 2^-52). rcp_nr, rsq_nr and
Huber carry the fixed 2 ulps instead. Seeds are fixed: a second run writes the same arrays.
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import device_math_spec as DS  # noqa: E402
import oracle_lib as O  # noqa: E402

mp.mp.dps = 50
mpf = mp.mpf
EPS = mpf(0.00001)  # g2o's `double eps = 0.00001` is the double nearest 1e-5
DBL_MIN = mpf(sys.float_info.min)
TOL_INDEP = mpf(10) ** -30
NAN = float("nan")


def f64(x):
    return float(x)


def M(v):
    return [mpf(float(x)) for x in v]


def ulps(x, k):
    """x moved by k ulps (k may be negative)."""
    x = float(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


# ---- mp statements of the formulas -------------------------------------------------------------
def skew(w):
    return [0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0]


def mat3(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j]
            for i in range(3) for j in range(3)]


def mat3v(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def lin3(ca, A, cb, B, cc):  # ca A + cb B + cc I
    return [ca * A[i] + cb * B[i] + (cc if i % 4 == 0 else 0) for i in range(9)]


def quat_from_R(R):
    """Eigen Quaternion(Matrix3): trace branch, else the largest diagonal entry i (first i = 0,
    replaced by 1 if R11 > R00, then by 2 if R22 > R(i, i)). Returns (x, y, z, w)."""
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        t = mp.sqrt(tr + 1)
        w = t / 2
        t = mpf(0.5) / t
        return [(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w]
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = mp.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1)
    q = [0, 0, 0, 0]
    q[i] = t / 2
    t = mpf(0.5) / t
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def quat_to_R(q):
    x, y, z, w = q
    return [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rotate(q, v):  # Eigen: v + w uv + qv x uv, uv = 2 qv x v
    uv = [2 * c for c in cross(q[:3], v)]
    c2 = cross(q[:3], uv)
    return [v[i] + q[3] * uv[i] + c2[i] for i in range(3)]


def quat_mul(p, q):
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return [pw * qx + px * qw + py * qz - pz * qy, pw * qy + py * qw + pz * qx - px * qz,
            pw * qz + pz * qw + px * qy - py * qx, pw * qw - px * qx - py * qy - pz * qz]


def normalize_rotation(q):
    if q[3] < 0:
        q = [-c for c in q]
    n = mp.sqrt(sum(c * c for c in q))
    return [c / n for c in q]


def se3_exp(u, small=None):
    """SE3Quat::exp: (q, t). `small` forces the theta < 1e-5 decision (None: g2o's rule)."""
    w, ups = u[:3], u[3:6]
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    Om = skew(w)
    Om2 = mat3(Om, Om)
    if (th < EPS) if small is None else small:
        R = lin3(1, Om, 1, Om2, 1)
        V = R
    else:
        R = lin3(mp.sin(th) / th, Om, (1 - mp.cos(th)) / (th * th), Om2, 1)
        V = lin3((1 - mp.cos(th)) / (th * th), Om, (th - mp.sin(th)) / th ** 3, Om2, 1)
    return normalize_rotation(quat_from_R(R)), mat3v(V, ups), R


def se3_left_update(u, Tq, Tt, small=None):
    """exp(u) * T with SE3Quat::operator*: (R(q), t) of the product, 12 values."""
    q, t, _ = se3_exp(u, small)
    rt = quat_rotate(q, Tt)
    qo = normalize_rotation(quat_mul(q, Tq))
    return quat_to_R(qo) + [t[i] + rt[i] for i in range(3)]


def sim3_coeffs(theta, sigma, s, small_t, small_s):
    if small_s:
        C = mpf(1)
        if small_t:
            A, B = mpf(1) / 2, mpf(1) / 6
        else:
            A = (1 - mp.cos(theta)) / theta ** 2
            B = (theta - mp.sin(theta)) / theta ** 3
    else:
        C = (s - 1) / sigma
        if small_t:
            A = ((sigma - 1) * s + 1) / sigma ** 2
            B = ((sigma ** 2 / 2 - sigma + 1) * s) / sigma ** 3
        else:
            a, b = s * mp.sin(theta), s * mp.cos(theta)
            c = theta ** 2 + sigma ** 2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    return A, B, C


def sim3_exp(u, small_t=None):
    """Sim3(Vector7d): (q, t, s) with the quaternion as Quaterniond(R) leaves it."""
    w, ups, sigma = u[:3], u[3:6], u[6]
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    Om = skew(w)
    Om2 = mat3(Om, Om)
    s = mp.exp(sigma)
    st = (th < EPS) if small_t is None else small_t
    ss = abs(sigma) < EPS
    A, B, C = sim3_coeffs(th, sigma, s, st, ss)
    if st:
        R = lin3(1, Om, 1, Om2, 1)
    else:
        R = lin3(mp.sin(th) / th, Om, (1 - mp.cos(th)) / (th * th), Om2, 1)
    return quat_from_R(R), mat3v(lin3(A, Om, B, Om2, C), ups), s


def sim3_log(q, t, s, flip_d=False, flip_s=False):
    sigma = mp.log(s)
    R = quat_to_R(q)
    d = (R[0] + R[4] + R[8] - 1) / 2
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    sd = (d > 1 - EPS) != flip_d
    ss = (abs(sigma) < EPS) != flip_s
    if sd:
        om = [c / 2 for c in dR]
        th = mpf(0)
    else:
        th = mp.acos(d)
        f = th / (2 * mp.sqrt(1 - d * d))
        om = [f * c for c in dR]
    A, B, C = sim3_coeffs(th, sigma, s, sd, ss)
    Om = skew(om)
    W = lin3(A, Om, B, mat3(Om, Om), C)
    ups = mp.lu_solve(mp.matrix([W[0:3], W[3:6], W[6:9]]), mp.matrix(t))  # W.lu().solve(t)
    return om + [ups[i] for i in range(3)] + [sigma]


def sim3_mul(a, b):
    (qa, ta, sa), (qb, tb, sb) = a, b
    rt = quat_rotate(qa, tb)
    return quat_mul(qa, qb), [sa * rt[i] + ta[i] for i in range(3)], sa * sb


def sim3_inverse(a):
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    return qc, quat_rotate(qc, [(-1 / s) * c for c in t]), 1 / s


def sim3_matrix(S):
    """4x4 homogeneous matrix of (q, t, s) as a similarity acting on points (map)."""
    q, t, s = S
    R = quat_to_R(q)
    return mp.matrix([[s * R[0], s * R[1], s * R[2], t[0]], [s * R[3], s * R[4], s * R[5], t[1]],
                      [s * R[6], s * R[7], s * R[8], t[2]], [0, 0, 0, 1]])


def ldlt_solve(H, b, lam):
    """g2o's dense LDLT (Eigen's rules): no pivoting, a zero pivot gives a zero component, a
    negative one fails. H: n x n list of lists. Returns (ok, x)."""
    n = len(b)
    L = [[mpf(0)] * n for _ in range(n)]
    d = [mpf(0)] * n
    for j in range(n):
        dj = H[j][j] + lam - sum(L[j][k] ** 2 * d[k] for k in range(j))
        d[j] = dj
        if dj < 0:
            return False, None
        for i in range(j + 1, n):
            s = H[i][j] - sum(L[i][k] * L[j][k] * d[k] for k in range(j))
            L[i][j] = s / dj if dj > DBL_MIN else mpf(0)
    y = [mpf(0)] * n
    for i in range(n):
        y[i] = b[i] - sum(L[i][k] * y[k] for k in range(i))
    y = [y[i] / d[i] if abs(d[i]) > DBL_MIN else mpf(0) for i in range(n)]
    x = [mpf(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - sum(L[k][i] * x[k] for k in range(i + 1, n))
    return True, x


def mp_err(a, b):
    return max(abs(x - y) for x, y in zip(a, b))


# ---- float64 baselines -------------------------------------------------------------------------
def np_ldlt_solve(H, b, lam):
    n = len(b)
    A = np.array(H, np.float64)
    d = np.zeros(n)
    for j in range(n):
        dj = A[j, j] + lam
        for k in range(j):
            dj -= A[j, k] * A[j, k] * d[k]
        d[j] = dj
        if dj < 0:
            return False, None
        for i in range(j + 1, n):
            s = A[i, j]
            for k in range(j):
                s -= A[i, k] * A[j, k] * d[k]
            A[i, j] = s / dj if dj > sys.float_info.min else 0.0
    y = np.zeros(n)
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= A[i, k] * y[k]
        y[i] = s
    for i in range(n):
        y[i] = y[i] / d[i] if abs(d[i]) > sys.float_info.min else 0.0
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= A[k, i] * x[k]
        x[i] = s
    return True, x


def np_quat_from_R(R):
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w])
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
    q = np.zeros(4)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def np_quat_rotate(q, v):
    uv = 2 * np.cross(q[:3], v)
    return v + q[3] * uv + np.cross(q[:3], uv)


# ---- random inputs -----------------------------------------------------------------------------
def rand_unit(rng, n=3):
    v = rng.standard_normal(n)
    return v / np.linalg.norm(v)


def rand_quat(rng):
    return rand_unit(rng, 4)


class Cases:
    """Collects one operation's cases."""

    def __init__(self, op):
        self.op, self.classes = op, []
        self.inp, self.ref, self.lo, self.alt, self.base, self.cls = [], [], [], [], [], []

    def add(self, cls, inp, ref, base, alt=None):
        """ref / alt: lists of mpf in comparable space; base: float64 baseline (comparable)."""
        if cls not in self.classes:
            self.classes.append(cls)
        r = [f64(x) for x in ref]
        self.inp.append([float(x) for x in inp])
        self.ref.append(r)
        self.lo.append([f64(mpf(x) - mpf(y)) for x, y in zip(ref, r)])
        self.alt.append([f64(x) for x in alt] if alt is not None else [NAN] * len(r))
        self.base.append(None if base is None else [float(x) for x in base])
        self.cls.append(self.classes.index(cls))

    def finish(self, out):
        op = self.op
        spec = DS.OPS[op]
        inp, ref = np.array(self.inp, np.float64), np.array(self.ref, np.float64)
        lo, alt = np.array(self.lo, np.float64), np.array(self.alt, np.float64)
        cls = np.array(self.cls, np.int32)
        if self.base[0] is None:  # the oracle's exported primitives are the float64 statement
            base = DS.oracle_baseline(op, inp)
        else:
            base = np.array(self.base, np.float64)
        assert inp.shape[1] == spec["win"], (op, inp.shape)
        is_ulp = any(g[2] == DS.ULP for g in spec["groups"])
        err = DS.case_errors(op, base, ref, lo if is_ulp else None, alt)
        ecpu = np.array([err[cls == c].max() for c in range(len(self.classes))])
        assert np.isfinite(ecpu).all(), (op, dict(zip(self.classes, ecpu)))
        if is_ulp:
            bound = np.full(len(ecpu), 2.0)
        else:
            bound = DS.MARGIN * np.maximum(ecpu, DS.EPS52)
        for c in DS.CAPPED.get(op, []):
            e = ecpu[self.classes.index(c)]
            assert e <= DS.CAP, f"{op}/{c}: E_cpu {e:.3g} past the cap"
        share = (~np.isnan(alt).any(1)).mean()
        assert share <= DS.ALT_SHARE, f"{op}: {share:.3f} of the cases may match either branch"
        for c, k in DS.MIN_CASES[op].items():
            assert c in self.classes and (cls == self.classes.index(c)).sum() >= k, (op, c)
        out[op + "/in"], out[op + "/ref"], out[op + "/alt"] = inp, ref, alt
        if is_ulp:
            out[op + "/ref_lo"] = lo
        out[op + "/cls"], out[op + "/classes"] = cls, np.array(self.classes)
        out[op + "/ecpu"], out[op + "/bound"] = ecpu, bound
        for c, e, b in zip(self.classes, ecpu, bound):
            print(f"{op:20s} {c:26s} n={int((cls == self.classes.index(c)).sum()):4d} "
                  f"E_cpu={e:9.3g} bound={b:9.3g}")


# ---- rcp_nr, rsq_nr, Huber ---------------------------------------------------------------------
def gen_recip(out):
    rng = np.random.default_rng(101)
    xs = {
        "log_uniform": 10.0 ** rng.uniform(-300, 300, 128),
        "pow2": 2.0 ** np.arange(-160, 160, 5),
        "near_one": np.array([ulps(1.0, k) for k in range(-16, 17)]),
        "pivots": 10.0 ** rng.uniform(-6, 12, 128),
    }
    for op, fn, nf in (("rcp_nr", lambda x: 1 / x, lambda x: 1.0 / x),
                       ("rsq_nr", lambda x: 1 / mp.sqrt(x), lambda x: 1.0 / np.sqrt(x))):
        C = Cases(op)
        for cls, v in xs.items():
            for x in v:
                C.add(cls, [x], [fn(mpf(float(x)))], [nf(float(x))])
        C.finish(out)


def gen_huber(out):
    for op, wout in (("huber", 4), ("huber_sim3", 2)):
        C = Cases(op)
        for cls, chi2 in (("mono", 5.991), ("stereo", 7.815)):
            # ORB-SLAM2's `const float delta = sqrt(5.991)`
            delta = float(np.float32(np.sqrt(chi2)))
            d2 = delta * delta  # the double g2o compares e with
            for e in (0.0, ulps(d2, -1), d2, ulps(d2, 1), 1e12):
                me, md = mpf(e), mpf(delta)
                if me > mpf(d2):
                    r0, r1 = 2 * mp.sqrt(me) * md - mpf(d2), md / mp.sqrt(me)
                    b0 = 2 * np.sqrt(e) * delta - d2
                    b1 = delta / np.sqrt(e)
                else:
                    r0, r1, b0, b1 = me, mpf(1), e, 1.0
                ref, base = [r0, r1], [b0, b1]
                if wout == 4:
                    ref, base = [r0, r0, r0, r1], [b0, b0, b0, b1]
                C.add(cls, [e, delta], ref, base)
        C.finish(out)


# ---- ldlt_solve6 / ldlt_solve7 -----------------------------------------------------------------
def packed_upper(H):
    n = len(H)
    return [H[i][j] for i in range(n) for j in range(i, n)]


def rand_normal_matrix(rng, n, ill, lo=1e8, hi=1e10):
    """H = J'J (float64) of n..50 random rows with column scales so that the entries span about
    1e2..1e8 (the units of a pose's rotation and translation, of a scale), and J'r: condition
    number <= 1e6, or in [lo, hi] for `ill`."""
    while True:
        rows = int(rng.integers(n, max(51, 2 * n)))
        scale = 10.0 ** rng.uniform(1, 4 if ill else 2.2, n)
        J = rng.standard_normal((rows, n)) * scale
        H = J.T @ J
        H = 0.5 * (H + H.T)
        cond = np.linalg.cond(H)
        if (lo <= cond <= hi) if ill else cond <= 1e6:
            return H, J.T @ rng.standard_normal(rows)


def gen_ldlt(out, n, op, seed):
    rng = np.random.default_rng(seed)
    C = Cases(op)

    def add(cls, H, b, lam, check=False):
        Hm = [M(r) for r in H]
        ok, x = ldlt_solve(Hm, M(b), mpf(lam))
        okb, xb = np_ldlt_solve(H, b, lam)
        if check:  # an mp linear solve as the independent definition
            A = mp.matrix(Hm) + mpf(lam) * mp.eye(n)
            xs = mp.lu_solve(A, mp.matrix(M(b)))
            assert mp_err(x, list(xs)) <= TOL_INDEP * max(abs(v) for v in x), (op, cls)
        sent = [DS.SENTINEL] * n
        C.add(cls, packed_upper(H) + [lam] + list(b),
              [1] + x if ok else [0] + sent, [1.0] + list(xb) if okb else [0.0] + sent)

    lams = (0.0, 1e-16, 1e-5, 1e3)
    for k in range(128):
        ill = k >= 64
        H, b = rand_normal_matrix(rng, n, ill)
        add("spd_ill" if ill else "spd_well", H, b, lams[k % 4] * np.trace(H), check=True)
    for p in range(n):  # an exact zero row and column at each position
        for lam in (0.0, 1e-5):
            H, b = rand_normal_matrix(rng, n, False)
            H[p, :] = 0.0
            H[:, p] = 0.0
            b[p] = 0.0
            add("zero_rowcol", H, b, lam * np.trace(H))
    if n == 7:  # OptimizeSim3 with bFixScale: no scale column
        for k in range(8):
            H, b = rand_normal_matrix(rng, n, False)
            H[6, :] = 0.0
            H[:, 6] = 0.0
            b[6] = 0.0
            add("fix_scale", H, b, (0.0 if k % 2 else 1e-5 * np.trace(H)))
    for p in range(n):  # a clearly negative pivot at position p
        H, b = rand_normal_matrix(rng, n, False)
        H[p, p] -= 3.0 * H[p, p]
        add("indefinite", H, b, 0.0)
    C.finish(out)


# ---- SE3 ---------------------------------------------------------------------------------------
def rot_matrix_f64(axis, th):
    """The float64 rounding of the exact rotation about `axis` (normalised in mp) by th."""
    a = M(axis)
    n = mp.sqrt(sum(c * c for c in a))
    w = [c / n * mpf(th) for c in a]
    Om = skew(w)
    t = mpf(th)
    return [f64(x) for x in lin3(mp.sin(t) / t, Om, (1 - mp.cos(t)) / (t * t), mat3(Om, Om), 1)]


NEAR_PI_AXES = [(1, 0.1, -0.2), (0.1, 1, 0.2), (-0.2, 0.1, 1), (1, 1, 0.1), (1, 0.1, 1),
                (0.1, 1, 1),
                (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1),
                (-1, 0.3, 0.2), (0.3, -1, 0.2), (0.2, 0.3, -1), (1, 1, 1)]


def gen_se3(out):
    rng = np.random.default_rng(202)
    C = Cases("left_update")

    def pose(k):
        q = rand_quat(rng)
        if k % 8 == 1:
            q = -np.abs(q)  # w < 0
        if k % 8 == 2:
            q[3] = 0.0
            q /= np.linalg.norm(q)
        return q, rng.standard_normal(3) * 10.0 ** rng.uniform(-1, 3)

    def add(cls, w, k, either=False, check=False):
        u = list(w) + list(rng.standard_normal(3) * 10.0 ** rng.uniform(-2, 1))
        Tq, Tt = pose(k)
        um, qm, tm = M(u), M(Tq), M(Tt)
        ref = se3_left_update(um, qm, tm)
        alt = None
        if either:
            th = mp.sqrt(sum(c * c for c in um[:3]))
            alt = se3_left_update(um, qm, tm, small=not (th < EPS))
            alt = alt + alt
        if check:  # exp(u) against expm of the 4x4 generator, the product against matrices
            _, t, R = se3_exp(um)
            Om = skew(um[:3])
            G = mp.matrix([[Om[0], Om[1], Om[2], um[3]], [Om[3], Om[4], Om[5], um[4]],
                           [Om[6], Om[7], Om[8], um[5]], [0, 0, 0, 0]])
            E = mp.expm(G)
            assert mp_err(R + t, [E[i, j] for i in range(3) for j in range(3)] +
                          [E[i, 3] for i in range(3)]) <= TOL_INDEP, cls
            qn = normalize_rotation(qm)
            RT = quat_to_R(qn)
            prod = mat3(R, RT) + [t[i] + mat3v(R, tm)[i] for i in range(3)]
            assert mp_err(ref, prod) <= TOL_INDEP * 1000, cls
        C.add(cls, u + list(Tq) + list(Tt), ref + ref, None, alt)

    for k in range(8):
        add("theta_zero", [0.0, 0.0, 0.0], k)
        add("theta_1e-12", rand_unit(rng) * 1e-12, k)
    for i, k in enumerate((-8, -2, -1, 1, 2, 8)):  # t2 = 1e-10 +- ulps, on one axis at a time
        w = [0.0, 0.0, 0.0]
        w[i % 3] = float(np.sqrt(ulps(1e-10, k)))
        add("thr_t2_1e-10", w, i, either=True)
    for i, k in enumerate((-8, -2, -1, 1, 2, 8)):
        w = [0.0, 0.0, 0.0]
        w[i % 3] = float(np.sqrt(ulps(1e-4, k)))
        add("thr_t2_1e-4", w, i, check=True)
    for k in range(96):
        add("taylor", rand_unit(rng) * 10.0 ** rng.uniform(-5, -2), k, check=k < 8)
    for k in range(64):
        add("generic", rand_unit(rng) * rng.uniform(1e-2, 3.0), k, check=k < 8)
    th0 = float(mp.acos(mpf(-1) / 2))  # 1 + 2 cos(theta) = 0
    for k in range(16):
        add("trace_sign", rand_unit(rng) * (th0 + (1e-12 if k % 2 else -1e-12)), k)
    for k in range(64):
        a = np.array(NEAR_PI_AXES[k % 16], np.float64)
        th = np.pi - (1e-9, 1e-6, 1e-3, 0.2)[k // 16]
        add("near_pi", a / np.linalg.norm(a) * th, k, check=k % 16 == 0)
    for k in range(64):
        add("past_pi", rand_unit(rng) * rng.uniform(np.pi, 50.0), k, check=k < 4)
    C.finish(out)

    # quat_from_R, quat_to_R, normalize_rotation, quat_rotate on the same rotation classes
    C = Cases("quat_from_R")
    for k in range(64):
        R = rot_matrix_f64(rand_unit(rng), rng.uniform(0.0, 2.0))
        C.add("generic", R, quat_from_R(M(R)), np_quat_from_R(np.array(R)))
    for k in range(64):
        th = np.pi - (1e-9, 1e-6, 1e-3, 0.2)[k // 16]
        R = rot_matrix_f64(NEAR_PI_AXES[k % 16], th)
        assert abs(R[0] + R[4] + R[8]) > 1e-9
        C.add("near_pi", R, quat_from_R(M(R)), np_quat_from_R(np.array(R)))
    ties = [[1, 0, 0, 0, -1, 0, 0, 0, -1], [-1, 0, 0, 0, 1, 0, 0, 0, -1],
            [-1, 0, 0, 0, -1, 0, 0, 0, 1], [0, 1, 0, 1, 0, 0, 0, 0, -1],
            [0, 0, 1, 0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, 0, 1, 0, 1, 0]]
    for R in ties:  # half turns about the axes and about axes with two equal components
        R = [float(x) for x in R]
        C.add("ties", R, quat_from_R(M(R)), np_quat_from_R(np.array(R)))
    C.finish(out)

    Cn, Cr, Ct = Cases("normalize_rotation"), Cases("quat_rotate"), Cases("quat_to_R")
    for k in range(96):
        q = rand_quat(rng)
        if k % 4 == 1:
            q = -np.abs(q)
        if k % 4 == 2:
            q[3] = 0.0
        qs = q * 10.0 ** rng.uniform(-3, 3)
        n = np.sqrt((qs * qs).sum())
        Cn.add("generic", qs, normalize_rotation(M(qs)), (-qs if qs[3] < 0 else qs) / n)
        v = rng.standard_normal(3) * 10.0 ** rng.uniform(-1, 3)
        qm = M(q)
        ref = quat_rotate(qm, M(v))
        assert mp_err(ref, mat3v(quat_to_R(qm), M(v))) <= TOL_INDEP * 1e4  # q * v = R(q) v
        Cr.add("generic", list(q) + list(v), ref, np_quat_rotate(q, v))
        Ct.add("generic", q, quat_to_R(qm), DS.quat_to_R(q[None])[0])
    Cn.finish(out)
    Cr.finish(out)
    Ct.finish(out)


# ---- Sim3 --------------------------------------------------------------------------------------
def s8(S):
    q, t, s = S
    return list(q) + list(t) + [s]


def comp_sim3(S):  # comparable of a Sim3: R(q), t, s
    q, t, s = S
    return quat_to_R(q) + list(t) + [s]


def rand_sim3(rng, smin=-2, smax=2, tmax=4):
    q = rand_quat(rng)
    t = rng.standard_normal(3) * 10.0 ** rng.uniform(-1, tmax)
    return list(q), list(t), float(10.0 ** rng.uniform(smin, smax))


def gen_sim3(out):
    rng = np.random.default_rng(303)
    C = Cases("sim3_exp")
    eps = 0.00001

    def add_exp(cls, w, sigma, either=False, check=False):
        u = list(w) + list(rng.standard_normal(3) * 10.0 ** rng.uniform(-1, 3)) + [float(sigma)]
        um = M(u)
        S = sim3_exp(um)
        alt = None
        if either:
            th = mp.sqrt(sum(c * c for c in um[:3]))
            alt = comp_sim3(sim3_exp(um, small_t=not (th < EPS)))
        if check:  # g2o's formula is exact here: expm of [[sigma I + Omega, upsilon], [0, 0]]
            Om = skew(um[:3])
            G = mp.matrix([[um[6], Om[1], Om[2], um[3]], [Om[3], um[6], Om[5], um[4]],
                           [Om[6], Om[7], um[6], um[5]], [0, 0, 0, 0]])
            E = mp.expm(G)
            Mx = sim3_matrix(S)
            assert max(abs(E[i, j] - Mx[i, j]) for i in range(3) for j in range(4)) <= \
                TOL_INDEP * max(1, max(abs(x) for x in S[1])), cls
        C.add(cls, u, comp_sim3(S), None, alt)

    for k in range(16):
        add_exp("small_theta_small_sigma", rand_unit(rng) * 10.0 ** rng.uniform(-12, -5.1),
                rng.choice([-1, 1]) * 10.0 ** rng.uniform(-12, -5.1) * (k % 4 != 0))
        add_exp("small_theta", rand_unit(rng) * 10.0 ** rng.uniform(-12, -5.1) * (k % 4 != 0),
                rng.choice([-1, 1]) * rng.uniform(1e-4, 2.0))
        add_exp("small_sigma", rand_unit(rng) * rng.uniform(1e-4, 3.0),
                rng.choice([-1, 1]) * 10.0 ** rng.uniform(-12, -5.1) * (k % 4 != 0))
    for i, k in enumerate((-8, -2, -1, 1, 2, 8)):
        add_exp("thr_theta", rand_unit(rng) * ulps(eps, k), (0.3, 1e-7)[i % 2], either=True)
        # sigma is an input: |sigma| < eps is decided exactly, on both sides
        add_exp("thr_sigma", rand_unit(rng) * 0.7, (-1, 1)[i % 2] * ulps(eps, k))
    add_exp("thr_sigma", rand_unit(rng) * 0.7, eps)
    add_exp("thr_sigma", rand_unit(rng) * 0.7, -eps)
    for k in range(64):
        add_exp("generic", rand_unit(rng) * rng.uniform(2e-5, np.pi), rng.choice([-1, 1]) *
                rng.uniform(2e-5, 2.0), check=k < 12)
        add_exp("past_pi", rand_unit(rng) * rng.uniform(np.pi, 12.0), rng.uniform(-2, 2),
                check=k < 4)
    C.finish(out)

    C = Cases("sim3_log")

    def add_log(cls, w, sigma, norm=1.0, either=None, check=False, s_ulps=0):
        u = list(w) + list(rng.standard_normal(3) * 10.0 ** rng.uniform(-1, 2)) + [float(sigma)]
        Sx = sim3_exp(M(u))
        if check:  # log(exp(u)) = u where both formulas are exact
            back = sim3_log(*Sx)
            assert mp_err(back, M(u)) <= TOL_INDEP * 1e3, (cls, mp_err(back, M(u)))
        v = np.array([f64(x) for x in s8(Sx)])
        v[:4] *= norm
        v[7] = ulps(v[7], s_ulps)
        S = (M(v[:4]), M(v[4:7]), mpf(v[7]))
        ref = sim3_log(*S)
        alt = None
        if either == "d":
            alt = sim3_log(*S, flip_d=True)
        if either == "s":
            alt = sim3_log(*S, flip_s=True)
        C.add(cls, v, ref, None, alt)

    for k in range(96):
        add_log("generic", rand_unit(rng) * rng.uniform(0.01, 3.0),
                rng.choice([-1, 1]) * rng.uniform(1e-3, 2.0), check=k < 12)
    for k in range(64):
        add_log("norm_off", rand_unit(rng) * rng.uniform(0.01, 2.5),
                rng.choice([-1, 1]) * rng.uniform(1e-3, 2.0), norm=(1 + 1e-3, 1 - 1e-3)[k % 2])
    thd = float(mp.acos(1 - EPS))  # d = 1 - 1e-5
    for i, k in enumerate((-8, -2, -1, 1, 2, 8)):
        add_log("thr_d", rand_unit(rng) * thd * (1 + k * 1e-12), 0.3, either="d")
        add_log("thr_sigma", rand_unit(rng) * 0.7, (-eps, eps)[i % 2], either="s", s_ulps=k)
    for k in range(16):
        add_log("pi_1e-2", rand_unit(rng) * (np.pi - 1e-2), rng.uniform(-1, 1))
        add_log("pi_1e-4", rand_unit(rng) * (np.pi - 1e-4), rng.uniform(-1, 1))
        add_log("small_theta_small_sigma", rand_unit(rng) * 10.0 ** rng.uniform(-9, -3),
                rng.choice([-1, 1]) * 10.0 ** rng.uniform(-9, -5.1))
        add_log("small_sigma", rand_unit(rng) * rng.uniform(0.01, 3.0),
                rng.choice([-1, 1]) * 10.0 ** rng.uniform(-9, -5.1))
        add_log("small_theta", rand_unit(rng) * 10.0 ** rng.uniform(-9, -3),
                rng.choice([-1, 1]) * rng.uniform(1e-3, 2.0))
    C.finish(out)

    Cm, Ci, Ca = Cases("sim3_mul"), Cases("sim3_inverse"), Cases("sim3_affine")
    for k in range(64):
        a, b = rand_sim3(rng), rand_sim3(rng)
        am, bm = (M(a[0]), M(a[1]), mpf(a[2])), (M(b[0]), M(b[1]), mpf(b[2]))
        pm, im = sim3_mul(am, bm), sim3_inverse(am)
        # products and inverses against the 4x4 matrices, with the quaternions made exactly unit
        # (the rounded ones are off by 1e-16, and R(p q) = R(p) R(q) holds for unit p, q only)
        au, bu = (normalize_rotation(am[0]),) + am[1:], (normalize_rotation(bm[0]),) + bm[1:]
        Pm = sim3_matrix(au) * sim3_matrix(bu) - sim3_matrix(sim3_mul(au, bu))
        assert max(abs(x) for x in Pm) <= TOL_INDEP * 1e8
        Im = sim3_matrix(au) * sim3_matrix(sim3_inverse(au)) - mp.eye(4)
        assert max(abs(x) for x in Im) <= TOL_INDEP * 1e8
        Cm.add("generic", s8(a) + s8(b), s8(pm), None)
        Ci.add("generic", s8(a), s8(im), None)
        Rm = quat_to_R(am[0])
        Ca.add("generic", s8(a), [am[2] * x for x in Rm] + am[1],
               list(a[2] * DS.quat_to_R(np.array(a[0])[None])[0]) + a[1])
    Cm.finish(out)
    Ci.finish(out)
    Ca.finish(out)

    C = Cases("lu3_solve")
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]

    def dominant():
        """W whose partial pivoting keeps the row order: |W00| largest of column 0 and, after
        the first elimination, |W11'| > |W21'|."""
        while True:
            W = rng.standard_normal((3, 3))
            W[0, 0] = 3.0 * np.sign(W[0, 0]) * (1 + abs(W[0, 0]))
            S = W[1:, 1:] - np.outer(W[1:, 0], W[0, 1:]) / W[0, 0]
            if abs(S[0, 0]) > 1.5 * abs(S[1, 0]) and abs(np.linalg.det(W)) > 0.3:
                return W

    def add_lu(cls, W):
        b = rng.standard_normal(3) * 10.0
        x = mp.lu_solve(mp.matrix([M(r) for r in W]), mp.matrix(M(b)))
        C.add(cls, list(W.ravel()) + list(b), list(x), np.linalg.solve(W, b))

    for k in range(48):
        add_lu("pivot_orders", dominant()[list(perms[k % 6])] * 10.0 ** rng.uniform(-3, 3))
    for k in range(16):
        W = dominant()
        W[1] = W[1] * (W[0, 0] / W[1, 0]) if W[1, 0] != 0 else W[1]
        W[1, 0] = ulps(abs(W[0, 0]), (k % 5) - 2) * (1 if k % 2 else -1)  # |W10| ~ |W00|
        if abs(np.linalg.det(W)) < 1e-2:
            W[1, 1] += 2.0
        add_lu("near_tied", W)
    C.finish(out)


# ---- essential graph ---------------------------------------------------------------------------
def gen_eg(out):
    rng = np.random.default_rng(404)
    C = Cases("eg_edge_error")

    def mp_s(S):
        return (M(S[0]), M(S[1]), mpf(S[2]))

    def rnd(S):
        return ([f64(x) for x in S[0]], [f64(x) for x in S[1]], f64(S[2]))

    def add(cls, Mji, Si, Sj):
        err = sim3_mul(sim3_mul(mp_s(Mji), mp_s(Si)), sim3_inverse(mp_s(Sj)))
        e = sim3_log(*err)
        C.add(cls, s8(Mji) + s8(Si) + s8(Sj), e + [sum(x * x for x in e)], None)

    for k in range(96):
        Si, Sj = rand_sim3(rng, -0.3, 0.3, 1.5), rand_sim3(rng, -0.3, 0.3, 1.5)
        if k < 32:  # Sji = Sj Si^-1 rounded: the error is rounding noise, the small branches
            add("consistent", rnd(sim3_mul(mp_s(Sj), sim3_inverse(mp_s(Si)))), Si, Sj)
        else:
            add("random", rand_sim3(rng, -0.3, 0.3, 1.5), Si, Sj)
    for k in range(16):  # relative rotation a half turn less 1e-2 .. 1e-3
        Si, Sj = rand_sim3(rng, -0.3, 0.3, 1.5), rand_sim3(rng, -0.3, 0.3, 1.5)
        w = rand_unit(rng) * (np.pi - (1e-2, 1e-3)[k % 2])
        D = sim3_exp(M(list(w) + [0.1, -0.2, 0.3, 0.05]))
        add("half_turn", rnd(sim3_mul(D, sim3_mul(mp_s(Sj), sim3_inverse(mp_s(Si))))), Si, Sj)
    C.finish(out)

    C = Cases("eg_oplus_axis")
    for fix in (0, 1):
        for d in range(7):
            for h in (1e-9, -1e-9, 0.3, -0.3, 2e-5, 1e-5):
                S = rand_sim3(rng, -1, 1, 2)
                u = [0.0] * 7
                u[d] = h
                if fix:
                    u[6] = 0.0
                ref = sim3_mul(sim3_exp(M(u)), mp_s(S))
                C.add("fix_scale_on" if fix else "fix_scale_off", s8(S) + [d, h, fix],
                      comp_sim3(ref), None)
    C.finish(out)


# ---- eval_edge ---------------------------------------------------------------------------------
CAM = [float(np.float32(v)) for v in (718.856, 718.856, 607.1928, 185.2157, 386.1448)]


def inv_sigma2():
    v, s2 = [], np.float32(1.0)
    for _ in range(8):
        v.append(float(np.float32(1.0) / s2))
        s2 = np.float32(s2 * np.float32(1.44))
    return v


def gen_eval_edge(out):
    rng = np.random.default_rng(505)
    C = Cases("eval_edge")
    isig = inv_sigma2()

    def add(cls, z, stereo, octave, cam=CAM):
        fx, fy, cx, cy, bf = cam
        q = rand_quat(rng) * np.array([0.1, 0.1, 0.1, 1.0])
        R = DS.quat_to_R((q / np.linalg.norm(q))[None])[0]
        t = rng.standard_normal(3)
        Xc = np.array([rng.uniform(-0.8, 0.8) * z, rng.uniform(-0.3, 0.3) * z, z])
        Xw = (R.reshape(3, 3).T @ (Xc - t)).astype(np.float32).astype(np.float64)
        pc = R.reshape(3, 3) @ Xw + t
        u = float(np.float32(fx * pc[0] / pc[2] + cx + rng.normal(0, 1)))
        v = float(np.float32(fy * pc[1] / pc[2] + cy + rng.normal(0, 1)))
        ur = float(np.float32(u - bf / pc[2] + rng.normal(0, 1))) if stereo else -1.0
        if stereo and ur < 0:
            ur = 0.0
        p = [mat3v(M(R), M(Xw))[i] + mpf(float(t[i])) for i in range(3)]
        zf = float(pc[2])  # the reference divides in double, then rounds to float
        info = isig[min(max(octave, 0), 7)]
        if stereo:
            invz = mpf(float(np.float32(1.0 / f64(p[2]))))
            uu, vv = p[0] * invz * mpf(fx) + mpf(cx), p[1] * invz * mpf(fy) + mpf(cy)
            e = [mpf(u) - uu, mpf(v) - vv, mpf(ur) - (uu - mpf(bf) * invz)]
            izf = float(np.float32(1.0 / zf))
            ub, vb = pc[0] * izf * fx + cx, pc[1] * izf * fy + cy
            eb = [u - ub, v - vb, ur - (ub - bf * izf)]
        else:
            e = [mpf(u) - (p[0] / p[2] * mpf(fx) + mpf(cx)),
                 mpf(v) - (p[1] / p[2] * mpf(fy) + mpf(cy)), mpf(0)]
            eb = [u - (pc[0] / pc[2] * fx + cx), v - (pc[1] / pc[2] * fy + cy), 0.0]
        chi2 = mpf(info) * sum(x * x for x in e)
        if cls == "quotient":
            # R = I, X = 0, a unit camera and a zero observation: x = t0, y = t1, z = t2 exactly,
            # so e = -(x / z, y / z): the projection's quotient itself, for the claim that
            # x * (1 / z) plus one residual step is the correctly rounded quotient
            R, Xw, u, v = np.eye(3).ravel(), np.zeros(3), 0.0, 0.0
            t = np.array([rng.standard_normal() * z, rng.standard_normal() * z, z])
            p, pc = M(t), t
            e = [-p[0] / p[2], -p[1] / p[2], mpf(0)]
            eb = [-(pc[0] / pc[2]), -(pc[1] / pc[2]), 0.0]
            chi2 = mpf(info) * sum(x * x for x in e)
        C.add(cls, list(Xw) + [u, v, ur, octave] + list(R) + list(t) + list(cam),
              [chi2] + e + [p[0], p[1], 1 / p[2], 1 if stereo else 0, info],
              [info * sum(x * x for x in eb)] + eb +
              [pc[0], pc[1], 1.0 / pc[2], float(stereo), info])

    for k in range(64):
        add("mono", 10.0 ** rng.uniform(-1, 2), False, k % 8)
        add("stereo", 10.0 ** rng.uniform(-1, 2), True, k % 8)
    for k, o in enumerate((-100, -3, -1, 0, 7, 8, 9, 100)):
        add("octave_clamps", 5.0, False, o)
        add("octave_clamps", 5.0, True, o)
    for k in range(256):
        add("quotient", 10.0 ** rng.uniform(-1, 2), False, 0, (1.0, 1.0, 0.0, 0.0, 1.0))
    C.finish(out)


# ---- ba_ldlt.h ---------------------------------------------------------------------------------
def tri(i):
    return i * (i + 1) // 2


def packed_lower(A):
    return [A[i][j] for i in range(len(A)) for j in range(i + 1)]


def diag_ldlt(A, y, num=mpf):
    """ba::diag_ldlt on a packed-lower 6x6 (list of 21) and y (6): right-looking LDLT, a zero
    pivot takes reciprocal 0. Returns good, A, y, rdg."""
    A, y, rdg, good = list(A), list(y), [num(0)] * 6, True
    for c in range(6):
        d = A[tri(c) + c]
        good = good and d != 0
        rd = 1 / d if d != 0 else num(0)
        rdg[c] = rd
        l = [num(0)] * 6
        for r in range(c + 1, 6):
            l[r] = A[tri(r) + c] * rd
            y[r] = y[r] - l[r] * y[c]
            A[tri(r) + c] = l[r]
        for r in range(c + 1, 6):
            ld = l[r] * d
            for k in range(c + 1, r + 1):
                A[tri(r) + k] = A[tri(r) + k] - ld * l[k]
    return good, A, y, rdg


def rand_spd(rng, n, cond_lo, cond_hi):
    """A Schur-complement-like SPD matrix (float64, symmetric) with a condition number in range."""
    while True:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        ev = 10.0 ** rng.uniform(0, np.log10(cond_hi), n)
        ev[0], ev[-1] = 1.0, 10.0 ** rng.uniform(np.log10(cond_lo), np.log10(cond_hi))
        S = (Q * ev) @ Q.T * 10.0 ** rng.uniform(0, 4)
        S = 0.5 * (S + S.T)
        if cond_lo * 0.5 <= np.linalg.cond(S) <= cond_hi * 2:
            return S


def gen_ba(out):
    rng = np.random.default_rng(606)
    C = Cases("tri_rc")
    for e in range(171):
        r = 0
        while tri(r + 1) <= e:
            r += 1
        C.add("all", [e], [r, e - tri(r)], [r, e - tri(r)])
    C.finish(out)

    C = Cases("diag_ldlt")

    def add_diag(cls, S, y):
        g, A, yy, rdg = diag_ldlt(M(packed_lower(S)), M(y))
        gb, Ab, yb, rb = diag_ldlt([np.float64(v) for v in packed_lower(S)],
                                   [np.float64(v) for v in y], np.float64)
        C.add(cls, packed_lower(S) + list(y), [int(g)] + A + yy + rdg, [float(gb)] + Ab + yb + rb)
        return A, yy, rdg

    for k in range(64):
        S = rand_spd(rng, 6, 1.0, 1e4)
        y = rng.standard_normal(6) * 10.0
        A, yy, _ = add_diag("spd", S, y)
        if k < 8:  # L D L' = S and L yy = y, by matrix products
            L = mp.matrix(6, 6)
            D = mp.matrix(6, 6)
            for i in range(6):
                L[i, i] = 1
                D[i, i] = A[tri(i) + i]
                for j in range(i):
                    L[i, j] = A[tri(i) + j]
            E = L * D * L.T - mp.matrix([M(r) for r in S])
            assert max(abs(x) for x in E) <= TOL_INDEP * 1e8
            assert mp_err(list(L * mp.matrix(yy)), M(y)) <= TOL_INDEP * 1e4
    for c in range(6):  # an exact zero pivot at c: row and column c are zero
        S = rand_spd(rng, 6, 1.0, 1e3)
        S[c, :] = 0.0
        S[:, c] = 0.0
        add_diag("zero_pivot", S, rng.standard_normal(6))
    for c in range(6):  # a negative pivot at c still factors
        S = rand_spd(rng, 6, 1.0, 1e2)
        S[c, c] -= 3.0 * S[c, c]
        add_diag("negative_pivot", S, rng.standard_normal(6))
    C.finish(out)

    Cp, Cb = Cases("panel_row"), Cases("block_back6")
    for k in range(64):
        a, L = rng.standard_normal(6) * 10.0, rng.standard_normal(15)
        rdg, yj, r = 10.0 ** rng.uniform(-3, 1, 6), rng.standard_normal(6), rng.standard_normal()

        def panel(a, L, rdg, yj, r):
            v, q = [None] * 6, 0
            for c in range(6):
                s = a[c]
                for kk in range(c):
                    s = s - v[kk] * L[q]
                    q += 1
                v[c] = s
            l = [v[c] * rdg[c] for c in range(6)]
            for c in range(6):
                r = r - l[c] * yj[c]
            return v + l + [r]

        Cp.add("generic", list(a) + list(L) + list(rdg) + list(yj) + [r],
               panel(M(a), M(L), M(rdg), M(yj), mpf(float(r))),
               panel(list(a), list(L), list(rdg), list(yj), r))
        z = rng.standard_normal(6)

        def back(Lb, x):
            x = list(x)
            for c in range(5, -1, -1):
                for rr in range(c):
                    x[rr] = x[rr] - Lb[c * (c - 1) // 2 + rr] * x[c]
            return x

        xm = back(M(L), M(z))
        Lt = mp.eye(6)  # L^T x = z with L(c, k) = Lb[c (c - 1) / 2 + k]
        for c in range(1, 6):
            for kk in range(c):
                Lt[kk, c] = mpf(float(L[c * (c - 1) // 2 + kk]))
        assert mp_err(list(mp.lu_solve(Lt, mp.matrix(M(z)))), xm) <= TOL_INDEP * 1e4
        Cb.add("generic", list(L) + list(z), xm, back(list(L), list(z)))
    Cp.finish(out)
    Cb.finish(out)

    C = Cases("factor_diag_block")
    for k in range(64):
        S = rand_spd(rng, 12, 1.0, 1e4)
        rhs = rng.standard_normal(12)
        Lp = packed_lower(S)

        def fdb(Lp, rhs, num):
            Lp, rhs = list(Lp), list(rhs)
            A = [Lp[tri(6 + r) + 6 + kk] for r in range(6) for kk in range(r + 1)]
            g, A, y, rdg = diag_ldlt(A, rhs[6:], num)
            dg, idg = [DS.SENTINEL] * 12, [DS.SENTINEL] * 12
            for r in range(6):
                for kk in range(r):
                    Lp[tri(6 + r) + 6 + kk] = A[tri(r) + kk]
                dg[6 + r], idg[6 + r], rhs[6 + r] = A[tri(r) + r], rdg[r], y[r]
            L15 = [Lp[tri(6 + c) + 6 + kk] for c in range(1, 6) for kk in range(c)]
            return [int(g)] + Lp + rhs + dg + idg + L15

        C.add("spd", Lp + list(rhs), fdb(M(Lp), M(rhs), mpf),
              fdb([np.float64(v) for v in Lp], [np.float64(v) for v in rhs], np.float64))
    C.finish(out)

    C = Cases("block_solve")
    for K in (1, 2, 3):
        for ill in (False, True):
            for k in range(16):
                n = 6 * K
                S, rhs = rand_normal_matrix(rng, n, ill, 1e7, 2e8)
                x = mp.lu_solve(mp.matrix([M(r) for r in S]), mp.matrix(M(rhs)))
                _, xb = np_ldlt_solve(S, rhs, 0.0)
                pad = [0.0] * (171 - tri(n))
                C.add(f"K{K}_{'ill' if ill else 'well'}", [K] + packed_lower(S) + pad + list(rhs) +
                      [0.0] * (18 - n), [1] + list(x) + [0] * (18 - n),
                      [1.0] + list(xb) + [0.0] * (18 - n))
    C.finish(out)


def generate() -> dict:
    O.build()
    out = {}
    gen_recip(out)
    gen_huber(out)
    gen_ldlt(out, 6, "ldlt_solve6", 111)
    gen_ldlt(out, 7, "ldlt_solve7", 112)
    gen_se3(out)
    gen_sim3(out)
    gen_eg(out)
    gen_eval_edge(out)
    gen_ba(out)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "device_math.npz")
    arrays = generate()
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")
