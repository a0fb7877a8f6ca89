"""Generator of tests/golden/eg_step.npz: 50-digit references and bounds for one linear step of
OptimizeEssentialGraph on the graphs of tests/eg_step_spec.py, and for eg_update / eg_finish.

    python tests/golden/make_eg_step.py [out.npz]

Per graph and lambda: x_ref solves (H + lambda I) x = b for the exact H and b (integers / 64,
eg_step_spec.dense_system) by iterative refinement: corrections from a float64 solve, residuals
in mpmath at 50 digits over H's nonzero entries only, until the last correction is below
1e-30 max|x|. The scale term sum x (lambda x + b) follows in mpmath, with components 6 mod 7 of x
zeroed for a fixed scale.

The float64 solve is a plain LDLT without pivoting written here (dense within the matrix's band).
Its first solve, before any refinement, is the baseline: E_cpu is its max|x - x_ref| / max|x_ref|
(and, for the scale term, its error relative to sum |x (lambda x + b)|), the largest over a
class's graphs, lambdas and scale modes; bound = MARGIN * max(E_cpu, 2^-52), device_math_spec's
rule and constants. No class's E_cpu may pass device_math_spec.CAP. The device's output plays no
part.

Discriminating power: for a graph's designated blocks, the solution with that one block of H
(and its transpose) zeroed differs from x_ref by at least 1000 * bound, or the generator fails.

eg_update and eg_finish: g2o's formulas in mpmath as tests/golden/make_device_math.py states
them; the finish values are the 50-digit values correctly rounded to float32.

The fixture holds no inputs, only a SHA-256 of the inputs eg_step_spec regenerates.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import device_math_spec as DS  # noqa: E402
import eg_step_spec as ES  # noqa: E402

mp.mp.dps = 50
mpf = mp.mpf
TOL_REFINE = mpf(10) ** -30
DISCRIMINATION = 1000.0


def _device_math_generator():
    spec = importlib.util.spec_from_file_location("make_device_math",
                                                  os.path.join(HERE, "make_device_math.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    mp.mp.dps = 50
    return m


# ---- the float64 baseline: LDLT without pivoting, dense within the band ------------------------
def ldlt(M, bw):
    n = len(M)
    L, d = np.zeros_like(M), np.zeros(n)
    for j in range(n):
        lo, hi = max(0, j - bw), min(n, j + bw + 1)
        v = L[j, lo:j] * d[lo:j]
        d[j] = M[j, j] - L[j, lo:j] @ v
        L[j + 1:hi, j] = (M[j + 1:hi, j] - L[j + 1:hi, lo:j] @ v) / d[j]
    return L, d


def ldlt_solve(L, d, bw, b):
    n = len(d)
    y = b.astype(np.float64).copy()
    for j in range(n):
        hi = min(n, j + bw + 1)
        y[j + 1:hi] -= L[j + 1:hi, j] * y[j]
    y /= d
    for j in range(n - 1, -1, -1):
        hi = min(n, j + bw + 1)
        y[j] -= L[j + 1:hi, j] @ y[j + 1:hi]
    return y


def bandwidth(st):
    F = st["F"]
    return 7 * int((np.arange(F) - st["start"]).max() if F else 0) + 6


# ---- the reference ---------------------------------------------------------------------------------
def refine(A64, b64, lam, L, d, bw):
    """(x as mpf list, the baseline's first solve): (A64 / 64 + lam I) x = b64 / 64."""
    n = len(b64)
    rows = [np.flatnonzero(A64[i]) for i in range(n)]
    a_int = [[int(v) for v in A64[i, rows[i]]] for i in range(n)]
    b_mp = [mpf(int(v)) / 64 for v in b64]
    lam_mp = mpf(lam)
    x = [mpf(0)] * n
    r = list(b_mp)
    first = None
    for _ in range(8):
        dx = ldlt_solve(L, d, bw, np.array([float(v) for v in r]))
        if first is None:
            first = dx.copy()
        x = [x[i] + mpf(float(dx[i])) for i in range(n)]
        xmax = max(abs(v) for v in x)
        if max(abs(mpf(float(v))) for v in dx) <= TOL_REFINE * xmax:
            return x, first
        r = [b_mp[i] - lam_mp * x[i] - mp.fdot(zip(a_int[i], (x[j] for j in rows[i]))) / 64
             for i in range(n)]
    raise AssertionError("the refinement did not converge")


def scale_terms(x, b64, lam, fix_scale):
    """(sum x (lam x + b), sum |x (lam x + b)|) in mpmath."""
    lam_mp = mpf(lam)
    t = [mpf(0) if (fix_scale and i % 7 == 6) else x[i] * (lam_mp * x[i] + mpf(int(b64[i])) / 64)
         for i in range(len(x))]
    return mp.fsum(t), mp.fsum(abs(v) for v in t)


def solve_graph(gr, out, ecpu):
    st = ES.structure(gr)
    A64, b64 = ES.dense_system(gr)
    bw = bandwidth(st)
    name, n = gr["name"], 7 * st["F"]
    out[name + "/sha256"] = np.array(ES.inputs_sha256(gr))
    out[name + "/lambdas"] = np.asarray(gr["lambdas"], np.float64)
    if gr["cls"] == "failure":  # nothing is solved: the isolated vertex's pivot is 0
        return
    b = b64 / 64.0
    for l, lam in enumerate(gr["lambdas"]):
        M = A64 / 64.0
        M[np.arange(n), np.arange(n)] += lam
        L, d = ldlt(M, bw)
        x, x0 = refine(A64, b64, lam, L, d, bw)
        xmax = max(abs(v) for v in x)
        e_x = float(max(abs(mpf(float(x0[i])) - x[i]) for i in range(n)) / xmax)
        out[f"{name}/x_ref/{l}"] = np.array([float(v) for v in x])
        sc, sa, e_s = [], [], 0.0
        for fs in (0, 1):
            s, s_abs = scale_terms(x, b64, lam, fs)
            xz = x0.copy()
            if fs:
                xz[6::7] = 0.0
            s0 = float(np.sum(xz * (lam * xz + b)))
            e_s = max(e_s, float(abs(mpf(s0) - s) / s_abs))
            sc.append(float(s))
            sa.append(float(s_abs))
        out[f"{name}/scale/{l}"] = np.array(sc)
        out[f"{name}/scale_abs/{l}"] = np.array(sa)
        c = ecpu.setdefault(gr["cls"], [0.0, 0.0])
        c[0], c[1] = max(c[0], e_x), max(c[1], e_s)


def check_discrimination(gr, out, bound_x):
    """Zeroing one designated block of H must move x by at least 1000 bounds."""
    if not gr["designated"]:
        return
    A64, b64 = ES.dense_system(gr)
    n = len(b64)
    for l, lam in enumerate(gr["lambdas"]):
        x_ref = out[f"{gr['name']}/x_ref/{l}"]
        for r, c in gr["designated"]:
            M = A64 / 64.0
            M[np.arange(n), np.arange(n)] += lam
            assert np.abs(M[7 * r:7 * r + 7, 7 * c:7 * c + 7]).max() > 0, (gr["name"], r, c)
            M[7 * r:7 * r + 7, 7 * c:7 * c + 7] = 0.0
            M[7 * c:7 * c + 7, 7 * r:7 * r + 7] = 0.0
            moved = np.abs(np.linalg.solve(M, b64 / 64.0) - x_ref).max() / np.abs(x_ref).max()
            assert moved >= DISCRIMINATION * bound_x, \
                f"{gr['name']}: zeroing block ({r}, {c}) moves x by {moved:.3g} only"


# ---- eg_update and eg_finish -----------------------------------------------------------------------
def round_f32(v):
    """The float32 nearest the mpf v (ties to even are out of reach of 50-digit values here)."""
    f = np.float32(float(v))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min(cands, key=lambda c: abs(mpf(float(c)) - v))


def gen_update(out):
    G = _device_math_generator()
    P = ES.update_problem()
    S, S_fin, x, fixed = P["S"], P["S_fin"], P["x"], P["fixed"]
    sim = lambda r: (G.M(r[0:4]), G.M(r[4:7]), mpf(float(r[7])))  # noqa: E731
    fidx = np.where(fixed != 0, -1, np.cumsum(fixed == 0) - 1)
    ref = np.zeros((2, len(S), 13))
    for fs in (0, 1):
        for v in range(len(S)):
            if fidx[v] < 0:
                q, t, s = sim(S[v])
            else:
                u = G.M(x[7 * fidx[v]:7 * fidx[v] + 7])
                if fs:
                    u[6] = mpf(0)
                q, t, s = G.sim3_mul(G.sim3_exp(u), sim(S[v]))
            ref[fs, v] = [float(c) for c in G.quat_to_R(q) + list(t) + [s]]
    out["update/ref"] = ref
    T = np.zeros((len(S), 16), np.float32)
    for v in range(len(S)):
        q, t, s = sim(S_fin[v])
        R = G.quat_to_R(q)
        for i in range(3):
            for j in range(3):
                T[v, 4 * i + j] = round_f32(R[3 * i + j])
            T[v, 4 * i + 3] = round_f32(t[i] / s)
        T[v, 15] = 1.0
    out["finish/Tcw"] = T
    pts = np.zeros_like(P["points"])
    for p, (X, v) in enumerate(zip(P["points"], P["point_ref"])):
        q1, t1, s1 = sim(S[v])
        q2, t2, s2 = G.sim3_inverse(sim(S_fin[v]))
        r1 = G.quat_rotate(q1, G.M(X))
        Y = [s1 * r1[i] + t1[i] for i in range(3)]
        r2 = G.quat_rotate(q2, Y)
        pts[p] = [round_f32(s2 * r2[i] + t2[i]) for i in range(3)]
    out["finish/points"] = pts
    out["update/sha256"] = np.array(ES.update_sha256(P))


def generate() -> dict:
    out, ecpu = {}, {}
    graphs = ES.graphs()
    for gr in graphs:
        solve_graph(gr, out, ecpu)
    classes = [c for c in ES.CLASSES if c in ecpu]
    e = np.array([ecpu[c] for c in classes])
    assert (e[:, 0] <= DS.CAP).all(), f"E_cpu past the cap: {dict(zip(classes, e[:, 0]))}"
    out["classes"] = np.array(classes)
    out["ecpu_x"], out["ecpu_scale"] = e[:, 0].copy(), e[:, 1].copy()
    out["bound_x"] = DS.MARGIN * np.maximum(e[:, 0], DS.EPS52)
    out["bound_scale"] = DS.MARGIN * np.maximum(e[:, 1], DS.EPS52)
    for gr in graphs:
        if gr["cls"] in classes:
            check_discrimination(gr, out, float(out["bound_x"][classes.index(gr["cls"])]))
    gen_update(out)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eg_step.npz")
    arrays = generate()
    np.savez_compressed(path, **arrays)
    for c, a, b in zip(arrays["classes"], arrays["ecpu_x"], arrays["ecpu_scale"]):
        print(f"{c:22s} E_cpu x {a:.3g}  scale {b:.3g}")
    print(path, os.path.getsize(path), "bytes")
