"""The CPU restatement of the monocular Initializer (tests/initializer_ref.c) without a GPU: its
SVD against np.linalg.svd, every stage against a float64 numpy model of the same formulas on the
same samples, three whole-call scenes against the truth, DecomposeE's rank-2 rule, and the
restatement under the sanitizers.

Tolerances are not chosen by hand: sens() measures how far the numpy model itself moves when its
float32 inputs move by one ulp, and a stage may differ from the model by 8 x that (never less than
8 ulp of the float32 result, which the restatement rounds to). The figures are in DESIGN.md
"Monocular Initializer"."""
import os
import subprocess

import numpy as np
import pytest

import initializer_ref as R
import initializer_scenario as S

SVD_RESIDUAL_FACTOR = 8  # the restated SVD's residual may be 8 x np.linalg.svd's own
TOL_FACTOR = 8
F32_EPS = float(np.finfo(np.float32).eps)


# ---- the float64 numpy model ---------------------------------------------------------------------

def Kmat(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float64)


def model_h21(p1, p2):
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    A = []
    for (u1, v1), (u2, v2) in zip(p1, p2):
        A.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
        A.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
    return np.linalg.svd(np.array(A))[2][8].reshape(3, 3)


def model_f21(p1, p2):
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    A = [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
         for (u1, v1), (u2, v2) in zip(p1, p2)]
    Fpre = np.linalg.svd(np.array(A))[2][8].reshape(3, 3)
    u, w, vt = np.linalg.svd(Fpre)
    w[2] = 0
    return u @ np.diag(w) @ vt


def model_chi_h(H21, k1, k2, sigma):
    H21 = np.asarray(H21, np.float64)
    H12 = np.linalg.inv(H21)
    h = lambda p: np.c_[np.asarray(p, np.float64), np.ones(len(p))]
    a = h(k2) @ H12.T
    b = h(k1) @ H21.T
    d1 = ((k1 - a[:, :2] / a[:, 2:]) ** 2).sum(1)
    d2 = ((k2 - b[:, :2] / b[:, 2:]) ** 2).sum(1)
    return d1 / sigma ** 2, d2 / sigma ** 2


def model_chi_f(F, k1, k2, sigma):
    F = np.asarray(F, np.float64)
    h = lambda p: np.c_[np.asarray(p, np.float64), np.ones(len(p))]
    l2 = h(k1) @ F.T
    l1 = h(k2) @ F
    d1 = (l2 * h(k2)).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
    d2 = (l1 * h(k1)).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return d1 / sigma ** 2, d2 / sigma ** 2


def model_score(chi1, chi2, th, th_score):
    return (np.where(chi1 <= th, th_score - chi1, 0) + np.where(chi2 <= th, th_score - chi2, 0)).sum()


def model_triangulate(kp1, kp2, P1, P2):
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    A = np.array([kp1[0] * P1[2] - P1[0], kp1[1] * P1[2] - P1[1], kp2[0] * P2[2] - P2[0],
                  kp2[1] * P2[2] - P2[1]], np.float64)
    x = np.linalg.svd(A)[2][3]
    return x[:3] / x[3]


def model_decompose_e(E):
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    R1, R2 = U @ W @ Vt, U @ W.T @ Vt
    return (R1 * np.sign(np.linalg.det(R1)), R2 * np.sign(np.linalg.det(R2)),
            U[:, 2] / np.linalg.norm(U[:, 2]))


def model_motions_h(H21, K):
    Km = Kmat(K)
    A = np.linalg.inv(Km) @ np.asarray(H21, np.float64) @ Km
    U, w, Vt = np.linalg.svd(A)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    out = []
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]])
        t = U @ (np.array([x1[i], 0, -x3[i]]) * (d1 - d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]])
        t = U @ (np.array([x1[i], 0, x3[i]]) * (d1 + d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def up_to_sign(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def sens(fn, inputs, dist, trials=8, seed=0):
    """How far fn(*inputs) moves, by `dist`, when every float32 input moves by one ulp at random."""
    rng = np.random.default_rng(seed)
    base = fn(*inputs)
    worst = 0.0
    for _ in range(trials):
        moved = []
        for a in inputs:
            a = np.asarray(a, np.float32)
            moved.append(np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf)
                                      .astype(np.float32)))
        worst = np.maximum(worst, dist(fn(*moved), base))
    return worst


def bound(s, out):
    return TOL_FACTOR * max(s, F32_EPS * float(np.abs(np.asarray(out, np.float64)).max()))


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for kind in ("general", "planar", "rotation"):
        for noise in (0.0, 0.5):
            s = S.make(kind, noise=noise)
            d = S.draws(s.n, 200, seed=3)
            out[kind, noise] = (s, d, R.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, d, 200))
    return out


def samples(s, o, d, count):
    """The normalised 8-point samples of the first `count` iterations."""
    nm = o.result["norm"][0]
    pairs = o.pairs[:s.n]
    for k in range(count):
        idx = R.resolve(s.n, d[k])
        p1 = ((s.keys1[pairs[idx, 0]] - nm[0:2]) * nm[2:4]).astype(np.float32)
        p2 = ((s.keys2[pairs[idx, 1]] - nm[4:6]) * nm[6:8]).astype(np.float32)
        yield p1, p2


# ---- the one SVD ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(16, 9), (8, 9), (3, 3), (4, 4)])
def test_svd_is_orthonormal_sorted_and_as_accurate_as_lapack(shape):
    rng = np.random.default_rng(shape[0])
    m, n = shape
    for trial in range(50):
        A = (rng.normal(0, 1, shape) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
        if trial % 5 == 0 and m >= n:
            A[:, n - 1] = A[:, 0] + A[:, 1]  # rank-deficient
        d, vt, ut = R.svd(A)
        assert np.all(np.diff(d) <= 0)
        assert np.abs(vt @ vt.T - np.eye(n)).max() < 16 * n * np.finfo(np.float64).eps
        keep = d > d[0] * 1e-12
        u = ut[keep]
        # columns above 1e-12 d[0]: the skip test leaves |u_p . u_q| <= 1e-15, the rest is the
        # rounding of m-term dot products
        assert np.abs(u @ u.T - np.eye(keep.sum())).max() < 16 * m * np.finfo(np.float64).eps
        mine = np.abs(A.astype(np.float64) - (ut[keep].T * d[keep]) @ vt[keep]).max()
        U, sv, Vt = np.linalg.svd(A.astype(np.float64), full_matrices=False)
        theirs = np.abs(A - (U * sv) @ Vt).max()
        floor = np.finfo(np.float64).eps * sv[0]
        assert mine <= SVD_RESIDUAL_FACTOR * max(theirs, floor), (shape, trial, mine, theirs)
        assert np.abs(d[:len(sv)] - sv).max() <= SVD_RESIDUAL_FACTOR * n * floor  # Weyl


# ---- the stages against the numpy model -------------------------------------------------------

def test_h21_and_f21_from_eight_points(scenes, record_property):
    worst = {"H": 0.0, "F": 0.0}
    for key in (("general", 0.5), ("planar", 0.5)):
        s, d, o = scenes[key]
        for p1, p2 in samples(s, o, d, 25):
            for name, ref, model in (("H", R.compute_h21, model_h21), ("F", R.compute_f21, model_f21)):
                got, want = ref(p1, p2), model(p1, p2)
                sn = sens(model, (p1, p2), up_to_sign)
                err = up_to_sign(got, want)
                assert err <= bound(sn, want), (name, err, sn)
                worst[name] = max(worst[name], err / bound(sn, want))
    record_property("worst_fraction_of_bound", worst)


def test_check_functions(scenes):
    for key in (("general", 0.5), ("planar", 0.5)):
        s, d, o = scenes[key]
        pairs = o.pairs[:s.n]
        k1, k2 = s.keys1[pairs[:, 0]], s.keys2[pairs[:, 1]]
        for model_id, th in ((0, 5.991), (1, 3.841)):
            for k in (int(o.result["best"][0][model_id]), 0, 1):
                M = o.hyp["M"][model_id, k].reshape(3, 3)
                if model_id == 0:
                    got_s, got_m = R.check_homography(M, R.inv3(M), s.keys1, s.keys2, pairs, s.sigma)
                    chi = lambda M_, a, b: np.concatenate(model_chi_h(M_.reshape(3, 3), a, b, s.sigma))
                else:
                    got_s, got_m = R.check_fundamental(M, s.keys1, s.keys2, pairs, s.sigma)
                    chi = lambda M_, a, b: np.concatenate(model_chi_f(M_.reshape(3, 3), a, b, s.sigma))
                c = chi(M, k1, k2)
                per = sens(chi, (M, k1, k2), lambda a, b: np.abs(a - b))  # per term
                tol = TOL_FACTOR * np.maximum(per, F32_EPS * np.maximum(np.abs(c), th))
                c1, c2, t1, t2 = c[:s.n], c[s.n:], tol[:s.n], tol[s.n:]
                sure = (np.abs(c1 - th) > t1) & (np.abs(c2 - th) > t2)
                want_m = (c1 <= th) & (c2 <= th)
                assert np.array_equal(got_m[sure], want_m[sure]) and sure.sum() > 0.9 * s.n
                want_s = model_score(c1, c2, th, 5.991)
                # every term may be off by its tolerance, and the float sum of 2 N terms by
                # 2 N half-ulps of the running score
                assert abs(float(got_s) - want_s) <= tol[np.concatenate([c1, c2]) <= th + tol].sum() \
                    + 2 * s.n * F32_EPS * max(want_s, 1.0)


def test_triangulate(scenes):
    s, d, o = scenes["general", 0.0]
    r = o.result[0]
    i = int(np.argmax(o.motion["n_good"][:r["n_motions"]]))
    Km = Kmat(s.K)
    P1 = np.hstack([Km, np.zeros((3, 1))]).astype(np.float32)
    Rt = np.hstack([o.motion["R"][i].reshape(3, 3), o.motion["t"][i].reshape(3, 1)])
    P2 = (Km @ Rt).astype(np.float32)
    good = np.nonzero(R.unpack_bits(o.good_bits[i], s.n1))[0][:60]
    assert len(good) == 60
    dist = lambda a, b: np.abs(a - b).max()
    for i1 in good:
        kp1, kp2 = s.keys1[i1], s.keys2[s.matches12[i1]]
        got, want = R.triangulate(kp1, kp2, P1, P2), model_triangulate(kp1, kp2, P1, P2)
        sn = sens(model_triangulate, (kp1, kp2, P1, P2), dist)
        assert dist(got, want) <= bound(sn, want), (i1, dist(got, want), sn)


def rt_set_distance(got, want):
    """Largest distance from a motion of `got` to its nearest in `want` (R and t, t up to what the
    set contains)."""
    worst = 0.0
    for Rg, tg in got:
        worst = max(worst, min(max(np.abs(Rg - Rw).max(), np.abs(tg - tw).max()) for Rw, tw in want))
    return worst


def motions_f_model(F, K):
    Km = Kmat(K)
    R1, R2, t = model_decompose_e(Km.T @ np.asarray(F, np.float64).reshape(3, 3) @ Km)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def test_both_decompositions(scenes):
    for key, model_id, model in ((("general", 0.0), 1, motions_f_model),
                                 (("general", 0.5), 1, motions_f_model),
                                 (("planar", 0.0), 0, model_motions_h),
                                 (("planar", 0.5), 0, model_motions_h)):
        s, d, o = scenes[key]
        M = o.hyp["M"][model_id, int(o.result["best"][0][model_id])]
        got = [(m["R"].reshape(3, 3).astype(np.float64), m["t"].astype(np.float64))
               for m in R.motions(M, s.K, model_id)]
        want = model(M.reshape(3, 3), s.K)
        assert len(got) == len(want)
        sn = sens(lambda M_: model(M_.reshape(3, 3), s.K), (M,), rt_set_distance)
        err = max(rt_set_distance(got, want), rt_set_distance(want, got))
        assert err <= bound(sn, 1.0), (key, err, sn)


# ---- whole calls -----------------------------------------------------------------------------------

def best_sample_model(s, o, d, clean=None, noise=None):
    """The numpy chain on the winning F sample: F from its 8 points, E, the motion nearest the
    truth. Returns (R21, unit t21)."""
    k = int(o.result["best"][0][1])
    idx = R.resolve(s.n, d[k])
    pairs = o.pairs[:s.n]
    nm = o.result["norm"][0].astype(np.float64)
    T1 = np.array([[nm[2], 0, -nm[0] * nm[2]], [0, nm[3], -nm[1] * nm[3]], [0, 0, 1]])
    T2 = np.array([[nm[6], 0, -nm[4] * nm[6]], [0, nm[7], -nm[5] * nm[7]], [0, 0, 1]])
    tt = s.t21 / np.linalg.norm(s.t21)

    def chain(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        F = T2.T @ model_f21((a - nm[0:2]) * nm[2:4], (b - nm[4:6]) * nm[6:8]) @ T1
        return min(motions_f_model(F, s.K),
                   key=lambda m: max(np.abs(m[0] - s.R21).max(), np.abs(m[1] - tt).max()))
    return chain, s.keys1[pairs[idx, 0]], s.keys2[pairs[idx, 1]], pairs[idx]


def rt_distance(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_general_scene_takes_the_f_path(scenes, noise):
    s, d, o = scenes["general", noise]
    ok, R21, t21, P, vb = R.reconstruct(o, s.n1)
    r = o.result[0]
    assert ok and r["model"] == 1 and not float(r["RH"]) > 0.40
    tt = s.t21 / np.linalg.norm(s.t21)
    chain, a, b, sel = best_sample_model(s, o, d)
    # against the numpy chain on the same sample: the one-ulp bound
    sn = sens(chain, (a, b), rt_distance)
    assert rt_distance((R21, t21), chain(a, b)) <= bound(sn, 1.0)
    # against the truth: the sample's keys are the true projections rounded to float (noise 0)
    # or moved by the pixel noise; the chain may move 8 x as far as it does under such moves
    clean1 = S.project(s.X[sel[:, 0]], np.eye(3), np.zeros(3))
    clean2 = S.project(s.X[sel[:, 0]], s.R21, s.t21)
    assert not np.isnan(clean1).any(), "the winning sample holds a wrong match"
    if noise == 0.0:
        truth_bound = bound(sn, 1.0)
    else:
        rng = np.random.default_rng(11)
        base = chain(clean1, clean2)
        moves = [rt_distance(chain(clean1 + noise * rng.standard_normal((8, 2)),
                                   clean2 + noise * rng.standard_normal((8, 2))), base)
                 for _ in range(8)]
        truth_bound = TOL_FACTOR * max(moves)
    assert rt_distance((R21, t21), (s.R21, tt)) <= truth_bound, (truth_bound, sn)
    # vP3D = the truth up to ONE scale (|t21| = 1): the spread of the per-point scales
    tri = vb & ~np.isnan(s.X[:, 0])
    assert tri.sum() >= 0.9 * (~np.isnan(s.X[:, 0])).sum() - 1 and not vb[s.wrong].any()
    scale = np.linalg.norm(P[tri], axis=1) / np.linalg.norm(s.X[tri], axis=1)
    # A point's depth moves by z / (f b) of itself per pixel of disparity error. The disparity
    # error is the keys' own (3 sigma of the noise, or the float rounding of a 1280-wide image,
    # 1e-3 px with margin) plus the pose's (truth_bound radians are truth_bound * f pixels).
    z, f, bl = np.linalg.norm(s.X[tri], axis=1), float(s.K[0]), np.linalg.norm(s.t21)
    px = 3 * max(noise, 1e-3) + truth_bound * f
    rel = TOL_FACTOR * z / (f * bl) * px
    assert np.all(np.abs(scale / np.median(scale) - 1) <= rel)
    assert abs(np.median(scale) * bl - 1) <= rel.max()  # |t21| = 1: the one scale is 1 / |t|


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_planar_scene_takes_the_h_path(scenes, noise):
    s, d, o = scenes["planar", noise]
    ok, R21, t21, P, vb = R.reconstruct(o, s.n1)
    r = o.result[0]
    assert float(r["RH"]) > 0.40 and r["model"] == 0 and r["n_motions"] == 8 and ok


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_pure_rotation_returns_false(scenes, noise):
    s, d, o = scenes["rotation", noise]
    assert not R.reconstruct(o, s.n1)[0]
    if noise == 0.0:
        assert o.result["n_motions"][0] == 0  # the early return of :601


def test_decompose_e_gives_the_left_null_vector(scenes):
    """t = u.col(2) of a rank-2 E: the normalised third column of A V is rounding noise, the
    restatement runs the routine on E^T instead. Checked against the true direction."""
    s, d, o = scenes["general", 0.0]
    F = o.hyp["M"][1, int(o.result["best"][0][1])].reshape(3, 3).astype(np.float64)
    Km = Kmat(s.K)
    E = (Km.T @ F @ Km).astype(np.float32)
    R1, R2, t = R.decompose_e(E)
    tt = s.t21 / np.linalg.norm(s.t21)
    chain, a, b, _ = best_sample_model(s, o, d)
    sn = sens(chain, (a, b), rt_distance)
    assert up_to_sign(t, tt) <= bound(sn, 1.0)
    # two float roundings per component (the reciprocal of the norm, the product)
    assert abs(np.linalg.norm(t.astype(np.float64)) - 1) < 4 * F32_EPS
    # the exact E has rank 2; rounding its nine entries to float leaves d3 <= 3 * eps / 2 * max|E|
    assert np.abs(E.astype(np.float64).T @ t).max() < TOL_FACTOR * 3 * F32_EPS * np.abs(E).max()
    # E of exact rank 2. Small integers, third row = the sum of the others: the left null vector
    # is (1, 1, -1) / sqrt(3). And [t]x for t = z, whose third column of E V is exactly zero: the
    # shortcut the rule forbids (that column over its norm) is 0 / 0, the rule gives z.
    E2 = np.array([[1, 2, 3], [4, 5, 7], [5, 7, 10]], np.float32)
    assert up_to_sign(R.decompose_e(E2)[2], np.array([1, 1, -1]) / np.sqrt(3)) <= 4 * F32_EPS
    E3 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    R1, R2, t = R.decompose_e(E3)
    assert up_to_sign(t, [0, 0, 1]) == 0 and np.isfinite(R1).all() and np.isfinite(R2).all()
    assert abs(np.linalg.det(R1.astype(np.float64)) - 1) < 4 * F32_EPS
    d3, vt, ut = R.svd(E3)
    assert d3[2] == 0 and np.isnan(ut[2]).all()


def test_best_is_the_lowest_iteration_with_the_greatest_positive_score(scenes):
    for (s, d, o) in scenes.values():
        for m in (0, 1):
            sc = o.hyp["score"][m]
            pos = np.nan_to_num(sc, nan=0.0) > 0
            want = int(np.argmax(np.where(pos, sc, -1))) if pos.any() else -1
            assert o.result["best"][0][m] == want


def test_no_winner_and_nan_scores():
    """All keys in one point: Normalize divides by zero, every score is NaN, no model has a best
    and Initialize returns false."""
    k1 = np.full((30, 2), 7.25, np.float32)
    o = R.ransac(k1, k1, np.arange(30, dtype=np.int32), S.K, 1.0, S.draws(30, 5), 5)
    r = o.result[0]
    assert r["status"] == 0 and np.isnan(o.hyp["score"]).all()
    assert r["best"].tolist() == [-1, -1] and r["n_motions"] == 0 and np.isnan(r["RH"])
    assert not R.reconstruct(o, 30)[0]


def test_invalid_jobs_write_only_the_status():
    s = S.make("general", n=20)
    d = S.draws(20, 4)
    for breaker in ("draw", "match", "few"):
        m, dd = s.matches12.copy(), d.copy()
        if breaker == "draw":
            dd[2, 3] = 20 - 3
        elif breaker == "match":
            m[0] = s.n2
        else:
            m[np.nonzero(m >= 0)[0][:13]] = -1
        o = R.ransac(s.keys1, s.keys2, m, s.K, s.sigma, dd, 4, fill=0xA5)
        assert o.result["status"][0] == -1
        for a in o.arrays():
            u = a.view(np.uint8).reshape(-1)
            assert (u[4:] == 0xA5).all() if a is o.result else (u == 0xA5).all()


# ---- sanitizers ------------------------------------------------------------------------------------

def test_restatement_is_clean_under_the_sanitizers(tmp_path):
    """tests/initializer_sanitizer_check.c (the restatement plus a main of its own: a general and
    a planar pair, all-identical points, an 8-match job, the 8192 cap and invalid jobs) built
    with the address and undefined-behaviour sanitizers and run as a program; the runtimes are
    linked statically, so it runs as it is whatever else is preloaded."""
    exe = str(tmp_path / "initializer_sanitizer_check")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-Wno-unused-parameter", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    os.path.join(R.HERE, "initializer_sanitizer_check.c"), "-o", exe, "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", r.stdout + r.stderr
    assert not r.stderr.strip(), r.stderr
