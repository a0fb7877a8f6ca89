"""GPU parity of the RANSAC EPnP solver (include/slamgpu_pnpsolver.h) against the CPU restatement
tests/pnpsolver_ref.c (pinned by tests/test_pnpsolver_ref.py), BIT FOR BIT: the float bit patterns
of Rcw / tcw (NaNs compared as NaN, not by payload), n_inliers, best, every mask word, the refined
rows and their masks, events and n_events -- on the smallest shapes at which the kernels can go
wrong, degenerate data, the batched device form with invalid jobs, guard bytes and two streams,
loud errors, the Python PnPsolver in the tracker's round robin, and one chain check into
PoseOptimization."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import pnpsolver_model as M
import pnpsolver_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def G(gpu_lib):
    gpu_lib.lib()
    return gpu_lib


@functools.lru_cache(maxsize=None)
def job(n):
    m, d, n_its, min_inliers = M.job(n)
    want = R.ransac(m, d, n_its, min_inliers, M.K, M.SIGMA2, M.TH2)
    for a in (m, d) + want[:5]:
        a.setflags(write=False)
    return m, d, n_its, min_inliers, want


def bits_equal_f32(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_rows_equal(got, want, n_its):
    """got / want: (hyp, bits, refined, refined_bits) with at least n_its rows."""
    for g, w, name in ((got[0], want[0], "hyp"), (got[2], want[2], "refined")):
        for f in ("Rcw", "tcw"):
            assert bits_equal_f32(g[f][:n_its], w[f][:n_its]), (name, f)
        for f in ("n_inliers", "best", "pad"):
            assert np.array_equal(g[f][:n_its], w[f][:n_its]), (name, f)
    for i in (1, 3):
        assert np.array_equal(np.asarray(got[i][:n_its], np.uint64), want[i][:n_its]), i


def run_single(G, m, d, n_its, min_inliers):
    return G.pnp_ransac(m, d, n_its, min_inliers, M.K, M.SIGMA2, M.TH2)


# ---- single jobs through the synchronous call -------------------------------------------------

@pytest.mark.parametrize("n", [
    4,      # all 24 draw orders of the one sample
    5,      # the smallest refine that can succeed
    10,     # N == min_inliers
    63, 64, 65,   # the mask-word boundary; at 65 a refine set of 65 > 64 inliers
    257,    # 5 words, 300 iterations
    4096,   # the cap
])
def test_single_job_bit_exact(G, n):
    m, d, n_its, min_inliers, want = job(n)
    wne = want[5]
    assert wne >= 0
    bests = np.unique(want[0]["best"][want[0]["best"] >= 0])
    if n in (5, 63, 64, 65, 257, 4096):
        assert wne >= 1  # the event and refine paths run
    if n in (64, 65, 257):
        assert len(bests) >= 2
    if n == 65:
        assert want[0]["n_inliers"][bests].max() == 65  # more than one point on a lane
    if n == 4:
        assert sorted(map(tuple, (R.resolve(4, r) for r in d))) == \
            sorted(itertools.permutations(range(4)))
    got = run_single(G, m, d, n_its, min_inliers)
    assert_rows_equal(got, want, n_its)
    assert len(got[4]) == wne and np.array_equal(got[4], want[4][:wne])
    tail = (-n) % 64
    if tail:
        for b in (got[1], got[3]):
            assert not (np.asarray(b, np.uint64)[:, -1] >> np.uint64(64 - tail)).any()


def test_running_best_tie_goes_to_the_first_iteration(G):
    """130 iterations: the same failing hypothesis 70 times, then the same winning one 60 times, so
    iterations 70 .. 129 tie exactly. In the wave that looks for the running best, lane 6 holds
    iteration 70 and lane 0 only iteration 128 as candidates: a tie decided by lane instead of by
    index would answer 128."""
    m, d, _, min_inliers, _ = job(64)
    d = np.ascontiguousarray(np.concatenate([np.repeat(d[0:1], 70, 0), np.repeat(d[12:13], 60, 0)]))
    want = R.ransac(m, d, 130, min_inliers, M.K, M.SIGMA2, M.TH2)
    assert min_inliers == 10
    assert (want[0]["n_inliers"][:70] == 0).all() and (want[0]["n_inliers"][70:130] == 32).all()
    assert (want[0]["best"][:70] == -1).all() and (want[0]["best"][70:130] == 70).all()
    assert want[5] == 60 and want[4][:3].tolist() == [70, 71, 72]
    got = run_single(G, m, d, 130, min_inliers)
    assert_rows_equal(got, want, 130)
    assert len(got[4]) == 60 and np.array_equal(got[4], want[4][:60])


def draws_for_samples(n, samples):
    """The draws that resolve to the given samples (searched with the Python swap-and-pop)."""
    want = {tuple(s) for s in samples}
    table = {}
    for r in itertools.product(range(n), range(n - 1), range(n - 2), range(n - 3)):
        s = tuple(M.resolve(n, r))
        if s in want and s not in table:
            table[s] = r
            if len(table) == len(want):
                break
    return np.array([table[tuple(s)] for s in samples], np.int32)


def test_degenerate_data_gives_the_same_bits(G):
    """A coplanar sample, a collinear one, a repeated world point, four identical world points
    (rho = 0: the betas of the second initialisation are all zero and qr_solve takes its
    zero-column return), a point at Zc = 0 and one behind the camera of the scene's pose, octaves
    outside the table: inf / NaN by IEEE rules, a NaN error is no inlier, no special cases."""
    n = 20
    m, Rt, tt = M.scene(77, n, 0.3, 0.0)
    m = m.copy()
    x = m["xw"].astype(np.float64)
    m["xw"][3] = (x[0] + 0.4 * (x[1] - x[0]) + 0.7 * (x[2] - x[0])).astype(np.float32)  # coplanar
    for j, a in ((5, 0.5), (6, 1.5), (7, 2.25)):                                         # collinear
        m["xw"][j] = (x[4] + a * np.array([1.0, 0.5, -0.25])).astype(np.float32)
    m["xw"][9] = m["xw"][8]                                                               # repeated
    m["xw"][13] = m["xw"][14] = m["xw"][15] = m["xw"][12]                                 # rho = 0
    for j, zc in ((16, 0.0), (17, -6.0)):                       # Zc = 0, behind the camera
        m["xw"][j] = (Rt.T @ (np.array([0.5, -0.25, zc]) - tt)).astype(np.float32)
    m["octave"][18], m["octave"][19] = -1, len(M.SIGMA2)
    samples = [(0, 1, 2, 3), (3, 2, 1, 0), (4, 5, 6, 7), (8, 9, 10, 11), (9, 8, 0, 1),
               (12, 13, 14, 15), (16, 0, 1, 2), (17, 10, 11, 2), (18, 19, 0, 1), (0, 1, 2, 10),
               (12, 13, 0, 1)]
    d = draws_for_samples(n, samples)
    before = R.qr_zero_returns()
    want = R.ransac(m, d, len(d), 4, M.K, M.SIGMA2, M.TH2)
    assert R.qr_zero_returns() > before  # the zero-column return ran
    assert want[5] >= 0
    got = run_single(G, m, d, len(d), 4)
    assert_rows_equal(got, want, len(d))
    assert np.array_equal(got[4], want[4][:want[5]])
    inl = R.unpack_bits(np.asarray(got[1], np.uint64), n)
    assert not inl[:, 18].any() and not inl[:, 19].any()  # never an inlier
    assert np.isnan(want[0]["Rcw"]).any()  # a NaN pose is among the hypotheses
    assert (want[0]["n_inliers"][np.isnan(want[0]["Rcw"]).any(axis=1)] == 0).all()


# ---- the batched device call --------------------------------------------------------------------

def run_batch(G, specs, max_n, max_its, break_jobs=None, stream=None):
    """specs: (matches, draws[n_its][4], min_inliers). Launches the device call (on `stream`, a
    torch stream, if given) and returns a function that synchronises, checks the guard bytes and
    gives (hyp[j][max_its], bits[j][max_its][words], refined, refined_bits, events[j][max_its],
    n_events)."""
    import torch
    nj = len(specs)
    words = (max_n + 63) // 64
    jobs = np.zeros(nj, G.PNP_JOB_DTYPE)
    ms, ds = [], []
    mb = db = 0
    for j, (m, d, mi) in enumerate(specs):
        d = np.asarray(d, np.int32).reshape(-1, 4)
        jobs[j] = (mb, len(m), db, len(d), mi, 0)
        ms.append(np.ascontiguousarray(m, G.PNP_MATCH_DTYPE))
        ds.append(d.reshape(-1))
        mb += len(m)
        db += d.size
    allm, alld = np.concatenate(ms), np.concatenate(ds)
    if break_jobs:
        break_jobs(jobs, len(allm), len(alld))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def out(nbytes):
        return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    d_m, d_d, d_j = dev(allm), dev(alld), dev(jobs)
    rows, masks = nj * max_its * 64, nj * max_its * words * 8
    sizes = (rows, masks, rows, masks, nj * max_its * 4, nj * 4)
    outs = [out(s) for s in sizes]
    torch.cuda.synchronize()
    G.pnp_ransac_device(M.K, M.SIGMA2, M.TH2, d_m, len(allm), d_d, len(alld), d_j, nj, max_n,
                        max_its, *outs, stream=stream.cuda_stream if stream else None)

    def finish():
        torch.cuda.synchronize()
        keep = (d_m, d_d, d_j)  # alive until the kernels are done
        host = [o.cpu().numpy() for o in outs]
        for h, s in zip(host, sizes):
            assert (h[s:] == FILL).all(), "guard bytes overwritten"
        hyp = host[0][:rows].view(G.PNP_HYP_DTYPE).reshape(nj, max_its)
        bits = host[1][:masks].view(np.uint64).reshape(nj, max_its, words)
        refined = host[2][:rows].view(G.PNP_HYP_DTYPE).reshape(nj, max_its)
        rbits = host[3][:masks].view(np.uint64).reshape(nj, max_its, words)
        events = host[4][:sizes[4]].view(np.int32).reshape(nj, max_its)
        return hyp, bits, refined, rbits, events, host[5][:sizes[5]].view(np.int32)
    return finish


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def check_batch(out, specs, max_n, max_its, invalid=()):
    hyp, bits, refined, rbits, events, ne = out
    for j, (m, d, mi) in enumerate(specs):
        if j in invalid:
            assert ne[j] == -1, j
            for a in (hyp[j], bits[j], refined[j], rbits[j], events[j]):
                assert untouched(a), j
            continue
        n_its = len(d)
        want = R.ransac(m, d, n_its, mi, M.K, M.SIGMA2, M.TH2, max_its=max_its,
                        words=(max_n + 63) // 64)
        assert ne[j] == want[5] >= 0, j
        assert_rows_equal((hyp[j], bits[j], refined[j], rbits[j]), want, n_its)
        assert np.array_equal(events[j][:want[5]], want[4][:want[5]])
        for a in (hyp[j], bits[j], refined[j], rbits[j]):
            assert untouched(a[n_its:]), j  # rows >= n_its
        assert untouched(events[j][want[5]:])


def batch_specs(seed):
    big = M.scene(300 + seed, 258, 0.5, 0.35)[0]
    shapes = [(40, 35), (64, 9), (3, 4), (257, 60), (258, 5), (64, 17), (65, 61), (100, 60),
              (65, 1), (50, 6), (80, 7), (90, 8), (40, 35)]
    specs = []
    for j, (n, its) in enumerate(shapes):
        m = np.roll(big, -3 * j)[:n]
        specs.append((m, M.draws_for(31 + j + seed, max(n, 4), its), 12 if n >= 40 else 4))
    return specs


def test_batched_jobs_with_invalid_ones(G):
    """Jobs of different n and n_its in one call, and between them one invalid job of each kind."""
    specs = batch_specs(0)
    max_n, max_its = 257, 60
    specs[11][1][5, 2] = 88  # job 11: the third draw of iteration 5 must be <= 87

    def break_jobs(jobs, n_matches, n_draws):
        jobs["match_begin"][1] = n_matches - 64 + 1   # the match range leaves the array
        assert jobs["n"][2] == 3                      # n < 4
        assert jobs["n"][4] == 258                    # n > max_n
        assert jobs["n_its"][6] == 61                 # n_its > max_its
        jobs["n_its"][8] = 0                          # n_its < 1
        jobs["min_inliers"][9] = 3                    # min_inliers < 4
        jobs["draw_begin"][10] = n_draws - 4 * 7 + 1  # the draw range leaves the array
    invalid = (1, 2, 4, 6, 8, 9, 10, 11)
    out = run_batch(G, specs, max_n, max_its, break_jobs)()
    check_batch(out, specs, max_n, max_its, invalid)
    assert any(out[5][j] > 0 for j in (0, 3, 5, 7, 12))


def test_two_streams_at_once(G):
    import torch
    a, b = batch_specs(1)[:1] + batch_specs(1)[7:8], batch_specs(2)[3:4] + batch_specs(2)[5:6]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f1 = run_batch(G, a, 100, 60, stream=s1)
    f2 = run_batch(G, b, 257, 64, stream=s2)
    check_batch(f1(), a, 100, 60)
    check_batch(f2(), b, 257, 64)


# ---- loud errors ----------------------------------------------------------------------------------

def test_synchronous_call_errors(G):
    L = G.lib()
    m, d, _, _, _ = job(64)
    m = np.ascontiguousarray(m, G.PNP_MATCH_DTYPE)
    K = np.ascontiguousarray(M.K, np.float32)
    s2 = np.ascontiguousarray(M.SIGMA2, np.float32)
    p = G._ptr

    def call(m, n, d, n_its, min_inliers=10, hyp=True, nlevels=len(s2)):
        rows = max(n_its, 1)
        h, r = np.zeros(rows, G.PNP_HYP_DTYPE), np.zeros(rows, G.PNP_HYP_DTYPE)
        b = np.zeros((rows, (max(n, 1) + 63) // 64), np.uint64)
        rb, e = b.copy(), np.zeros(rows, np.int32)
        ne = C.c_int()
        rc = L.slamgpu_pnp_ransac(p(K), p(s2), nlevels, M.TH2, p(m), n, p(d), n_its, min_inliers,
                                  p(h) if hyp else None, p(b), p(r), p(rb), p(e), C.byref(ne))
        return rc, L.slamgpu_pnpsolver_last_error().decode()

    d = np.ascontiguousarray(d[:4]).reshape(-1)
    assert call(m, 64, d, 4, hyp=False) == (-1, "NULL argument")
    big = np.zeros(G.PNP_MAX_MATCHES + 1, G.PNP_MATCH_DTYPE)
    assert call(big, len(big), d, 4) == (-3, "4097 matches > SLAMGPU_PNP_MAX_MATCHES (4096)")
    d513 = M.draws_for(1, 64, 513).reshape(-1)
    assert call(m, 64, d513, 513) == (-1, "n_its 513 outside [1, SLAMGPU_PNP_RANSAC_MAX_ITS (512)]")
    assert call(m, 3, d, 4) == (-1, "3 matches < 4")
    assert call(m, 64, d, 4, min_inliers=3) == (-1, "min_inliers 3 < 4")
    assert call(m, 64, d, 4, nlevels=0)[1].startswith("nlevels 0 outside [1, ")
    bad = d.copy()
    bad[6] = 62  # iteration 1, third draw: at most 61
    assert call(m, 64, bad, 4) == (-1, "iteration 1: draw 2 = 62 outside [0, 61]")

    class Ptr:  # never dereferenced: the call fails before it launches
        def data_ptr(self):
            return 256
    q = Ptr()
    with pytest.raises(G.SlamGpuError, match="max_its 513 outside"):
        G.pnp_ransac_device(K, s2, M.TH2, q, 64, q, 16, q, 1, 64, 513, q, q, q, q, q, q)
    with pytest.raises(G.SlamGpuError, match="draw 2 = 62"):
        G.pnp_ransac(m, bad, 4, 10, K, s2, M.TH2)
    with pytest.raises(G.SlamGpuError, match="minSet 5 is not supported"):
        G.pnp_ransac_parameters(40, 0.99, 10, 300, 5, 0.5)


def test_parameters_match_the_restatement(G):
    assert G.pnp_ransac_parameters(40, 0.99, 10, 300, 4, 0.5) == (20, 35)
    for N in (4, 9, 10, 11, 20, 40, 41, 100, 500, 4096):
        for args in ((0.99, 10, 300, 4, 0.5), (0.99, 8, 300, 4, 0.4), (0.5, 15, 300, 4, 0.5)):
            assert G.pnp_ransac_parameters(N, *args) == R.parameters(N, *args), (N, args)


# ---- the Python PnPsolver in Tracker::Relocalization's round robin -----------------------------

def test_pnpsolver_round_robin_with_overrun(G):
    """Three candidates, iterate(5) in turn as tracker.cpp:904-988 (going on after a success, up
    to 12 calls each): every outcome against the C replay fed the draws the solver made. The
    first candidate is test_pnpsolver_ref's overrun scene and is handed the same first 35 draws:
    its last event is at iteration 31 of 35, so the call after it runs past mRansacMaxIts and the
    solver evaluates a longer schedule."""
    rng = np.random.default_rng(11)
    fixed = list(M.draws_for(0, 40, 35).reshape(-1))
    w = R.ransac(M.scene(4, 40, 0.5, 0.3)[0], fixed, 35, 20, M.K, M.SIGMA2, M.TH2)
    assert w[5] >= 2 and w[4][w[5] - 1] >= 30

    def random_int(lo, hi):
        if fixed:
            r = int(fixed.pop(0))
            assert lo <= r <= hi
            return r
        return int(rng.integers(lo, hi + 1))

    # (scene seed, n, outliers)
    shapes = [(4, 40, 0.3), (12, 64, 0.35), (13, 100, 0.6)]
    dev, ms = [], []
    for seed, n, out in shapes:
        m, _, _ = M.scene(seed, n, 0.5, out)
        idx = np.arange(n) * 2 + 1
        s = G.PnPsolver(m, M.K, M.SIGMA2, indices=idx, n_kp=2 * n + 5, random_int=random_int)
        s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
        assert (s.mRansacMinInliers, s.mRansacMaxIts) == R.parameters(n, 0.99, 10, 300, 4, 0.5)
        dev.append(s)
        ms.append((m, idx, n))
    calls = [0] * 3
    log = [[] for _ in shapes]
    discarded = [False] * 3
    while not all(discarded):
        for i in range(3):
            if discarded[i]:
                continue
            log[i].append(dev[i].iterate(5) + (dev[i].mnIterations,))
            calls[i] += 1
            discarded[i] = log[i][-1][1] or calls[i] >= 12
    successes = 0
    for i, (m, idx, n) in enumerate(ms):
        s = dev[i]
        c = R.Solver(m, s.draws, s.mRansacMinInliers, s.mRansacMaxIts, M.K, M.SIGMA2, M.TH2,
                     indices=idx, n_kp=2 * n + 5)
        for T, no_more, vb, ni, its in log[i]:
            wT, w_no_more, w_vb, w_ni = c.iterate(5)
            assert (no_more, ni, its) == (w_no_more, w_ni, c.iterations), i
            assert np.array_equal(vb, w_vb) and (T is None) == (wT is None)
            if T is not None:
                assert np.array_equal(T[:3, :3].reshape(-1), wT["Rcw"])
                assert np.array_equal(T[:3, 3], wT["tcw"]) and vb.sum() == ni
                successes += not no_more
    assert successes >= 2
    assert max(s.device_calls for s in dev) >= 2 and max(len(s.draws) for s in dev) > 35


def test_pnpsolver_too_few_correspondences(G):
    m, _, _ = M.scene(1, 9, 0.5)
    s = G.PnPsolver(m, M.K, M.SIGMA2, random_int=lambda lo, hi: pytest.fail("nothing is drawn"))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, no_more, vb, ni = s.iterate(5)
    assert T is None and no_more and ni == 0 and not vb.any() and s.device_calls == 0


# ---- the chain: the returned pose and inliers into PoseOptimization ------------------------------

def test_pose_feeds_pose_optimization(G):
    """Tracker::Relocalization's next step (tracker.cpp:925-946): the inliers become the frame's
    map points, Tcw the initial pose. The scene has 0.5 px of noise on the 60 % of its 100 points
    that are no outliers, at depths up to 20 m. One such point alone fixes the camera to
    sigma = 0.5 px * 20 m / fx = 14 mm sideways and to 0.5 px / fx = 0.7 mrad in angle; a pose
    from >= 50 of them must not be worse than three such single-point sigmas."""
    n = 100
    m, Rt, tt = M.scene(31, n, 0.5, 0.4)
    rng = np.random.default_rng(2)
    s = G.PnPsolver(m, M.K, M.SIGMA2, random_int=lambda lo, hi: int(rng.integers(lo, hi + 1)))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, vb, ni = s.find()
    assert T is not None and ni >= 50
    edges = np.zeros(ni, G.POSE_EDGE_DTYPE)
    sel = np.flatnonzero(vb)
    edges["xw"], edges["u"], edges["v"] = m["xw"][sel], m["u"][sel], m["v"][sel]
    edges["ur"], edges["octave"] = -1.0, m["octave"][sel]
    cam = (*[float(k) for k in M.K], 386.1448)
    n_good, T_opt, outlier = G.Optimizer.PoseOptimization(edges, T, cam, 1 / M.SIGMA2)
    assert n_good >= 50 and n_good == ni - outlier.sum()
    fx = float(M.K[0])
    assert np.linalg.norm(T_opt[:3, 3] - tt) <= 3 * 0.5 * 20 / fx
    assert np.max(np.abs(T_opt[:3, :3] - Rt)) <= 3 * 0.5 / fx
