"""The monocular Initializer on the device (include/slamgpu_initializer.h, csrc/init_ransac.hip)
against its CPU restatement (tests/initializer_ref.c), bit for bit, NaN compared as NaN: every H
and F hypothesis with its score and mask, the selection, the motions and CheckRT of each."""
import ctypes as C
import functools

import numpy as np
import pytest

import initializer_ref as R
import initializer_scenario as S

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def G(gpu_lib):
    gpu_lib.lib()
    return gpu_lib


@functools.lru_cache(maxsize=None)
def case(kind, n, noise, n_its, extra1=40, extra2=25):
    s = S.make(kind, n=n, noise=noise, extra1=extra1, extra2=extra2)
    d = S.draws(n, n_its, seed=7 + n)
    want = R.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, d, n_its)
    for a in [s.keys1, s.keys2, s.matches12, d] + want.arrays():
        a.setflags(write=False)
    return s, d, want


def f32_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_job_equal(got, want, n1, n_its):
    """got: (hyp[2][>= n_its], bits, result record, pairs, motion, good_bits, p3d) of one job;
    want: R.Outputs."""
    hyp, bits, r, pairs, motion, good, p3d = got
    w = want.result[0]
    assert w["status"] == 0 and r["status"] == 0
    for f in ("n", "best", "model", "n_motions", "pad"):
        assert np.array_equal(r[f], w[f]), (f, r[f], w[f])
    for f in ("SH", "SF", "RH", "norm"):
        assert f32_equal(r[f], w[f]), (f, r[f], w[f])
    words = (n1 + 63) // 64
    for f in ("M", "score"):
        assert f32_equal(hyp[f][:, :n_its], want.hyp[f][:, :n_its]), f
    assert np.array_equal(hyp["pad"][:, :n_its], want.hyp["pad"][:, :n_its])
    assert np.array_equal(np.asarray(bits, np.uint64)[:, :n_its, :words],
                          want.bits[:, :n_its, :words])
    n, nm = int(w["n"]), int(w["n_motions"])
    assert np.array_equal(pairs[:n], want.pairs[:n])
    for f in ("R", "t", "cos_parallax"):
        assert f32_equal(motion[f][:nm], want.motion[f][:nm]), f
    for f in ("n_good", "pad"):
        assert np.array_equal(motion[f][:nm], want.motion[f][:nm]), f
    assert np.array_equal(np.asarray(good, np.uint64)[:nm, :words], want.good_bits[:nm, :words])
    assert f32_equal(p3d[:nm, :n1], want.p3d[:nm, :n1])


def run_single(G, s, d, n_its):
    return G.init_ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, d, n_its)


# ---- one job through the synchronous call ------------------------------------------------------

@pytest.mark.parametrize("n,n_its", [(8, 200), (9, 200), (63, 200), (64, 1), (64, 200), (65, 200),
                                     (257, 200)])
def test_single_job_bit_exact(G, n, n_its):
    """n1 > N with -1 holes in matches12, n1 != n2."""
    s, d, want = case("general", n, 0.5, n_its)
    assert s.n1 > n and s.n1 != s.n2 and (s.matches12 < 0).any()
    assert_job_equal(run_single(G, s, d, n_its), want, s.n1, n_its)


def test_best_tie_goes_to_the_first_iteration(G):
    """130 iterations: one hypothesis 70 times, then a better one 60 times, so iterations 70 .. 129
    tie exactly in both models. In the selecting wave lane 6 holds iteration 70 and lane 0 only
    iteration 128 as candidates: a tie decided by lane instead of by index would answer 128."""
    s = S.make("planar", n=64, noise=0.5, extra1=40, extra2=25)
    d0 = S.draws(64, 130, seed=71)
    d = np.ascontiguousarray(np.concatenate([np.repeat(d0[3:4], 70, 0), np.repeat(d0[5:6], 60, 0)]))
    want = R.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, d, 130)
    w = want.result[0]
    assert w["best"].tolist() == [70, 70] and (w["model"], w["n_motions"]) == (0, 8)
    score = np.ascontiguousarray(want.hyp["score"][:, :130]).view(np.uint32)
    for model in (0, 1):
        assert (score[model, 70:] == score[model, 70]).all()
        assert (want.hyp["score"][model, :70] < want.hyp["score"][model, 70]).all()
    assert_job_equal(run_single(G, s, d, 130), want, s.n1, 130)


def test_cap(G):
    """N = n1 = SLAMGPU_INIT_MAX_KEYS."""
    s, d, want = case("general", G.INIT_MAX_KEYS, 0.0, 16, 0, 0)
    assert want.result["n"][0] == G.INIT_MAX_KEYS == s.n1
    assert want.motion["n_good"].max() > 51
    assert_job_equal(run_single(G, s, d, 16), want, s.n1, 16)


@pytest.mark.parametrize("kind,noise,model,n_motions", [
    ("general", 0.0, 1, 4), ("general", 0.5, 1, 4), ("planar", 0.0, 0, 8), ("planar", 0.5, 0, 8),
    ("rotation", 0.0, 0, 0), ("rotation", 0.5, 0, 8)])
def test_scenes_bit_exact(G, kind, noise, model, n_motions):
    """The E motions, the H motions and the zero-motion return of :601 all run."""
    s, d, want = case(kind, 300, noise, 200)
    w = want.result[0]
    assert (w["model"], w["n_motions"]) == (model, n_motions)
    assert_job_equal(run_single(G, s, d, 200), want, s.n1, 200)


def test_rank_clamp(G):
    """Fewer than 51 good points: the cosine at rank nGood - 1; more: at rank 50."""
    s, d, want = case("general", 40, 0.0, 200)
    ng = want.motion["n_good"][:want.result["n_motions"][0]]
    assert 0 < ng.max() < 51
    assert_job_equal(run_single(G, s, d, 200), want, s.n1, 200)
    big = case("general", 300, 0.0, 200)[2]
    assert big.motion["n_good"].max() > 51


def test_identical_points(G):
    """All keys of both frames in one point: Normalize divides by zero and NaN runs through."""
    n = 70
    k1 = np.full((n, 2), 100.5, np.float32)
    k2 = np.full((n + 3, 2), 100.5, np.float32)
    m = np.arange(n, dtype=np.int32)
    m[5] = -1
    d = S.draws(n - 1, 9)
    want = R.ransac(k1, k2, m, S.K, 1.0, d, 9)
    assert np.isinf(want.result["norm"][0][2]) and np.isnan(want.hyp["score"]).any()
    assert want.result["best"][0].tolist() == [-1, -1] and want.result["n_motions"][0] == 0
    assert_job_equal(G.init_ransac(k1, k2, m, S.K, 1.0, d, 9), want, n, 9)


# ---- the batched device call ---------------------------------------------------------------------

def run_batch(G, specs, max_n1, max_its, break_jobs=None, stream=None):
    """specs: (scene, draws[n_its][8]). Launches the device call and returns a function that
    synchronises, checks the guard bytes and gives the seven output arrays indexed by job."""
    import torch
    nj = len(specs)
    words = (max_n1 + 63) // 64
    jobs = np.zeros(nj, G.INIT_JOB_DTYPE)
    b1 = b2 = bd = 0
    for j, (s, d) in enumerate(specs):
        jobs[j] = (b1, s.n1, b2, s.n2, bd, len(d), s.K, s.sigma, 0)
        b1, b2, bd = b1 + s.n1, b2 + s.n2, bd + d.size
    k1 = np.concatenate([s.keys1 for s, _ in specs])
    k2 = np.concatenate([s.keys2 for s, _ in specs])
    m12 = np.concatenate([s.matches12 for s, _ in specs])
    dr = np.concatenate([d.reshape(-1) for _, d in specs])
    if break_jobs:
        break_jobs(jobs, b1, b2, bd)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    sizes = (nj * 2 * max_its * 48, nj * 2 * max_its * words * 8, nj * 80, nj * max_n1 * 8,
             nj * 8 * 64, nj * 8 * words * 8, nj * 8 * max_n1 * 12)
    ins = [dev(a) for a in (k1, m12, k2, dr, jobs)]
    outs = [torch.full((s + GUARD,), FILL, dtype=torch.uint8, device="cuda") for s in sizes]
    torch.cuda.synchronize()
    G.init_ransac_device(ins[0], ins[1], b1, ins[2], b2, ins[3], bd, ins[4], nj, max_n1, max_its,
                         *outs, stream=stream.cuda_stream if stream else None)

    def finish():
        torch.cuda.synchronize()
        keep = ins  # alive until the kernels are done
        host = [o.cpu().numpy() for o in outs]
        for h, s in zip(host, sizes):
            assert (h[s:] == FILL).all(), "guard bytes overwritten"
        h = [a[:s] for a, s in zip(host, sizes)]
        return (h[0].view(G.INIT_HYP_DTYPE).reshape(nj, 2, max_its),
                h[1].view(np.uint64).reshape(nj, 2, max_its, words),
                h[2].view(G.INIT_RESULT_DTYPE), h[3].view(np.int32).reshape(nj, max_n1, 2),
                h[4].view(G.INIT_MOTION_DTYPE).reshape(nj, 8),
                h[5].view(np.uint64).reshape(nj, 8, words),
                h[6].view(np.float32).reshape(nj, 8, max_n1, 3))
    return finish


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def check_batch(out, specs, max_n1, max_its, invalid=()):
    for j, (s, d) in enumerate(specs):
        got = [a[j] for a in out]
        if j in invalid:
            assert got[2]["status"] == -1, j
            assert untouched(got[2].reshape(1).view(np.uint8)[4:])
            for i in (0, 1, 3, 4, 5, 6):
                assert untouched(got[i]), (j, i)
            continue
        n_its = len(d)
        want = R.ransac(s.keys1, s.keys2, s.matches12, s.K, s.sigma, d, n_its, max_n1=max_n1,
                        max_its=max_its, fill=FILL)
        assert_job_equal(got, want, s.n1, n_its)
        # what the job does not write: the integer arrays byte for byte against the restatement
        # run over the same fill, then rows >= n_its, pairs >= N, motions >= n_motions, keys >= n1
        for i in (1, 3, 5):
            assert np.array_equal(np.ascontiguousarray(got[i]).view(np.uint8),
                                  want.arrays()[i].view(np.uint8)), (j, i)
        assert untouched(got[0][:, n_its:]) and untouched(got[1][:, n_its:]), j
        nm, n = int(want.result["n_motions"][0]), int(want.result["n"][0])
        assert untouched(got[3][n:]) and untouched(got[4][nm:]) and untouched(got[5][nm:]), j
        assert untouched(got[6][nm:]) and untouched(got[6][:, s.n1:]), j


def batch_specs(seed):
    shapes = [("general", 40, 35), ("planar", 64, 9), ("general", 8, 4), ("rotation", 100, 60),
              ("general", 258, 5), ("general", 64, 61), ("planar", 65, 17), ("general", 90, 8),
              ("general", 50, 6), ("general", 80, 7), ("planar", 120, 60)]
    specs = []
    for j, (kind, n, its) in enumerate(shapes):
        s = S.make(kind, n=n, noise=0.5, seed=seed + j, extra1=7 + j, extra2=3 + 2 * j)
        specs.append((s, S.draws(n, its, seed=31 + j + seed).copy()))
    return specs


def test_batched_jobs_with_invalid_ones(G):
    """Jobs of different sizes in one call, and between them one invalid job of each kind."""
    specs = batch_specs(0)
    max_n1, max_its = 140, 60
    specs[7][1][5, 2] = 88                    # job 7: the third draw of iteration 5 must be <= 87
    specs[8][0].matches12 = specs[8][0].matches12.copy()
    specs[8][0].matches12[3] = specs[8][0].n2  # job 8: a match outside frame 2

    def break_jobs(jobs, n_keys1, n_keys2, n_draws):
        jobs["key1_begin"][1] = n_keys1 - jobs["n1"][1] + 1  # the key range leaves the array
        assert jobs["n1"][4] > max_n1                        # n1 > max_n1
        assert jobs["n_its"][5] == 61                        # n_its > max_its
        jobs["n_its"][9] = 0                                 # n_its < 1
        jobs["draw_begin"][6] = n_draws - 8 * 17 + 1         # the draw range leaves the array
    invalid = (1, 4, 5, 6, 7, 8, 9)
    out = run_batch(G, specs, max_n1, max_its, break_jobs)()
    check_batch(out, specs, max_n1, max_its, invalid)


def test_fewer_than_eight_matches_is_invalid(G):
    s = S.make("general", n=8, noise=0.0, extra1=5, extra2=5)
    s.matches12 = s.matches12.copy()
    s.matches12[np.nonzero(s.matches12 >= 0)[0][0]] = -1
    specs = [(s, S.draws(8, 3))]
    check_batch(run_batch(G, specs, 16, 4)(), specs, 16, 4, invalid=(0,))


def test_two_streams_at_once(G):
    import torch
    a, b = batch_specs(1)[:1] + batch_specs(1)[3:4], batch_specs(2)[2:3] + batch_specs(2)[10:11]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f1 = run_batch(G, a, 128, 60, stream=s1)
    f2 = run_batch(G, b, 192, 64, stream=s2)
    check_batch(f1(), a, 128, 60)
    check_batch(f2(), b, 192, 64)


# ---- loud errors ----------------------------------------------------------------------------------

def test_synchronous_call_errors(G):
    s, d, _ = case("general", 64, 0.5, 200)

    def fails(code_text, keys1=s.keys1, keys2=s.keys2, m=s.matches12, draws=d, n_its=200):
        with pytest.raises(G.SlamGpuError) as e:
            G.init_ransac(keys1, keys2, m, s.K, s.sigma, draws, n_its)
        assert code_text in str(e.value), str(e.value)

    fails("SLAMGPU_INIT_MAX_ITS", draws=S.draws(64, G.INIT_MAX_ITS + 1), n_its=G.INIT_MAX_ITS + 1)
    fails("n_its 0", n_its=0)
    big = np.zeros((G.INIT_MAX_KEYS + 1, 2), np.float32)
    fails("SLAMGPU_INIT_MAX_KEYS", keys1=big, m=np.full(len(big), -1, np.int32))
    fails("SLAMGPU_INIT_MAX_KEYS", keys2=big)
    bad = s.matches12.copy()
    bad[np.nonzero(bad >= 0)[0][2]] = s.n2
    fails("outside [-1,", m=bad)
    few = np.full(s.n1, -1, np.int32)
    few[:7] = np.arange(7)
    fails("7 matches < 8", m=few)
    bd = d.copy()
    bd[9, 7] = 64 - 7
    fails("iteration 9: draw 7", draws=bd)
    bd[9, 7] = -1
    fails("iteration 9: draw 7", draws=bd)
    L = G.lib()
    assert L.slamgpu_init_ransac(*[None] * 2, 64, None, 64, None, C.c_float(1.0), None, 1,
                                 *[None] * 7) != 0
    assert b"NULL" in L.slamgpu_initializer_last_error()


# ---- slamgpu.Initializer -------------------------------------------------------------------------

@pytest.mark.parametrize("kind,noise,ok", [("general", 0.5, True), ("planar", 0.5, True),
                                           ("rotation", 0.0, False), ("rotation", 0.5, False)])
def test_initializer_end_to_end(G, kind, noise, ok):
    s = S.make(kind, noise=noise)
    init = G.Initializer(s.keys1, s.K, s.sigma, 200, random_int=S.Lcg(5))
    got = init.Initialize(s.keys2, s.matches12)
    want, o = R.initialize(s.keys1, s.keys2, s.matches12, s.K, s.sigma, 200, S.Lcg(5))
    assert got[0] == want[0] == ok and init.device_calls == 1
    if ok:
        for g, w in zip(got[1:4], want[1:4]):
            assert f32_equal(g, w)
        assert np.array_equal(got[4], want[4]) and got[4].sum() >= 50


def test_initializer_default_generator(G):
    """The default generator is rand() after SeedRandOnce(0): the schedule is in range and the
    call succeeds on the general scene."""
    s = S.make("general", noise=0.0)
    init = G.Initializer(s.keys1, s.K, s.sigma, 200)
    ok, R21, t21, P, vb = init.Initialize(s.keys2, s.matches12)
    assert ok and R21.shape == (3, 3) and vb.sum() >= 50 and init.device_calls == 1
