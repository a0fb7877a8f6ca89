"""InitializerCore (include/slamgpu_adapters.hpp) driven from C++ on the device
(tests/initializer_adapter_check.cpp, the default rand() functor) as
Tracker::MonocularInitialization drives the reference's Initializer: one reference frame, a pure
rotation that must fail and then a general scene that must succeed, against the CPU restatement
fed the draws the program printed. The first call's draws are rand() after SeedRandOnce(0)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import initializer_ref as R
import initializer_scenario as S

pytestmark = pytest.mark.gpu

ITERATIONS = 200


def test_adapter_core_follows_the_restatement(gpu_lib, tmp_path):
    from slam_framework_amd import build
    exe = build.build_initializer_adapter_check()
    a = S.make("general", noise=0.5)
    b = S.make("rotation", noise=0.5, seed=0)
    # one reference frame: the rotation scene's frame 2 re-matched onto frame 1 of the general one
    n = min(a.n, b.n)
    keys2_rot = b.keys2.copy()
    m_rot = np.full(a.n1, -1, np.int32)
    pos = np.nonzero(a.matches12 >= 0)[0][:n]
    Rm = S.rot([0.2, 1.0, 0.1], 0.12)
    rays = np.stack([(a.keys1[pos, 0] - a.K[2]) / a.K[0], (a.keys1[pos, 1] - a.K[3]) / a.K[1],
                     np.ones(n)], 1)
    keys2_rot[:n] = S.project(rays * 10.0, Rm, np.zeros(3)).astype(np.float32)
    m_rot[pos] = np.arange(n)
    calls = [(keys2_rot, m_rot), (a.keys2, a.matches12)]
    assert a.n2 == b.n2
    path = tmp_path / "scenario.bin"
    with open(path, "wb") as f:
        f.write(np.array([a.n1, a.n2, ITERATIONS, len(calls)], np.int32).tobytes())
        f.write(a.K.astype(np.float32).tobytes())
        f.write(np.float32(a.sigma).tobytes())
        f.write(a.keys1.tobytes())
        for k2, m in calls:
            f.write(np.ascontiguousarray(k2, np.float32).tobytes())
            f.write(np.ascontiguousarray(m, np.int32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    heads = [i for i, f in enumerate(lines) if f[0] == "call"]
    assert len(heads) == len(calls)
    oks = []
    for c, (h, (k2, m)) in enumerate(zip(heads, calls)):
        f = lines[h]
        ok, dev_calls = int(f[3]), int(f[9])
        assert dev_calls == c + 1  # ONE device call per Initialize
        draws = np.array([int(x) for x in lines[h + 1][1:]], np.int32).reshape(-1, 8)
        N = int((m >= 0).sum())
        assert draws.shape == (ITERATIONS, 8)
        assert (draws >= 0).all() and (draws <= N - 1 - np.arange(8)).all()
        if c == 0:  # SeedRandOnce(0), then DUtils::Random::RandomInt on rand()
            libc = C.CDLL(None)
            libc.srand(0)
            want = [gpu_lib.reference_random_int(0, N - 1 - j) for _ in range(ITERATIONS)
                    for j in range(8)]
            assert draws.reshape(-1).tolist() == want
        o = R.ransac(a.keys1, k2, m, a.K, a.sigma, draws, ITERATIONS)
        w_ok, w_R, w_t, w_P, w_vb = R.reconstruct(o, a.n1)
        assert ok == int(w_ok), c
        assert (int(f[5]), int(f[7])) == (o.result["model"][0], o.result["n_motions"][0])
        oks.append(ok)
        if not ok:
            assert lines[h + 2][0] in ("call", "ok")  # nothing is given on failure
            continue
        hexs = lambda row: np.array([int(x, 16) for x in row[1:]], np.uint32)
        pose = hexs(lines[h + 2])
        assert np.array_equal(pose[:9], w_R.reshape(-1).view(np.uint32))
        assert np.array_equal(pose[9:], w_t.view(np.uint32))
        assert [int(x) for x in lines[h + 3][1:]] == np.nonzero(w_vb)[0].tolist()
        assert np.array_equal(hexs(lines[h + 4]), w_P.reshape(-1).view(np.uint32))
    assert oks == [0, 1]
