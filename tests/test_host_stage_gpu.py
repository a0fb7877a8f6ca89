"""The per-thread staging buffer shared by the synchronous wrappers (csrc/host_stage.h), on the
GPU through the Python bindings: calls of different modules on one thread reuse one buffer, a
large call grows it past its 1 MiB floor without disturbing later small calls, and two host
threads that share one vocabulary stage through their own buffers.

The inputs are small seeded arrays made here; what is compared is each call's output against
the same call's earlier output (bit for bit), and the large gray image against the formula the
gray oracle test pins (tests/test_bow_oracle.py gray_formula)."""
import threading

import numpy as np
import pytest

from kf_scenario import CAM, fundamental
from test_bow_oracle import gray_formula
from slam_framework_amd import synthetic as S

pytestmark = pytest.mark.gpu

COLS, ROWS = 1241, 376


def _keypoints(rng, n):
    from slam_framework_amd.slamgpu import KP_DTYPE
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(40, COLS - 40, n).astype(np.float32)
    k["y"] = rng.uniform(40, ROWS - 40, n).astype(np.float32)
    k["size"] = 31.0
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["octave"] = rng.integers(0, 3, n)
    return k


class Case:
    """One thread's inputs: every array a call reads is made once and kept."""

    def __init__(self, seed, vocab):
        from slam_framework_amd import kfmatch as K
        rng = np.random.default_rng(seed)
        self.vocab = vocab
        self.img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        self.dd_desc = rng.integers(0, 256, (8, 32), dtype=np.uint8)
        self.dd_start = np.array([0, 2, 5, 8], np.int32)  # 3 points with 2, 3, 3 descriptors
        self.edges, self.T0, _, self.isig, _ = S.pose_problem(seed, n=8)
        # two 64-feature views of the same descriptors (the second with a few bits flipped)
        self.desc_a = rng.integers(0, 256, (64, 32), dtype=np.uint8)
        flip = np.zeros((64, 32), np.uint8)
        flip[np.arange(64), rng.integers(0, 32, 64)] = 1 << rng.integers(0, 8, 64).astype(np.uint8)
        self.desc_b = self.desc_a ^ flip
        self.kps_a = _keypoints(rng, 64)
        self.kps_b = self.kps_a.copy()
        self.kps_b["x"] -= 6.0  # the same row: on the epipolar line of a sideways baseline
        self.fv_a = vocab.transform(self.desc_a, 1)[1]
        self.fv_b = vocab.transform(self.desc_b, 1)[1]
        self.lv, self.grid = K.levels(), K.kf_grid(COLS, ROWS)
        # a keyframe pair one baseline apart (all keypoints stereo, none with a map point)
        T1, T2 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
        T2[0, 3] = -0.5
        disparity = np.float32(CAM[4] / 10.0)  # of a point 10 m away (the Fuse points below)
        ur_a = (self.kps_a["x"] - disparity).astype(np.float32)
        ur_b = (self.kps_b["x"] - disparity).astype(np.float32)
        none = np.zeros(64, np.uint8)
        self.kf1 = K.host_kf(self.kps_a, self.desc_a, ur_a, T1, none, self.fv_a)
        self.kf2 = K.host_kf(self.kps_b, self.desc_b, ur_b, T2, none, self.fv_b)
        self.F12 = fundamental(T1, T2)
        # 65 map points: the keyframe's own keypoints unprojected at 10 m, and one behind it
        fx, fy, cx, cy, _ = CAM
        sc = np.array([self.lv.scale[i] for i in range(8)], np.float64)
        self.pts = np.zeros(65, K.FUSE_POINT_DTYPE)
        for i in range(64):
            kp = self.kps_a[i]
            X = np.array([(kp["x"] - cx) * 10.0 / fx, (kp["y"] - cy) * 10.0 / fy, 10.0])
            d = float(np.linalg.norm(X))
            self.pts[i]["xyz"], self.pts[i]["normal"] = X, X / d
            self.pts[i]["max_dist"] = d * sc[kp["octave"]]
            self.pts[i]["min_dist"] = d * sc[kp["octave"]] / sc[-1]
            self.pts[i]["desc"] = self.desc_a[i]
        self.pts[64] = self.pts[0]
        self.pts[64]["xyz"] = -self.pts[0]["xyz"]
        self.fuse_kf = K.host_kf(self.kps_a, self.desc_a, ur_a, T1)

    # each returns its outputs as one tuple of arrays / ints
    def gray(self):
        from slam_framework_amd import bow as B
        return (B.cvt_gray(self.img, True),)

    def distinctive(self):
        from slam_framework_amd import bow as B
        return B.distinctive_descriptors(self.dd_desc, self.dd_start)

    def pose(self):
        from slam_framework_amd.slamgpu import Optimizer
        return Optimizer.PoseOptimization(self.edges, self.T0, CAM, self.isig)

    def search_by_bow(self):
        from slam_framework_amd import bow as B
        return B.search_by_bow(self.desc_a, self.kps_a, None, self.fv_a, self.desc_b, self.kps_b,
                               self.fv_b, nnratio=0.9)

    def fuse(self):
        from slam_framework_amd import kfmatch as K
        return K.fuse(self.fuse_kf, self.pts, 3.0, CAM, self.lv, self.grid)

    def transform(self):
        bv, fv = self.vocab.transform(self.desc_a, 1)
        return (bv.words, bv.values) + tuple(fv.arrays())

    def search_tri(self):
        from slam_framework_amd import kfmatch as K
        return K.search_for_triangulation(self.kf1, self.kf2, self.F12, CAM, self.lv)

    def small_calls(self):
        return [self.gray(), self.distinctive(), self.pose(), self.search_by_bow(), self.fuse()]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def vocab(gpu_lib):
    from slam_framework_amd import bow as B
    return B.ORBVocabulary.from_arrays(S.vocabulary(17, k=4, L=2))


def test_one_thread_shares_and_grows_the_stage(vocab):
    c = Case(5, vocab)
    first = c.small_calls()
    np.testing.assert_array_equal(first[0][0], gray_formula(c.img, True))
    assert first[3][0] > 0 and first[4][0] > 0, "the small scenes should match and fuse"
    big = np.random.default_rng(6).integers(0, 256, (1024, 1280, 3), dtype=np.uint8)  # 3.75 MiB
    from slam_framework_amd import bow as B
    np.testing.assert_array_equal(B.cvt_gray(big, True), gray_formula(big, True))
    for got, want in zip(c.small_calls(), first):
        _same(got, want)


def test_two_threads_share_one_vocabulary(vocab):
    cases = [Case(11, vocab), Case(12, vocab)]
    serial = [(c.transform(), c.search_tri()) for c in cases]
    assert all(len(s[0][0]) > 0 and s[1][0] > 0 for s in serial), "words and matches expected"
    errors = []

    def run(c, want):
        try:
            for _ in range(20):
                _same(c.transform(), want[0])
                _same(c.search_tri(), want[1])
        except BaseException as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(c, w)) for c, w in zip(cases, serial)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
