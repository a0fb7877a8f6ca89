"""CreateNewMapPoints at KITTI size (2000 keypoints, 10 neighbours; 1 job and 16 jobs), two ways on
the same device in one process, alternating:

  chain   slamgpu_create_new_map_points_device: every neighbour's search and triangulation
          enqueued at once, one synchronisation at the end, then the download of n_new and of the
          point lists;
  host    what a caller had before: per neighbour one slamgpu_search_for_triangulation_device
          call over all jobs, a synchronisation, the download of match12, the triangulation and
          the acceptance tests on the host (tests/newpoints_ref.c, the restatement of
          local_mapper.cpp:332-490 in C), and the upload of the updated has_mp.

Both leave the same points on the host (checked). Times are host-clock medians around work that
ends in a device synchronise, after warm-up runs; has_mp is restored outside the timed window.

  python tools/newpoints_bench.py [--n 2000] [--nbors 10] [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def centers(n):
    """n neighbour centres 0.6 .. 1.5 m from the current keyframe, all directions."""
    rng = np.random.default_rng(9)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return [tuple(v) for v in d * rng.uniform(0.6, 1.5, (n, 1)) * np.array([1.0, 0.4, 0.5])]


class Setup:
    def __init__(self, K, torch, jobs):
        self.K, self.torch, self.jobs = K, torch, jobs
        self.dev = torch.device("cuda", 0)
        self.keep = []
        all_kfs, jrec, nrec = [], [], []
        for cur, nbors in jobs:
            jrec.append((len(all_kfs), len(nrec), len(nbors)))
            all_kfs.append(cur)
            for nb in nbors:
                nrec.append((len(all_kfs), nb))
                all_kfs.append(nb["kf"])
        self.nj, self.nn = len(jobs), max(r[2] for r in jrec)
        self.n1 = [len(c["desc"]) for c, _ in jobs]
        self.stride = max(self.n1)
        kfs = np.zeros(len(all_kfs), K.KF_DTYPE)
        kst = np.zeros(len(all_kfs), K.KF_STEREO_DTYPE)
        for i, k in enumerate(all_kfs):
            T = np.asarray(k["T"], np.float32)
            kfs[i]["kps"], kfs[i]["desc"] = self.up(k["kps"]), self.up(k["desc"])
            kfs[i]["u_right"], kfs[i]["has_mp"] = self.up(k["ur"]), self.up(k["mp"])
            kfs[i]["nodes"] = self.up(k["fv"][0].astype(np.uint32))
            kfs[i]["node_start"] = self.up(k["fv"][1].astype(np.int32))
            kfs[i]["node_feats"] = self.up(k["fv"][2].astype(np.uint32))
            kfs[i]["n"], kfs[i]["n_nodes"] = len(k["desc"]), len(k["fv"][0])
            kfs[i]["Rcw"], kfs[i]["tcw"], kfs[i]["Ow"] = T[:3, :3].reshape(-1), T[:3, 3], k["Ow"]
            kst[i]["depth"], kst[i]["raw_kps"] = self.up(k["depth"]), 0
            kst[i]["cam"], kst[i]["mb"] = k["cam"], k["mb"]
        # every job's has_mp1 in one tensor, so that one copy restores all of them
        self.mp0 = torch.from_numpy(np.stack([np.pad(c["mp"], (0, self.stride - len(c["mp"])))
                                              for c, _ in jobs])).to(self.dev)
        self.mp = self.mp0.clone()
        jarr = np.zeros(self.nj, K.NP_JOB_DTYPE)
        for j, (kf1, first, nn) in enumerate(jrec):
            ptr = int(self.mp.data_ptr()) + j * self.stride
            kfs[kf1]["has_mp"] = ptr
            jarr[j] = (kf1, first, nn, 0, ptr)
        narr = np.zeros(len(nrec), K.NP_NBOR_DTYPE)
        for r, (kf2, nb) in enumerate(nrec):
            narr[r] = (kf2, np.asarray(nb["F12"], np.float32).reshape(-1), nb["skip"],
                       nb["first_obs"])
        self.d_kfs, self.d_kst = self.up(kfs), self.up(kst)
        self.d_jobs, self.d_nbors = self.up(jarr), self.up(narr)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.dev)  # noqa: E731
        self.n_new = z(self.nj, torch.int32)
        self.points = z(self.nj * self.stride * 80, torch.uint8)
        self.news = z(self.nj * self.stride * 16, torch.uint8)
        self.status = z(self.nj * self.nn * self.stride, torch.int8)
        self.sb = K.create_new_map_points_scratch_bytes(self.nj, self.nn)
        self.scratch = z(self.sb, torch.uint8)
        # the host path: the pairs of neighbour k of every job, match rows, counts
        self.d_pairs = []
        for k in range(self.nn):
            pairs = np.zeros(self.nj, K.TRI_PAIR_DTYPE)
            for j, (kf1, first, nn) in enumerate(jrec):
                kf2, nb = nrec[first + k]
                pairs[j] = (kf1, kf2, np.asarray(nb["F12"], np.float32).reshape(-1), 0)
            self.d_pairs.append(self.up(pairs))
        self.match = z(self.nj * self.stride, torch.int32)
        self.nmatch = z(self.nj, torch.int32)
        self.cam, self.lv = all_kfs[0]["cam"], K.levels()
        self.stream = torch.cuda.current_stream().cuda_stream

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(
            self.dev)
        self.keep.append(t)
        return int(t.data_ptr())

    def restore(self):
        self.mp.copy_(self.mp0)
        self.torch.cuda.synchronize()

    def chain(self):
        """Returns (seconds to the synchronise, seconds with the results on the host, results)."""
        K, torch = self.K, self.torch
        t0 = time.perf_counter()
        K.create_new_map_points_device(self.d_kfs, self.d_kst, self.d_jobs, self.nj, self.d_nbors,
                                       self.nn, self.cam, self.lv, False, self.n_new, self.points,
                                       self.news, self.stride, self.status, self.stride,
                                       self.scratch, self.sb, self.stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n_new = self.n_new.cpu().numpy()
        m = int(n_new.max())
        pts = self.points.view(self.nj, self.stride * 80)[:, :m * 80].cpu().numpy()
        nws = self.news.view(self.nj, self.stride * 16)[:, :m * 16].cpu().numpy()
        t2 = time.perf_counter()
        return t1 - t0, t2 - t0, [(int(n), pts[j, :80 * n].tobytes(), nws[j, :16 * n].tobytes())
                                  for j, n in enumerate(n_new)]

    def host(self, R, sc, s2):
        K, torch = self.K, self.torch
        t0 = time.perf_counter()
        hmp = [np.ascontiguousarray(c["mp"], np.uint8).copy() for c, _ in self.jobs]
        pts = [np.zeros(n, R.FUSE_POINT_DTYPE) for n in self.n1]
        nws = [np.zeros(n, R.NEW_POINT_DTYPE) for n in self.n1]
        n_new = [0] * self.nj
        for k in range(self.nn):
            K.search_for_triangulation_device(self.d_kfs, self.d_pairs[k], self.nj, self.cam,
                                              self.lv, False, self.match, self.stride, self.nmatch,
                                              self.stream)
            torch.cuda.synchronize()
            m = self.match.cpu().numpy().reshape(self.nj, self.stride)
            for j, (cur, nbors) in enumerate(self.jobs):
                nb = nbors[k]
                n_new[j], _ = R.pair(cur, nb["kf"], m[j, :self.n1[j]], k, sc, s2, nb["first_obs"],
                                     pts[j], nws[j], n_new[j], hmp[j])
            self.mp.copy_(torch.from_numpy(np.stack(
                [np.pad(h, (0, self.stride - len(h))) for h in hmp])), non_blocking=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return t1 - t0, [(n_new[j], pts[j][:n_new[j]].tobytes(), nws[j][:n_new[j]].tobytes())
                         for j in range(self.nj)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--nbors", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("newpoints_bench: no GPU")
    from slam_framework_amd import build, kfmatch as K
    build.build()
    import newpoints_ref as R
    import newpoints_scenario as NS
    sc, s2 = NS.levels_arrays()
    R.lib()
    result = dict(n=a.n, nbors=a.nbors, reps=a.reps, warmup=a.warmup,
                  device=torch.cuda.get_device_name(0), cases=[])
    for nj in a.jobs:
        jobs = [NS.scene(a.n, 900 + j, a.nbors, "mixed", centers=centers(a.nbors), n_nodes=250)
                for j in range(nj)]
        S = Setup(K, torch, jobs)
        t_chain, t_chain_dl, t_host = [], [], []
        for it in range(a.warmup + a.reps):
            S.restore()
            c0, c1, out_c = S.chain()
            S.restore()
            h0, out_h = S.host(R, sc, s2)
            if out_c != out_h:
                sys.exit("newpoints_bench: the two ways disagree")
            if it >= a.warmup:
                t_chain.append(c0)
                t_chain_dl.append(c1)
                t_host.append(h0)
        ms = lambda v: round(1e3 * float(np.median(v)), 4)  # noqa: E731
        sp = lambda v: [round(1e3 * float(np.percentile(v, p)), 4) for p in (10, 90)]  # noqa: E731
        case = dict(jobs=nj, new_points=[o[0] for o in out_c],
                    launches_chain=2 * a.nbors + 1, synchronisations_chain=1,
                    launches_host=a.nbors, synchronisations_host=a.nbors,
                    chain_ms=ms(t_chain), chain_p10_p90_ms=sp(t_chain),
                    chain_with_download_ms=ms(t_chain_dl),
                    chain_with_download_p10_p90_ms=sp(t_chain_dl),
                    host_ms=ms(t_host), host_p10_p90_ms=sp(t_host))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
