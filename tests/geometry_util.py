"""tests/geometry_check (compute_geometry + build_cells on the host, as JSON) from Python."""
import json
import subprocess

import numpy as np


def geometry_check_bin():
    from slam_framework_amd import build
    return build.build_geometry_check()


def geometries(configs, lds=None):
    """[(cols, rows, nfeatures, scale, nlevels), ...] -> one dict per configuration. lds: the
    octree kernels' (img, lvl) dynamic LDS limits; None: unlimited, as slamgpu_create computes the
    geometry without a usable device (the gfx950 budgets then apply alone)."""
    out = []
    for i in range(0, len(configs), 40):
        args = [geometry_check_bin()]
        if lds is not None:
            args += ["--lds", str(lds[0]), str(lds[1])]
        for c in configs[i:i + 40]:
            args += [str(int(c[0])), str(int(c[1])), str(int(c[2])), repr(float(c[3])),
                     str(int(c[4]))]
        r = subprocess.run(args, check=True, capture_output=True, text=True, timeout=120)
        out += [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(configs)
    for g in out:
        if g["rc"] == 0:
            g["cells"] = np.array(g["cells"], np.int64).reshape(-1, 5)
            for L in g["lv"]:
                L["ry"] = np.array(L["ry"], np.int64).reshape(-1, 2)
                L["band"] = np.array(L["band"], np.int64).reshape(-1, 2)
    return out


def geometry(cols, rows, nfeatures=2000, scale=1.2, nlevels=8, lds=None):
    return geometries([(cols, rows, nfeatures, scale, nlevels)], lds)[0]
