"""Host-side sweep of compute_geometry / build_cells (tests/geometry_check.cpp: orb_geometry.cpp
alone, no device code) over the accepted image sizes, 64x64 .. 4095x2047.

The expectations restate the reference in NumPy float32, statement by statement:
* ORBextractor's ctor (src/orb_features/orb_extractor.cpp:356-387): mvScaleFactor[i] =
  mvScaleFactor[i-1] * scaleFactor (float * double -> float), mvInvScaleFactor = 1.0f / it, the
  per-level feature budget from factor = 1.0f / scaleFactor with cvRound;
* ComputePyramid (:1051-1057): level size cvRound((float)cols * mvInvScaleFactor[level]) -- also
  taken from the oracle's oc_pyramid_alloc;
* ComputeKeyPointsOctTree (:712-733): the borders, nCols = width / W, wCell = ceil(width / nCols);
* DistributeOctTree (:484-486): nIni = round((float)(maxX - minX) / (maxY - minY)), hX;
* OpenCV 3.3.1 resize (INTER_LINEAR): source rows sy = floor((dy + 0.5) * scale_y - 0.5), sy + 1,
  clamped to the source.
Nothing here is derived from orb_geometry.cpp; the layout invariants are what the kernels that
consume the geometry need (csrc/orb_*.hip), stated where they are asserted."""
import numpy as np
import pytest

import geometry_util as GU

f32 = np.float32
EDGE = 19
MIN_BORDER = EDGE - 3

# the sizes the GPU tests run (test_geometry_gpu.py and the older files) and the sizes that take
# the other geometry branches: (cols, rows, nfeatures, scale, nlevels)
NAMED = [
    (1241, 376, 2000, 1.2, 8), (1226, 370, 2000, 1.2, 8), (752, 480, 1200, 1.2, 8),
    (640, 480, 1000, 1.2, 8), (320, 240, 2000, 1.2, 8),
    (1536, 400, 2000, 1.2, 8), (1344, 376, 2000, 1.2, 8), (1504, 960, 2000, 1.2, 8),
    (1280, 720, 2000, 1.2, 8), (1600, 1200, 2000, 1.2, 8), (1280, 112, 600, 1.2, 2),
    (2048, 160, 1000, 1.2, 4), (480, 752, 1200, 1.2, 8), (1440, 1080, 2000, 1.2, 8),
    (1920, 1080, 2000, 1.2, 8), (4095, 2047, 2000, 1.2, 8), (64, 64, 500, 1.2, 1),
    (1241, 376, 4000, 1.2, 8), (1241, 376, 2000, 1.2, 12), (4095, 64, 1000, 1.2, 1),
]
# rejected: the return code each must give
REJECTED = [((4096, 2047, 2000, 1.2, 8), -1), ((4095, 2048, 2000, 1.2, 8), -1),
            ((63, 64, 2000, 1.2, 1), -1), ((376, 1241, 2000, 1.2, 8), -3),
            ((160, 120, 2000, 1.2, 8), -2)]


def random_configs(n=200, seed=20240611):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(64, 4096)), int(rng.integers(64, 2048)),
             int(rng.choice([500, 1000, 2000, 4000])), float(rng.choice([1.2, 1.3, 1.5, 2.0])),
             int(rng.choice([1, 2, 4, 8, 12]))) for _ in range(n)]


def cv_round(v):
    return int(np.rint(f32(v)))  # cvRound: lrint, ties to even


def restate(cols, rows, nfeatures, scale, nlevels):
    """The reference's per-level quantities; 'rc' is the return code its formulas imply: -1
    outside 64..4095 x 64..2047, -2 at the first level under 2 * 19 + 8 pixels, -3 at the first
    level whose nIni is 0 (checked level by level, size first), else 0."""
    sf = float(f32(scale))  # ORBextractor::scaleFactor is a double holding the float argument
    sc = [f32(1.0)]
    for i in range(1, nlevels):
        sc.append(f32(float(sc[i - 1]) * sf))
    inv = [f32(1.0) / s for s in sc]
    factor = f32(1.0 / sf)
    nd = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** float(nlevels)))
    budget, tot = [], 0
    for _ in range(nlevels - 1):
        budget.append(cv_round(nd))
        tot += budget[-1]
        nd = f32(nd * factor)
    budget.append(max(nfeatures - tot, 0))
    R = dict(rc=0, lv=[])
    if cols < 64 or rows < 64 or cols > 4095 or rows > 2047:
        R["rc"] = -1
        return R
    for l in range(nlevels):
        w, h = cv_round(f32(cols) * inv[l]), cv_round(f32(rows) * inv[l])
        if w < 2 * EDGE + 8 or h < 2 * EDGE + 8:
            R["rc"] = -2
            return R
        max_bx, max_by = w - EDGE + 3, h - EDGE + 3
        width, height = f32(max_bx - MIN_BORDER), f32(max_by - MIN_BORDER)
        ncols, nrows = int(width / f32(30)), int(height / f32(30))
        # a level under 62 pixels has no cell column / row: the reference's loops then never run
        # and its wCell / hCell (a float division by zero) is never used
        wcell = int(np.ceil(width / f32(ncols))) if ncols else None
        hcell = int(np.ceil(height / f32(nrows))) if nrows else None
        q = f32(max_bx - MIN_BORDER) / f32(max_by - MIN_BORDER)
        n_ini = int(np.floor(float(q) + 0.5))  # C round(): half away from zero, q > 0
        if n_ini < 1:
            R["rc"] = -3
            return R
        R["lv"].append(dict(w=w, h=h, max_bx=max_bx, max_by=max_by, ncols=ncols, nrows=nrows,
                            wcell=wcell, hcell=hcell, n_ini=n_ini,
                            hx=f32(max_bx - MIN_BORDER) / f32(n_ini), budget=budget[l]))
    return R


def resize_rows(h_dst, h_src):
    """OpenCV resize's source rows of every destination row: (y0, y1) clamped to the source."""
    scale_y = 1.0 / (float(h_dst) / float(h_src))
    fy = ((np.arange(h_dst) + 0.5) * scale_y - 0.5).astype(f32)
    sy = np.floor(fy).astype(np.int64)
    return np.clip(sy, 0, h_src - 1), np.clip(sy + 1, 0, h_src - 1)


@pytest.fixture(scope="module")
def sweep():
    configs = NAMED + [c for c, _ in REJECTED] + random_configs()
    return list(zip(configs, GU.geometries(configs)))


def test_return_codes(sweep):
    """rc is 0 exactly when the restatement accepts the size: every level at least 46 pixels,
    every nIni at least 1, cols <= 4095 and rows <= 2047. The only other outcomes are the two
    capacity rejections slamgpu_create reports with a message, each only where its cause exists:
    -5 (four adjacent output columns span more than pyr_down's 8-byte source window) needs a
    level more than twice as wide as the next (scale factor 2 and an odd width), -7 (a level's
    octree node lists overflow octree_lvl_kernel's LDS) a level budget above 1024 nodes, which
    slamgpu_create refuses on its own."""
    want = dict(REJECTED)
    seen = {}
    for c, g in sweep:
        R = restate(*c)
        if c in want:
            assert g["rc"] == want[c] == R["rc"], c
        if R["rc"] != 0:
            assert g["rc"] == R["rc"], (c, g["rc"], R["rc"])
        elif g["rc"] != 0:
            ws = [L["w"] for L in R["lv"]]
            if g["rc"] == -5:
                assert any(a > 2 * b for a, b in zip(ws, ws[1:])), c
            else:
                assert g["rc"] == -7 and max(L["budget"] for L in R["lv"]) + 3 > 1024, (c, g["rc"])
        seen[g["rc"]] = seen.get(g["rc"], 0) + 1
    assert seen[0] > 100 and seen.get(-2, 0) > 5 and seen.get(-3, 0) > 0, seen
    assert [g["rc"] for c, g in sweep if c == (4095, 2047, 2000, 1.2, 8)] == [0]


def accepted(sweep):
    return [(c, g, restate(*c)) for c, g in sweep if g["rc"] == 0]


def test_fields_equal_the_restatement(sweep, oracle):
    for c, g, R in accepted(sweep):
        assert R["rc"] == 0, c
        t = oracle.tables(c[2], c[3], c[4], 20, 7)
        pyr = oracle.OraclePyramid(t, c[0], c[1])
        for l, (L, E) in enumerate(zip(g["lv"], R["lv"])):
            assert (L["w"], L["h"]) == (pyr.p.w[l], pyr.p.h[l]), (c, l)
            assert E["budget"] == t.features_per_level[l], (c, l)
            for f in ("w", "h", "max_bx", "max_by", "ncols", "nrows", "n_ini", "budget"):
                assert L[f] == E[f], (c, l, f, L[f], E[f])
            for f in ("wcell", "hcell"):
                if E[f] is not None:
                    assert L[f] == E[f], (c, l, f, L[f], E[f])
            assert f32(L["hx"]) == E["hx"], (c, l)
            if l > 0:  # the resize table rows the band / ring checks below rely on
                y0, y1 = resize_rows(L["h"], g["lv"][l - 1]["h"])
                assert np.array_equal(L["ry"][:, 0], y0), (c, l)
                assert np.array_equal(L["ry"][:, 1], y1), (c, l)


def test_key_packing(sweep):
    """pack_key: x_rel 12 bits, y_rel 11 bits from (minBorder, minBorder). orient_desc's gv_k:
    x 12 bits, y 12 bits, level 4 bits; gv_wh: w and h 16 bits each."""
    for c, g, _ in accepted(sweep):
        for l, L in enumerate(g["lv"]):
            assert L["max_bx"] - 16 <= 4095 and L["max_by"] - 16 <= 2047, (c, l)
            assert L["w"] - 1 <= 0xfff and L["h"] - 1 <= 0xfff and l <= 0xf, (c, l)
            assert L["w"] <= 0xffff and L["h"] <= 0xffff, (c, l)


def test_cell_layout(sweep):
    for c, g, _ in accepted(sweep):
        G = g["cell_group"]
        base = 0
        cells = g["cells"]
        for l, L in enumerate(g["lv"]):
            n = L["ncols"] * L["nrows"]
            assert L["cell_base"] == base and base % G == 0, (c, l)
            v = cells[base:base + n]
            assert (v[:, 0] == l).all(), (c, l)
            base += (n + G - 1) // G * G
            pad = cells[L["cell_base"] + n:base]
            assert (pad[:, 3] == 0).all() and (pad[:, 4] == 0).all(), (c, l)  # padding is empty
            # the reference's cell views (:730-749), cell by cell
            ci, cj = np.divmod(np.arange(n), max(L["ncols"], 1))
            ini_y, ini_x = 16 + ci * L["hcell"], 16 + cj * L["wcell"]
            skip = (ini_y >= L["max_by"] - 3) | (ini_x >= L["max_bx"] - 6)
            vh = np.where(skip, 0, np.minimum(ini_y + L["hcell"] + 6, L["max_by"]) - ini_y)
            vw = np.where(skip, 0, np.minimum(ini_x + L["wcell"] + 6, L["max_bx"]) - ini_x)
            assert np.array_equal(v[:, 1], ini_x) and np.array_equal(v[:, 2], ini_y), (c, l)
            assert np.array_equal(v[:, 3], vw) and np.array_equal(v[:, 4], vh), (c, l)
            # the FAST tile: the view's rows, and its columns from ini_x & ~15 plus the
            # prefilter's spare right-neighbour dword
            assert (v[:, 4] <= g["fast_tile_rows"]).all(), (c, l)
            assert ((v[:, 1] & 15) + v[:, 3] + 4 <= g["fast_tile_stride"]).all(), (c, l)
            assert (v[:, 4] - 6 + 2 <= g["fast_score_rows"]).all(), (c, l)
            # cell_cap is the bound the code uses (orb_geometry.cpp's NMS comment): the strict
            # 8-neighbour maximum keeps at most one pixel per 2 x 2 block of the view's detect
            # area, (vw - 6) x (vh - 6)
            live = v[v[:, 3] > 0]
            kept = ((live[:, 3] - 6 + 1) // 2) * ((live[:, 4] - 6 + 1) // 2)
            assert (kept <= g["cell_cap"]).all(), (c, l)
            assert L["key_cap"] == min(n * g["cell_cap"], 65536), (c, l)
        assert g["cells_per_image"] == base == len(cells), c


def test_octree_lds_layout(sweep):
    """octree_img_kernel: [keys u32 x oct_kcap][per level: two lists of oct_nc 12-byte nodes]
    [per level: sort keys u32, pt / pe / pu / vnext i16, processed u8 per node]; octree_lvl_kernel
    takes one layout for every level."""
    for c, g, _ in accepted(sweep):
        lv = g["lv"]
        assert g["oct_lds_bytes"] <= 156 * 1024 and g["oct2_lds_bytes"] <= 144 * 1024, c
        for l, L in enumerate(lv):
            assert L["node_cap"] == max(4 * L["n_ini"], L["budget"] + 3), (c, l)
            assert L["oct_nc"] >= L["node_cap"] and L["oct_nc"] % 64 == 0, (c, l)
        if g["oct_kcap"]:
            spans = [(0, 4 * g["oct_kcap"])]
            for L in lv:
                spans.append((L["oct_list_off"], L["oct_list_off"] + 2 * L["oct_nc"] * 12))
                spans.append((L["oct_work_off"], L["oct_work_off"] + L["oct_nc"] * (4 + 4 * 2 + 1)))
                assert L["oct_list_off"] % 4 == 0 and L["oct_work_off"] % 4 == 0, c
            spans.sort()
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 <= b0, (c, spans)
            assert spans[-1][1] <= g["oct_lds_bytes"], c
            assert g["oct_kcap"] >= 1024 and g["oct_kcap"] <= 65535, c  # OctNodeS: 16-bit kbeg
        else:
            assert g["oct_lds_bytes"] == 0, c
        ncell = [L["ncols"] * L["nrows"] for L in lv]
        assert g["oct2_ccap"] >= max(ncell) + 1, c
        assert g["oct2_nc"] >= max(L["oct_nc"] for L in lv), c
        assert g["oct2_kcap"] >= 1024, c
        # [keys][staging][cell prefix][two lists][work: 32 bytes per node + 16 alignment]
        assert g["oct2_tmp_off"] >= 4 * g["oct2_kcap"], c
        assert g["oct2_cpre_off"] >= g["oct2_tmp_off"] + 4 * g["oct2_kcap"], c
        assert g["oct2_list_off"] >= g["oct2_cpre_off"] + 4 * g["oct2_ccap"], c
        assert g["oct2_work_off"] >= g["oct2_list_off"] + 2 * g["oct2_nc"] * 12, c
        assert g["oct2_lds_bytes"] >= g["oct2_work_off"] + g["oct2_nc"] * 32 + 16, c
        # the gather fast path (<= 512 cells): a key slot finds its group of cell_group cells by
        # a binary search from 0 with steps 256 / cell_group .. 1, which reaches indices up to
        # 512 / cell_group - 1: the level's last group index must not exceed that
        reach = 512 // g["cell_group"] - 1
        for l, n in enumerate(ncell):
            if n <= 512:
                assert (n + g["cell_group"] - 1) // g["cell_group"] - 1 <= reach, (c, l)


def test_pyramid_bands_and_ring(sweep):
    some_bands = some_ring = 0
    for c, g, _ in accepted(sweep):
        lv, nb, nl = g["lv"], g["pyr_bands"], len(g["lv"])
        assert 0 <= nb <= g["max_bands"], c
        if nb:
            some_bands += 1
            assert nl > 2 and 2 * g["pyr_band_lds"] <= 64 * 1024, c
            for l in range(2, nl):
                b = lv[l]["band"]
                assert len(b) == nb and (b[:, 0] <= b[:, 1]).all(), (c, l)
                assert b[0, 0] == 0 and b[-1, 1] == lv[l]["h"], (c, l)
                assert (b[1:, 0] <= b[:-1, 1]).all(), (c, l)  # no gap between consecutive bands
                assert b[:, 0].min() >= 0 and b[:, 1].max() <= lv[l]["h"], (c, l)
                assert ((b[:, 1] - b[:, 0]) * lv[l]["pitch"] <= g["pyr_band_lds"]).all(), (c, l)
                if l + 1 < nl:  # a band holds the source rows of its own rows of the next level
                    y0, y1 = resize_rows(lv[l + 1]["h"], lv[l]["h"])
                    for (lo, hi), (a, e) in zip(b, lv[l + 1]["band"]):
                        if e > a:
                            assert lo <= y0[a:e].min() and y1[a:e].max() < hi, (c, l)
        if g["pyr_ring_slots"]:
            some_ring += 1
            strip = g["pyr_ring_strip"]
            for l in range(1, nl):
                L = lv[l]
                assert L["pyr_rpi"] > 0 and 0 < L["pyr_slots"] <= g["pyr_ring_slots"], (c, l)
                assert L["pyr_lpr"] * L["pyr_rpi"] <= 64, (c, l)  # rows of a 1 KiB slot
                y0, y1 = resize_rows(L["h"], lv[l - 1]["h"])
                d0 = np.arange(0, L["h"], strip)
                d1 = np.minimum(d0 + strip, L["h"]) - 1
                assert (y1[d1] - y0[d0] + 1).max() <= L["pyr_slots"] * L["pyr_rpi"], (c, l)
    assert some_bands > 20 and some_ring > 20


def test_output_layout(sweep):
    for c, g, _ in accepted(sweep):
        run = 0
        for l, L in enumerate(g["lv"]):
            assert L["out_base"] == run and L["out_cap"] >= L["node_cap"], (c, l)
            run += L["out_cap"]
        assert g["kp_cap"] == run == g["out_per_image"], c


def test_named_sizes_take_their_branches(sweep):
    """The geometry facts the GPU cases of test_geometry_gpu.py are chosen for."""
    by = {c: g for c, g in sweep}
    ncell = lambda g, l: g["lv"][l]["ncols"] * g["lv"][l]["nrows"]
    g = by[(1536, 400, 2000, 1.2, 8)]
    assert ncell(g, 0) == 600 and ncell(g, 1) == 410
    assert [L["n_ini"] for L in g["lv"]] == [4, 4, 4, 4, 4, 5, 5, 5]
    g = by[(1344, 376, 2000, 1.2, 8)]
    assert ncell(g, 0) == 473
    for c in ((1504, 960, 2000, 1.2, 8), (1440, 1080, 2000, 1.2, 8), (1920, 1080, 2000, 1.2, 8),
              (1280, 112, 600, 1.2, 2)):
        assert by[c]["pyr_bands"] == 0, c
    assert by[(1280, 720, 2000, 1.2, 8)]["pyr_bands"] == 32
    assert by[(1241, 376, 2000, 1.2, 8)]["pyr_bands"] == 21
    for c in ((1600, 1200, 2000, 1.2, 8), (1920, 1080, 2000, 1.2, 8)):
        assert by[c]["casc_waves"] == 0, c
    assert by[(1241, 376, 2000, 1.2, 8)]["casc_waves"] > 0
    assert [L["n_ini"] for L in by[(1280, 112, 600, 1.2, 2)]["lv"]] == [16, 17]
    assert [L["n_ini"] for L in by[(2048, 160, 1000, 1.2, 4)]["lv"]] == [16, 17, 18, 19]
    assert all(L["n_ini"] == 1 for L in by[(480, 752, 1200, 1.2, 8)]["lv"])
