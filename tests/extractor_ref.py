"""ORBextractor (orb_extractor.cpp:18-88, 351-411, 422-794, 985-1075) restated in numpy, in the
reference's own order, sharing no code with oracle/ or csrc/ (it reads the sampling pattern
csrc/orb_pattern.inc as data). Integer steps are numpy integers, float steps explicit
numpy.float32 operations; the two fused multiply-adds of the Release build's descriptor
(DESIGN.md "FMA association") are computed exactly (float64 product, round-to-odd sum, one
rounding to float32).

The third-party primitives are restated from their published algorithms, as DESIGN.md cites them:
  cvRound            round half to even (cvtss2si)
  FAST(9_16, nonmax) as its definition: a pixel is a corner at threshold t if 9 contiguous ring
                     pixels are all darker than v - t or all brighter than v + t; its score is
                     max(t, best dark arc, best bright arc) - 1 where an arc's value is the
                     smallest |difference| in it (what cornerScore's two min/max sweeps compute);
                     non-maximum suppression is strict against the eight neighbours inside the
                     view FAST was called on, a pixel outside the tested interior scoring 0
  resize             INTER_LINEAR on u8: 11-bit coefficients, the (b*(r>>4))>>16 vertical pass
  GaussianBlur       7x7, sigma 2: integer kernel cvRound(256 k), exact integer row pass, column
                     pass rounded half to even (the vector path) or half up (the last w % 4)
  fastAtan2          OpenCV 3.3.1's atan_f32 polynomial in float steps
  cos / sin          glibc's sincosf (the FMA variant) in float64 steps with exact fma

Stages are callable on their own: tables(), level_sizes(), resize(), fast_cells(),
distribute_octree(), ic_angle(), blur(), descriptor(); extract() chains them as Compute does and
returns (keypoints[N] in the oracle's record layout, descriptors[N, 32], trace). trace is
  trace["tables"], trace["pyramid"]   the constructor's tables and the levels
  trace["levels"][l]  dict(w, h, cells, candidates, kept, n_candidates, octree=dict(passes,
                      inner_passes, exit, n_ini, n_nodes, N), skipped_cells=[(w, h), ...], xmax, dw)
  trace["kp"][i]      dict(level, lx, ly, cell=(i, j), fallback, passes, m01, m10, angle, reach)
                      for output keypoint i (lx, ly: level coordinates; cell: the FAST cell that
                      reported it; fallback: whether that cell ran at minThFAST; reach: the
                      largest |offset| a descriptor sample of it has)

rule=NAME replaces exactly one comparison, rounding or tie order by its nearest wrong variant;
RULES lists them with the line of orb_extractor.cpp (or the OpenCV / glibc routine) each belongs
to."""
import os
from fractions import Fraction

import numpy as np

F = np.float32
PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD = 31, 15, 19

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

RULES = {
    # name: (where, the rule, the wrong variant)
    "budget_round": (383, "cvRound(nDesired): half to even", "half away from zero"),
    "budget_last": (387, "last level takes nfeatures - sum", "last level rounds like the others"),
    "level_size_round": (1056, "cvRound(cols * invScale): half to even", "half away from zero"),
    "resize_coef_round": ("resize", "coefficients saturate_cast<short>(f * 2048): rounded",
                          "truncated"),
    "resize_final_round": ("resize", "(... + 2) >> 2", "(...) >> 2"),
    "resize_right_edge": ("resize", "dx >= xmax reads one source pixel", "no such columns"),
    "fast_strict_dark": ("FAST", "ring < v - t", "ring <= v - t"),
    "fast_strict_bright": ("FAST", "ring > v + t", "ring >= v + t"),
    "fast_arc": ("FAST", "9 contiguous ring pixels", "8"),
    "fast_first_col": ("FAST", "first tested column is 3", "4"),
    "fast_last_col": ("FAST", "last tested column is w - 4", "w - 5"),
    "fast_first_row": ("FAST", "first tested row is 3", "4"),
    "fast_last_row": ("FAST", "last tested row is h - 4", "h - 5"),
    "nms_w": ("FAST", "score > prev[j - 1]", ">="),
    "nms_e": ("FAST", "score > prev[j + 1]", ">="),
    "nms_nw": ("FAST", "score > pprev[j - 1]", ">="),
    "nms_n": ("FAST", "score > pprev[j]", ">="),
    "nms_ne": ("FAST", "score > pprev[j + 1]", ">="),
    "nms_sw": ("FAST", "score > curr[j - 1]", ">="),
    "nms_s": ("FAST", "score > curr[j]", ">="),
    "nms_se": ("FAST", "score > curr[j + 1]", ">="),
    "nms_cell_local": (750, "suppression sees the cell's own view only", "the whole level"),
    "fallback_empty": (753, "minThFAST only in a cell with no iniThFAST corner", "never"),
    "fallback_only_empty": (753, "minThFAST only in a cell with no iniThFAST corner", "always"),
    "cell_skip": (735, "iniY >= maxBorderY - 3, iniX >= maxBorderX - 6 skip the cell",
                  "no cell is skipped"),
    "nini_round": (484, "round(width / height): half away from zero", "half to even"),
    "ini_node_edge": (496, "(int)(hX * i): truncated", "rounded"),
    "bucket_div": (510, "initial node kp.x / hX, truncated", "the node whose [UL.x, UR.x) holds x"),
    "nomore_ini": (519, "an initial node with one key is final", "it is divided like the others"),
    "divide_x": (449, "kp.x < n1.UR.x goes left", "<="),
    "divide_y": (451, "kp.y < n1.BR.y goes up", "<="),
    "divide_ceil_x": (424, "halfX = ceil(width / 2)", "floor"),
    "divide_ceil_y": (425, "halfY = ceil(height / 2)", "floor"),
    "nomore_child": (469, "a child with one key is final", "it is divided again"),
    "oct_outer_finish": (610, "lNodes.size() >= N ends the passes", ">"),
    "oct_prev_exit": (610, "a pass that adds no node ends the passes",
                      "only a pass that divides no node does"),
    "oct_expand_threshold": (614, "size + 3 nToExpand > N enters the sorted phase", ">="),
    "oct_sort_order": (626, "largest node first", "smallest first"),
    "oct_sort_tie": (625, "equal sizes: the node created later first", "created earlier first"),
    "oct_inner_break": (671, "size >= N stops the sorted pass", ">"),
    "oct_inner_finish": (675, "size >= N ends the sorted phase", ">"),
    "oct_inner_prev_exit": (675, "a sorted pass that adds no node ends the phase",
                            "only one that divides no node does"),
    "retain_best": (693, "response > maxResponse: the first of equals", ">=: the last"),
    "umax_in": (34, "row v reaches u = +-umax[v]", "umax[v] - 1"),
    "umax_out": (34, "row v reaches u = +-umax[v]", "umax[v] + 1"),
    "atan_branch": ("fastAtan2", "ax >= ay takes the first octant formula", ">"),
    "atan_sign_x": ("fastAtan2", "x < 0 mirrors", "x <= 0"),
    "atan_sign_y": ("fastAtan2", "y < 0 mirrors", "y <= 0"),
    "factor_pi": (48, "angle * (float)(pi / 180)", "angle * (float)pi / 180"),
    "sincos_glibc": (54, "glibc's sincosf polynomial", "the correctly rounded sine and cosine"),
    "desc_fma": (60, "fma(x, b, y * a), fma(x, a, -(y * b))", "x * b + y * a, x * a - y * b"),
    "desc_round": (60, "cvRound of a coordinate: half to even", "half away from zero"),
    "desc_lt": (68, "t0 < t1", "t0 <= t1"),
    "blur_reflect101": (1030, "BORDER_REFLECT_101", "BORDER_REFLECT"),
    "blur_tail": ("GaussianBlur", "half up in the scalar tail x >= w - w % 4",
                  "half to even everywhere"),
    "blur_round": ("GaussianBlur", "half to even in the vector columns", "half up everywhere"),
}

# the rules no input reaches: test_extractor_boundaries.py asserts the argument instead
UNREACHABLE = ("resize_right_edge", "cell_skip")


def _pattern():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "slam_framework_amd", "csrc", "orb_pattern.inc")
    text = open(path).read()
    text = text[text.index("*/") + 2:]
    v = np.array([int(s) for s in text.replace(",", " ").split()], np.int64)
    assert v.size == 1024
    return v.reshape(512, 2)


PATTERN = _pattern()


def cv_round(v, away=False):
    """cvRound of float32 value(s) -> int64."""
    v = np.asarray(v, F)
    if away:
        return (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(np.int64)
    return np.rint(v).astype(np.int64)


# ---- :351-411 -------------------------------------------------------------------------------
class Tables:
    pass


def tables(nfeatures, scale_factor, nlevels, ini_th, min_th, rule=None):
    t = Tables()
    t.nfeatures, t.nlevels, t.ini_th, t.min_th = nfeatures, nlevels, ini_th, min_th
    sf = F(scale_factor)
    t.scale = [F(1.0)]
    for _ in range(1, nlevels):
        t.scale.append(F(t.scale[-1] * sf))
    t.inv_scale = [F(F(1.0) / s) for s in t.scale]
    factor = F(F(1.0) / sf)
    p = F(np.float64(factor) ** np.float64(nlevels))
    nd = F(F(F(nfeatures) * F(F(1) - factor)) / F(F(1) - p))
    t.budget, total = [], 0
    for _ in range(nlevels - 1):
        t.budget.append(int(cv_round(nd, away=rule == "budget_round")))
        total += t.budget[-1]
        nd = F(nd * factor)
    last = int(cv_round(nd)) if rule == "budget_last" else nfeatures - total
    t.budget.append(max(last, 0))
    vmax = int(np.floor(HALF_PATCH_SIZE * np.sqrt(F(2.0)) / 2 + 1))
    vmin = int(np.ceil(HALF_PATCH_SIZE * np.sqrt(F(2.0)) / 2))
    umax = [0] * (HALF_PATCH_SIZE + 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v))))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    t.umax = umax[:HALF_PATCH_SIZE + 1]
    return t


def level_sizes(t, cols, rows, rule=None):
    away = rule == "level_size_round"
    return [(int(cv_round(F(F(cols) * s), away)), int(cv_round(F(F(rows) * s), away)))
            for s in t.inv_scale]


# ---- resize ---------------------------------------------------------------------------------
def _short(v, trunc):
    v = np.asarray(v, F)
    i = np.trunc(v).astype(np.int64) if trunc else np.rint(v).astype(np.int64)
    return np.clip(i, -32768, 32767)


def resize(src, dw, dh, rule=None, info=None):
    sh, sw = src.shape
    trunc = rule == "resize_coef_round"

    def coef(n_dst, n_src):
        scale = 1.0 / (np.float64(n_dst) / np.float64(n_src))
        f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(F)).astype(F)
        return f, s

    fx, sx = coef(dw, sw)
    fx[sx < 0] = 0
    sx[sx < 0] = 0
    edge = sx + 1 >= sw
    xmax = int(np.nonzero(edge)[0][0]) if edge.any() else dw
    if rule == "resize_right_edge":
        xmax = dw
    last = sx >= sw - 1
    fx[last] = 0
    sx[last] = sw - 1
    a0 = _short((F(1.0) - fx) * F(2048), trunc)
    a1 = _short(fx * F(2048), trunc)
    fy, sy = coef(dh, sh)
    b0 = _short((F(1.0) - fy) * F(2048), trunc)
    b1 = _short(fy * F(2048), trunc)
    y0 = np.clip(sy, 0, sh - 1)
    y1 = np.clip(sy + 1, 0, sh - 1)
    S = src.astype(np.int64)
    sx1 = np.minimum(sx + 1, sw - 1)
    inside = np.arange(dw) < xmax
    H = np.where(inside[None, :], S[:, sx] * a0[None, :] + S[:, sx1] * a1[None, :],
                 S[:, sx] * 2048)
    r0, r1 = H[y0], H[y1]
    add = 0 if rule == "resize_final_round" else 2
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + add) >> 2
    if info is not None:
        info["xmax"], info["dw"] = xmax, dw
    return out.astype(np.uint8)


def pyramid(t, img, rule=None, infos=None):
    rows, cols = img.shape
    levels = [np.ascontiguousarray(img)]
    for l, (w, h) in enumerate(level_sizes(t, cols, rows, rule)):
        if l == 0:
            continue
        info = {}
        levels.append(resize(levels[-1], w, h, rule, info))
        if infos is not None:
            infos.append(info)
    return levels


# ---- FAST in cells (:712-770) ---------------------------------------------------------------
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3),
        (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def _arc_maps(img, arc):
    """Per pixel: the best dark and the best bright arc value (the largest, over the 16 arcs of
    `arc` contiguous ring pixels, of the smallest v - ring resp. ring - v in it); -256 on the
    3-pixel frame where the ring leaves the image."""
    h, w = img.shape
    I = img.astype(np.int16)
    d = np.full((16, h, w), -256, np.int16)
    for k, (dx, dy) in enumerate(RING):
        d[k, 3:h - 3, 3:w - 3] = I[3:h - 3, 3:w - 3] - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
    dark = np.full((h, w), -256, np.int16)
    bright = np.full((h, w), -256, np.int16)
    for s in range(16):
        idx = [(s + k) % 16 for k in range(arc)]
        dark = np.maximum(dark, d[idx].min(axis=0))
        bright = np.maximum(bright, (-d[idx]).min(axis=0))
    frame = np.ones((h, w), bool)
    frame[3:h - 3, 3:w - 3] = False
    dark[frame] = -256
    bright[frame] = -256
    return dark, bright


def fast_cells(t, img, rule=None, info=None):
    """The cell loop of ComputeKeyPointsOctTree on one level -> candidate list of
    (x, y, response, cell_i, cell_j, fallback) in octree coordinates, in the reference's order."""
    h, w = img.shape
    W = F(30)
    minBX = minBY = EDGE_THRESHOLD - 3
    maxBX, maxBY = w - EDGE_THRESHOLD + 3, h - EDGE_THRESHOLD + 3
    width, height = F(maxBX - minBX), F(maxBY - minBY)
    nCols, nRows = int(F(width / W)), int(F(height / W))
    wCell, hCell = int(np.ceil(F(width / F(nCols)))), int(np.ceil(F(height / F(nRows))))
    dark9, bright9 = _arc_maps(img, 9)
    dark, bright = (dark9, bright9) if rule != "fast_arc" else _arc_maps(img, 8)

    def corners(th):
        cd = dark >= th if rule == "fast_strict_dark" else dark > th
        cb = bright >= th if rule == "fast_strict_bright" else bright > th
        c = cd | cb
        score = np.where(c, np.maximum(np.maximum(dark9, bright9), th) - 1, 0)
        return c, score.astype(np.uint8).astype(np.int16)

    maps = {th: corners(th) for th in {t.ini_th, t.min_th}}
    out, skipped = [], []
    for i in range(nRows):
        iniY = F(minBY + i * hCell)
        maxY = F(iniY + F(hCell + 6))
        if iniY >= maxBY - 3:
            skipped.append((None, int(maxBY - iniY)))
            if rule != "cell_skip":
                continue
        if maxY > maxBY:
            maxY = F(maxBY)
        for j in range(nCols):
            iniX = F(minBX + j * wCell)
            maxX = F(iniX + F(wCell + 6))
            if iniX >= maxBX - 6:
                skipped.append((int(maxBX - iniX), None))
                if rule != "cell_skip":
                    continue
            if maxX > maxBX:
                maxX = F(maxBX)
            r0, r1, c0, c1 = int(iniY), int(maxY), int(iniX), int(maxX)
            vh, vw = r1 - r0, c1 - c0
            ya = 4 if rule == "fast_first_row" else 3
            yb = vh - 4 if rule == "fast_last_row" else vh - 3
            xa = 4 if rule == "fast_first_col" else 3
            xb = vw - 4 if rule == "fast_last_col" else vw - 3
            if yb <= ya or xb <= xa:
                continue

            def run(th):
                c, score = maps[th]
                S = np.zeros((vh + 2, vw + 2), np.int16)  # the view's score, zero frame
                S[1 + ya:1 + yb, 1 + xa:1 + xb] = score[r0 + ya:r0 + yb, c0 + xa:c0 + xb]
                if rule == "nms_cell_local":  # the whole level's score at this threshold
                    big = np.zeros((h + 2, w + 2), np.int16)
                    big[1:-1, 1:-1] = score
                    S = big[r0:r0 + vh + 2, c0:c0 + vw + 2].copy()
                C = np.zeros((vh + 2, vw + 2), bool)
                C[1 + ya:1 + yb, 1 + xa:1 + xb] = c[r0 + ya:r0 + yb, c0 + xa:c0 + xb]
                keep = C.copy()
                mid = S[1:-1, 1:-1]
                for name, dy, dx in (("nms_e", 0, 1), ("nms_w", 0, -1), ("nms_nw", -1, -1),
                                     ("nms_n", -1, 0), ("nms_ne", -1, 1), ("nms_sw", 1, -1),
                                     ("nms_s", 1, 0), ("nms_se", 1, 1)):
                    nb = S[1 + dy:vh + 1 + dy, 1 + dx:vw + 1 + dx]
                    keep[1:-1, 1:-1] &= (mid >= nb) if rule == name else (mid > nb)
                ys, xs = np.nonzero(keep[1:-1, 1:-1])
                return [(int(x), int(y), int(mid[y, x])) for y, x in zip(ys, xs)]

            found, fallback = run(t.ini_th), False
            if rule == "fallback_only_empty" or (not found and rule != "fallback_empty"):
                found, fallback = run(t.min_th), True
            for x, y, s in found:
                out.append((x + j * wCell, y + i * hCell, s, i, j, fallback))
    if info is not None:
        info.update(cells=(nRows, nCols, hCell, wCell), skipped_cells=skipped,
                    n_candidates=len(out))
    return out


# ---- DistributeOctTree (:422-704) -----------------------------------------------------------
class Node:
    __slots__ = ("keys", "ulx", "uly", "urx", "bry", "nomore", "seq")

    def __init__(self, ulx, uly, urx, bry):
        self.keys, self.ulx, self.uly, self.urx, self.bry = [], ulx, uly, urx, bry
        self.nomore, self.seq = False, 0


def _divide(n, K, rule):
    rx = np.floor if rule == "divide_ceil_x" else np.ceil
    ry = np.floor if rule == "divide_ceil_y" else np.ceil
    halfX = int(rx(F(F(n.urx - n.ulx) / F(2))))
    halfY = int(ry(F(F(n.bry - n.uly) / F(2))))
    mx, my = n.ulx + halfX, n.uly + halfY
    c = [Node(n.ulx, n.uly, mx, my), Node(mx, n.uly, n.urx, my),
         Node(n.ulx, my, mx, n.bry), Node(mx, my, n.urx, n.bry)]
    for k in n.keys:
        x, y = K[k][0], K[k][1]
        left = x <= mx if rule == "divide_x" else x < mx
        up = y <= my if rule == "divide_y" else y < my
        c[(0 if left else 1) + (0 if up else 2)].keys.append(k)
    for q in c:
        if len(q.keys) == 1 and rule != "nomore_child":
            q.nomore = True
    return c


def distribute_octree(K, minX, maxX, minY, maxY, N, rule=None, info=None):
    """K: candidates (x, y, response, ...) in octree coordinates -> indices into K of the kept
    keypoints, in the order of the node list."""
    if not K:
        return []
    q = F(F(maxX - minX) / F(maxY - minY))
    nIni = int(np.rint(q)) if rule == "nini_round" else int(cv_round(q, away=True))
    hX = F(F(maxX - minX) / F(nIni))
    seq = 0
    L = []
    edge = (lambda v: int(cv_round(v, away=True))) if rule == "ini_node_edge" else int
    for i in range(nIni):
        n = Node(edge(F(hX * F(i))), 0, edge(F(hX * F(i + 1))), maxY - minY)
        n.seq, seq = seq, seq + 1
        L.append(n)
    ini = list(L)
    for k, kp in enumerate(K):
        if rule == "bucket_div":
            b = next((i for i, n in enumerate(ini) if kp[0] < n.urx), nIni - 1)
        else:
            b = int(F(F(kp[0]) / hX))
        ini[b].keys.append(k)
    for n in ini:
        if len(n.keys) == 1 and rule != "nomore_ini":
            n.nomore = True
    L = [n for n in L if n.keys]

    def expand(n, sizes):
        nonlocal seq
        grown = 0
        for c in _divide(n, K, rule):
            if c.keys:
                c.seq, seq = seq, seq + 1
                L.insert(0, c)
                if len(c.keys) > 1:
                    grown += 1
                    sizes.append((len(c.keys), c))
        L.remove(n)
        return grown

    passes = inner = 0
    why = None
    finish = False
    while not finish:
        passes += 1
        prev = len(L)
        nToExpand, sizes, divided = 0, [], 0
        for n in list(L):
            if n.nomore:
                continue
            nToExpand += expand(n, sizes)
            divided += 1
        full = len(L) > N if rule == "oct_outer_finish" else len(L) >= N
        same = divided == 0 if rule == "oct_prev_exit" else len(L) == prev
        if passes > 64:
            same = True
        if full or same:
            finish, why = True, "full" if full else "no_growth"
        elif (len(L) + nToExpand * 3 >= N) if rule == "oct_expand_threshold" else \
                (len(L) + nToExpand * 3 > N):
            while not finish:
                inner += 1
                prev = len(L)
                prevs, sizes = sizes, []
                if rule == "oct_sort_tie":
                    prevs.sort(key=lambda s: (s[0], -s[1].seq))
                else:
                    prevs.sort(key=lambda s: (s[0], s[1].seq))
                order = prevs if rule == "oct_sort_order" else prevs[::-1]
                for _, n in order:
                    expand(n, sizes)
                    if (len(L) > N) if rule == "oct_inner_break" else (len(L) >= N):
                        break
                full = len(L) > N if rule == "oct_inner_finish" else len(L) >= N
                same = (not order) if rule == "oct_inner_prev_exit" else len(L) == prev
                if inner > 64:
                    same = True
                if full or same:
                    finish, why = True, "inner_full" if full else "inner_no_growth"
    out = []
    for n in L:
        best = n.keys[0]
        for k in n.keys[1:]:
            if (K[k][2] >= K[best][2]) if rule == "retain_best" else (K[k][2] > K[best][2]):
                best = k
        out.append(best)
    if info is not None:
        info["octree"] = dict(passes=passes, inner_passes=inner, exit=why, n_ini=nIni,
                              n_nodes=len(L), N=N)
    return out


# ---- IC_Angle (:18-45) and fastAtan2 --------------------------------------------------------
def fast_atan2(y, x, rule=None):
    y, x = F(y), F(x)
    k = F(180.0 / np.pi)
    p1, p3 = F(F(0.9997878412794807) * k), F(F(-0.3258083974640975) * k)
    p5, p7 = F(F(0.1555786518463281) * k), F(F(-0.04432655554792128) * k)
    eps = F(2.2204460492503131e-16)
    ax, ay = np.abs(x), np.abs(y)

    def poly(c):
        c2 = F(c * c)
        return F(F(F(F(F(F(F(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)

    if (ax > ay) if rule == "atan_branch" else (ax >= ay):
        a = poly(F(ay / F(ax + eps)))
    else:
        a = F(F(90.0) - poly(F(ax / F(ay + eps))))
    if (x <= 0) if rule == "atan_sign_x" else (x < 0):
        a = F(F(180.0) - a)
    if (y <= 0) if rule == "atan_sign_y" else (y < 0):
        a = F(F(360.0) - a)
    return a


def moments(img, x, y, umax, rule=None):
    grow = -1 if rule == "umax_in" else 1 if rule == "umax_out" else 0
    m01 = m10 = 0
    row = img[y].astype(np.int64)
    for u in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        m10 += u * int(row[x + u])
    for v in range(1, HALF_PATCH_SIZE + 1):
        d = umax[v] + grow
        plus = img[y + v, x - d:x + d + 1].astype(np.int64)
        minus = img[y - v, x - d:x + d + 1].astype(np.int64)
        u = np.arange(-d, d + 1)
        m01 += v * int((plus - minus).sum())
        m10 += int((u * (plus + minus)).sum())
    return m01, m10


def ic_angle(img, x, y, umax, rule=None):
    m01, m10 = moments(img, x, y, umax, rule)
    return fast_atan2(F(m01), F(m10), rule), m01, m10


# ---- GaussianBlur ---------------------------------------------------------------------------
def gauss_kernel():
    x = np.arange(7, dtype=np.float64) - 3.0
    cf = np.exp(-0.5 / 4.0 * x * x).astype(F)
    s = 1.0 / cf.astype(np.float64).sum()
    cf = (cf.astype(np.float64) * s).astype(F)
    return np.rint(cf.astype(np.float64) * 256.0).astype(np.int64)


def blur(img, rule=None):
    h, w = img.shape
    k = gauss_kernel()
    mode = "symmetric" if rule == "blur_reflect101" else "reflect"
    P = np.pad(img.astype(np.int64), 3, mode=mode)
    Hh = sum(k[i] * P[:, i:i + w] for i in range(7))
    V = sum(k[i] * Hh[i:i + h, :] for i in range(7))
    even = np.rint(V.astype(np.float64) / 65536.0).astype(np.int64)  # exact: V < 2^24
    up = (V + 32768) >> 16
    xvec = w if rule == "blur_tail" else 0 if rule == "blur_round" else w - w % 4
    out = np.where(np.arange(w)[None, :] < xvec, even, up)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- cos / sin: glibc sincosf, FMA variant --------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_HPI_INV = float.fromhex("0x1.45f306dc9c883p+23")
_HPI = float.fromhex("0x1.921fb54442d18p+0")
_SC = [[float.fromhex(s) for s in row] for row in (
    ("0x1p+0", "-0x1.ffffffd0c621cp-2", "-0x1.555545995a603p-3", "0x1.55553e1068f19p-5",
     "0x1.1107605230bc4p-7", "-0x1.6c087e89a359dp-10", "-0x1.994eb3774cf24p-13",
     "0x1.99343027bf8c3p-16"),
    ("-0x1p+0", "0x1.ffffffd0c621cp-2", "-0x1.555545995a603p-3", "-0x1.55553e1068f19p-5",
     "0x1.1107605230bc4p-7", "0x1.6c087e89a359dp-10", "-0x1.994eb3774cf24p-13",
     "-0x1.99343027bf8c3p-16"))]  # c0 c1 s1 c2 s2 c3 s3 c4; the second row for quadrants n & 2
_SIGN = (1.0, -1.0, -1.0, 1.0)


def _sin_poly(x, x2, p):
    s1 = _fma(x2, p[6], p[4])
    x3 = x2 * x
    x7 = x2 * x3
    s = _fma(x3, p[2], x)
    return F(_fma(s1, x7, s))


def _cos_poly(x2, p):
    x4 = x2 * x2
    c1 = _fma(x2, p[1], p[0])
    c2 = _fma(x2, p[7], p[5])
    x6 = x2 * x4
    c = _fma(x4, p[3], c1)
    return F(_fma(c2, x6, c))


def sincosf(y, rule=None):
    """(sin, cos) of a float32 in [0, 120) as glibc 2.35's x86-64 FMA sinf / cosf give them."""
    y = F(y)
    x = float(y)
    if rule == "sincos_glibc":
        return F(np.sin(np.longdouble(x))), F(np.cos(np.longdouble(x)))
    top = (int(y.view(np.uint32)) >> 20) & 0x7ff
    if top < 0x3f4:
        if top < 0x398:
            return y, F(1.0)
        return _sin_poly(x, x * x, _SC[0]), _cos_poly(x * x, _SC[0])
    assert top < 0x42f
    n = (int(x * _HPI_INV) + 0x800000) >> 24
    r = _fma(-float(n), _HPI, x)
    p = _SC[1] if n & 2 else _SC[0]
    if n & 1:
        return _cos_poly(r * r, p), _sin_poly(r * _SIGN[n & 3], r * r, p)
    return _sin_poly(r * _SIGN[n & 3], r * r, p), _cos_poly(r * r, p)


# ---- computeOrbDescriptor (:49-88) ----------------------------------------------------------
def _fma32(x, y, z):
    """fmaf on float32 arrays: the product is exact in float64; the sum is rounded to odd in
    float64, so that the one rounding to float32 is the fused result's."""
    p = x.astype(np.float64) * y.astype(np.float64)
    z = z.astype(np.float64)
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0)
    up = (err > 0) == (s > 0)
    bits[fix & up] += 1
    bits[fix & ~up] -= 1
    return bits.view(np.float64).astype(F)


def sample_coords(angle, rule=None):
    """The 512 (rx, ry) of a keypoint with `angle` degrees, and (a, b)."""
    angle = F(angle)
    if rule == "factor_pi":
        rad = F(F(angle * F(np.pi)) / F(180.0))
    else:
        rad = F(angle * F(np.pi / 180.0))
    b, a = sincosf(rad, rule)
    px, py = PATTERN[:, 0].astype(F), PATTERN[:, 1].astype(F)
    A, B = np.full(512, a, F), np.full(512, b, F)
    if rule == "desc_fma":
        fy = (px * B).astype(F) + (py * A).astype(F)
        fx = (px * A).astype(F) - (py * B).astype(F)
    else:
        fy = _fma32(px, B, (py * A).astype(F))
        fx = _fma32(px, A, -(py * B).astype(F))
    away = rule == "desc_round"
    return cv_round(fx, away), cv_round(fy, away), a, b


def descriptor(blurred, x, y, angle, rule=None):
    rx, ry, _, _ = sample_coords(angle, rule)
    v = blurred[y + ry, x + rx].astype(np.int64).reshape(256, 2)
    bits = (v[:, 0] <= v[:, 1]) if rule == "desc_lt" else (v[:, 0] < v[:, 1])
    reach = int(max(np.abs(rx).max(), np.abs(ry).max()))
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32), reach


# ---- Compute (:985-1049) --------------------------------------------------------------------
def extract(orb, img, rule=None):
    """orb = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)."""
    assert rule is None or rule in RULES, rule
    t = tables(*orb, rule=rule)
    infos = []
    levels = pyramid(t, img, rule, infos)
    trace = dict(levels=[], kp=[], pyramid=levels, tables=t)
    per_level = []
    for l, lv in enumerate(levels):
        h, w = lv.shape
        info = dict(w=w, h=h)
        if l:
            info.update(infos[l - 1])
        K = fast_cells(t, lv, rule, info)
        info["candidates"] = K
        kept = distribute_octree(K, 16, w - 16, 16, h - 16, t.budget[l], rule, info)
        info["kept"] = kept
        size = F(int(F(F(PATCH_SIZE) * t.scale[l])))
        kps = []
        for k in kept:
            x, y, s, ci, cj, fb = K[k]
            kps.append(dict(x=x + 16, y=y + 16, response=s, size=size, cell=(ci, cj), fallback=fb))
        per_level.append(kps)
        trace["levels"].append(info)
    for l, kps in enumerate(per_level):  # computeOrientation, after every level's octree
        for kp in kps:
            kp["angle"], kp["m01"], kp["m10"] = ic_angle(levels[l], kp["x"], kp["y"], t.umax, rule)
    n = sum(len(k) for k in per_level)
    out = np.zeros(n, KP_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    i = 0
    for l, kps in enumerate(per_level):
        if not kps:
            continue
        B = blur(levels[l], rule)
        for kp in kps:
            desc[i], reach = descriptor(B, kp["x"], kp["y"], kp["angle"], rule)
            x, y = F(kp["x"]), F(kp["y"])
            if l != 0:
                x, y = F(x * t.scale[l]), F(y * t.scale[l])
            out[i] = (x, y, kp["size"], kp["angle"], F(kp["response"]), l, -1)
            trace["kp"].append(dict(level=l, cell=kp["cell"], fallback=kp["fallback"],
                                    passes=trace["levels"][l]["octree"]["passes"],
                                    m01=kp["m01"], m10=kp["m10"], angle=kp["angle"], reach=reach,
                                    lx=kp["x"], ly=kp["y"]))
            i += 1
    return out, desc, trace
