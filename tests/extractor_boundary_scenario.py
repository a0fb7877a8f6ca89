"""Constructed images on which each comparison of ORBextractor (orb_extractor.cpp:18-88, 351-411,
422-794, 985-1075) decides at equality or one step beside it (numpy only).

All cases but `levels`, `saturated` and `size_tie` are a flat background of 100 at 282 x 132 with
four levels of scale 1.2 (282 x 132, 235 x 110, 196 x 92, 163 x 76): level 0's border box is
250 x 100, so width / height is 2.5 (nIni is 3 by round(), 2 by half-to-even), its FAST cells are
32 x 34 with tested interiors [19 + 32 j, 51 + 32 j) x [19 + 34 i, 53 + 34 i) that tile the box
(no pixel is tested by two cells: the 6-pixel overlap of the views is FAST's own 3-pixel frame
twice, so a corner beside a cell edge is suppressed by its own cell's scores only), and its
initial octree nodes are [0, 83), [83, 166), [166, 250) in octree coordinates (level - 16).

  dot     one pixel at 100 + c. Every ring pixel differs from it by |c|: a corner iff |c| > the
          threshold, with response |c| - 1. |c| <= 9 leaves at most 0.81 |c| < 7.3 of it on level
          1, so it is a keypoint of level 0 only, with moments (0, 0), angle 0 and the all-zero
          descriptor; |c| > 20 is found at iniThFAST and shows on the upper levels too.
  extra   a pixel of contrast <= 6, at least 4 pixels from its dot (off the radius-3 ring and the
          NMS neighbours): no corner, it adds u * k to m_10 and v * k to m_01 exactly.
  block   a square of contrast <= 6 and its mirror image about the dot: no corner, no moment; it
          tilts the blurred image under chosen descriptor samples.

Each case names the rules (extractor_ref.RULES) it is there for and carries its precondition
(check()): what extractor_ref's trace must show on it, with the value the cited line gives and
what the nearest wrong rule would give. Searched constants (moment pairs, block places) were
found once by the searches described in DESIGN.md; check() catches drift."""
import numpy as np

import extractor_ref as R

COLS, ROWS = 282, 132
BG = 100
F = np.float32


def orb(nfeatures):
    return (nfeatures, 1.2, 4, 20, 7)


class Case:
    def __init__(self, name, nfeatures, dots, rules, expect=(), doc="", bg=BG, size=(COLS, ROWS),
                 paint=None):
        self.orb = nfeatures if isinstance(nfeatures, tuple) else orb(nfeatures)
        self.name, self.dots, self.rules = name, list(dots), tuple(rules)
        self.expect, self.doc, self.bg, self.size, self.paint = list(expect), doc, bg, size, paint

    def image(self):
        img = np.full((self.size[1], self.size[0]), self.bg, np.int16)
        if self.paint:
            self.paint(img)
        for x, y, c in self.dots:
            img[y, x] += c
        assert img.min() >= 0 and img.max() <= 255
        img = img.astype(np.uint8)
        img.setflags(write=False)
        return img


def okey(x, y, c=9):
    """A dot given in octree coordinates of level 0."""
    return (x + 16, y + 16, c)


def find(kps, x, y, octave=0):
    hit = np.nonzero((kps["x"] == F(x)) & (kps["y"] == F(y)) & (kps["octave"] == octave))[0]
    return [int(i) for i in hit]


# ---- FAST -----------------------------------------------------------------------------------
def _arc(cx, cy, n, c=30):
    return [(cx + dx, cy + dy, c) for dx, dy in R.RING[:n]]


FAST_DOTS = (
    [(25, 25, 20), (40, 40, 25)] +            # cell (0,0): ring == v - t at iniThFAST, one above
    [(57, 25, -20), (72, 40, -25)] +          # cell (0,1): the same, dark dots (ring == v + t)
    [(95, 30, 8)] +                           # cell (0,2): found at minThFAST only
    [(130, 30, 7)] +                          # cell (0,3): ring == v - t at minThFAST: nothing
    [(160, 30, -7)] +                         # cell (0,4): ring == v + t at minThFAST: nothing
    [(190, 30, -8), (200, 19, 9)] +           # cell (0,5): dark at minThFAST; first tested row
    _arc(225, 35, 9) +                        # cell (0,6): an arc of exactly 9
    _arc(252, 35, 8) +                        # cell (0,7): an arc of 8
    [(30, 65, 9), (31, 65, 9)] +              # cell (1,0): equal scores E / W
    [(65, 65, 9), (65, 66, 9)] +              # cell (1,1): N / S
    [(95, 65, 9), (96, 66, 9)] +              # cell (1,2): NW / SE
    [(130, 66, 9), (131, 65, 9)] +            # cell (1,3): SW / NE
    [(147, 60, 9), (178, 70, 9), (160, 53, 9), (165, 86, 9)] +  # cell (1,4): its first and last
    #                                           tested column and row
    [(195, 65, 25), (196, 65, 9)] +           # cell (1,5): a weaker neighbour is suppressed
    [(19, 100, 9), (262, 100, 9), (100, 112, 9)] +  # the level's first / last column, last row
    [(50, 100, 9), (51, 100, 9)] +            # cells (2,0) | (2,1): equal neighbours across the edge
    [(146, 100, 25), (147, 101, 9)]           # cells (2,3) | (2,4): a weaker one across the edge
)


def _check_fast(case, kps, desc, tr):
    def has(x, y, **kw):
        i = find(kps, x, y)
        assert len(i) == 1, (case.name, x, y, len(i))
        for k, v in kw.items():
            got = tr["kp"][i[0]][k] if k in tr["kp"][i[0]] else kps[i[0]][k]
            assert got == v, (case.name, x, y, k, got, v)

    def absent(x, y):
        assert not find(kps, x, y), (case.name, x, y)

    # :751 FAST at iniThFAST = 20: contrast 25 is a corner (response 24), contrast 20 is not
    # (strict); <= would report it, and the fallback (:753) would report it at 7
    has(40, 40, fallback=False, response=24.0), absent(25, 25)
    has(72, 40, fallback=False, response=24.0), absent(57, 25)
    # :755 the cell's only corner appears at minThFAST = 7: contrast 8 found, 7 not
    has(95, 30, fallback=True, response=7.0), absent(130, 30), absent(160, 30)
    has(190, 30, fallback=True, response=7.0), has(200, 19, fallback=True, response=8.0)
    has(225, 35, response=29.0), absent(252, 35)
    for x, y in ((30, 65), (31, 65), (65, 65), (65, 66), (95, 65), (96, 66), (130, 66), (131, 65)):
        absent(x, y)  # equal scores suppress each other; >= would keep one of each pair
    for x, y in ((147, 60), (178, 70), (160, 53), (165, 86), (19, 100), (262, 100), (100, 112)):
        has(x, y, response=8.0)
    has(195, 65, response=24.0), absent(196, 65)
    has(50, 100, cell=(2, 0)), has(51, 100, cell=(2, 1))  # a level-wide NMS would drop both
    has(146, 100, cell=(2, 3)), has(147, 101, cell=(2, 4), fallback=True)
    cand = tr["levels"][0]["candidates"]
    assert len({(c[0], c[1]) for c in cand}) == len(cand), "a pixel is reported by one cell only"


# ---- octree ---------------------------------------------------------------------------------
def _check_octree(want):
    def check(case, kps, desc, tr):
        o = tr["levels"][0]["octree"]
        for k, v in want.items():
            if k == "n0":
                got = int((kps["octave"] == 0).sum())
            elif k == "n_candidates":
                got = tr["levels"][0]["n_candidates"]
            else:
                got = o[k]
            assert got == v, (case.name, k, got, v)
    return check


def _quad(x0, y0, w, h, n=2):
    """n keys in each quadrant of the node [x0, x0 + w) x [y0, y0 + h), apart in both axes."""
    out = []
    for qx in (0, 1):
        for qy in (0, 1):
            bx, by = x0 + qx * ((w + 1) // 2), y0 + qy * ((h + 1) // 2)
            for k in range(n):
                out.append(okey(bx + 4 + 11 * k + 3 * qy, by + 5 + 12 * k + 2 * qx,
                                9 if k == 0 else 8))
    return out


def _cases():
    C = []
    C.append(Case("fast", 1000, FAST_DOTS,
                  ("fast_strict_dark", "fast_strict_bright", "fast_arc", "fast_first_col",
                   "fast_last_col", "fast_first_row", "fast_last_row", "nms_w", "nms_e", "nms_nw",
                   "nms_n", "nms_ne", "nms_sw", "nms_s", "nms_se", "nms_cell_local",
                   "fallback_empty", "fallback_only_empty", "desc_lt"),
                  [_check_fast],
                  doc="FAST(9_16) and the cell loop :730-770: ring differences equal to the "
                      "threshold in both signs at both thresholds, arcs of 9 and 8, equal scores "
                      "in each of the eight NMS neighbours, the first and last column and row a "
                      "cell and the level test, neighbours on both sides of a cell edge"))
    # :484 nIni = round(250 / 100) = 3 (2 by half-to-even); :496 UL.x = (int)(hX * 2) = 166 (167
    # rounded), so node 2 divides at 208 (209): the keys at 208 and 230 stay together, the pass
    # adds no node and :610 ends with one of them lost (the first of equal responses kept, :693).
    # :510 keys at 83 and 166 are 0.996 and 1.992 initial nodes from the left: nodes 0 and 1,
    # though UR.x of those nodes is 83 and 166.
    C.append(Case("ini_edge", 1000, [okey(10, 20), okey(120, 30), okey(208, 20), okey(230, 30)],
                  ("nini_round", "ini_node_edge", "nomore_ini", "oct_prev_exit", "retain_best"),
                  [_check_octree(dict(n_ini=3, n_candidates=4, n0=3, passes=1, exit="no_growth")),
                   lambda c, k, d, tr: (find(k, 224, 36) and not find(k, 246, 46)) or _fail(c)],
                  doc=":484-526 the initial nodes' edges; :610 a pass that adds no node; :693"))
    C.append(Case("ini_bucket", 1000,
                  [okey(10, 20), okey(83, 60), okey(120, 30), okey(166, 70), okey(200, 20)],
                  ("nini_round", "bucket_div"),
                  [_check_octree(dict(n_ini=3, n_candidates=5, n0=5, passes=2))],
                  doc=":510 kp.x / hX just under a whole number at x = UR.x of nodes 0 and 1"))
    # :449-451 keys exactly on n1.UR.x = 42 and n1.BR.y = 50 of node [0, 83) x [0, 100) go right
    # and down; 83 is odd: halfX = ceil(41.5) = 42 (41 by floor). Node 1 [83, 166) and node 2
    # hold the same layout for y; every key is alone after the first pass.
    C.append(Case("divide_edges", 1000,
                  [okey(41, 10), okey(42, 30), okey(100, 49), okey(110, 50), okey(200, 10),
                   okey(230, 60)],
                  ("divide_x", "divide_y", "divide_ceil_x", "nomore_child"),
                  [_check_octree(dict(n0=6, passes=2, exit="no_growth"))],
                  doc=":422-478 DivideNode, keys on the dividing lines, an odd width"))
    # an odd height two passes down: node [0, 21) x [0, 25) of the third pass divides at y = 13
    # (12 by floor) and x = 11; the keys (11, 12), (20, 13) part there, one pass later by floor.
    # Nodes 1 and 2 carry two keys per quadrant and per quadrant's quadrant so that every pass adds nodes.
    C.append(Case("divide_deep", 1000,
                  [okey(11, 12), okey(20, 13)] + _quad(83, 0, 83, 100) +
                  [okey(170, 5), okey(180, 9, 8), okey(172, 20), okey(190, 40, 8), okey(240, 90)],
                  ("divide_ceil_y",),
                  [_check_octree(dict(n0=15))],
                  doc=":424-425 ceil of an odd half, below the first pass"))
    # :610-679 the counts. After the first pass of COUNT_KEYS the list holds 6 nodes, 4 of them to
    # expand (sizes 2, 3, 2, 3 in creation order); there are 12 keys in all.
    #   N = 6   size == N after a full pass: :610 ends (6 keypoints); > would go on to 7
    #   N = 18  size + 3 nToExpand == N: :614 is false, the next pass is a plain one in list
    #           order (n4, n3, n2, n1); >= would take them in sorted order (n4, n2, n3, n1)
    #   N = 17  one more: the sorted phase; the two 3-key nodes first, the later created of
    #           equals first (:625 sorts pair<int, ExtractorNode*>, DESIGN.md on the tie)
    #   N = 7   the sorted pass reaches N exactly when n4 has split 2 + 1: :671 breaks, :675 ends
    for nf, N, rules, want in (
            (19, 6, ("oct_outer_finish", "retain_best"), dict(n0=6, passes=1, exit="full")),
            (56, 18, ("oct_expand_threshold",), dict(n0=12, inner_passes=0, exit="no_growth")),
            (53, 17, ("oct_sort_order", "oct_sort_tie"),
             dict(n0=12, passes=1, inner_passes=3, exit="inner_no_growth")),
            (22, 7, ("oct_inner_break", "oct_inner_finish"),
             dict(n0=7, passes=1, inner_passes=1, exit="inner_full"))):
        want.update(N=N, n_candidates=12)
        C.append(Case(f"count_{N}", nf, COUNT_KEYS, rules, [_check_octree(want)],
                      doc=f":610-679 with N = {N}"))
    # :675 a sorted pass that divides a node and adds none: the keys (3, 3), (10, 9) share the
    # boxes [0, 42) x [0, 50), [0, 21) x [0, 25) and [0, 11) x [0, 13); the other quadrants part at
    # once, the second sorted pass divides that node alone and the phase ends with 9 keypoints.
    C.append(Case("count_stall", 53,
                  [okey(3, 3, 8), okey(10, 9), okey(46, 5), okey(70, 40), okey(5, 55), okey(30, 90),
                   okey(46, 55), okey(70, 90), okey(120, 30), okey(200, 60)],
                  ("oct_inner_prev_exit",),
                  [_check_octree(dict(N=17, n_candidates=10, n0=9, passes=1, inner_passes=2,
                                      exit="inner_no_growth"))],
                  doc=":675 size == prevSize inside the sorted phase"))
    # :383 with (7, 1.8, 2 levels): nDesired = 7 * (1 - 1/1.8f) / (1 - (1/1.8f)^2) is 4.5 in
    # float: cvRound gives 4 (5 away from zero). The first pass leaves 4 nodes, one of them the
    # pair (170, 5), (200, 40) that parts one division later: 4 >= 4 ends with 4 keypoints.
    C.append(Case("budget_tie", (7, 1.8, 2, 20, 7),
                  [okey(10, 20), okey(60, 70), okey(120, 30), okey(170, 5), okey(200, 40)],
                  ("budget_round", "oct_outer_finish"),
                  [_check_octree(dict(N=4, n_candidates=5, n0=4, passes=1, exit="full"))],
                  doc=":377-387 the per-level budget on a tie"))
    # :1056 279 * (1/1.2f) is 232.5 and 135 * (1/1.2f) is 112.5 in float: level 1 is 232 x 112
    # (233 x 113 away from zero). Contrast 25 and 60 dots are keypoints of the upper levels too.
    C.append(Case("size_tie", 1000,
                  [(30 + 37 * i, 30 + 25 * (i % 4), 60 if i % 2 else -25) for i in range(7)],
                  ("level_size_round", "resize_final_round"),
                  [lambda c, k, d, tr: (tr["levels"][1]["w"], tr["levels"][1]["h"]) == (232, 112)
                   and (k["octave"] == 1).sum() > 0 or _fail(c)],
                  size=(279, 135), doc=":1055-1056 level sizes on a tie"))
    C.append(Case("angles", 1000, _angle_dots(), ("umax_in", "umax_out", "atan_branch",
                                                  "atan_sign_x", "atan_sign_y"),
                  [_check_angles], doc=":18-45 IC_Angle's patch edge and fastAtan2's branches"))
    C.append(Case("descriptor", 1000, _desc_dots(),
                  ("desc_fma", "desc_round", "sincos_glibc", "factor_pi", "blur_round"),
                  [_check_desc], doc=":49-88 samples whose coordinate the rule decides, over a "
                                     "blurred slope that makes the bit follow the pixel; "
                                     "GaussianBlur's rounding on a tie"))
    C.append(Case("blur_border", 1000, _border_dots(), ("blur_reflect101", "blur_tail"),
                  [_check_border],
                  doc=":1030 a sample 18 pixels from a keypoint on the level's first and last "
                      "tested column: the mirrored border and the blur's scalar tail are read"))
    C.append(Case("saturated", 1000,
                  [(40 + 40 * i, 40 + 20 * (i % 3), -9 if i % 2 else -60) for i in range(6)],
                  ("desc_lt",), [_check_saturated], bg=255,
                  doc="a patch of 255: blurred row sums of 255 * 257 = 65535"))
    C.append(Case("levels", 131, [], ("resize_coef_round", "resize_final_round", "budget_last"),
                  [_check_levels], paint=_paint_levels,
                  doc="magnified neighbourhoods of real keypoints: every octave, fractional "
                      "coordinates, angles in every octant, the budget binding on level 0"))
    return C


# ---- IC_Angle -------------------------------------------------------------------------------
# extra pixels (u, v, k) per site and the moments (m_01, m_10) they give; umax is
# 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3 for v = 0..15
ANGLE_SITES = [
    ((), (0, 0)),
    (((5, 0, 5),), (0, 25)), (((-5, 0, 5),), (0, -25)),
    (((0, 5, 5),), (25, 0)), (((0, -5, 5),), (-25, 0)),
    (((5, 5, 5),), (25, 25)), (((-5, 5, 5),), (25, -25)),
    (((-5, -5, 5),), (-25, -25)), (((5, -5, 5),), (-25, 25)),
    (((11, 10, 5),), (50, 55)), (((12, 10, 5),), (0, 0)),      # u = umax[10] and one beyond
    (((-11, -10, 5),), (-50, -55)), (((-12, -10, 5),), (0, 0)),
    (((3, 15, 5),), (75, 15)), (((4, 15, 5),), (0, 0)),        # umax[15] = 3
    (((15, 0, 5),), (0, 75)), (((15, 3, 5),), (15, 75)), (((15, 4, 5),), (0, 0)),
    (((5, 0, -5),), (0, -25)), (((0, 5, -5), (7, 0, 3)), (-25, 21)),
    (((-15, -3, 6), (6, 9, -2)), (-36, -102)),
]


def _site_xy(i):
    return 35 + 36 * (i % 7), 30 + 36 * (i // 7)


def _angle_dots():
    out = []
    for i, (extras, _) in enumerate(ANGLE_SITES):
        x, y = _site_xy(i)
        out.append((x, y, 9))
        out += [(x + u, y + v, k) for u, v, k in extras]
    return out


def _check_angles(case, kps, desc, tr):
    exact = {(0, 25): 0.0, (0, -25): 180.0, (25, 0): 90.0, (-25, 0): 270.0, (0, 0): 0.0}
    for i, (_, (m01, m10)) in enumerate(ANGLE_SITES):
        x, y = _site_xy(i)
        j = find(kps, x, y)
        assert len(j) == 1, (case.name, i)
        t = tr["kp"][j[0]]
        assert (t["m01"], t["m10"]) == (m01, m10), (case.name, i, t["m01"], t["m10"])
        if (m01, m10) in exact:  # the values atan_f32 gives on the axes and at the origin
            assert float(kps[j[0]]["angle"]) == exact[(m01, m10)], (case.name, i)
    # on the diagonals the two octant formulas differ: 90 - p(1) is not p(1) in float
    assert R.fast_atan2(25, 25) != R.fast_atan2(25, 25, "atan_branch")
    # at the origin x <= 0 would give 180 and y <= 0 would give 360
    assert float(R.fast_atan2(0, 0, "atan_sign_x")) == 180.0
    assert float(R.fast_atan2(0, 0, "atan_sign_y")) == 360.0


# ---- computeOrbDescriptor --------------------------------------------------------------------
# (rule, m_01, m_10, sample, its (x, y) by the rule, by the wrong variant, block (x0, y0, side, k)).
# The moment pairs come from a search over |m| <= 300 (about 258000 distinct angles): the pairs at
# which the rule moves a sample to the neighbouring pixel. The moments are built from extras on
# the two axes (_axis_extras), the block and its mirror image put a slope of one grey level under
# the two pixels, the sample's partner lies on the flat part: the bit follows the pixel.
DESC_SITES = [
    ("desc_fma", -157, -6, 192, (-13, -5), (-13, -4), (-15, -10, 5, -1)),
    ("desc_fma", -25, 263, 153, (-6, 6), (-5, 6), (-10, 4, 5, 2)),
    ("desc_fma", 164, -149, 121, (-14, 3), (-14, 4), (-16, 1, 5, 1)),
    ("desc_round", -157, 6, 113, (4, 13), (5, 13), (2, 11, 5, 1)),
    ("desc_round", -281, -107, 270, (8, -9), (9, -9), (3, -11, 5, -1)),
    ("sincos_glibc", -107, -281, 135, (-9, 8), (-9, 9), (-11, 6, 5, 1)),
    ("factor_pi", 49, 3, 273, (8, 5), (8, 6), (6, 3, 5, 1)),
    ("factor_pi", -137, 166, 175, (7, 6), (6, 6), (6, 3, 7, 1)),
]
# GaussianBlur on a tie: with these differences around sample 56 = (-10, -12) of a keypoint at
# angle 0 (and mirrored about it, so that the moments stay (0, 0)) the column sum there is
# 100 * 65536 + 32768: 100 by half-to-even, 101 by half-up; the partner sees the flat 101.
TIE_SAMPLE, TIE_AT = 56, (-10, -12)
TIE_ROWS = ((-3, -3, -3, -2, -3, -3, -3), (0, -2, -2, 0, 0, 0, 0))  # rows -3 and -2 of the 7 x 7


def _axis_extras(m):
    """[(offset, k)] with sum(offset * k) == m: distinct offsets of 4..15 pixels, |k| <= 6."""
    offs = list(range(15, 3, -1))

    def rec(rem, i):
        if rem == 0:
            return []
        if i == len(offs):
            return None
        o = offs[i]
        rest = 12 * sum(offs[i + 1:])
        for k in sorted(range(-6, 7), key=lambda k: abs(rem - o * k)):
            for sgn in ((1,) if k == 0 else (1, -1)):
                r = rem - sgn * o * k
                if abs(r) <= rest:
                    sub = rec(r, i + 1)
                    if sub is not None:
                        return ([(sgn * o, k)] if k else []) + sub
        return None
    return rec(m, 0)


def _desc_xy(i):
    return 30 + 40 * (i % 6), 30 + 40 * (i // 6)


def _desc_dots():
    out = []
    for i, (_, m01, m10, _, _, _, (x0, y0, side, k)) in enumerate(DESC_SITES):
        x, y = _desc_xy(i)
        out.append((x, y, 9))
        out += [(x, y + v, kk) for v, kk in _axis_extras(m01)]
        out += [(x + u, y, kk) for u, kk in _axis_extras(m10)]
        for yy in range(y0, y0 + side):
            for xx in range(x0, x0 + side):
                out += [(x + xx, y + yy, k), (x - xx, y - yy, k)]
    x, y = _desc_xy(len(DESC_SITES))
    out.append((x, y, 9))
    for r, row in zip((-3, -2), TIE_ROWS):
        for c, d in zip(range(-3, 4), row):
            if d:
                out += [(x + TIE_AT[0] + c, y + TIE_AT[1] + r, d),
                        (x - TIE_AT[0] - c, y - TIE_AT[1] - r, d)]
    return out


def _check_desc(case, kps, desc, tr):
    B = R.blur(case.image())
    for i, (rule, m01, m10, s, at, wrong, _) in enumerate(DESC_SITES):
        x, y = _desc_xy(i)
        j = find(kps, x, y)
        assert len(j) == 1, (case.name, i)
        t = tr["kp"][j[0]]
        assert (t["m01"], t["m10"]) == (m01, m10), (case.name, i, t["m01"], t["m10"])
        bx, by, _, _ = R.sample_coords(t["angle"])
        mx, my, _, _ = R.sample_coords(t["angle"], rule)
        assert (bx[s], by[s]) == at and (mx[s], my[s]) == wrong, (case.name, i)
        assert (bx[s ^ 1], by[s ^ 1]) == (mx[s ^ 1], my[s ^ 1])
        v, vw, vp = (int(B[y + at[1], x + at[0]]), int(B[y + wrong[1], x + wrong[0]]),
                     int(B[y + by[s ^ 1], x + bx[s ^ 1]]))
        bit = (v < vp, vw < vp) if s % 2 == 0 else (vp < v, vp < vw)
        assert bit[0] != bit[1], (case.name, i, v, vw, vp)
        assert int(desc[j[0]][s // 16] >> (s // 2 % 8)) & 1 == int(bit[0])
    x, y = _desc_xy(len(DESC_SITES))
    j = find(kps, x, y)
    assert len(j) == 1 and float(kps[j[0]]["angle"]) == 0.0
    assert tuple(R.PATTERN[TIE_SAMPLE]) == TIE_AT
    img = case.image().astype(np.int64)
    k = R.gauss_kernel()
    px, py = x + TIE_AT[0], y + TIE_AT[1]
    V = int(k @ img[py - 3:py + 4, px - 3:px + 4] @ k)
    assert V == 100 * 65536 + 32768, V
    q = R.PATTERN[TIE_SAMPLE + 1]
    assert B[py, px] == 100 and R.blur(case.image(), "blur_round")[py, px] == 101
    assert B[y + q[1], x + q[0]] == 101


# The pattern's farthest points are (-13, -13) (samples 14 and 184) and their like, 18.4 pixels
# out: at 315 degrees sample 14 lies at (-18, 0), at 135 degrees at (18, 0). A keypoint on column
# 19 then reads blurred column 1, which GaussianBlur computes from the mirrored columns -2 and -1
# (REFLECT_101: columns 2 and 1; REFLECT: 1 and 0); one on column 262 = w - 20 reads column 280 =
# w - w % 4, the first of the scalar tail that rounds half up.
#   left   column 0 is darker by 1 beside the keypoint (19, 60): 257 * 257 * 100 - 49 * 257 gives
#          101 at column 1, - (49 + 34) * 257 with REFLECT gives 100; the partner reads the flat 101
#   right  the differences BORDER_TIE at columns 278..281 (outside the moment patch of (262, 100))
#          make the sum at (280, 100) 100 * 65536 + 32768: 101 half up, 100 half to even
BORDER_LEFT, BORDER_RIGHT, FAR_SAMPLE = (19, 60), (262, 100), 14
BORDER_TIE = ((-3, 278, -2), (-3, 280, -1), (-3, 281, -1), (-2, 278, -3), (-2, 279, -1),
              (-2, 280, -3))  # (row - 100, column, difference)


def _border_dots():
    (xl, yl), (xr, yr) = BORDER_LEFT, BORDER_RIGHT
    out = [(xl, yl, 9), (xl + 5, yl - 5, 5), (xr, yr, 9), (xr - 5, yr + 5, 5)]
    out += [(0, y, -1) for y in range(yl - 10, yl + 11)]
    out += [(c, yr + r, d) for r, c, d in BORDER_TIE]
    return out


def _check_border(case, kps, desc, tr):
    img = case.image()
    B = R.blur(img)
    w = img.shape[1]
    assert tuple(R.PATTERN[FAR_SAMPLE]) == (-13, -13) and w % 4 == 2
    for (x, y), m, dx, wrong_rule in ((BORDER_LEFT, (-25, 25), -18, "blur_reflect101"),
                                      (BORDER_RIGHT, (25, -25), 18, "blur_tail")):
        j = find(kps, x, y)
        assert len(j) == 1, (case.name, x, y)
        t = tr["kp"][j[0]]
        assert (t["m01"], t["m10"]) == m and t["reach"] == 18
        bx, by, _, _ = R.sample_coords(t["angle"])
        assert (bx[FAR_SAMPLE], by[FAR_SAMPLE]) == (dx, 0)
        px = x + dx
        assert px == (1 if dx < 0 else w - w % 4)
        partner = int(B[y + by[FAR_SAMPLE + 1], x + bx[FAR_SAMPLE + 1]])
        assert (int(B[y, px]), int(R.blur(img, wrong_rule)[y, px]), partner) == (101, 100, 101)
        assert int(desc[j[0]][0] >> 7) & 1 == 0  # bit 7 of byte 0: 101 < 101; 100 < 101 sets it
    k = R.gauss_kernel()
    P = np.pad(img.astype(np.int64), 3, mode="reflect")
    x, y = BORDER_RIGHT
    V = int(k @ P[y:y + 7, x + 18:x + 25] @ k)
    assert V == 100 * 65536 + 32768, V


def _check_saturated(case, kps, desc, tr):
    assert len(kps) >= 6 and (kps["octave"] == 0).sum() == 6
    img = case.image()
    k = R.gauss_kernel()
    assert int(k.sum()) == 257 and int(img[100:107, 200].astype(np.int64) @ k) == 65535
    assert R.blur(img)[103, 200] == 255


# ---- the levels case ------------------------------------------------------------------------
# Three neighbourhoods of level-0 keypoints of synthetic.stereo_pair(77, 640, 240)[0], magnified
# by 1.2, 1.44 and 1.728 (stereo_boundary_scenario._zoom_patch: tapered into the background).
LEVELS_SPEC = [((242, 160), 1.2), ((143, 157), 1.44), ((203, 133), 1.728)]


def _paint_levels(img):
    from slam_framework_amd import synthetic
    from stereo_boundary_scenario import _zoom_patch, BG as SBG
    src = synthetic.stereo_pair(77, 640, 240)[0]
    for i, ((x, y), z) in enumerate(LEVELS_SPEC):
        p = _zoom_patch(src, x, y, z)
        r = p.shape[0] // 2
        cx, cy = 47 + 94 * i, 66
        img[cy - r:cy + r + 1, cx - r:cx + r + 1] += p
    assert SBG == 128
    np.clip(img, 0, 255, out=img)


def _check_levels(case, kps, desc, tr):
    assert set(kps["octave"].tolist()) == {0, 1, 2, 3}, np.bincount(kps["octave"])
    up = kps[kps["octave"] > 0]
    assert (up["x"] != np.floor(up["x"])).any(), "fractional coordinates above level 0"
    octants = {int(a // 45) for a in kps["angle"]}
    assert len(octants) == 8, octants
    # every level's budget binds; the last level's is 131 - (42 + 35 + 29) = 25, where cvRound
    # of the running nDesired would give 24
    assert tr["tables"].budget == [42, 35, 29, 25]
    assert all(lv["octree"]["exit"] in ("full", "inner_full") for lv in tr["levels"])


def _fail(case):
    raise AssertionError(case.name)


COUNT_KEYS = [okey(5, 5, 8), okey(30, 40, 9),                      # n1 [0, 42) x [0, 50)
              okey(46, 5), okey(55, 15, 8), okey(70, 40),          # n2 [42, 83) x [0, 50)
              okey(5, 55), okey(30, 90),                           # n3 [0, 42) x [50, 100)
              okey(46, 55, 8), okey(55, 65), okey(70, 90),         # n4 [42, 83) x [50, 100)
              okey(120, 30), okey(200, 60)]                        # initial nodes 1 and 2

CASES ={c.name: c for c in _cases()}
