"""Frame::ComputeStereoMatches (frame.cpp:406-577) restated in plain Python, in the reference's own
order, sharing no code with oracle/ or csrc/. Every float step is an explicit numpy.float32
operation, as the C++ has it (float operands, float results, no contraction is possible: no
product feeds a sum except through a rounded float).

maxD follows DESIGN.md's note on :436: the reference reads baseline_ before it is assigned, so
the value is baseline = bf / fx and maxD = bf / baseline, all float (and not fx: the two differ
for some cameras). An empty match list skips the median filter (:566 indexes an empty vector).

stereo_matches(...) returns (u_right, depth, trace); trace[iL] is a dict with
  stage       how far the keypoint got, one of STAGES
  candidates  right indices left by the row band, the level window and the disparity window, in
              the row table's order
  bestDist, bestIdxR              the Hamming stage's result
  sads                            the 11 SADs as floats (offset -5 first)
  bestincR, deltaR, disparity     the sub-pixel stage (disparity before the <= 0 replacement)
  sad                             the SAD the match enters the median filter with
and trace["median"] = dict(sorted=[(sad, iL), ...], n, median, thDist).

rule=NAME replaces exactly one comparison by its nearest wrong variant; RULES lists them with the
line of frame.cpp each belongs to."""
import numpy as np

F = np.float32

STAGES = ("no_candidates", "maxU_negative", "hamming_rejected", "window_outside", "sad_at_end",
          "deltaR_rejected", "disparity_rejected", "median_rejected", "matched")

RULES = {
    # name: (line of frame.cpp, the rule, the wrong variant)
    "band_radius": (426, "r = 2.0f * scale", "r = 1.0f * scale"),
    "band_octave": (426, "scale of the RIGHT keypoint's octave", "of the left keypoint's octave"),
    "band_inclusive": (430, "yi <= maxr", "yi < maxr"),
    "band_rounding": (427, "ceil(kpY + r), floor(kpY - r)", "floor(kpY + r), ceil(kpY - r)"),
    "row_index": (450, "vRowIndices[(int)vL]", "vRowIndices[round(vL)]"),
    "max_d": (438, "maxD = bf / (bf / fx) in float", "maxD = fx"),
    "level_window_0": (473, "octave within levelL +- 1", "octave == levelL"),
    "level_window_2": (473, "octave within levelL +- 1", "octave within levelL +- 2"),
    "min_u": (479, "uR >= minU", "uR > minU"),
    "max_u": (479, "uR <= maxU", "uR < maxU"),
    "hamming_tie": (483, "dist < bestDist (first of equals)", "dist <= bestDist (last)"),
    "hamming_threshold": (491, "bestDist < 75", "bestDist <= 75"),
    "scaled_round": (495, "round(x * inv_scale)", "trunc(x * inv_scale)"),
    "ur0_scale": (497, "uR0 * inv_scale[LEFT octave]", "uR0 * inv_scale[right octave]"),
    "sad_first_min": (525, "dist < bestDist (first minimum)", "dist <= bestDist (last)"),
    "reject_minus_l": (533, "bestincR == -L rejects", "it does not (dist1 read as dist2)"),
    "reject_plus_l": (533, "bestincR == +L rejects", "it does not (dist3 read as dist2)"),
    "disparity_min": (553, "disparity >= minD", "disparity > minD"),
    "disparity_max": (553, "disparity < maxD", "disparity <= maxD"),
    "disparity_zero": (554, "disparity <= 0 becomes 0.01", "disparity < 0"),
    "median_rank": (566, "element n / 2 of the sorted SADs", "element (n - 1) / 2"),
    "median_keep": (570, "first < thDist keeps", "first <= thDist keeps"),
}

TH_HIGH, TH_LOW = 100, 50


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _round(x):
    """std::round of a float: half away from zero."""
    x = F(x)
    return F(np.floor(x + F(0.5))) if x >= 0 else F(-np.floor(-x + F(0.5)))


def stereo_matches(kl, dl, kr, dr, pyr_l, pyr_r, scale, inv_scale, fx, bf, rule=None):
    """kl / kr: keypoint records with x, y, octave; dl / dr: [N, 32] u8; pyr_l / pyr_r: the
    levels as 2-D u8 arrays; scale / inv_scale: the extractor's float tables; fx, bf: floats."""
    assert rule is None or rule in RULES, rule
    is_ = lambda name: rule == name  # noqa: E731
    N, Nr = len(kl), len(kr)
    scale = [F(s) for s in scale]
    inv_scale = [F(s) for s in inv_scale]
    fx, bf = F(fx), F(bf)
    u_right = np.full(N, -1.0, F)
    depth = np.full(N, -1.0, F)
    trace = {iL: dict(stage="no_candidates", candidates=[]) for iL in range(N)}
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyr_l[0].shape[0]

    # :415-433 the row table. With band_octave the radius depends on the left keypoint too, so
    # the table is kept per left octave.
    def row_table(left_octave):
        rows = [[] for _ in range(nRows)]
        for iR in range(Nr):
            kpY = F(kr[iR]["y"])
            s = scale[left_octave] if is_("band_octave") else scale[int(kr[iR]["octave"])]
            r = F((F(1.0) if is_("band_radius") else F(2.0)) * s)
            if is_("band_rounding"):
                maxr, minr = int(np.floor(F(kpY + r))), int(np.ceil(F(kpY - r)))
            else:
                maxr, minr = int(np.ceil(F(kpY + r))), int(np.floor(F(kpY - r)))
            last = maxr - 1 if is_("band_inclusive") else maxr
            # the reference indexes vRowIndices without a test: keypoints lie at least 19 level
            # pixels inside, the band reaches 2 * scale beyond them
            assert 0 <= minr and last < nRows, (iR, minr, last)
            for yi in range(minr, last + 1):
                rows[yi].append(iR)
        return rows

    tables = {}
    # :436-438
    minZ = F(bf / fx)
    minD = F(0)
    maxD = fx if is_("max_d") else F(bf / minZ)
    vDistIdx = []
    for iL in range(N):
        tr = trace[iL]
        levelL = int(kl[iL]["octave"])
        vL, uL = F(kl[iL]["y"]), F(kl[iL]["x"])
        key = levelL if is_("band_octave") else 0
        if key not in tables:
            tables[key] = row_table(key)
        row = int(_round(vL)) if is_("row_index") else int(vL)
        vCandidates = tables[key][row]
        tr["row"] = row
        if not vCandidates:
            continue
        minU, maxU = F(uL - maxD), F(uL - minD)
        tr["minU"], tr["maxU"] = minU, maxU
        if maxU < 0:
            tr["stage"] = "maxU_negative"
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        reach = 0 if is_("level_window_0") else 2 if is_("level_window_2") else 1
        for iR in vCandidates:
            octR = int(kr[iR]["octave"])
            if octR < levelL - reach or octR > levelL + reach:
                continue
            uR = F(kr[iR]["x"])
            lo = uR > minU if is_("min_u") else uR >= minU
            hi = uR < maxU if is_("max_u") else uR <= maxU
            if lo and hi:
                tr["candidates"].append(iR)
                dist = _hamming(dl[iL], dr[iR])
                if (dist <= bestDist) if is_("hamming_tie") else (dist < bestDist):
                    bestDist, bestIdxR = dist, iR
        tr["bestDist"], tr["bestIdxR"] = bestDist, bestIdxR
        tr["stage"] = "hamming_rejected"
        if not ((bestDist <= thOrbDist) if is_("hamming_threshold") else (bestDist < thOrbDist)):
            continue
        # :493-497
        uR0 = F(kr[bestIdxR]["x"])
        scaleFactor = inv_scale[levelL]
        rnd = (lambda v: F(np.trunc(v))) if is_("scaled_round") else _round
        scaleduL = rnd(F(uL * scaleFactor))
        scaledvL = rnd(F(vL * scaleFactor))
        sR = inv_scale[int(kr[bestIdxR]["octave"])] if is_("ur0_scale") else scaleFactor
        scaleduR0 = rnd(F(uR0 * sR))
        tr["scaled"] = (scaleduL, scaledvL, scaleduR0)
        w = L = 5
        IL_img, IR_img = pyr_l[levelL], pyr_r[levelL]
        yc, xl, xr = int(scaledvL), int(scaleduL), int(scaleduR0)
        iniu = F(scaleduR0 + F(L) - F(w))
        endu = F(F(scaleduR0 + F(L)) + F(w) + F(1))
        tr["stage"] = "window_outside"
        tr["iniu"], tr["endu"], tr["cols"] = iniu, endu, IR_img.shape[1]
        if iniu < 0 or endu >= IR_img.shape[1]:
            continue
        # the ROIs the reference takes without a test of its own (cv::Mat would assert)
        tr["roi_ok"] = (yc - w >= 0 and yc + w < IL_img.shape[0] and xl - w >= 0 and
                        xl + w < IL_img.shape[1] and xr - L - w >= 0)
        assert tr["roi_ok"], (iL, yc, xl, xr)
        IL = IL_img[yc - w:yc + w + 1, xl - w:xl + w + 1].astype(F)
        IL = IL - IL[w, w]
        bestSad, bestincR = 2**31 - 1, 0
        vDists = [F(0)] * (2 * L + 1)
        for incR in range(-L, L + 1):
            c = xr + incR
            IR = IR_img[yc - w:yc + w + 1, c - w:c + w + 1].astype(F)
            IR = IR - IR[w, w]
            dist = F(np.abs(IL.astype(np.float64) - IR.astype(np.float64)).sum())  # cv::norm L1
            better = dist <= F(bestSad) if is_("sad_first_min") else dist < F(bestSad)
            if better:
                bestSad, bestincR = int(dist), incR
            vDists[L + incR] = dist
        tr["sads"], tr["bestincR"], tr["sad"] = vDists, bestincR, bestSad
        tr["stage"] = "sad_at_end"
        if bestincR == -L and not is_("reject_minus_l"):
            continue
        if bestincR == L and not is_("reject_plus_l"):
            continue
        dist2 = vDists[L + bestincR]
        dist1 = vDists[L + bestincR - 1] if bestincR > -L else dist2
        dist3 = vDists[L + bestincR + 1] if bestincR < L else dist2
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
        tr["deltaR"] = deltaR
        tr["stage"] = "deltaR_rejected"
        if deltaR < -1 or deltaR > 1:
            continue
        bestuR = F(scale[levelL] * F(F(scaleduR0 + F(bestincR)) + deltaR))
        disparity = F(uL - bestuR)
        tr["disparity"], tr["maxD"] = disparity, maxD
        tr["stage"] = "disparity_rejected"
        lo = disparity > minD if is_("disparity_min") else disparity >= minD
        hi = disparity <= maxD if is_("disparity_max") else disparity < maxD
        if lo and hi:
            if (disparity < 0) if is_("disparity_zero") else (disparity <= 0):
                disparity = F(0.01)
                bestuR = F(uL - F(0.01))
            with np.errstate(divide="ignore"):
                depth[iL] = F(bf / disparity)
            u_right[iL] = bestuR
            vDistIdx.append((bestSad, iL))
            tr["stage"] = "matched"
    # :565-576
    vDistIdx.sort()
    med = dict(sorted=vDistIdx, n=len(vDistIdx), median=None, thDist=None)
    if vDistIdx:
        rank = (len(vDistIdx) - 1) // 2 if is_("median_rank") else len(vDistIdx) // 2
        median = F(vDistIdx[rank][0])
        thDist = F(F(F(1.5) * F(1.4)) * median)
        med["median"], med["thDist"] = median, thDist
        for sad, iL in reversed(vDistIdx):
            if (F(sad) <= thDist) if is_("median_keep") else (F(sad) < thDist):
                break
            u_right[iL] = F(-1.0)
            depth[iL] = F(-1.0)
            trace[iL]["stage"] = "median_rejected"
    trace["median"] = med
    return u_right, depth, trace
