"""Frame::ComputeStereoMatches (reference src/Frame.cc:802-977) restated in plain Python / numpy, independently of the C oracle and of
the HIP kernels, with the OUTCOME of every left keypoint and the FLAGS of the decisions it went through.

The restatement: row table (floor / ceil of y -+ 2 scale[octave], rows outside the image dropped), candidates in list order with the
octave and disparity gates, strict-< best Hamming distance from TH_HIGH = 100, the (TH_HIGH + TH_LOW) / 2 = 75 cut, 11 x 11
centred-patch SAD over 11 shifts on the left keypoint's pyramid level (the level images as the reference's reflect-101 padded
mvImagePyramid views), first minimum, parabola refinement in float, disparity gates with the 0.01 clamp, the 1.5 x 1.4 x median cut on
the sorted (SAD, index) pairs.

Two branches of the reference no input can reach; nobody writes tests for them:
  * deltaR outside [-1, 1] (:945-946).  The shift of the FIRST minimum is interior here (-5 and +5 have left at :938-939), so with
    d1, d2, d3 the SADs left of, at and right of it: a = d1 - d2 > 0 (strictly: an equal SAD on the left would have been the first
    minimum) and b = d3 - d2 >= 0.  deltaR = (d1 - d3) / (2 (d1 + d3 - 2 d2)) = (a - b) / (2 (a + b)), and |a - b| <= a + b, so
    deltaR lies in [-1/2, 1/2].  The SADs are integers below 2^16, so every float operation on them is exact up to the division.
  * a NaN deltaR.  The denominator 2 (a + b) is positive by the same argument (a > 0), and the numerator is finite.
OUTCOMES keeps a code for them ("delta_outside") so that the model can say so if it ever happens; the tests assert it never does.

`wrong` switches ONE decision to a plausible mistake (WRONG_RULES); the crafted lists of stereo_cases.py are proven to tell every one
of them from the oracle (test_stereo_cases.py), which is what makes them able to catch that mistake on the device."""
import numpy as np

f32 = np.float32
OUTCOMES = ("row_outside",        # (int)vL is no row of the image (the reference indexes vRowIndices out of range there)
            "empty_row",          # vRowIndices[vL] is empty (:853-854)
            "maxu_negative",      # maxU < 0 (:859-860)
            "no_candidate",       # no admitted candidate under thOrbDist = 75 (:890)
            "strip_left",         # iniu < 0 (:915)
            "strip_right",        # endu >= cols (:915)
            "shift_m5",           # bestincR == -L (:938)
            "shift_p5",           # bestincR == +L (:938)
            "disp_negative",      # disparity < minD = 0 (:953)
            "disp_ge_maxd",       # disparity >= maxD (:953)
            "accepted",
            "accepted_clamped",   # accepted through disparity <= 0 -> 0.01 (:954-958)
            "median_removed",     # SAD >= 1.5 * 1.4 * median (:966-980)
            "delta_outside")      # unreachable, see above
UNREACHABLE = ("delta_outside",)
FLAGS = ("reflected_read",        # the strip reached columns left of the image (scaleduR0 < 10): the reflect-101 padding was read
         "hamming_tie",           # the best distance is held by two or more admitted candidates
         "tie_across_64",         # ... and the winner and a tie partner lie on two sides of a multiple of 64 in right-index order
         "sad_tie")               # the minimal SAD is reached at two or more shifts
WRONG_RULES = ("best_le",             # <= for the best Hamming distance: the last of equals wins
               "upper_row_floor",     # floor instead of ceil for the upper row edge
               "median_low_rank",     # the median at rank (V - 1) / 2
               "median_le",           # <= at the median threshold: a SAD equal to it is kept
               "last_min_sad",        # the last minimum among equal SADs
               "reflect_minus_one")   # columns left of the image read as c = -c - 1 (BORDER_REFLECT, not BORDER_REFLECT_101)
E = 19                                # EDGE_THRESHOLD: the border of the padded views
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _rnd(v):
    """round(): half away from zero"""
    v = np.float64(v)
    return f32(np.sign(v) * np.floor(np.abs(v) + 0.5))


def stereo_model(pyrL, pyrR, sf, kpL, dL, kpR, dR, mb, mbf, wrong=None):
    """pyrL / pyrR: the padded level images (border E) of the left and right pyramid; sf: mvScaleFactor; kp*: structured keypoints
    (x, y, octave are read); d*: [n, 32] descriptors.  Returns ((kept, uRight, depth), outcome [nL] indices into OUTCOMES,
    flags [nL] bit masks over FLAGS)."""
    assert wrong is None or wrong in WRONG_RULES
    sf = np.asarray(sf, f32); isf = (f32(1.0) / sf).astype(f32)
    pyrL = [np.asarray(p).astype(np.int32) for p in pyrL]; pyrR = [np.asarray(p).astype(np.int32) for p in pyrR]
    cols = [p.shape[1] - 2 * E for p in pyrR]
    nrows = pyrL[0].shape[0] - 2 * E
    rows = [[] for _ in range(nrows)]
    for iR in range(len(kpR)):
        y = f32(kpR["y"][iR]); r = f32(f32(2.0) * sf[kpR["octave"][iR]])
        hi = np.floor(f32(y + r)) if wrong == "upper_row_floor" else np.ceil(f32(y + r))
        for yi in range(int(np.floor(f32(y - r))), int(hi) + 1):
            if 0 <= yi < nrows:
                rows[yi].append(iR)
    minD, maxD = f32(0), f32(f32(mbf) / f32(mb))
    N = len(kpL)
    ur_m = np.full(N, -1, f32); dp_m = np.full(N, -1, f32)
    outcome = np.full(N, -1, np.int32); flags = np.zeros(N, np.int32)
    O = {k: i for i, k in enumerate(OUTCOMES)}; F = {k: 1 << i for i, k in enumerate(FLAGS)}
    pairs = []
    for iL in range(N):
        lv = int(kpL["octave"][iL]); uL = f32(kpL["x"][iL]); vL = f32(kpL["y"][iL])
        row = int(vL)                                                                            # C's (int): towards zero
        if row < 0 or row >= nrows:
            outcome[iL] = O["row_outside"]; continue
        cand = rows[row]
        if not cand:
            outcome[iL] = O["empty_row"]; continue
        minU, maxU = f32(uL - maxD), f32(uL - minD)
        if maxU < 0:
            outcome[iL] = O["maxu_negative"]; continue
        best, bR, holders = 100, 0, []
        for iR in cand:
            o = int(kpR["octave"][iR])
            if o < lv - 1 or o > lv + 1:
                continue
            uR = f32(kpR["x"][iR])
            if minU <= uR <= maxU:
                dist = int(_POP[dL[iL] ^ dR[iR]].sum())
                if dist < best:
                    holders = []
                if dist <= best and dist < 100:
                    holders.append(iR)
                if dist <= best if wrong == "best_le" else dist < best:
                    best, bR = dist, iR
        if len(holders) >= 2:
            flags[iL] |= F["hamming_tie"]
            if any(h // 64 != bR // 64 for h in holders):
                flags[iL] |= F["tie_across_64"]
        if best >= 75:                                                                           # thOrbDist = (TH_HIGH + TH_LOW) / 2
            outcome[iL] = O["no_candidate"]; continue
        s = isf[lv]
        su, sv, su0 = int(_rnd(uL * s)), int(_rnd(vL * s)), int(_rnd(f32(kpR["x"][bR]) * s))
        w, L = 5, 5
        if su0 + L - w < 0:
            outcome[iL] = O["strip_left"]; continue
        if su0 + L + w + 1 >= cols[lv]:
            outcome[iL] = O["strip_right"]; continue
        if su0 < 10:
            flags[iL] |= F["reflected_read"]
        IL = pyrL[lv][E + sv - w:E + sv + w + 1, E + su - w:E + su + w + 1]
        IL = IL - IL[w, w]
        strip = pyrR[lv][E + sv - w:E + sv + w + 1, E + su0 - L - w:E + su0 + L + w + 1]
        if wrong == "reflect_minus_one":
            c = np.arange(su0 - L - w, su0 + L + w + 1)
            strip = pyrR[lv][E + sv - w:E + sv + w + 1, E + np.where(c < 0, -c - 1, c)]
        dists = []
        for inc in range(-L, L + 1):
            IR = strip[:, L + inc:L + inc + 2 * w + 1]
            dists.append(int(np.abs(IL - (IR - IR[w, w])).sum()))
        bd = min(dists)
        if dists.count(bd) >= 2:
            flags[iL] |= F["sad_tie"]
        binc = (len(dists) - 1 - dists[::-1].index(bd) if wrong == "last_min_sad" else dists.index(bd)) - L      # strict <: the first minimum
        if binc == -L:
            outcome[iL] = O["shift_m5"]; continue
        if binc == L:
            outcome[iL] = O["shift_p5"]; continue
        d1, d2, d3 = f32(dists[L + binc - 1]), f32(dists[L + binc]), f32(dists[L + binc + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if not (-1 <= delta <= 1):                                                               # unreachable under the right rules (docstring)
            outcome[iL] = O["delta_outside"]
            if delta < -1 or delta > 1:
                continue
        buR = f32(sf[lv] * f32(f32(f32(su0) + f32(binc)) + delta))
        disp = f32(uL - buR)
        if disp >= minD and disp < maxD:
            clamped = bool(disp <= 0)
            if clamped:
                disp = f32(0.01); buR = f32(np.float64(uL) - 0.01)
            dp_m[iL] = f32(f32(mbf) / disp); ur_m[iL] = buR
            pairs.append((bd, iL))
            if outcome[iL] < 0:
                outcome[iL] = O["accepted_clamped"] if clamped else O["accepted"]
        elif outcome[iL] < 0:
            outcome[iL] = O["disp_ge_maxd"] if disp >= maxD else O["disp_negative"]
    pairs.sort()
    if pairs:
        V = len(pairs)
        th = f32(f32(1.5) * f32(1.4)) * f32(pairs[(V - 1) // 2 if wrong == "median_low_rank" else V // 2][0])
        for bd, iL in reversed(pairs):
            if f32(bd) <= th if wrong == "median_le" else f32(bd) < th:
                break
            ur_m[iL] = -1; dp_m[iL] = -1; outcome[iL] = O["median_removed"]
    assert (outcome >= 0).all()
    return (int((ur_m >= 0).sum()), ur_m, dp_m), outcome, flags


def histogram(outcomes, flags):
    """counts per outcome name and per flag name over lists of the arrays stereo_model returns"""
    oc = np.concatenate([np.asarray(o).ravel() for o in outcomes] + [np.zeros(0, np.int32)])
    fl = np.concatenate([np.asarray(f).ravel() for f in flags] + [np.zeros(0, np.int32)])
    return ({k: int((oc == i).sum()) for i, k in enumerate(OUTCOMES)}, {k: int(((fl >> i) & 1).sum()) for i, k in enumerate(FLAGS)})
