"""Plain numpy / Python model of the matchers that walk the DBoW2 FeatureVector, with the outcome of every feature named.  TEST INFRASTRUCTURE ONLY.

Restated from the reference text: ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:273-475, F.Nleft == -1 and the rig branch
of :346-373 / :407-436), SearchByBoW(KeyFrame*, KeyFrame*, ...) (:827-967), SearchForTriangulation (:969-1210, single cameras) with
Pinhole::epipolarConstrain (Pinhole.cpp:122-144) and ComputeThreeMaxima (:2307-2348).  The two std::map walks with lower_bound are the
intersection of the two node sets in ascending order; float32 exactly where the reference computes in float.

Besides the result the model names, per keyframe feature (BoW) or KF1 keypoint (triangulation), an outcome and flags, and for
triangulation the gate bits of its candidates.  It also states which form of the device kernel a node is given to -- a pure function of the
node's size on the frame side and of Nleft, restated from the kernel's documented switch points, not from its code: `lane` below
BOW_BIG_NODE frame features or on a rig frame, `wave` from there on, `wave+tail` beyond the REG_POSITIONS positions a wave keeps in
registers; position p of a wave node belongs to lane p % WAVE.  arith=F64 evaluates the triangulation geometry in double instead, to name the
rows that sit on a rounding boundary."""
import bisect
import math
import numpy as np

f32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30
BOW_BIG_NODE, WAVE, REG_POSITIONS = 32, 64, 512

BOW_OUTCOMES = ("no_mappoint", "absent_before", "absent_between", "absent_end", "no_candidate", "above_th_low", "ratio_failed", "accept")
BOW_FLAGS = ("no_second", "tie", "second_same_lane", "second_other_lane", "skipped_claimed", "rot_removed", "rig_left", "rig_right", "rig_both",
             "rig_right_blocked")
BF = {n: 1 << i for i, n in enumerate(BOW_FLAGS)}
PATHS = ("lane", "wave", "wave+tail")

TRI_OUTCOMES = ("has_mappoint", "not_stereo", "node_absent", "all_gated", "accept")
TRI_GATES = ("mp2", "only_stereo2", "dist_gt_th", "dist_gt_best", "epipole", "epipolar", "den0")
TG = {n: 1 << i for i, n in enumerate(TRI_GATES)}
TRI_FLAGS = ("tie_replaced", "tie_kept", "coarse", "ep_skip_st1", "ep_skip_st2", "rot_removed")
TF = {n: 1 << i for i, n in enumerate(TRI_FLAGS)}

F32, F64 = np.float32, np.float64


def roundf(v):
    """C round(): half away from zero"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def rot_bin(a1, a2):
    """ORBmatcher.cc:395-400: float rot = kp.angle - Fkp.angle; if (rot < 0.0) rot += 360.0f; bin = round(rot * factor)"""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = roundf(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (:2307-2348); returns the kept bins"""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if f32(m2) < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif f32(m3) < f32(0.1) * f32(m1):
        i3 = -1
    return {i1, i2, i3}


def feat_vec(nids):
    """DBoW2::FeatureVector: node -> feature indices in ascending order"""
    fv = {}
    for i, n in enumerate(nids):
        fv.setdefault(int(n), []).append(i)
    return fv


def node_path(size, nleft):
    if nleft >= 0 or size < BOW_BIG_NODE:
        return "lane"
    return "wave+tail" if size > REG_POSITIONS else "wave"


def _dist_matrix(da, db):
    return np.unpackbits(da[:, None, :] ^ db[None, :, :], axis=2).sum(2).astype(np.int64)


def search_by_bow(c, ratio, check_ori, form="frame", nleft=-1):
    """form: "frame" (Nleft == -1), "rig" (nleft >= 0), "kf" (second keyframe with c["valid2"]).  Returns a dict: nm, m (the oracle's output
    array: per frame feature the keyframe feature, or per KF1 feature the KF2 feature), outcome / flags / match / match_r [nK] (before the
    rotation check; match_r: the right camera's frame feature), paths {node: path} and tails {node: bool} for the shared nodes."""
    kf = form == "kf"
    if form != "rig":
        nleft = -1
    nK, nF = len(c["kp_k"]), len(c["kp_f"])
    fk, ff = feat_vec(c["nid_k"]), feat_vec(c["nid_f"])
    fids = sorted(ff)
    outcome = np.full(nK, -1, np.int64); flags = np.zeros(nK, np.int64)
    match = np.full(nK, -1, np.int64); match_r = np.full(nK, -1, np.int64)
    claimed = np.full(nF, -1, np.int64)
    nm = 0
    hist = [[] for _ in range(HISTO_LENGTH)]
    paths, tails = {}, {}
    rt = f32(ratio)
    O = {n: i for i, n in enumerate(BOW_OUTCOMES)}
    for node in sorted(fk):
        if node not in ff:
            lb = bisect.bisect_left(fids, node)
            oc = "absent_end" if lb == len(fids) else ("absent_before" if lb == 0 else "absent_between")
            outcome[fk[node]] = O[oc]
            continue
        cand = ff[node]
        paths[node] = node_path(len(cand), nleft); tails[node] = paths[node] == "wave+tail"
        wave = paths[node] != "lane"
        D = _dist_matrix(c["d_k"][fk[node]], c["d_f"][cand])
        for a, ri in enumerate(fk[node]):
            if not c["valid"][ri]:                                       # :305-311 / :866-870
                outcome[ri] = O["no_mappoint"]
                continue
            b1 = [256, 256]; b2 = [256, 256]; bi = [-1, -1]
            free = [[], []]
            skipped = False
            for p, rj in enumerate(cand):
                if claimed[rj] >= 0:                                     # :328 / :888
                    skipped = True
                    continue
                if kf and not c["valid2"][rj]:                           # :888-892
                    continue
                dist = int(D[a, p])
                s = 0 if (nleft < 0 or rj < nleft) else 1
                free[s].append((dist, p))
                if dist < b1[s]:
                    b2[s], b1[s], bi[s] = b1[s], dist, rj
                elif dist < b2[s]:
                    b2[s] = dist
            fl = BF["skipped_claimed"] if skipped else 0
            if not free[0] and not free[1]:
                outcome[ri] = O["no_candidate"]; flags[ri] = fl
                continue
            if b2[0] == b1[0] and b1[0] < 256:
                fl |= BF["tie"]
            if wave and len(free[0]) > 1:
                k = sorted(free[0])
                fl |= BF["second_same_lane"] if k[0][1] % WAVE == k[1][1] % WAVE else BF["second_other_lane"]
            if not (b1[0] < TH_LOW if kf else b1[0] <= TH_LOW):          # :377 / :910
                outcome[ri] = O["above_th_low"]
                if nleft >= 0 and b1[1] <= TH_LOW:
                    fl |= BF["rig_right_blocked"]
                flags[ri] = fl
                continue
            picks = []
            left = bool(f32(b1[0]) < rt * f32(b2[0]))                    # :379 / :912
            if left:
                picks.append(bi[0]); match[ri] = bi[0]
                if b2[0] == 256:
                    fl |= BF["no_second"]
            right = nleft >= 0 and b1[1] <= TH_LOW                       # :407-409 ("|| true")
            if right:
                picks.append(bi[1]); match_r[ri] = bi[1]
            if nleft >= 0 and picks:
                fl |= BF["rig_both"] if left and right else (BF["rig_left"] if left else BF["rig_right"])
            outcome[ri] = O["accept" if picks else "ratio_failed"]
            flags[ri] = fl
            for j in picks:
                claimed[j] = ri; nm += 1
                if check_ori:
                    hist[rot_bin(c["kp_k"]["angle"][ri], c["kp_f"]["angle"][j])].append(j)
    if check_ori:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i not in keep:
                for j in hist[i]:
                    flags[claimed[j]] |= BF["rot_removed"]
                    claimed[j] = -1; nm -= 1
    if kf:
        m = np.full(nK, -1, np.int64)
        for j in np.flatnonzero(claimed >= 0):
            m[claimed[j]] = j
    else:
        m = claimed.copy()
    return dict(nm=nm, m=m, outcome=outcome, flags=flags, match=match, match_r=match_r, paths=paths, tails=tails)


# ------------------------------------------------------------------ SearchForTriangulation
def epiline(t, x1, y1, F):
    """Pinhole.cpp:130-132 in type t"""
    x1, y1 = t(x1), t(y1)
    F = [t(v) for v in F]
    return tuple(t(t(t(x1 * F[k]) + t(y1 * F[3 + k])) + F[6 + k]) for k in range(3))


def epipolar_dsqr(t, line, x2, y2):
    """Pinhole.cpp:134-141; returns (den, dsqr or None)"""
    a, b, c = line
    num = t(t(t(a * t(x2)) + t(b * t(y2))) + c)
    den = t(t(a * a) + t(b * b))
    if den == 0:
        return den, None
    return den, t(t(num * num) / den)


def epipole_inside(t, ep, x2, y2, scale):
    """ORBmatcher.cc:1095-1097"""
    ex, ey = t(t(ep[0]) - t(x2)), t(t(ep[1]) - t(y2))
    return bool(t(t(ex * ex) + t(ey * ey)) < t(t(100) * t(scale)))


def search_for_triangulation(c, check_ori, mono=False, arith=F32):
    """Returns a dict: nm, m [n1], outcome / gates / flags / match [n1] (match before the rotation check)."""
    t = arith
    n1 = len(c["kp1"])
    f1, f2 = feat_vec(c["nid1"]), feat_vec(c["nid2"])
    outcome = np.full(n1, -1, np.int64); gates = np.zeros(n1, np.int64); flags = np.zeros(n1, np.int64)
    match = np.full(n1, -1, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    O = {n: i for i, n in enumerate(TRI_OUTCOMES)}
    nm = 0
    for node in sorted(f1):
        if node not in f2:
            outcome[f1[node]] = O["node_absent"]
            continue
        D = _dist_matrix(c["d1"][f1[node]], c["d2"][f2[node]])
        for a, i1 in enumerate(f1[node]):
            if c["mp1"][i1]:                                             # :1040
                outcome[i1] = O["has_mappoint"]
                continue
            st1 = (not mono) and c["ur1"][i1] >= 0                       # :1045
            if c["only_stereo"] and not st1:
                outcome[i1] = O["not_stereo"]
                continue
            k1 = c["kp1"][i1]
            line = epiline(t, k1["x"], k1["y"], c["F12"])
            best, bi = TH_LOW, -1
            g = fl = 0
            for p, i2 in enumerate(f2[node]):
                if c["mp2"][i2]:                                         # :1071
                    g |= TG["mp2"]
                    continue
                st2 = (not mono) and c["ur2"][i2] >= 0
                if c["only_stereo"] and not st2:                         # :1076
                    g |= TG["only_stereo2"]
                    continue
                dist = int(D[a, p])
                if dist > TH_LOW:                                        # :1084
                    g |= TG["dist_gt_th"]
                    continue
                if dist > best:
                    g |= TG["dist_gt_best"]
                    continue
                k2 = c["kp2"][i2]
                equal = bi >= 0 and dist == best
                inside = epipole_inside(t, c["ep"], k2["x"], k2["y"], c["scale"][k2["octave"]])
                if not st1 and not st2:                                  # :1093-1101
                    if inside:
                        g |= TG["epipole"]
                        if equal:
                            fl |= TF["tie_kept"]
                        continue
                elif inside:
                    fl |= TF["ep_skip_st1"] if st1 else TF["ep_skip_st2"]
                den, dsqr = epipolar_dsqr(t, line, k2["x"], k2["y"])
                if dsqr is None:
                    ok = False; why = "den0"
                else:
                    ok = bool(float(dsqr) < 3.84 * float(c["sigma2"][k2["octave"]])); why = "epipolar"
                if not ok and not c["coarse"]:                           # :1136
                    g |= TG[why]
                    if equal:
                        fl |= TF["tie_kept"]
                    continue
                if equal:
                    fl |= TF["tie_replaced"]
                fl = (fl & ~TF["coarse"]) | (0 if ok else TF["coarse"])
                bi, best = i2, dist
            gates[i1] = g; flags[i1] = fl
            if bi < 0:
                outcome[i1] = O["all_gated"]
                continue
            outcome[i1] = O["accept"]; match[i1] = bi; nm += 1
            if check_ori:
                hist[rot_bin(k1["angle"], c["kp2"]["angle"][bi])].append(i1)
    m = match.copy()
    if check_ori:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i not in keep:
                for i1 in hist[i]:
                    m[i1] = -1; nm -= 1; flags[i1] |= TF["rot_removed"]
    return dict(nm=nm, m=m, outcome=outcome, gates=gates, flags=flags, match=match)
