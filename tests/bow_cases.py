"""Crafted pairs for the matchers that walk the DBoW2 FeatureVector: SearchByBoW (keyframe / frame, keyframe / keyframe, rig frames) and
SearchForTriangulation (single Pinhole cameras).

Every pair is assembled node by node and DECLARES, per keyframe feature (BoW) or KF1 keypoint (triangulation), the outcome, the flags, for
triangulation the gate bits, and the match.  tests/test_bow_cases.py holds bow_model.py and the C oracle to these declarations;
tests/test_gpu_bow_cases.py holds the device to the oracle.  Descriptors: the first `bits` bits are set, so every Hamming distance is
|bits - qbits|, chosen by hand.  FILL is a frame descriptor far (> 139) from every keyframe descriptor of its node: it fills a node up to the
size under test and is the second best of 200-ish where a second best is wanted that decides nothing.

Node sizes sit on the device's switch points (bow_model.node_path): 31 / 32 / 33 frame features (one lane walks the node / the wave works on
it together), 63 / 64 / 65 (a lane's second position), 511 / 512 / 513 (the last position a wave keeps in registers / the first of its tail
loop), 600 (best and second best both in the tail, or one of them); pairs of 0, 1, 63, 64, 65 and 130 shared nodes (the node loop runs in
trips of 64); KF1 counts of 127 ... 257 keypoints for the triangulation kernels' strides of 128 and 256.

A BoW case is a dict: name, form ("frame" | "kf" | "rig"), ratio, the make_bow_case fields (kp_k, d_k, nid_k, valid, kp_f, d_f, nid_f) plus
valid2 (kf) and nleft (rig), labels [nK], expect [nK] of (outcome, flags, match, match_r), sizes {node: frame features under it}.
A triangulation case: name, stereo (its uRight arrays matter), the make_tri_case fields, labels [n1], expect [n1] of (outcome, gates, flags,
match).  The flag rot_removed is declared for check_orientation on; with it off the feature keeps its match."""
import functools
from fractions import Fraction
import numpy as np

import bow_model as bm
import oracle_match_bind as om
from oracle_bind import KP_DTYPE
from case_floats import first_f32, below, round_f32, ordinal, from_ordinal, desc

f32 = np.float32
FILL = 200

# rows float64 arithmetic decides differently from float32 (they sit on a rounding boundary by construction): "case:label"
F64_EXCEPTIONS = frozenset([
    "tri-chi-boundary:fma_chi_den", "tri-chi-boundary:fma_chi_la", "tri-chi-boundary:fma_chi_lc", "tri-chi-boundary:fma_chi_num",
    "tri-epipole-boundary:fma_ep0", "tri-epipole-boundary:fma_ep1", "tri-epipole-boundary:fma_ep2", "tri-epipole-boundary:fma_ep3",
])
# rows whose decision one fused multiply-add would flip: four epipole rows (two per square of ex*ex + ey*ey), and one epipolar-distance row per
# sum of Pinhole.cpp:130-141 (EPI_SUMS)
N_FMA_ROWS = 4

TOTALS = {
    'cases:bow': 78, 'cases:tri': 16, 'features:bow': 1899, 'features:frame-side:bow': 13155, 'features:kf2:tri': 66, 'features:tri': 1204,
    'flag:coarse': 7, 'flag:ep_skip_st1': 2, 'flag:ep_skip_st2': 1, 'flag:no_second': 725, 'flag:rig_both': 23, 'flag:rig_left': 132,
    'flag:rig_right': 1, 'flag:rig_right_blocked': 2, 'flag:rot_removed': 6, 'flag:second_other_lane': 713, 'flag:second_same_lane': 12,
    'flag:skipped_claimed': 739, 'flag:tie': 293, 'flag:tie_kept': 1, 'flag:tie_replaced': 2, 'gate:den0': 1, 'gate:dist_gt_best': 1,
    'gate:dist_gt_th': 1, 'gate:epipolar': 7, 'gate:epipole': 4, 'gate:mp2': 1, 'gate:only_stereo2': 1, 'outcome:above_th_low': 19,
    'outcome:absent_before': 2, 'outcome:absent_between': 2, 'outcome:absent_end': 11, 'outcome:accept': 1571, 'outcome:no_candidate': 6,
    'outcome:no_mappoint': 94, 'outcome:ratio_failed': 194, 'path:lane': 774, 'path:wave': 107, 'path:wave+tail': 8,
    'tri:outcome:accept': 44, 'tri:outcome:all_gated': 14, 'tri:outcome:has_mappoint': 1141, 'tri:outcome:node_absent': 4,
    'tri:outcome:not_stereo': 1,
}

# every case by name: none can leave the suite unnoticed
CASE_NAMES = (
    "frame-0.7-sizes", "frame-0.7-size511", "frame-0.7-size512", "frame-0.7-size513", "frame-0.7-tail-both", "frame-0.7-tail-reg-best",
    "frame-0.7-tail-tail-best", "frame-0.7-positions", "frame-0.7-kf-side", "frame-0.7-chain-distinct-40-40",
    "frame-0.7-chain-distinct-65-64", "frame-0.7-chain-distinct-65-65", "frame-0.7-chain-distinct-31-31",
    "frame-0.7-chain-distinct-40-12-rot", "frame-0.7-chain-distinct-31-12-rot", "frame-0.7-alone-in-wave-node", "frame-0.7-shared-0",
    "frame-0.7-shared-1", "frame-0.7-shared-63", "frame-0.7-shared-64", "frame-0.7-shared-65", "frame-0.7-shared-130",
    "frame-0.7-empty-keyframe", "frame-0.7-empty-frame", "frame-0.7-thresholds-lane", "frame-0.7-thresholds-wave",
    "frame-0.75-thresholds-lane", "frame-0.75-thresholds-wave", "frame-0.7-ties", "frame-0.7-chain-identical-40",
    "frame-0.7-chain-identical-31", "frame-1.25-ties", "frame-1.25-chain-identical-40", "frame-1.25-chain-identical-31", "kf-0.75-sizes",
    "kf-0.75-size511", "kf-0.75-size512", "kf-0.75-size513", "kf-0.75-tail-both", "kf-0.75-tail-reg-best", "kf-0.75-tail-tail-best",
    "kf-0.75-positions", "kf-0.75-kf-side", "kf-0.75-chain-distinct-40-40", "kf-0.75-chain-distinct-65-64", "kf-0.75-chain-distinct-65-65",
    "kf-0.75-chain-distinct-31-31", "kf-0.75-chain-distinct-40-12-rot", "kf-0.75-chain-distinct-31-12-rot", "kf-0.75-alone-in-wave-node",
    "kf-0.75-shared-0", "kf-0.75-shared-1", "kf-0.75-shared-63", "kf-0.75-shared-64", "kf-0.75-shared-65", "kf-0.75-shared-130",
    "kf-0.75-empty-keyframe", "kf-0.75-empty-frame", "kf-0.7-thresholds-lane", "kf-0.7-thresholds-wave", "kf-0.75-thresholds-lane",
    "kf-0.75-thresholds-wave", "kf-0.75-ties", "kf-0.75-chain-identical-40", "kf-0.75-chain-identical-31", "kf-1.25-ties",
    "kf-1.25-chain-identical-40", "kf-1.25-chain-identical-31", "kf-0.75-invalid-second-kf-lane", "kf-0.75-invalid-second-kf-wave",
    "rig-0.7-rig-nleft0", "rig-0.7-rig-mid", "rig-0.7-chain-distinct-40-40", "rig-0.7-sizes", "rig-0.7-chain-distinct-40-12-rot",
    "rig-0.7-shared-65", "rig-0.7-empty-keyframe", "rig-0.7-empty-frame", "tri-outcomes", "tri-epipole-boundary", "tri-chi-boundary",
    "tri-den0", "tri-den0-coarse", "tri-stereo", "tri-only-stereo", "tri-rotation", "tri-empty-kf1", "tri-empty-kf2", "tri-n127",
    "tri-n128", "tri-n129", "tri-n255", "tri-n256", "tri-n257",
)


def lane_flag(p1, p2):
    return "second_same_lane" if p1 % bm.WAVE == p2 % bm.WAVE else "second_other_lane"


# ------------------------------------------------------------------ SearchByBoW
class BowBuilder:
    def __init__(self, name, form, ratio):
        self.name, self.form, self.ratio = "%s-%s-%s" % (form, ratio, name), form, ratio
        self.f, self.k, self.labels, self.expect = [], [], [], []
        self.next_nid = 100

    def nid(self):
        self.next_nid += 3
        return self.next_nid

    def node(self, nid, bits, valid=None, right=None):
        """the frame-side features of one node, in position order; returns their handles"""
        h = []
        for p, b in enumerate(bits):
            self.f.append([nid, b, 1 if valid is None else valid[p], 0 if right is None else right[p], 0.0])
            h.append(len(self.f) - 1)
        return h

    def filled(self, nid, size, at, **kw):
        """a node of `size` frame features: FILL everywhere but {position: bits} of `at`"""
        return self.node(nid, [at.get(p, FILL) for p in range(size)], **kw)

    def kfeat(self, label, nid, bits, outcome, flags=(), match=None, match_r=None, valid=True, angle=0.0):
        flags = set(flags)
        if self.form == "rig":                 # every node of a rig frame is a lane node; an accept by the left camera alone is rig_left
            flags -= {"second_same_lane", "second_other_lane"}
            if outcome == "accept" and match_r is None:
                flags.add("rig_left")
        self.k.append((nid, bits, 1 if valid else 0, angle))
        self.labels.append(label); self.expect.append((outcome, flags, match, match_r))

    def done(self):
        nF, nK = len(self.f), len(self.k)
        order = [i for i in range(nF) if not self.f[i][3]] + [i for i in range(nF) if self.f[i][3]]      # left camera first
        new = {o: k for k, o in enumerate(order)}
        kp_k, kp_f = np.zeros(nK, KP_DTYPE), np.zeros(nF, KP_DTYPE)
        kp_k["angle"] = [k[3] for k in self.k]
        kp_f["angle"] = [self.f[o][4] for o in order]
        d = lambda bits: np.stack([desc(b) for b in bits]) if len(bits) else np.zeros((0, 32), np.uint8)
        nid_f = np.array([self.f[o][0] for o in order], np.int64)
        assert len(set(self.labels)) == nK, self.name
        c = dict(name=self.name, form=self.form, ratio=self.ratio, kp_k=kp_k, d_k=d([k[1] for k in self.k]),
                 nid_k=np.array([k[0] for k in self.k], np.int64), valid=np.array([k[2] for k in self.k], np.uint8), kp_f=kp_f,
                 d_f=d([self.f[o][1] for o in order]), nid_f=nid_f, labels=list(self.labels),
                 expect=[(e[0], frozenset(e[1]), None if e[2] is None else new[e[2]], None if e[3] is None else new[e[3]]) for e in self.expect],
                 sizes={int(n): int((nid_f == n).sum()) for n in set(nid_f.tolist())})
        if self.form == "kf":
            c["valid2"] = np.array([self.f[o][2] for o in order], np.uint8)
        if self.form == "rig":
            c["nleft"] = nF - sum(f[3] for f in self.f)
        return c


def _size_node(b, S, tag):
    """S frame features, the best (10) at the LAST position and the second best (30) at position 0; two equal keyframe features"""
    n = b.nid()
    h = b.filled(n, S, {S - 1: 10, 0: 30} if S > 1 else {0: 10})
    wave = S >= bm.BOW_BIG_NODE
    if S == 1:
        b.kfeat(tag + "first", n, 0, "accept", ("no_second",), h[0])
        b.kfeat(tag + "second", n, 0, "no_candidate", ("skipped_claimed",))
        return
    b.kfeat(tag + "first", n, 0, "accept", (lane_flag(S - 1, 0),) if wave else (), h[S - 1])
    fl = {"skipped_claimed"} | ({"no_second"} if S == 2 else set()) | ({lane_flag(0, 1)} if wave and S > 2 else set())
    b.kfeat(tag + "second", n, 0, "accept", fl, h[0])


def case_sizes(form, ratio):
    b = BowBuilder("sizes", form, ratio)
    for S in (1, 31, 32, 33, 63, 64, 65):                   # lane and wave nodes alternate within the pair
        _size_node(b, S, "s%d_" % S)
    return b.done()


def case_size_big(form, ratio, S):
    b = BowBuilder("size%d" % S, form, ratio)
    _size_node(b, S, "s%d_" % S)
    return b.done()


def _two_of(b, S, p1, p2, tag):
    """best (10) at p1 and second best (13) at p2 of a wave node: A fails the ratio test BECAUSE of the second best (10 >= ratio * 13; with the
    filler for a second best it would pass), B (6 against 9) takes p1, C takes p2"""
    n = b.nid()
    h = b.filled(n, S, {p1: 10, p2: 13})
    fill0 = min(p for p in range(S) if p not in (p1, p2))
    b.kfeat(tag + "A", n, 0, "ratio_failed", (lane_flag(p1, p2),))
    b.kfeat(tag + "B", n, 4, "accept", (lane_flag(p1, p2),), h[p1])
    b.kfeat(tag + "C", n, 4, "accept", ("skipped_claimed", lane_flag(p2, fill0)), h[p2])


def case_tail(form, ratio, which):
    b = BowBuilder("tail-" + which, form, ratio)
    p1, p2 = {"both": (530, 590), "reg-best": (100, 599), "tail-best": (599, 100)}[which]
    _two_of(b, 600, p1, p2, "t_")
    return b.done()


POSITIONS = ((1, 65), (5, 6), (15, 16), (16, 15), (31, 32), (32, 31), (47, 48), (48, 47), (0, 63), (63, 0), (65, 3))


def case_positions(form, ratio):
    """same lane (p and p + 64), adjacent lanes, the row seams 15/16, 31/32, 47/48 of the wave reduction from both sides, lanes 0 and 63,
    the best at the node's last position"""
    b = BowBuilder("positions", form, ratio)
    for p1, p2 in POSITIONS:
        _two_of(b, 66, p1, p2, "p%d_%d_" % (p1, p2))
    return b.done()


def case_ties(form, ratio):
    """two candidates at the equal minimum: b2 = b1, so the ratio test fails below a ratio of 1; at 1.25 the LOWER position is taken"""
    b = BowBuilder("ties", form, ratio)
    for S, p1, p2 in ((70, 3, 40), (70, 3, 67), (31, 3, 20)):
        n = b.nid()
        h = b.filled(n, S, {p1: 10, p2: 10})
        fl = {"tie"} | ({lane_flag(p1, p2)} if S >= bm.BOW_BIG_NODE else set())
        if ratio > 1:
            b.kfeat("tie%d_%d_%d" % (S, p1, p2), n, 0, "accept", fl, h[p1])
        else:
            b.kfeat("tie%d_%d_%d" % (S, p1, p2), n, 0, "ratio_failed", fl)
    return b.done()


def case_chain_identical(form, ratio, S):
    """S identical frame descriptors against S identical keyframe features.  Every distance is 10, so b2 = b1 and below a ratio of 1 NOTHING is
    accepted: S times ratio_failed.  At 1.25 feature k takes position k (the first free one); the last has no second best."""
    b = BowBuilder("chain-identical-%d" % S, form, ratio)
    n = b.nid()
    h = b.node(n, [10] * S)
    wave = S >= bm.BOW_BIG_NODE
    for k in range(S):
        if ratio > 1:
            fl = ({"skipped_claimed"} if k else set()) | ({"no_second"} if k == S - 1 else {"tie"} | ({lane_flag(k, k + 1)} if wave else set()))
            b.kfeat("c%d" % k, n, 0, "accept", fl, h[k])
        else:
            b.kfeat("c%d" % k, n, 0, "ratio_failed", {"tie"} | ({lane_flag(0, 1)} if wave else set()))
    c = b.done(); c["expected_counts"] = {"accept": S if ratio > 1 else 0, "ratio_failed": 0 if ratio > 1 else S}
    return c


def case_chain_distinct(form, ratio, S, nkf, step, rot=None):
    """frame position j: 1 + step * j bits, keyframe feature k: step * k bits: k takes j = k at distance 1 against step + 1, in order.
    rot: index of one keyframe feature turned by 120 degrees, alone in its bin among nkf >= 12 matches: the rotation check removes it"""
    b = BowBuilder("chain-distinct-%d-%d%s" % (S, nkf, "" if rot is None else "-rot"), form, ratio)
    n = b.nid()
    h = b.node(n, [1 + step * j for j in range(S)])
    wave = S >= bm.BOW_BIG_NODE
    for k in range(nkf):
        fl = ({"skipped_claimed"} if k else set()) | ({"no_second"} if k == S - 1 else ({lane_flag(k, k + 1)} if wave else set()))
        if k == rot:
            fl.add("rot_removed")
        b.kfeat("d%d" % k, n, step * k, "accept", fl, h[k], angle=120.0 if k == rot else 0.0)
    c = b.done(); c["expected_counts"] = {"accept": nkf}
    return c


PREFETCH = ((1,), (1, 1), (1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0))


def case_prefetch(form, ratio):
    """1, 2 and 3 keyframe features on a wave node (the device fetches them two ahead), with the first, the last, all but the middle and all
    of them without a map point.  The valid ones take 10, then 40; the third finds 70 > TH_LOW."""
    b = BowBuilder("kf-side", form, ratio)
    for pat in PREFETCH:
        n = b.nid()
        h = b.filled(n, 34, {5: 10, 20: 40, 33: 70})
        seq = [("accept", {lane_flag(5, 20)}, h[5]), ("accept", {"skipped_claimed", lane_flag(20, 33)}, h[20]),
               ("above_th_low", {"skipped_claimed", lane_flag(33, 0)}, None)]
        v = 0
        for i, ok in enumerate(pat):
            tag = "v%s_%d" % ("".join(map(str, pat)), i)
            if not ok:
                b.kfeat(tag, n, 0, "no_mappoint", valid=False)
            else:
                b.kfeat(tag, n, 0, seq[v][0], seq[v][1], seq[v][2]); v += 1
    return b.done()


def ratio_row(ratio):
    """(b2, N): the first b2 >= 20 whose product with the ratio is the integer N in float32, found by evaluation"""
    for b2 in range(20, 70):
        p = f32(ratio) * f32(b2)
        if float(p) == int(p):
            return b2, int(p)
    raise AssertionError("no integer product")


def case_thresholds(form, ratio, wave):
    """best distance 49 / 50 / 51 (50 is accepted by the frame form only); the ratio product on an integer in float32, one row on each side
    and one on it; one candidate alone at 50 (b2 = 256) in a lane node"""
    b = BowBuilder("thresholds-%s" % ("wave" if wave else "lane"), form, ratio)
    S, pb, ps = (33, 17, 30) if wave else (2, 0, 1)
    kf = form == "kf"
    for d in (49, 50, 51):
        n = b.nid()
        h = b.filled(n, S, {pb: d})
        ok = d < 50 if kf else d <= 50
        b.kfeat("th%d" % d, n, 0, "accept" if ok else "above_th_low", {lane_flag(pb, 0 if pb else 1)} if wave else (), h[pb] if ok else None)
    b2, N = ratio_row(ratio)
    assert N + 1 < 50
    for d in (N - 1, N, N + 1):
        n = b.nid()
        h = b.filled(n, S, {pb: d, ps: b2})
        b.kfeat("ratio%+d" % (d - N), n, 0, "accept" if d < N else "ratio_failed", {lane_flag(pb, ps)} if wave else (), h[pb] if d < N else None)
    if not wave:
        n = b.nid()
        h = b.node(n, [50])
        b.kfeat("alone50", n, 0, "above_th_low" if kf else "accept", () if kf else ("no_second",), None if kf else h[0])
    return b.done()


def case_alone_in_wave_node(form, ratio):
    """b2 = 256 in a wave node.  Frame form: 31 keyframe features claim 31 of the 32 positions in order, the 32nd finds one free candidate at
    50: accepted (50 <= TH_LOW, 50 < ratio * 256).  Keyframe form: 32 of 33 second-keyframe features carry no map point; the one left at 49 is
    accepted, at 50 it is not (strict)."""
    b = BowBuilder("alone-in-wave-node", form, ratio)
    if form != "kf":
        n = b.nid()
        h = b.node(n, [1 + 4 * j for j in range(31)] + [180])
        for k in range(31):
            b.kfeat("d%d" % k, n, 4 * k, "accept", ({"skipped_claimed"} if k else set()) | {lane_flag(k, k + 1)}, h[k])
        b.kfeat("alone50", n, 130, "accept", ("skipped_claimed", "no_second"), h[31])
    else:
        for d in (49, 50):
            n = b.nid()
            h = b.filled(n, 33, {17: d}, valid=[p == 17 for p in range(33)])
            b.kfeat("alone%d" % d, n, 0, "accept" if d < 50 else "above_th_low", ("no_second",) if d < 50 else (), h[17] if d < 50 else None)
        n = b.nid()
        b.filled(n, 33, {}, valid=[0] * 33)
        b.kfeat("all_invalid", n, 0, "no_candidate")
    return b.done()


def case_kf_invalid(ratio, wave):
    """keyframe form: a second-keyframe feature without a map point holds the best distance (the valid 20 against 60 wins), or the second
    best (10 against 100 passes; counted, 10 against 12 would fail); n1 = 40 + 5 > n2 and the matched KF1 indices lie above n2 (lane pair)"""
    b = BowBuilder("invalid-second-kf-%s" % ("wave" if wave else "lane"), "kf", ratio)
    S = 40 if wave else 3
    pad = b.nid()
    b.node(pad, [FILL])
    for i in range(40):
        b.kfeat("pad%d" % i, pad, 0, "no_mappoint", valid=False)
    n = b.nid()
    h = b.filled(n, S, {0: 5, 1: 20, 2: 60}, valid=[p != 0 for p in range(S)])
    b.kfeat("invalid_best", n, 0, "accept", {lane_flag(1, 2)} if wave else (), h[1])
    n = b.nid()
    h = b.filled(n, S, {0: 10, 1: 12, 2: 100}, valid=[p != 1 for p in range(S)])
    b.kfeat("invalid_second", n, 0, "accept", {lane_flag(0, 2)} if wave else (), h[0])
    n = b.nid()
    b.filled(n, S, {}, valid=[0] * S)
    b.kfeat("all_invalid", n, 0, "no_candidate")
    return b.done()


def case_shared(form, ratio, N):
    """N shared nodes of one frame feature each (the node loop runs in trips of 64).  N = 0: no node in common, the keyframe's nodes land before
    the frame's first node, between two and behind the last.  N = 130: the first, the 65th and the last node are wave nodes."""
    b = BowBuilder("shared-%d" % N, form, ratio)
    if N == 0:
        b.node(10, [10]); b.node(20, [10])
        for nid, oc in ((5, "absent_before"), (15, "absent_between"), (25, "absent_end")):
            b.kfeat("n%d" % nid, nid, 0, oc)
        return b.done()
    for i in range(N):
        n = b.nid()
        if N == 130 and i in (0, 64, 129):
            h = b.filled(n, 33, {32: 10})
            b.kfeat("w%d" % i, n, 0, "accept", (lane_flag(32, 0),), h[32])
        else:
            h = b.node(n, [10])
            b.kfeat("n%d" % i, n, 0, "accept", ("no_second",), h[0])
    return b.done()


def case_empty(form, ratio, side):
    b = BowBuilder("empty-" + side, form, ratio)
    if side == "keyframe":
        b.node(b.nid(), [10] * 5)
    else:
        for i in range(3):
            b.kfeat("k%d" % i, 7, 0, "absent_end")
    return b.done()


def case_rig(variant):
    b = BowBuilder("rig-" + variant, "rig", 0.7)
    if variant == "nleft0":                                 # every feature is the right camera's: the left best stays 256
        n = b.nid()
        b.node(n, [5, 40], right=[1, 1])
        b.kfeat("blocked", n, 0, "above_th_low", ("rig_right_blocked",))
        return b.done()
    def node(label, left, right_, outcome, flags, m=None, mr=None, kbits=0):
        n = b.nid()
        h = b.node(n, left + right_, right=[0] * len(left) + [1] * len(right_))
        b.kfeat(label, n, kbits, outcome, flags, None if m is None else h[m], None if mr is None else h[mr])
    node("left_only", [10, 100], [60], "accept", ("rig_left",), 0)
    node("right_only", [10, 12], [50], "accept", ("rig_right",), None, 2)          # no ratio test on the right, <= TH_LOW
    node("both", [10, 100], [30], "accept", ("rig_both",), 0, 2)
    node("blocked", [51], [5], "above_th_low", ("rig_right_blocked",))              # the right accept is nested in the left TH_LOW branch
    node("right_tie", [10, 100], [20, 20], "accept", ("rig_both",), 0, 2)          # the lower index of two equal right candidates
    node("right_51", [10, 100], [51], "accept", ("rig_left",), 0)
    node("both_50", [50], [50], "accept", ("rig_both", "no_second"), 0, 1)
    node("ratio_fails", [10, 12], [51], "ratio_failed", ())
    node("left_tie", [10, 10], [51], "ratio_failed", ("tie",))
    # a node of 40 with both cameras: it stays a lane node; keyframe feature k takes left k (1 against 5) and right k (2; right k - 1, also at
    # 2 and earlier in the node, was claimed by k - 1)
    n = b.nid()
    h = b.node(n, [1 + 4 * j for j in range(20)] + [2 + 4 * j for j in range(20)], right=[0] * 20 + [1] * 20)
    for k in range(20):
        b.kfeat("mixed%d" % k, n, 4 * k, "accept", {"rig_both"} | ({"skipped_claimed"} if k else set()) | ({"no_second"} if k == 19 else set()),
                h[k], h[20 + k])
    return b.done()


FORM_RATIO = {"frame": 0.7, "kf": 0.75, "rig": 0.7}


@functools.lru_cache(maxsize=None)
def bow_cases():
    out = []
    for form in ("frame", "kf"):
        r = FORM_RATIO[form]
        out += [case_sizes(form, r)] + [case_size_big(form, r, S) for S in (511, 512, 513)]
        out += [case_tail(form, r, w) for w in ("both", "reg-best", "tail-best")] + [case_positions(form, r), case_prefetch(form, r)]
        out += [case_chain_distinct(form, r, *a) for a in ((40, 40, 4), (65, 64, 3), (65, 65, 3), (31, 31, 4))]
        out += [case_chain_distinct(form, r, 40, 12, 4, rot=7), case_chain_distinct(form, r, 31, 12, 4, rot=3)]
        out += [case_alone_in_wave_node(form, r)] + [case_shared(form, r, N) for N in (0, 1, 63, 64, 65, 130)]
        out += [case_empty(form, r, s) for s in ("keyframe", "frame")]
        for ratio in (0.7, 0.75):
            out += [case_thresholds(form, ratio, False), case_thresholds(form, ratio, True)]
        for ratio in (r, 1.25):
            out += [case_ties(form, ratio), case_chain_identical(form, ratio, 40), case_chain_identical(form, ratio, 31)]
    out += [case_kf_invalid(0.75, False), case_kf_invalid(0.75, True)]
    out += [case_rig(v) for v in ("nleft0", "mid")]
    # rig frames whose features are all the left camera's (nleft = nF): the frame form's results, on the lane path whatever the node size
    out += [case_chain_distinct("rig", 0.7, 40, 40, 4), case_sizes("rig", 0.7), case_chain_distinct("rig", 0.7, 40, 12, 4, rot=7),
            case_shared("rig", 0.7, 65), case_empty("rig", 0.7, "keyframe"), case_empty("rig", 0.7, "frame")]
    assert len({c["name"] for c in out}) == len(out)
    return out


def run_bow_model(c, check_ori):
    return bm.search_by_bow(c, c["ratio"], check_ori, c["form"], c.get("nleft", -1))


def run_bow_oracle(c, check_ori):
    form = c["form"]
    if form == "kf":
        return om.search_by_bow_kf(c, c["ratio"], check_ori)
    if form == "rig":
        return om.search_by_bow_rig(c, c.get("nleft", -1), c["ratio"], check_ori)
    return om.search_by_bow(c, c["ratio"], check_ori)


# ------------------------------------------------------------------ SearchForTriangulation
@functools.lru_cache(maxsize=None)
def tri_geometry():
    """the fixed Pinhole pair of make_tri_case: F12, epipole, scale and sigma^2 tables"""
    g = om.make_tri_case(np.random.default_rng(0), 0, 0)
    return g["F12"].astype(f32), (f32(g["ep"][0]), f32(g["ep"][1])), g["scale"], g["sigma2"]


def _fr(v):
    return Fraction(float(v))


def _fma(a, b, c):
    return round_f32(_fr(a) * _fr(b) + _fr(c))


def _mad(a, b, c, d, mode):
    """a * b + c * d in float32: unfused (0), the first product fused into the addition (1), the second (2)"""
    a, b, c, d = f32(a), f32(b), f32(c), f32(d)
    if mode == 1:
        return _fma(a, b, f32(c * d))
    if mode == 2:
        return _fma(c, d, f32(a * b))
    return f32(f32(a * b) + f32(c * d))


EPI_SUMS = ("la", "lb", "lc", "num", "den")
# F12[1][1] of the fixed pair (a rotation about y) is exactly 0: y1 * 0 is exact, so no fusion in lb = x1 * F[1] + y1 * F[4] + F[7] changes a bit
FMA_INERT_SUMS = ("lb",)


def epipolar_forms(x1, y1, F, x2, y2):
    """dsqr of Pinhole.cpp:130-141 unfused; with ONE product of ONE of its five sums fused into the addition (10 forms); with the first product
    of every sum fused"""
    def ev(modes):
        l = [f32(_mad(x1, F[k], y1, F[3 + k], modes.get(EPI_SUMS[k], 0)) + f32(F[6 + k])) for k in range(3)]
        num = f32(_mad(l[0], x2, l[1], y2, modes.get("num", 0)) + l[2])
        den = _mad(l[0], l[0], l[1], l[1], modes.get("den", 0))
        return float(f32(f32(num * num) / den))
    return ev({}), [ev({e: m}) for e in EPI_SUMS for m in (1, 2)], ev({e: 1 for e in EPI_SUMS})


def epipole_forms(ep, x2, y2):
    """ex^2 + ey^2 of ORBmatcher.cc:1095-1097 unfused, and with either square fused into the addition"""
    ex, ey = f32(ep[0] - f32(x2)), f32(ep[1] - f32(y2))
    return float(_mad(ex, ex, ey, ey, 0)), [float(_mad(ex, ex, ey, ey, 1)), float(_mad(ex, ex, ey, ey, 2))]


class TriBuilder:
    def __init__(self, name, only_stereo=False, coarse=False, F12=None, stereo=False):
        self.F12, self.ep, self.scale, self.sigma2 = tri_geometry()
        if F12 is not None:
            self.F12 = np.asarray(F12, f32)
        self.name, self.only_stereo, self.coarse, self.stereo = name, only_stereo, coarse, stereo
        self.k1, self.k2, self.labels, self.expect = [], [], [], []
        self.npt = 0

    def point(self):
        """a fresh node and a KF1 position whose epipolar line is neither flat nor upright"""
        k = self.npt; self.npt += 1
        return 100 + 3 * k, f32(120 + 37 * (k % 9)), f32(60 + 29 * (k % 7))

    def line(self, x1, y1):
        return [float(v) for v in bm.epiline(bm.F64, x1, y1, self.F12)]

    def on_line(self, x1, y1, x2, off=0.0):
        """the KF2 point at column x2, `off` pixels (perpendicular) off the epipolar line of (x1, y1)"""
        a, b, c = self.line(x1, y1)
        assert abs(b) > 0.2 * abs(a)
        return f32(x2), f32(-(a * float(f32(x2)) + c) / b + off * np.hypot(a, b) / abs(b))

    def kp2(self, nid, x, y, bits=0, octave=0, mp=0, ur=-1.0, angle=0.0):
        self.k2.append((nid, f32(x), f32(y), bits, octave, mp, ur, angle))
        return len(self.k2) - 1

    def kp1(self, label, nid, x, y, outcome, gates=(), flags=(), match=None, bits=0, octave=0, mp=0, ur=-1.0, angle=0.0):
        self.k1.append((nid, f32(x), f32(y), bits, octave, mp, ur, angle))
        self.labels.append(label); self.expect.append((outcome, frozenset(gates), frozenset(flags), match))

    def done(self):
        def side(rows):
            n = len(rows)
            kp = np.zeros(n, KP_DTYPE)
            kp["x"] = [r[1] for r in rows]; kp["y"] = [r[2] for r in rows]; kp["octave"] = [r[4] for r in rows]; kp["angle"] = [r[7] for r in rows]
            d = np.stack([desc(r[3]) for r in rows]) if n else np.zeros((0, 32), np.uint8)
            return (kp, d, np.array([r[0] for r in rows], np.int32), np.array([r[5] for r in rows], np.uint8),
                    np.array([r[6] for r in rows], f32))
        kp1, d1, nid1, mp1, ur1 = side(self.k1); kp2, d2, nid2, mp2, ur2 = side(self.k2)
        assert len(set(self.labels)) == len(self.labels), self.name
        g = np.zeros(1, om.TRI_GENERAL_DTYPE)[0]                          # the same pair for the general oracle / kernel: one Pinhole camera
        g["F12"][0] = self.F12; g["ep_x"], g["ep_y"] = self.ep; g["nleft1"] = g["nleft2"] = -1
        g["only_stereo"], g["coarse"] = int(self.only_stereo), int(self.coarse)
        g["cam1"][0] = g["cam2"][0] = (458.0, 457.0, 367.0, 248.0, 0, 0, 0, 0)
        return dict(name=self.name, stereo=self.stereo, kp1=kp1, d1=d1, nid1=nid1, mp1=mp1, ur1=ur1, kp2=kp2, d2=d2, nid2=nid2, mp2=mp2, ur2=ur2,
                    F12=self.F12.copy(), ep=self.ep, scale=self.scale, sigma2=self.sigma2, sigma2_1=self.sigma2.copy(), geom=g,
                    only_stereo=self.only_stereo, coarse=self.coarse, labels=list(self.labels), expect=list(self.expect))


def tri_outcomes():
    b = TriBuilder("tri-outcomes")
    X2 = 300.0

    def row(label, cands, outcome, gates=(), flags=(), match=None, **kw):
        """cands: (bits, perpendicular offset in pixels, column or None, kp2 keywords)"""
        nid, x1, y1 = b.point()
        h = [b.kp2(nid, *b.on_line(x1, y1, X2 + 7 * i if c[2] is None else c[2], c[1]), bits=c[0], **c[3]) for i, c in enumerate(cands)]
        b.kp1(label, nid, x1, y1, outcome, gates, flags, None if match is None else h[match], **kw)
    on = lambda bits, **kw: (bits, 0.0, None, kw)
    off = lambda bits, **kw: (bits, 10.0, None, kw)
    row("d49", [on(49)], "accept", match=0)
    row("d50", [on(50)], "accept", match=0)
    row("d51", [on(51)], "all_gated", ("dist_gt_th",))
    row("has_mp", [on(10)], "has_mappoint", mp=1)
    row("mp2", [on(10, mp=1)], "all_gated", ("mp2",))
    row("gt_best", [on(5), on(10)], "accept", ("dist_gt_best",), match=0)
    row("order_10_10", [on(10), on(10)], "accept", (), ("tie_replaced",), match=1)           # a later equal distance replaces
    row("order_10_10off", [on(10), off(10)], "accept", ("epipolar",), ("tie_kept",), match=0)  # ... unless it fails the geometry
    row("order_10_5_5", [on(10), on(5), on(5)], "accept", (), ("tie_replaced",), match=2)
    row("far", [off(10)], "all_gated", ("epipolar",))
    row("near_epipole", [(10, 0.0, float(b.ep[0]) - 4.0, {})], "all_gated", ("epipole",))
    nid, x1, y1 = b.point()
    b.kp1("node_absent", nid, x1, y1, "node_absent")
    return b.done()


def _steep_point(b, pt, octave):
    """a fresh KF1 point whose epipolar line passes `pt` at 1.5 times the distance (float64) that octave's 3.84 sigma^2 allows: geometry refuses"""
    for _ in range(63):
        nid, x1, y1 = b.point()
        a, bb, c = b.line(x1, y1)
        if abs(a * float(pt[0]) + bb * float(pt[1]) + c) / np.hypot(a, bb) > 1.5 * 1.96 * float(b.scale[octave]):
            return nid, x1, y1
    raise AssertionError("no such point")


def tri_epipole_boundary():
    """coarse pair (the epipolar distance decides nothing): a candidate is accepted exactly when the epipole gate lets it through"""
    b = TriBuilder("tri-epipole-boundary", coarse=True)
    ep = b.ep

    def row(label, x2, y2, octave):
        inside = bm.epipole_inside(bm.F32, ep, x2, y2, b.scale[octave])
        nid, x1, y1 = _steep_point(b, (x2, y2), octave)
        h = b.kp2(nid, x2, y2, bits=10, octave=octave)
        if inside:
            b.kp1(label, nid, x1, y1, "all_gated", ("epipole",))
        else:
            b.kp1(label, nid, x1, y1, "accept", (), ("coarse",), h)
    for octave in (0, 7):
        x_in = first_f32(lambda x: bm.epipole_inside(bm.F32, ep, x, ep[1], b.scale[octave]), float(ep[0]) - 40.0, float(ep[0]) - 1.0)
        row("ep%d_in" % octave, x_in, ep[1], octave)                 # the first float with ex^2 + ey^2 below 100 * scale
        row("ep%d_out" % octave, below(x_in), ep[1], octave)         # the last one not below
    rng = np.random.default_rng(7)
    n = 0
    while n < N_FMA_ROWS:
        octave = int(rng.integers(0, 4)); phi = rng.uniform(0.3, 1.2)
        r = 10.0 * np.sqrt(float(b.scale[octave]))
        x2 = f32(float(ep[0]) - r * np.cos(phi)); y0 = float(ep[1]) - r * np.sin(phi)
        y_in = first_f32(lambda y: bm.epipole_inside(bm.F32, ep, x2, y, b.scale[octave]), y0 - 3.0, y0 + 3.0)
        th = float(f32(f32(100) * b.scale[octave]))
        for k in range(-3, 4):
            y2 = from_ordinal(ordinal(y_in) + k)
            plain, fused = epipole_forms(ep, x2, y2)
            if any((plain < th) != (v < th) for v in fused):
                row("fma_ep%d" % n, x2, y2, octave); n += 1
                break
    return b.done()


def _chi_ok(b, x1, y1, x2, y2, octave):
    _, d = bm.epipolar_dsqr(bm.F32, bm.epiline(bm.F32, x1, y1, b.F12), f32(x2), f32(y2))
    return float(d) < 3.84 * float(b.sigma2[octave])


def tri_chi_boundary():
    """dsqr the last float32 below 3.84 * sigma2[octave] (in double) and the first not below, octaves 0 and 7; for each of the five sums of the expression a row that a
    product fused into that sum alone flips"""
    b = TriBuilder("tri-chi-boundary")

    def boundary(x1, y1, x2, octave):
        _, y_on = b.on_line(x1, y1, x2)
        reach = 6.0 * float(b.scale[octave])
        return first_f32(lambda y: not _chi_ok(b, x1, y1, x2, y, octave), float(y_on) + 0.25, float(y_on) + reach)

    def row(label, nid, x1, y1, x2, y2, octave):
        h = b.kp2(nid, x2, y2, bits=10, octave=octave)
        if _chi_ok(b, x1, y1, x2, y2, octave):
            b.kp1(label, nid, x1, y1, "accept", match=h)
        else:
            b.kp1(label, nid, x1, y1, "all_gated", ("epipolar",))
    for octave in (0, 7):
        for side in ("in", "out"):
            nid, x1, y1 = b.point()
            y_out = boundary(x1, y1, f32(300), octave)
            row("chi%d_%s" % (octave, side), nid, x1, y1, f32(300), y_out if side == "out" else below(y_out), octave)
    # row j: a product fused into sum j of (la, lb, lc, num, den) ALONE flips the decision, and so does fusing every sum
    rng = np.random.default_rng(11)
    for j, name in enumerate(EPI_SUMS):
        if name in FMA_INERT_SUMS:
            continue
        for _ in range(2000):
            nid, x1, y1 = b.point()
            octave = int(rng.integers(0, 8)); x2 = f32(rng.uniform(150, 450))
            y_out = boundary(x1, y1, x2, octave)
            th = 3.84 * float(b.sigma2[octave])
            hit = None
            for k in range(-4, 4):
                y2 = from_ordinal(ordinal(y_out) + k)
                plain, singles, every = epipolar_forms(x1, y1, b.F12, x2, y2)
                if any((plain < th) != (v < th) for v in singles[2 * j:2 * j + 2]) and (plain < th) != (every < th):
                    hit = y2
                    break
            if hit is not None:
                row("fma_chi_%s" % name, nid, x1, y1, x2, hit, octave)
                break
        else:
            raise AssertionError("no row for " + name)
    return b.done()


def tri_den0(coarse):
    """F12 with a zero left 3x2 block: la = lb = 0 for every keypoint, den == 0: refused (Pinhole.cpp:138), accepted under bCoarse"""
    F = np.zeros(9, f32); F[2], F[5], F[8] = 1e-3, -2e-3, 0.25
    b = TriBuilder("tri-den0" + ("-coarse" if coarse else ""), coarse=coarse, F12=F)
    nid = 100
    h = b.kp2(nid, 300, 200, bits=10)
    if coarse:
        b.kp1("den0", nid, 200, 150, "accept", (), ("coarse",), h)
    else:
        b.kp1("den0", nid, 200, 150, "all_gated", ("den0",))
    return b.done()


def tri_stereo():
    """stereo keypoints on either side skip the epipole gate: a candidate ON the epipolar line, 4 pixels from the epipole"""
    b = TriBuilder("tri-stereo", stereo=True)
    for label, ur1, ur2, outcome, gates, flags in (("st1", 50.0, -1.0, "accept", (), ("ep_skip_st1",)), ("st2", -1.0, 50.0, "accept", (), ("ep_skip_st2",)),
                                                   ("mono", -1.0, -1.0, "all_gated", ("epipole",), ()), ("ur_zero", 0.0, -1.0, "accept", (), ("ep_skip_st1",))):     # uRight == 0 is stereo (>= 0)
        nid, x1, y1 = b.point()
        h = b.kp2(nid, *b.on_line(x1, y1, float(b.ep[0]) - 4.0), bits=10, ur=ur2)
        b.kp1(label, nid, x1, y1, outcome, gates, flags, h if outcome == "accept" else None, ur=ur1)
    return b.done()


def tri_only_stereo():
    b = TriBuilder("tri-only-stereo", only_stereo=True, stereo=True)
    for label, ur1, ur2, outcome, gates in (("kp1_mono", -1.0, 50.0, "not_stereo", ()), ("kp2_mono", 50.0, -1.0, "all_gated", ("only_stereo2",)),
                                            ("both", 50.0, 50.0, "accept", ())):
        nid, x1, y1 = b.point()
        h = b.kp2(nid, *b.on_line(x1, y1, 300.0), bits=10, ur=ur2)
        b.kp1(label, nid, x1, y1, outcome, gates, (), h if outcome == "accept" else None, ur=ur1)
    return b.done()


def tri_count(n1):
    """n1 KF1 keypoints, one accepted at each end (the kernels stride over KF1 by 128 and by 256); the ones between hold map points"""
    b = TriBuilder("tri-n%d" % n1)
    nid, x1, y1 = b.point()
    h0 = b.kp2(nid, *b.on_line(x1, y1, 300.0), bits=10)
    nid2, xe, ye = b.point()
    h1 = b.kp2(nid2, *b.on_line(xe, ye, 320.0), bits=10)
    b.kp1("first", nid, x1, y1, "accept", match=h0)
    for i in range(1, n1 - 1):
        b.kp1("fill%d" % i, nid, x1, y1, "has_mappoint", mp=1)
    b.kp1("last", nid2, xe, ye, "accept", match=h1)
    return b.done()


def tri_rotation():
    b = TriBuilder("tri-rotation")
    for k in range(12):
        nid, x1, y1 = b.point()
        h = b.kp2(nid, *b.on_line(x1, y1, 300.0), bits=10)
        b.kp1("r%d" % k, nid, x1, y1, "accept", (), ("rot_removed",) if k == 5 else (), h, angle=120.0 if k == 5 else 0.0)
    return b.done()


def tri_empty(side):
    b = TriBuilder("tri-empty-kf%d" % side)
    if side == 1:
        b.kp2(100, 300, 200, bits=10)
    else:
        for i in range(3):
            b.kp1("k%d" % i, 100, 200, 150, "node_absent")
    return b.done()


@functools.lru_cache(maxsize=None)
def tri_cases():
    out = [tri_outcomes(), tri_epipole_boundary(), tri_chi_boundary(), tri_den0(False), tri_den0(True), tri_stereo(), tri_only_stereo(),
           tri_rotation(), tri_empty(1), tri_empty(2)] + [tri_count(n) for n in (127, 128, 129, 255, 256, 257)]
    assert len({c["name"] for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in bow_cases() + tri_cases() if c["name"] == name)
