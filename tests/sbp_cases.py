"""Crafted frames for the projection-window matchers: SearchByProjection (last frame / local map, one camera and rig) and Fuse's search.

Every case is built from blocks.  A block puts a few keypoints and queries into a slot of its own (slots are 60 pixels apart, a block's
keypoints stay within 14 pixels of the slot centre and its radius is at most 15, so no window reaches a neighbour's keypoints) and DECLARES,
per query, the outcome, the gate bits, the accept flags and the keypoint it must end up with.  tests/test_sbp_cases.py holds sbp_model.py and
the C oracle to these declarations; tests/test_gpu_sbp_cases.py holds the device to the oracle.  Descriptors: a keypoint's descriptor has its
first `bits` bits set and a query's its first `qbits` (default 0), so every Hamming distance is |bits - qbits|, chosen by hand.

Two geometries: "vga" = (0, 0, 640, 480) and "undist" = undistorted-style bounds with negative fractional minima; rig cases use 512 x 512.
Boundary values (a cell coordinate of k + 0.5, the window exits, the chi-square products) are searched in float32 for the geometry at hand
(first_f32), each row next to its float neighbour.

A case is a dict: name, kind ("frame" | "map" | "rig0" | "rig1" | "fuse"), geom, bounds, q, dq, kp, d, ur (or None), tm, th_high, ratio,
check_ori, nleft, mirror, sig, labels [nq], expect [nq] of (outcome, gates, flags, match), handback (None | False | reason).  gates is None in
the two bulk cases (a lattice of a thousand keypoints), whose rows are about sizes and positions, not gates."""
import functools
from fractions import Fraction
import numpy as np

import sbp_model as sm
from oracle_bind import KP_DTYPE
from oracle_match_bind import PROJ_QUERY_DTYPE
from case_floats import ordinal as _ordinal, from_ordinal as _from_ordinal, first_f32, below, above, round_f32 as _round_f32, desc as _desc

f32 = np.float32
GEOMS = {"vga": (0.0, 0.0, 640.0, 480.0), "undist": (-13.7, -9.3, 652.4, 488.6)}
RIG_BOUNDS = (0.0, 0.0, 512.0, 512.0)
SIG = (f32(1.0) / (f32(1.2) ** np.arange(8, dtype=f32)) ** 2).astype(f32)          # mvInvLevelSigma2 of an 8-level pyramid

# float64 would decide these rows differently from float32 (they sit on a rounding boundary by construction): "case:label"
F64_EXCEPTIONS = frozenset([
    "cells-undist-frame:y_half_on", "cells-undist-map:y_half_on",            # a cell coordinate of exactly k + 0.5 in float32, below it in double
    "cells-undist-frame:col63_last", "cells-undist-map:col63_last",          # the last float of column 63
    "windows-undist-frame:r1_out", "windows-undist-map:r1_out",              # the last float with r1 < 0
    "fuse-chi-vga:fma0", "fuse-chi-vga:fma3", "fuse-chi-undist:fma0", "fuse-chi-undist:fma3",       # products within a float of the threshold
])
# rows whose chi-square decision a fused multiply-add (either product fused into the sum) would flip; per fuse-chi case
N_FMA_ROWS = 4


class Geom:
    def __init__(self, bounds):
        self.bounds = bounds
        self.lo_x, self.lo_y, self.inv_w, self.inv_h = sm.F32.grid(bounds)
        self.max_x, self.max_y = f32(bounds[2]), f32(bounds[3])

    def col(self, x): return sm.F32.cell(x, self.lo_x, self.inv_w)
    def row(self, y): return sm.F32.cell(y, self.lo_y, self.inv_h)

    def col_edge(self, k):
        """smallest x in column k + 1 (cell coordinate k + 0.5 or the first float product above it)"""
        x0 = float(self.lo_x) + (k + 0.5) / float(self.inv_w)
        return first_f32(lambda x: self.col(x) >= k + 1, x0 - 1, x0 + 1)

    def row_edge(self, k):
        y0 = float(self.lo_y) + (k + 0.5) / float(self.inv_h)
        return first_f32(lambda y: self.row(y) >= k + 1, y0 - 1, y0 + 1)

    def exact_half(self, axis, near):
        """a cell k near `near` whose edge product is exactly k + 0.5 in float32; returns (k, edge coordinate)"""
        lo, inv, edge = (self.lo_x, self.inv_w, self.col_edge) if axis == 0 else (self.lo_y, self.inv_h, self.row_edge)
        for k in sorted(range(2, 44), key=lambda k: abs(k - near)):
            e = edge(k)
            if f32(f32(e - lo) * inv) == f32(k + 0.5):
                return k, e
        raise AssertionError("no exact half")


# ------------------------------------------------------------------ the builder
class Builder:
    def __init__(self, name, kind, geom, th_high=100, ratio=0.8, check_ori=None, stereo=True, nleft=None, slots=True):
        self.name, self.kind, self.geom = name, kind, geom
        self.bounds = RIG_BOUNDS if kind.startswith("rig") else GEOMS[geom]
        self.G = Geom(self.bounds)
        self.mode = {"frame": 0, "map": 1, "rig0": 0, "rig1": 1, "fuse": 2}[kind]
        self.th_high, self.ratio, self.stereo = th_high, ratio, stereo and not kind.startswith("rig")
        self.check_ori = (self.mode == 0) if check_ori is None else check_ori
        self.kp, self.bits, self.ur, self.tm, self.mirror, self.side = [], [], [], [], [], []
        self.q, self.qbits, self.labels, self.expect = [], [], [], []
        self.nslot = 0
        self.handback = None
        self.rig = kind.startswith("rig")

    def slot(self):
        w = 7 if self.rig else 9
        s = self.nslot; self.nslot += 1
        assert s < w * (7 if not self.rig else 7), "out of slots"
        return f32(60 + 60 * (s % w)), f32(60 + 60 * (s // w))

    def add_kp(self, x, y, octave=0, bits=0, ur=-1.0, held=False, angle=0.0, right=False):
        self.kp.append((x, y, octave, angle)); self.bits.append(bits); self.ur.append(ur); self.tm.append(7 if held else -1)
        self.mirror.append(-1); self.side.append(1 if right else 0)
        return len(self.kp) - 1

    def add_q(self, label, u, v, r, expect, match=None, gates=(), flags=(), flags_map=None, ur=0.0, lv=(-1, -1), obs=1, angle=0.0, qbits=0,
              right=False):
        if self.mode == 1 and flags_map is not None:
            flags = flags_map
        self.q.append((u, v, r, ur, angle, lv[0], lv[1], obs | (2 if right else 0))); self.qbits.append(qbits)
        self.labels.append(label); self.expect.append([expect, None if gates is None else tuple(gates), set(flags), match])
        return len(self.q) - 1

    def lost(self, t, *extra):
        self.expect[t][2] |= {"lost", *extra}

    def done(self):
        n, nq = len(self.kp), len(self.q)
        order = list(range(n))
        nleft = None
        if self.rig:                                      # left camera's keypoints first; declared matches follow the permutation
            order = [i for i in range(n) if not self.side[i]] + [i for i in range(n) if self.side[i]]
            nleft = n - sum(self.side)
        new = {o: k for k, o in enumerate(order)}
        kp = np.zeros(n, KP_DTYPE)
        for k, o in enumerate(order):
            kp["x"][k], kp["y"][k], kp["octave"][k], kp["angle"][k] = self.kp[o]
        d = np.stack([_desc(self.bits[o]) for o in order]) if n else np.zeros((0, 32), np.uint8)
        q = np.array(self.q, PROJ_QUERY_DTYPE) if nq else np.zeros(0, PROJ_QUERY_DTYPE)
        dq = np.stack([_desc(b) for b in self.qbits]) if nq else np.zeros((0, 32), np.uint8)
        ur = np.array([self.ur[o] for o in order], f32) if self.stereo else None
        tm = np.array([self.tm[o] for o in order], np.int32)
        mirror = np.array([new[self.mirror[o]] if self.mirror[o] >= 0 else -1 for o in order], np.int32)
        expect = [(e[0], e[1], frozenset(e[2]), None if e[3] is None else new[e[3]]) for e in self.expect]
        assert len(set(self.labels)) == nq, self.name
        return dict(name=self.name, kind=self.kind, mode=self.mode, geom=self.geom, bounds=tuple(float(f32(b)) for b in self.bounds), q=q, dq=dq,
                    kp=kp, d=d, ur=ur, tm=tm, th_high=self.th_high, ratio=self.ratio, check_ori=self.check_ori, nleft=nleft,
                    mirror=mirror if self.kind == "rig1" else None, sig=SIG, labels=list(self.labels), expect=expect, handback=self.handback)


# ------------------------------------------------------------------ blocks shared by SearchByProjection's two modes
NS = ("no_second",)


def blk_cells(b):
    G = b.G
    # a cell coordinate of exactly k + 0.5 rounds up: A (lower index) lands one column right of B and is visited AFTER it, so B wins the tie;
    # one float below, A shares B's column and row and wins by insertion order
    for axis, nm in ((0, "x"), (1, "y")):
        for side in ("on", "below"):
            cx, cy = b.slot()
            k, e = G.exact_half(axis, int(G.col(cx) if axis == 0 else G.row(cy)))
            e = e if side == "on" else below(e)
            if axis == 0:
                A = b.add_kp(e, cy, bits=5); B = b.add_kp(e - f32(2), cy, octave=1, bits=5); u, v = e, cy
                assert (G.col(e), G.col(e - f32(2))) == ((k + 1, k) if side == "on" else (k, k)) and G.row(cy) == G.row(cy)
            else:
                A = b.add_kp(cx, e, bits=5); B = b.add_kp(cx, e - f32(2), octave=1, bits=5); u, v = cx, e
                assert (G.row(e), G.row(e - f32(2))) == ((k + 1, k) if side == "on" else (k, k))
            b.add_q("%s_half_%s" % (nm, side), u, v, f32(8), "accept", match=B if side == "on" else A, flags=("tie",),
                    flags_map=("tie", "second_other_octave"))         # (local map: a tie inside one octave fails the ratio test, so B is of another)
    # x == max_x: cell 64, never a candidate although inside the radius; one float below max_x it is no better (63.999.. rounds to 64)
    cx, cy = b.slot()
    b.add_kp(G.max_x, cy, bits=1)
    b.add_q("x_is_max", G.max_x - f32(3), cy, f32(10), "empty")
    # the last x of column 63, and the first of column 64
    e = G.col_edge(63)
    cx, cy = b.slot()
    K = b.add_kp(below(e), cy + f32(240), bits=1); b.add_kp(e, cy + f32(240), bits=0)
    b.add_q("col63_last", below(e), cy + f32(240), f32(4), "accept", match=K, flags_map=NS)
    # a coordinate rounding to -1 (outside the grid) and one rounding to -0 (column 0)
    e = G.col_edge(-1)                                     # smallest x of column 0: products in (-0.5, 0.5) round to -0 / 0
    assert G.col(e) == 0 and G.col(below(e)) == -1 and float(f32(e - G.lo_x)) < 0
    b.add_kp(below(e), cy + f32(300), bits=1)
    b.add_q("col_minus1", below(e), cy + f32(300), f32(4), "empty")
    K = b.add_kp(e, cy + f32(360), bits=1)
    b.add_q("col_minus0", e, cy + f32(360), f32(4), "accept", match=K, flags_map=NS)
    e = G.row_edge(-1)
    b.add_kp(cx + f32(120), below(e), bits=1)
    b.add_q("row_minus1", cx + f32(120), below(e), f32(4), "empty")
    K = b.add_kp(cx + f32(180), e, bits=1)
    b.add_q("row_minus0", cx + f32(180), e, f32(4), "accept", match=K, flags_map=NS)


def blk_windows(b):
    G = b.G
    lo_x, lo_y, iw, ih = G.lo_x, G.lo_y, G.inv_w, G.inv_h
    r = f32(12)
    W = lambda x, lo, inv, last: sm.F32.window(x, r, lo, inv, last)
    # keypoints in the last / first column and row, too far from the query to pass |d| < r: "static" proves the window reached their cell
    ymid, xmid = f32(200), f32(300)
    b.add_kp(G.max_x - f32(8), ymid, bits=1); b.add_kp(G.lo_x + f32(3), ymid + f32(60), bits=1)
    b.add_kp(xmid, G.max_y - f32(8), bits=1); b.add_kp(xmid + f32(60), G.lo_y + f32(3), bits=1)
    # c0 == 63 (one column wide) | c0 >= 64
    u = first_f32(lambda x: W(x, lo_x, iw, 63)[2] == 0, float(G.max_x), float(G.max_x) + 40)
    assert W(below(u), lo_x, iw, 63)[:2] == (63, 63)
    b.add_q("c0_in", below(u), ymid, r, "static", gates=("dx",)); b.add_q("c0_out", u, ymid, r, "exit_c0")
    # c1 < 0 | c1 == 0
    u = first_f32(lambda x: W(x, lo_x, iw, 63)[2] != 1, float(G.lo_x) - 40, float(G.lo_x))
    assert W(u, lo_x, iw, 63)[:2] == (0, 0)
    b.add_q("c1_out", below(u), ymid + f32(60), r, "exit_c1"); b.add_q("c1_in", u, ymid + f32(60), r, "static", gates=("dx",))
    # r0 == 47 | r0 >= 48
    v = first_f32(lambda y: W(y, lo_y, ih, 47)[2] == 0, float(G.max_y), float(G.max_y) + 40)
    assert W(below(v), lo_y, ih, 47)[:2] == (47, 47)
    b.add_q("r0_in", xmid, below(v), r, "static", gates=("dy",)); b.add_q("r0_out", xmid, v, r, "exit_r0")
    # r1 < 0 | r1 == 0
    v = first_f32(lambda y: W(y, lo_y, ih, 47)[2] != 1, float(G.lo_y) - 40, float(G.lo_y))
    assert W(v, lo_y, ih, 47)[:2] == (0, 0)
    b.add_q("r1_out", xmid + f32(60), below(v), r, "exit_r1"); b.add_q("r1_in", xmid + f32(60), v, r, "static", gates=("dy",))
    # a radius of 0: the square is empty (strict <), whatever lies in the window's cells
    cx, cy = f32(120), f32(120)
    b.add_kp(cx, cy, bits=0)
    b.add_q("radius0", cx, cy, f32(0), "static", gates=("dx", "dy"))


def blk_square(b):
    """|dx| == r and |dy| == r are outside (strict <); one float nearer is inside"""
    for nm, ax in (("dx", 0), ("dy", 1)):
        for side in ("on", "in"):
            cx, cy = b.slot()
            r = f32(13) if side == "on" else above(f32(13))         # the difference is exactly 13 in both rows; the radius moves by one float
            K = b.add_kp(cx + f32(13), cy, bits=2) if ax == 0 else b.add_kp(cx, cy + f32(13), bits=2)
            if side == "on":
                b.add_q("%s_on" % nm, cx, cy, r, "static", gates=(nm,))
            else:
                b.add_q("%s_in" % nm, cx, cy, r, "accept", match=K, flags_map=NS)


def blk_levels(b):
    """the four level modes of Frame.cc:676-701 over keypoints of octaves 1..4 (nearest descriptor at octave 1, then 4, 2, 3)"""
    def four(cx, cy):
        return [b.add_kp(cx + f32(3 * o), cy, octave=o, bits=bits) for o, bits in ((1, 1), (2, 5), (3, 7), (4, 3))]
    so = ("second_other_octave",)
    for label, lv, best, gates, fm in (("lv_none", (-1, -1), 0, (), so), ("lv_none0", (0, -1), 0, (), so), ("lv_lower", (2, -1), 3, ("lv_below",), so),
                                       ("lv_upper", (0, 3), 0, ("lv_above",), so), ("lv_upper_m1", (-1, 3), 0, ("lv_above",), so),
                                       ("lv_both", (2, 3), 1, ("lv_below", "lv_above"), so), ("lv_both_one", (3, 3), 2, ("lv_below", "lv_above"), NS),
                                       ("lv_all_below", (5, -1), None, ("lv_below",), ())):
        cx, cy = b.slot()
        ks = four(cx, cy)
        if best is None:
            b.add_q(label, cx, cy, f32(15), "static", gates=gates, lv=lv)
        else:
            b.add_q(label, cx, cy, f32(15), "accept", match=ks[best], gates=gates, lv=lv, flags_map=fm)


def blk_uright(b):
    """ORBmatcher.cc:2041-2047 / :100-105: only uRight > 0 is gated, and |q.ur - ur2| == r is kept"""
    r = f32(13)
    for label, ur2, qur, ok in (("ur_on", f32(40), f32(53), True), ("ur_out", f32(40), above(f32(53)), False), ("ur_zero", f32(0), f32(500), True),
                                ("ur_minus1", f32(-1), f32(500), True), ("ur_neg_side", f32(40), below(f32(27)), False), ("ur_neg_on", f32(40), f32(27), True)):
        cx, cy = b.slot()
        K = b.add_kp(cx + f32(2), cy, bits=3, ur=ur2)
        if ok:
            b.add_q(label, cx, cy, r, "accept", match=K, ur=qur, flags_map=NS)
        else:
            b.add_q(label, cx, cy, r, "static", gates=("uright",), ur=qur)


def blk_thresholds(b):
    """dist == th_high | th_high + 1; an all-equal window whose first keypoint in grid order is not the one of smallest index"""
    th = b.th_high
    for label, bits in (("th_on", th), ("th_over", th + 1)):
        cx, cy = b.slot()
        K = b.add_kp(cx, cy, bits=bits)
        if bits <= th:
            b.add_q(label, cx, cy, f32(9), "accept", match=K, flags_map=NS)
        else:
            b.add_q(label, cx, cy, f32(9), "high")
    cx, cy = b.slot()
    ks = [b.add_kp(cx + f32(dx), cy + f32(dy), octave=o, bits=9) for dx, dy, o in ((12, 0, 0), (0, 12, 1), (-12, 0, 2), (0, -12, 3), (0, 0, 4))]
    assert b.G.col(cx - f32(12)) < b.G.col(cx) < b.G.col(cx + f32(12))
    b.add_q("all_equal", cx, cy, f32(14), "accept", match=ks[2], flags=("tie",), flags_map=("tie", "second_other_octave"))


def blk_claims(b):
    cx, cy = b.slot()                                        # pre-held: never a candidate
    b.add_kp(cx, cy, bits=0, held=True)
    b.add_q("preheld_only", cx, cy, f32(9), "static", gates=("preheld",))
    cx, cy = b.slot()                                        # pre-held best: the other one is taken
    b.add_kp(cx, cy, bits=0, held=True); K = b.add_kp(cx + f32(3), cy, bits=20)
    b.add_q("preheld_best", cx, cy, f32(9), "accept", match=K, gates=("preheld",), flags_map=NS)
    cx, cy = b.slot()                                        # held with observations: blocks; the second query finds nothing else
    K = b.add_kp(cx, cy, bits=1)
    b.add_q("blocker", cx, cy, f32(9), "accept", match=K, obs=1, flags_map=NS)
    b.add_q("blocked", cx, cy, f32(9), "held", obs=1)
    cx, cy = b.slot()                                        # held without observations: taken over, both count
    K = b.add_kp(cx, cy, bits=1)
    t = b.add_q("loser", cx, cy, f32(9), "accept", match=None, obs=0, flags_map=NS)
    b.add_q("taker", cx, cy, f32(9), "accept", match=K, obs=1, flags=("took_over",), flags_map=("took_over", "no_second"))
    b.lost(t)


def blk_ratio(b):
    """local-map mode only: d1 == ratio * d2 passes (strict >), the neighbour above fails"""
    assert b.mode == 1
    rows = {0.75: (("r_on", 6, 8, True), ("r_over", 7, 8, False), ("r_on2", 3, 4, True)), 0.8: (("r_on", 4, 5, True), ("r_on2", 8, 10, True), ("r_over", 5, 6, False), ("r_over2", 9, 11, False))}
    for label, d1, d2, ok in rows[b.ratio]:
        assert (f32(d1) > f32(b.ratio) * f32(d2)) == (not ok)
        cx, cy = b.slot()
        b.add_kp(cx + f32(4), cy, bits=d2); K = b.add_kp(cx - f32(4), cy, bits=d1)
        b.add_q(label, cx, cy, f32(9), "accept" if ok else "ratio", match=K if ok else None)
    cx, cy = b.slot()                                        # second best at another octave: the ratio is not asked
    K = b.add_kp(cx, cy, bits=9, octave=1); b.add_kp(cx + f32(3), cy, bits=10, octave=2)
    b.add_q("r_other_octave", cx, cy, f32(9), "accept", match=K, flags=("second_other_octave",))
    cx, cy = b.slot()                                        # the second best is claimed by an earlier query: the third becomes second
    B = b.add_kp(cx, cy, bits=6); S = b.add_kp(cx + f32(30), cy, bits=7); b.add_kp(cx - f32(5), cy, bits=10)
    b.add_q("r_claims_second", cx + f32(30), cy, f32(4), "accept", match=S, obs=1, flags=NS)
    b.nslot += 1
    b.add_q("r_third_is_second", cx + f32(12), cy, f32(20), "accept", match=B)
    cx, cy = b.slot()
    K = b.add_kp(cx, cy, bits=50)
    b.add_q("r_single", cx, cy, f32(9), "accept", match=K, flags=NS)


def sbp_general(kind, geom, ratio=0.8):
    out = []
    for nm, blocks in (("cells", (blk_cells,)), ("windows", (blk_windows,)), ("gates", (blk_square, blk_levels, blk_uright)),
                       ("claims", (blk_thresholds, blk_claims) + ((blk_ratio,) if kind == "map" else ()))):
        b = Builder("%s-%s-%s%s" % (nm, geom, kind, "" if ratio == 0.8 else "-%g" % ratio), kind, geom, ratio=ratio)
        for blk in blocks:
            blk(b)
        out.append(b.done())
    return out


# ------------------------------------------------------------------ single-purpose SearchByProjection cases
def case_all_columns(kind, geom):
    """one keypoint per grid column, a radius that covers all 64 columns and 48 rows (every lane owns a column); the nearest is in column 63"""
    b = Builder("all-columns-%s-%s" % (geom, kind), kind, geom)
    G = b.G
    ks = [b.add_kp(f32(float(G.lo_x) + (k + 0.2) / float(G.inv_w)), f32(240), octave=k % 2, bits=70 - k) for k in range(64)]
    assert [G.col(b.kp[k][0]) for k in ks] == list(range(64))
    b.add_q("all_columns", f32(320), f32(240), f32(340), "accept", match=ks[63], flags_map=("second_other_octave",))
    assert sm.window(np.array([(320, 240, 340, 0, 0, -1, -1, 1)], PROJ_QUERY_DTYPE), 0, b.bounds)[0] == (0, 63, 0, 47)
    return b.done()


def case_256(kind, geom):
    """th_high = 256: a distance of 256 is still no match (the reference's `dist < bestDist` with bestDist = 256), and it is no second best"""
    b = Builder("dist256-%s-%s" % (geom, kind), kind, geom, th_high=256)
    cx, cy = b.slot()
    b.add_kp(cx, cy, bits=256)
    b.add_q("d256_only", cx, cy, f32(9), "high")
    cx, cy = b.slot()
    K = b.add_kp(cx, cy, bits=255)
    b.add_q("d255", cx, cy, f32(9), "accept", match=K, flags_map=NS)
    cx, cy = b.slot()                      # best 210 > 0.8 * 256 at the same octave: a second best of 256 does not exist, so no ratio test
    K = b.add_kp(cx, cy, bits=210); b.add_kp(cx + f32(3), cy, bits=256)
    b.add_q("d210_second256", cx, cy, f32(9), "accept", match=K, flags_map=NS)
    return b.done()


def case_chain(kind, geom, nq):
    """keypoints on a line, bits rising; query t sees keypoints t-15 .. t+16 (32 static candidates: no truncated list), all want the lowest free
    one: in the replay form every trip of 64 needs 64 speculative rounds, and query t gets keypoint t"""
    b = Builder("chain%d-%s-%s" % (nq, geom, kind), kind, geom)
    X0, y = f32(100), f32(240)
    ks = [b.add_kp(X0 + f32(3 * i), y, octave=i % 2, bits=i + 1) for i in range(nq + 16)]
    for t in range(nq):
        fl = ("second_other_octave",)
        b.add_q("chain%d" % t, X0 + f32(3 * t + 1.5), y, f32(48), "accept", match=ks[t], gates=("dx",), obs=1, flags_map=fl)
    b.handback = False
    return b.done()


def case_blocked(kind, geom, nkp, second_off=False):
    """nkp keypoints in one window, queries that take them in order of distance.  32: the last query finds all 32 list entries blocked and
    the list complete -- no match, the pair stays.  33: the list is truncated and dry -- the pair is handed back (the sequential kernel finds
    keypoint 33).  second_off (local map): 31 claimed, the best is list entry 32 and the second best lies beyond the list."""
    b = Builder("%s%d-%s-%s" % ("secondoff" if second_off else "blocked", nkp, geom, kind), kind, geom)
    cx, cy = f32(300), f32(240)
    ks = [b.add_kp(cx + f32(3 * (i % 7) - 9), cy + f32(3 * (i // 7) - 6), octave=i % 2, bits=i + 1) for i in range(nkp)]
    ntake = nkp - 2 if second_off else nkp
    for t in range(ntake):
        last = t == nkp - 1
        b.add_q("take%d" % t, cx, cy, f32(14), "accept", match=ks[t], obs=1, flags_map=NS if last else ("second_other_octave",))
    if second_off:
        b.add_q("best_is_entry32", cx, cy, f32(14), "accept", match=ks[ntake], obs=1, flags_map=("second_other_octave",))
        b.handback = "second" if kind == "map" else False
    else:
        b.add_q("all_blocked", cx, cy, f32(14), "held", obs=1)
        b.handback = "best" if nkp > sm.SBPL_K else False
    return b.done()


def case_buffer(kind, geom, nkp):
    """512 | 513 static candidates of one query (SBPL_BUF): 512 stay with the replay form, 513 give up"""
    b = Builder("buffer%d-%s-%s" % (nkp, geom, kind), kind, geom)
    cx, cy = f32(300), f32(240)
    ks = [b.add_kp(cx + f32(i % 27 - 13), cy + f32(i // 27 - 9), octave=i % 2, bits=(i * 7) % 90) for i in range(nkp)]
    best = [k for k in ks if b.bits[k] == 0]           # distance 0: 0 > ratio * 0 is false, the tie passes the local map's ratio test
    order = sorted(best, key=lambda k: (b.G.col(b.kp[k][0]), b.G.row(b.kp[k][1]), k))
    b.add_q("wide", cx, cy, f32(20), "accept", match=order[0], obs=1, flags=("tie",), flags_map=("tie",))
    b.add_q("wide_again", cx, cy, f32(20), "accept", match=order[1], obs=1, flags=("tie",), flags_map=("tie",))
    b.handback = "buffer" if nkp > sm.SBPL_BUF else False
    return b.done()


def case_loop_switch(kind, geom, n_in):
    """n_in keypoints inside the grid (1024: the register loop's last size, 1025: the LDS loop's first) and 30 outside it, spread through the
    index range, so n != n_items; single-candidate queries on the first, the last and every 50th in-grid keypoint"""
    b = Builder("loop%d-%s-%s" % (n_in, geom, kind), kind, geom)
    G = b.G
    rng = np.random.default_rng(n_in)
    ins = []
    for i in range(n_in):
        if i % 34 == 17 and len(b.kp) - len(ins) < 30:
            b.add_kp(G.max_x + f32(3), f32(20 + i % 400), bits=0)                 # column 64: in no cell
        ins.append(b.add_kp(f32(20 + 13 * (i % 45)), f32(30 + 18 * (i // 45)), octave=int(rng.integers(0, 8)), bits=int(rng.integers(0, 60))))
    assert len(b.kp) - len(ins) == 30 and all(G.col(b.kp[k][0]) == 64 for k in range(len(b.kp)) if k not in set(ins))
    for i in sorted(set(list(range(0, n_in, 50)) + [n_in - 1])):
        k = ins[i]
        b.add_q("at%d" % i, b.kp[k][0], b.kp[k][1], f32(5), "accept", match=k, gates=None, obs=i % 2, flags_map=NS)
    b.handback = False
    return b.done()


def case_2048(kind, geom, reverse):
    """2048 keypoints, all in the grid, one per (column, row < 32) cell: index == CSR position (reverse: index == 2047 - position); the
    queries accept index 2047, CSR position 2047 and a few in between (11-bit key fields of the replay form)"""
    b = Builder("full2048%s-%s-%s" % ("r" if reverse else "", geom, kind), kind, geom)
    G = b.G
    pos = [(f32(float(G.lo_x) + (c + 0.2) / float(G.inv_w)), f32(float(G.lo_y) + (r + 0.2) / float(G.inv_h))) for c in range(64) for r in range(32)]
    assert [(G.col(x), G.row(y)) for x, y in pos] == [(c, r) for c in range(64) for r in range(32)]
    seq = pos[::-1] if reverse else pos
    ks = [b.add_kp(x, y, octave=i % 3, bits=(i * 11) % 97) for i, (x, y) in enumerate(seq)]
    for i in (0, 1, 1023, 1024, 2046, 2047):
        b.add_q("idx%d" % i, seq[i][0], seq[i][1], f32(4), "accept", match=ks[i], gates=None, obs=1, flags_map=NS)
    b.handback = False
    return b.done()


def case_rotation_takeover(geom):
    """frame mode with the rotation check: twelve matches in bin 0, one (without observations) in bin 3, whose keypoint a later query of bin 0
    takes over: the dropped bin clears the keypoint although the later query owns it, and counts once"""
    b = Builder("rotation-takeover-%s-frame" % geom, "frame", geom, check_ori=True)
    for i in range(12):
        cx, cy = b.slot()
        K = b.add_kp(cx, cy, bits=1)
        b.add_q("bin0_%d" % i, cx, cy, f32(9), "accept", match=K)
    cx, cy = b.slot()
    b.add_kp(cx, cy, bits=1, angle=0.0)
    t = b.add_q("bin3", cx, cy, f32(9), "accept", match=None, obs=0, angle=100.0)
    b.lost(t, "rot_removed")
    b.add_q("takes_bin3s", cx, cy, f32(9), "accept", match=None, obs=1, angle=0.0, flags=("took_over",))      # cleared by the rotation check
    return b.done()


def case_empty(kind, geom, side):
    b = Builder("empty-%s-%s-%s" % (side, geom, kind), kind, geom, nleft=0)
    if side == "n0":
        for i in range(3):
            b.add_q("q%d" % i, f32(100 + 50 * i), f32(100), f32(10), "empty", lv=(0, 3) if kind == "fuse" else (-1, -1))
    else:
        for i in range(5):
            b.add_kp(f32(100 + 20 * i), f32(100), bits=i)
    return b.done()


# ------------------------------------------------------------------ rig frames
def case_rig(mode, variant):
    """512 x 512 rig frames: queries of the left camera, of the right camera (has_obs bit 1) and both; the same position in both halves; the
    mirror rule of the local-map mode.  variant: "mixed", "left" (nleft == n) or "right" (nleft == 0)."""
    b = Builder("rig%d-%s" % (mode, variant), "rig%d" % mode, None)
    L, R = variant != "right", variant != "left"
    fm = NS
    if L:
        cx, cy = b.slot()
        K = b.add_kp(cx, cy, bits=1)
        b.add_q("left_only", cx, cy, f32(9), "accept", match=K, flags_map=fm)
    if R:
        cx, cy = b.slot()
        K = b.add_kp(cx, cy, bits=1, right=True)
        b.add_q("right_only", cx, cy, f32(9), "accept", match=K, right=True, flags_map=fm)
    if L and R:
        cx, cy = b.slot()                                   # the same position in both halves: each query sees its own camera's keypoint only
        KL = b.add_kp(cx, cy, bits=4); KR = b.add_kp(cx, cy, bits=2, right=True)
        b.add_q("same_pos_left", cx, cy, f32(9), "accept", match=KL, flags_map=fm)
        b.add_q("same_pos_right", cx, cy, f32(9), "accept", match=KR, right=True, flags_map=fm)
        cx, cy = b.slot()                                   # a left-camera keypoint is no candidate of a right-camera query
        b.add_kp(cx, cy, bits=1)
        b.add_q("wrong_camera", cx, cy, f32(9), "empty", right=True)
        cx, cy = b.slot()                                   # has_obs bit 1 is the camera, bit 0 the observations: this right-camera claim does not block
        K = b.add_kp(cx, cy, bits=1, right=True)
        t = b.add_q("right_no_obs", cx, cy, f32(9), "accept", match=None, obs=0, right=True, flags_map=fm)
        b.add_q("right_takes_over", cx, cy, f32(9), "accept", match=K, obs=1, right=True, flags=("took_over",), flags_map=("took_over", "no_second"))
        b.lost(t)
        if mode == 1:
            cx, cy = b.slot()                               # mirror onto a free keypoint: both are assigned, the match counts twice
            A = b.add_kp(cx, cy, bits=1); M = b.add_kp(cx + f32(200), cy, bits=9, right=True)
            b.mirror[A] = M; b.mirror[M] = A
            b.add_q("mirror_free", cx, cy, f32(9), "accept", match=A, flags=("mirrored", "no_second"))
            cx, cy = b.slot()                               # mirror onto a pre-held keypoint: overwritten
            A = b.add_kp(cx, cy, bits=1); M = b.add_kp(cx + f32(200), cy, bits=9, right=True, held=True)
            b.mirror[A] = M
            b.add_q("mirror_preheld", cx, cy, f32(9), "accept", match=A, flags=("mirrored", "mirror_overwrote", "no_second"))
            cx, cy = b.slot()                               # mirror onto a keypoint a later right-camera query would have taken: it finds it held
            A = b.add_kp(cx, cy, bits=1); M = b.add_kp(cx, cy, bits=3, right=True)
            b.mirror[A] = M
            b.add_q("mirror_first", cx, cy, f32(9), "accept", match=A, obs=1, flags=("mirrored", "no_second"))
            b.add_q("mirror_taken", cx, cy, f32(9), "held", obs=1, right=True)
            cx, cy = b.slot()                               # mirror onto a keypoint an earlier query holds: that query loses it
            A = b.add_kp(cx, cy, bits=1); M = b.add_kp(cx, cy, bits=3, right=True)
            b.mirror[A] = M
            t = b.add_q("holds_mirror", cx, cy, f32(9), "accept", match=None, obs=1, right=True, flags=NS)
            b.add_q("mirror_overwrites_claim", cx, cy, f32(9), "accept", match=A, obs=1, flags=("mirrored", "mirror_overwrote", "no_second"))
            b.lost(t)
            cx, cy = b.slot()                               # mirror -1: one assignment
            A = b.add_kp(cx, cy, bits=1)
            b.add_q("mirror_none", cx, cy, f32(9), "accept", match=A, flags=NS)
    return b.done()


# ------------------------------------------------------------------ Fuse
def chi_forms(ex, ey, er, sig):
    """e2 * sig for the unfused sum and for the sums with one product fused into an addition"""
    ex, ey = f32(ex), f32(ey)
    xx, yy = f32(ex * ex), f32(ey * ey)
    FX, FY = Fraction(float(ex)) ** 2, Fraction(float(ey)) ** 2
    if er is None:
        plain = f32(xx + yy)
        fused = [_round_f32(FX + Fraction(float(yy))), _round_f32(Fraction(float(xx)) + FY)]
    else:
        er = f32(er); rr = f32(er * er); FR = Fraction(float(er)) ** 2
        s = f32(xx + yy)
        plain = f32(s + rr)
        fused = [_round_f32(Fraction(float(s)) + FR), f32(_round_f32(FX + Fraction(float(yy))) + rr), f32(_round_f32(Fraction(float(xx)) + FY) + rr)]
    return float(f32(plain * sig)), [float(f32(v * sig)) for v in fused]


def fma_row(cx, cy, stereo, seed):
    """(u, v, er, lv, over) for a keypoint at (cx, cy): a query, found by search, whose unfused chi-square lies on the other side of the
    threshold than one with a product fused into an addition.  ex, ey are the float32 differences the code under test forms itself."""
    rng = np.random.default_rng(seed)
    th = 7.8 if stereo else 5.99
    while True:
        lv = int(rng.integers(0, 3))
        u = f32(cx + f32(rng.uniform(0.8, 1.6))); ex = f32(u - cx); er = f32(int(rng.integers(4, 10)) / 8.0) if stereo else None
        rest = th / float(SIG[lv]) - float(ex) ** 2 - (float(er) ** 2 if stereo else 0.0)
        v0 = f32(cy + f32(np.sqrt(rest)))
        for k in range(-3, 4):
            v = _from_ordinal(_ordinal(v0) + k)
            plain, fused = chi_forms(ex, f32(v - cy), er, SIG[lv])
            if any((plain > th) != (w > th) for w in fused):
                return u, v, er, lv, plain > th


def case_fuse_chi(geom):
    b = Builder("fuse-chi-%s" % geom, "fuse", geom)
    # the largest product not above the threshold and the next one above, mono and stereo, octave 0 and 2
    for stereo in (False, True):
        for lv in (0, 2):
            th = 7.8 if stereo else 5.99
            cx, cy = b.slot()
            er = f32(1.0) if stereo else None
            chi = lambda u: sm.F32.chi2(f32(u - cx), f32(0), er, SIG[lv])
            u_out = first_f32(lambda u: chi(u) > th, float(cx) + 0.5, float(cx) + 7)
            for side, u in (("in", below(u_out)), ("out", u_out)):
                if side == "out":
                    cx2, cy = b.slot(); u = u + (cx2 - cx); cxx = cx2
                    assert (sm.F32.chi2(f32(u - cxx), f32(0), er, SIG[lv]) > th)
                else:
                    cxx = cx
                K = b.add_kp(cxx, cy, octave=lv, bits=3, ur=f32(30) if stereo else f32(-1))
                label = "%s%d_%s" % ("stereo" if stereo else "mono", lv, side)
                if side == "in":
                    b.add_q(label, u, cy, f32(8), "accept", match=K, ur=f32(31), lv=(lv - 1, lv))
                else:
                    b.add_q(label, u, cy, f32(8), "static", gates=("chi_stereo" if stereo else "chi_mono",), ur=f32(31), lv=(lv - 1, lv))
    # rows a fused multiply-add would decide the other way
    for j in range(N_FMA_ROWS):
        cx, cy = b.slot()
        u, v, er, lv, over = fma_row(cx, cy, j >= N_FMA_ROWS // 2, 100 + j)
        K = b.add_kp(cx, cy, octave=lv, bits=3, ur=f32(-1) if er is None else f32(64))
        qur = f32(0) if er is None else f32(f32(64) + er)
        if over:
            b.add_q("fma%d" % j, u, v, f32(8), "static", gates=("chi_mono" if er is None else "chi_stereo",), ur=qur, lv=(lv, lv))
        else:
            b.add_q("fma%d" % j, u, v, f32(8), "accept", match=K, ur=qur, lv=(lv, lv))
    return b.done()


def case_fuse_gates(geom):
    b = Builder("fuse-gates-%s" % geom, "fuse", geom)
    # uRight == 0 takes the stereo branch (>= 0), -1 the mono one.  e2 = 5 passes mono; with er = 2 the stereo sum 9 > 7.8
    for label, ur2, qur, ex, ok, gate in (("ur0_stereo_fails", f32(0), f32(2), f32(2), False, "chi_stereo"), ("urm1_mono_passes", f32(-1), f32(2), f32(2), True, None),
                                          ("ur0_stereo_passes", f32(0), f32(0), f32(2.6), True, None), ("urm1_mono_fails", f32(-1), f32(0), f32(2.6), False, "chi_mono")):
        cx, cy = b.slot()
        K = b.add_kp(cx, cy, octave=0, bits=4, ur=ur2)
        if ok:
            b.add_q(label, cx + ex, cy + f32(1), f32(6), "accept", match=K, ur=qur, lv=(-1, 0))
        else:
            b.add_q(label, cx + ex, cy + f32(1), f32(6), "static", gates=(gate,), ur=qur, lv=(-1, 0))
    # [min, max] always checks both ends, also with min = -1 and max = -1 (nothing passes o > -1)
    for label, lv, best, gates in (("lv_both", (2, 3), 1, ("lv_below", "lv_above")), ("lv_max_m1", (-1, -1), None, ("lv_above",)), ("lv_low", (0, 1), 0, ("lv_above",))):
        cx, cy = b.slot()
        ks = [b.add_kp(cx + f32(0.5 * o), cy, octave=o, bits=bits) for o, bits in ((1, 1), (2, 5), (3, 7), (4, 3))]
        if best is None:
            b.add_q(label, cx, cy, f32(8), "static", gates=gates, lv=lv)
        else:
            b.add_q(label, cx + f32(0.5), cy, f32(8), "accept", match=ks[best], gates=gates, lv=lv)
    # the square (strict), a distance tie (first in grid order), distance 256 (best stays -1 / 256), and an empty window
    cx, cy = b.slot()
    b.add_kp(cx + f32(6), cy, bits=1)
    b.add_q("dx_on", cx, cy, f32(6), "static", gates=("dx",), lv=(0, 0))
    cx, cy = b.slot()
    e = b.G.col_edge(b.G.col(cx))
    A = b.add_kp(e + f32(0.5), cy, bits=5); B = b.add_kp(e - f32(1), cy, bits=5)
    assert b.G.col(e + f32(0.5)) == b.G.col(e - f32(1)) + 1
    b.add_q("tie", e, cy, f32(6), "accept", match=B, lv=(0, 0))
    cx, cy = b.slot()
    b.add_kp(cx, cy, bits=256)
    b.add_q("d256", cx, cy, f32(6), "high", lv=(0, 0))
    cx, cy = b.slot()
    b.add_q("nothing", cx, cy, f32(6), "empty", lv=(0, 0))
    b.add_q("far_right", b.G.max_x + f32(40), cy, f32(6), "exit_c0", lv=(0, 0))
    b.add_q("far_up", cx, b.G.lo_y - f32(40), f32(6), "exit_r1", lv=(0, 0))
    return b.done()


# ------------------------------------------------------------------ the case list
@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for geom in GEOMS:
        for kind in ("frame", "map"):
            out += sbp_general(kind, geom)
            out += [case_all_columns(kind, geom), case_256(kind, geom), case_chain(kind, geom, 64), case_chain(kind, geom, 65),
                    case_blocked(kind, geom, 32), case_blocked(kind, geom, 33), case_blocked(kind, geom, 33, second_off=True),
                    case_buffer(kind, geom, 512), case_buffer(kind, geom, 513), case_empty(kind, geom, "n0"), case_empty(kind, geom, "nq0")]
        out += sbp_general("map", geom, ratio=0.75)[3:]
        out += [case_rotation_takeover(geom), case_fuse_chi(geom), case_fuse_gates(geom), case_empty("fuse", geom, "n0"), case_empty("fuse", geom, "nq0")]
    out += [case_loop_switch("frame", "vga", 1024), case_loop_switch("frame", "vga", 1025), case_loop_switch("map", "undist", 1024),
            case_loop_switch("map", "undist", 1025), case_2048("frame", "undist", False), case_2048("map", "vga", True)]
    for mode in (0, 1):
        out += [case_rig(mode, v) for v in ("mixed", "left", "right")]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def cases(kind=None):
    return [c for c in all_cases() if kind is None or c["kind"] == kind]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ------------------------------------------------------------------ model and oracle on a case
def run_model(c, arith=sm.F32, stereo=True):
    ur = c["ur"] if stereo else None
    if c["kind"] == "fuse":
        return sm.fuse(c["q"], c["dq"], c["kp"], c["d"], ur, c["sig"], c["bounds"], arith)
    return sm.search(c["mode"], c["q"], c["dq"], c["kp"], c["d"], ur, c["bounds"], c["tm"], c["th_high"], c["ratio"], c["check_ori"],
                     c["nleft"], c["mirror"], arith)


def run_oracle(c, stereo=True):
    """fuse: (best_idx, best_dist); the others: (nmatches, train_match)"""
    import oracle_match_bind as om
    ur = c["ur"] if stereo else None
    if c["kind"] == "fuse":
        return om.fuse_search(c["q"], c["dq"], c["kp"], c["d"], ur, c["sig"], c["bounds"])
    if c["kind"] == "frame":
        return om.search_by_projection(c["q"], c["dq"], c["kp"], c["d"], ur, c["bounds"], c["tm"], c["th_high"], c["check_ori"])
    if c["kind"] == "map":
        return om.search_by_projection_map(c["q"], c["dq"], c["kp"], c["d"], ur, c["bounds"], c["tm"], c["th_high"], c["ratio"])
    return om.search_by_projection_rig(c["mode"], c["q"], c["dq"], c["kp"], c["d"], c["nleft"], c["mirror"], c["bounds"], c["tm"], c["th_high"],
                                       c["ratio"], c["check_ori"])


# declared totals over all_cases(): tests/test_sbp_cases.py asserts them (and DESIGN.md lists them)
TOTALS = {
    "outcome:exit_c0": 6, "outcome:exit_c1": 4, "outcome:exit_r0": 4, "outcome:exit_r1": 6, "outcome:empty": 34, "outcome:static": 66,
    "outcome:held": 15, "outcome:high": 12, "outcome:ratio": 6, "outcome:accept": 1244,
    "gate:lv_below": 18, "gate:lv_above": 22, "gate:dx": 534, "gate:dy": 16, "gate:preheld": 12, "gate:uright": 8, "gate:chi_mono": 6,
    "gate:chi_stereo": 10,
    "flag:no_second": 120, "flag:second_other_octave": 478, "flag:tie": 38, "flag:took_over": 10, "flag:lost": 11, "flag:rot_removed": 2,
    "flag:mirrored": 4, "flag:mirror_overwrote": 2,
    "handback:best": 4, "handback:second": 2, "handback:buffer": 4,
}
