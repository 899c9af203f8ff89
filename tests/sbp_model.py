"""Plain numpy model of the projection-window matchers, with the outcome of every query named.  TEST INFRASTRUCTURE ONLY.

Restated from the reference text: ORBmatcher::SearchByProjection(Frame&, const Frame&, ...) (ORBmatcher.cc:1965-2181), SearchByProjection(Frame&,
vector<MapPoint*>&, ...) (:48-218), both also for rig frames (Nleft != -1, with the mirror rule of :142-146 / :203-207), the window search of
Fuse (:1499-1570), Frame::GetFeaturesInArea (Frame.cc:645-714) and the grid of Frame.cc:377-408 / :716-726.  float32 exactly where the reference
computes in float (arith=F32); arith=F64 evaluates the window, cell and chi-square arithmetic in double instead, to tell which rows sit on a
rounding boundary.  search() also predicts whether the device's replay form (k_sbp_candidates keeps the SBPL_K smallest keys of at most SBPL_BUF
candidates per query, k_sbp_replay walks them) has to hand the pair back to the sequential kernel."""
import math
import numpy as np

COLS, ROWS = 64, 48
SBPL_K, SBPL_BUF = 32, 512
f32 = np.float32

# outcome of one query
OUTCOMES = ("exit_c0", "exit_c1", "exit_r0", "exit_r1", "empty", "static", "held", "high", "ratio", "accept")
# gate bits: the reasons seen among a query's in-window keypoints
GATES = ("lv_below", "lv_above", "dx", "dy", "preheld", "uright", "chi_mono", "chi_stereo")
G = {n: 1 << i for i, n in enumerate(GATES)}
# accept flags
FLAGS = ("no_second", "second_other_octave", "tie", "took_over", "lost", "rot_removed", "mirrored", "mirror_overwrote")
F = {n: 1 << i for i, n in enumerate(FLAGS)}
HANDBACK_REASONS = ("best", "second", "buffer")


def roundf(v):
    """C roundf: half away from zero (np.round is half to even)"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


class Arith:
    """the float type of the window / cell / chi-square arithmetic"""
    def __init__(self, t):
        self.t = t

    def grid(self, bounds):
        t = self.t
        b = [t(f32(v)) for v in bounds]
        return b[0], b[1], t(COLS) / (b[2] - b[0]), t(ROWS) / (b[3] - b[1])          # Frame.cc:334-335

    def cell(self, x, lo, inv):                                                        # Frame.cc:718-719
        t = self.t
        return roundf((t(x) - lo) * inv)

    def window(self, x, r, lo, inv, last):                                             # Frame.cc:656-674; returns (first, last, exit)
        t = self.t
        a = int(math.floor((t(x) - lo - t(r)) * inv))
        a = max(a, 0)
        if a > last:
            return a, 0, 0
        b = int(math.ceil((t(x) - lo + t(r)) * inv))
        b = min(b, last)
        if b < 0:
            return a, b, 1
        return a, b, None

    def inside(self, kx, x, r):                                                        # Frame.cc:704-708 (strict)
        t = self.t
        return abs(t(kx) - t(x)) < t(r)

    def ur_fails(self, qur, ur2, r):                                                   # ORBmatcher.cc:2041-2047 / :100-105
        t = self.t
        return abs(t(qur) - t(ur2)) > t(r)

    def chi2(self, ex, ey, er, sig):                                                   # ORBmatcher.cc:1530-1556, unfused in float
        t = self.t
        e2 = t(t(ex) * t(ex)) + t(t(ey) * t(ey))
        if er is not None:
            e2 = t(e2) + t(t(er) * t(er))
        return float(t(t(e2) * t(sig)))

    def sub(self, a, b):
        return self.t(a) - self.t(b)


F32, F64 = Arith(np.float32), Arith(np.float64)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def build_grid(kp, bounds, arith=F32):
    """cells[ix*ROWS+iy] = keypoint indices in insertion order; cell_of[i] = cell or -1 (outside the grid)"""
    lo_x, lo_y, inv_w, inv_h = arith.grid(bounds)
    cells = [[] for _ in range(COLS * ROWS)]
    cell_of = np.full(len(kp), -1, np.int64)
    for i in range(len(kp)):
        px, py = arith.cell(kp["x"][i], lo_x, inv_w), arith.cell(kp["y"][i], lo_y, inv_h)
        if 0 <= px < COLS and 0 <= py < ROWS:
            cell_of[i] = px * ROWS + py
            cells[px * ROWS + py].append(i)
    return cells, cell_of


def window(q, t, bounds, arith=F32):
    """(c0, c1, r0, r1) and the outcome name of the exit taken, or None"""
    lo_x, lo_y, inv_w, inv_h = arith.grid(bounds)
    c0, c1, e = arith.window(q["u"][t], q["radius"][t], lo_x, inv_w, COLS - 1)
    if e is not None:
        return (c0, c1, 0, 0), ("exit_c0", "exit_c1")[e]
    r0, r1, e = arith.window(q["v"][t], q["radius"][t], lo_y, inv_h, ROWS - 1)
    if e is not None:
        return (c0, c1, r0, r1), ("exit_r0", "exit_r1")[e]
    return (c0, c1, r0, r1), None


def in_window(cells, win):
    c0, c1, r0, r1 = win
    return [i for ix in range(c0, c1 + 1) for iy in range(r0, r1 + 1) for i in cells[ix * ROWS + iy]]


def _area_gates(q, t, kp, i, arith):
    """gate bits of keypoint i under GetFeaturesInArea (level modes of Frame.cc:676-701, then the strict square of :704-708)"""
    lo, hi, o = int(q["min_level"][t]), int(q["max_level"][t]), int(kp["octave"][i])
    if lo > 0 or hi >= 0:
        if o < lo:
            return G["lv_below"]
        if hi >= 0 and o > hi:
            return G["lv_above"]
    g = 0
    if not arith.inside(kp["x"][i], q["u"][t], q["radius"][t]):
        g |= G["dx"]
    if not arith.inside(kp["y"][i], q["v"][t], q["radius"][t]):
        g |= G["dy"]
    return g


def search(mode, q, dq, kp, d, u_right, bounds, tm, th_high, ratio=0.0, check_ori=False, nleft=None, mirror=None, arith=F32):
    """mode 0: frame to frame (rotation check when check_ori), mode 1: local map (ratio test, mirror rule).  nleft is None: one camera.
    Returns a dict: nm, tm, outcome [nq] (index into OUTCOMES), gates [nq], flags [nq], nstatic [nq], handback (bool), reasons (set)."""
    nq, n = len(q), len(kp)
    tm = np.asarray(tm, np.int32).copy(); tm[tm != -1] = -2
    rig = nleft is not None
    if rig:
        grids = [build_grid(kp[:nleft], bounds, arith)[0], build_grid(kp[nleft:], bounds, arith)[0]]
    else:
        grids = [build_grid(kp, bounds, arith)[0]]
    outcome = np.zeros(nq, np.int64); gates = np.zeros(nq, np.int64); flags = np.zeros(nq, np.int64); nstatic = np.zeros(nq, np.int64)
    obs = lambda h: bool(int(q["has_obs"][h]) & 1) if rig else bool(q["has_obs"][h])
    nm = 0
    hist = [[] for _ in range(30)]
    reasons = set()
    O = {nme: k for k, nme in enumerate(OUTCOMES)}
    for t in range(nq):
        cam = (int(q["has_obs"][t]) >> 1) & 1 if rig else 0
        off = nleft if cam else 0
        win, ex = window(q, t, bounds, arith)
        if ex is not None:
            outcome[t] = O[ex]; continue
        inw = [i + off for i in in_window(grids[cam], win)]
        if not inw:
            outcome[t] = O["empty"]; continue
        stat = []
        for i in inw:
            g = _area_gates(q, t, kp, i, arith)
            if not g:
                if tm[i] == -2:
                    g = G["preheld"]
                elif u_right is not None and u_right[i] > 0 and arith.ur_fails(q["ur"][t], u_right[i], q["radius"][t]):
                    g = G["uright"]
            gates[t] |= g
            if not g:
                stat.append(i)
        nstatic[t] = len(stat)
        dist = {i: hamming(dq[t], d[i]) for i in stat}
        # ---- what the replay form would do with this query (keys: distance, then visiting order)
        if not rig:
            if len(stat) > SBPL_BUF:
                reasons.add("buffer")
            elif len(stat) > SBPL_K:
                order = sorted(range(len(stat)), key=lambda k: (dist[stat[k]], k))[:SBPL_K]
                free = [stat[k] for k in order if not (tm[stat[k]] >= 0 and obs(tm[stat[k]]))]
                if not free:
                    reasons.add("best")
                elif dist[free[0]] <= th_high and dist[free[0]] < 256 and mode == 1 and len(free) < 2:
                    reasons.add("second")
        if not stat:
            outcome[t] = O["static"]; continue
        live = [i for i in stat if not (tm[i] >= 0 and obs(tm[i]))]                   # ORBmatcher.cc:2037-2039 / :96-98
        if not live:
            outcome[t] = O["held"]; continue
        b1, l1, b2, l2, bi = 256, -1, 256, -1, -1
        for i in live:
            if dist[i] < b1:
                b2, l2, b1, l1, bi = b1, l1, dist[i], int(kp["octave"][i]), i
            elif dist[i] < b2:
                b2, l2 = dist[i], int(kp["octave"][i])
        if b1 > th_high or bi < 0:                                                      # (bi < 0: nothing below 256; the reference would index [-1])
            outcome[t] = O["high"]; continue
        if mode == 1:
            if l1 == l2 and f32(b1) > f32(ratio) * f32(b2):                             # ORBmatcher.cc:131-137
                outcome[t] = O["ratio"]; continue
            if l2 == -1:
                flags[t] |= F["no_second"]
            elif l2 != l1:
                flags[t] |= F["second_other_octave"]
        outcome[t] = O["accept"]
        if sum(1 for i in live if dist[i] == b1) > 1:
            flags[t] |= F["tie"]
        if tm[bi] >= 0:
            flags[t] |= F["took_over"]; flags[tm[bi]] |= F["lost"]
        tm[bi] = t; nm += 1
        if mode == 1 and mirror is not None and mirror[bi] >= 0:                         # ORBmatcher.cc:142-146 / :203-207
            m = int(mirror[bi])
            flags[t] |= F["mirrored"]
            if tm[m] != -1:
                flags[t] |= F["mirror_overwrote"]
                if tm[m] >= 0:
                    flags[tm[m]] |= F["lost"]
            tm[m] = t; nm += 1
        if mode == 0 and check_ori:
            rot = f32(q["angle"][t]) - f32(kp["angle"][bi])
            if rot < 0:
                rot = f32(rot + f32(360.0))
            b = roundf(f32(rot * f32(1.0 / 30)))
            hist[0 if b == 30 else b].append((bi, t))
    if mode == 0 and check_ori:                                                          # ORBmatcher.cc:2156-2178, ComputeThreeMaxima :2307-2348
        sizes = [len(h) for h in hist]
        m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
        for i, s in enumerate(sizes):
            if s > m1: m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
            elif s > m2: m3, m2, i3, i2 = m2, s, i2, i
            elif s > m3: m3, i3 = s, i
        if m2 < f32(0.1) * f32(m1): i2 = i3 = -1
        elif m3 < f32(0.1) * f32(m1): i3 = -1
        for i in range(30):
            if i not in (i1, i2, i3):
                for bi, t in hist[i]:
                    tm[bi] = -1; nm -= 1; flags[t] |= F["rot_removed"]
    return dict(nm=nm, tm=tm, outcome=outcome, gates=gates, flags=flags, nstatic=nstatic, handback=bool(reasons), reasons=reasons)


def fuse(q, dq, kp, d, u_right, sig, bounds, arith=F32):
    """window search of Fuse: best index / distance per query, with outcome, gate bits and static candidate count"""
    nq = len(q)
    cells = build_grid(kp, bounds, arith)[0]
    bi = np.full(nq, -1, np.int32); bd = np.full(nq, 256, np.int32)
    outcome = np.zeros(nq, np.int64); gates = np.zeros(nq, np.int64); nstatic = np.zeros(nq, np.int64)
    O = {nme: k for k, nme in enumerate(OUTCOMES)}
    for t in range(nq):
        win, ex = window(q, t, bounds, arith)
        if ex is not None:
            outcome[t] = O[ex]; continue
        inw = in_window(cells, win)
        if not inw:
            outcome[t] = O["empty"]; continue
        for i in inw:
            # GetFeaturesInArea is called without levels (:1503): the square is tested first, the octave after it (:1527-1528, both ends always)
            lv = int(kp["octave"][i])
            gsq = 0
            if not arith.inside(kp["x"][i], q["u"][t], q["radius"][t]): gsq |= G["dx"]
            if not arith.inside(kp["y"][i], q["v"][t], q["radius"][t]): gsq |= G["dy"]
            if gsq:
                gates[t] |= gsq; continue
            if lv < q["min_level"][t]:
                gates[t] |= G["lv_below"]; continue
            if lv > q["max_level"][t]:
                gates[t] |= G["lv_above"]; continue
            ex_, ey_ = arith.sub(q["u"][t], kp["x"][i]), arith.sub(q["v"][t], kp["y"][i])
            if u_right is not None and u_right[i] >= 0:                                  # ORBmatcher.cc:1530-1545
                if arith.chi2(ex_, ey_, arith.sub(q["ur"][t], u_right[i]), sig[lv]) > 7.8:
                    gates[t] |= G["chi_stereo"]; continue
            elif arith.chi2(ex_, ey_, None, sig[lv]) > 5.99:                             # ORBmatcher.cc:1546-1556
                gates[t] |= G["chi_mono"]; continue
            nstatic[t] += 1
            dist = hamming(dq[t], d[i])
            if dist < bd[t]:
                bd[t], bi[t] = dist, i
        outcome[t] = O["static"] if nstatic[t] == 0 else O["high"] if bi[t] < 0 else O["accept"]
    return dict(bi=bi, bd=bd, outcome=outcome, gates=gates, nstatic=nstatic)


# ---- the restatements test_oracle_match_ba.py holds the C oracle to (results only)
def _sbp_python(q, dq, kp, d, u_right, bounds, tm, th_high, check_ori):
    r = search(0, q, dq, kp, d, u_right, bounds, tm, th_high, check_ori=check_ori)
    return r["nm"], r["tm"]


def _sbp_map_python(q, dq, kp, d, u_right, bounds, tm, th_high, ratio):
    r = search(1, q, dq, kp, d, u_right, bounds, tm, th_high, ratio=ratio)
    return r["nm"], r["tm"]


def _rig_sbp_python(mode, q, dq, kp, d, nleft, mirror, bounds, tm, th_high, ratio, check_ori):
    r = search(mode, q, dq, kp, d, None, bounds, tm, th_high, ratio=ratio, check_ori=check_ori, nleft=nleft, mirror=mirror)
    return r["nm"], r["tm"]


def _fuse_python(q, dq, kp, d, u_right, sig, bounds):
    r = fuse(q, dq, kp, d, u_right, sig, bounds)
    return r["bi"], r["bd"]
