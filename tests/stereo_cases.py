"""Crafted keypoint lists on real pyramids for Frame::ComputeStereoMatches (reference src/Frame.cc:802-980).

A case is a small real stereo pair, extracted by both extractors (so the pyramids are the real ones), whose keypoints, descriptors
and counts are then REPLACED by lists built here from blocks, each block aimed at one outcome or flag of tests/stereo_model.py:
Hamming distances around the 75 cut and the 100 start value, equal best distances (also across a multiple of 64 in right-index
order), the row band one row inside / outside each edge, the octave gate, the ends of the disparity window one ulp inside / outside,
strips at the left and right image border (reflected columns), SAD minima at -5 / +5 / outside both disparity gates, the 0.01 clamp,
equal SADs, and left / right counts around the wave and tile size of the kernel (0, 1, 63, 64, 65, 128, 129, 200).

Images (all from the synthetic scene generator):
  shifted   one constant disparity d (negative: the scene sits further RIGHT in the right view), +-2 noise on the right view
  same      left == right, no noise: every true match has SAD 0, the median is 0 and 0 < 0 fails, so the cut removes everything
  mirror    left == right below row 90 (noise above), with a band that is mirror-symmetric about column 160 (SAD(-k) == SAD(+k):
            deltaR == 0, disparity exactly 0, the clamp runs), a flat region (all 11 SADs equal: the first minimum is -5) and a
            region of vertical stripes of period 4 (SAD equal at shifts -4, 0, +4: the first minimum -4 is accepted, the last is not)
All cases use maxD = mbf / mb = 8 exactly.

SAFETY of the crafted input is part of the generator (check_safe, asserted before anything is uploaded): the device reads the
11 x 11 patch of every left keypoint that finds a candidate without a bounds check, which is right for extractor output.
  * every left keypoint: finite coordinates, octave in [0, nlevels), and 5 <= round(x inv) <= w_l - 6, 5 <= round(y inv) <= h_l - 6
    at its own level -- OR, for the three outcomes that only exist outside those bounds (a row outside the image, the last row,
    maxU < 0), NO right keypoint of its frame with x in [uL - maxD, uL]: such a keypoint can find no candidate whatever the gates
    of the code under test do, so its patch is never read.  (On the device these keypoints check that -1 is written and that
    they do not disturb their wave; the gates themselves are told apart by the oracle against the model.)
  * every right keypoint: finite coordinates, octave in range, x >= 0 -- OR -5 < x < 0 for the one block that reaches iniu < 0:
    even without that gate the strip's columns round(x inv) - 10 .. + 10 are reflected into [0, 15], inside every level.
  * counts <= max_keypoints.
No case relies on the device tolerating an out-of-image patch."""
import functools
import numpy as np

f32 = np.float32
MB, MBF = 5.0, 40.0                    # maxD = 8 exactly
MAXD = 8.0
NFEAT = 300
GEOMS = {"qvga8": (320, 240, 8), "qqvga4": (160, 120, 4)}      # level 7 of 320 x 240 is 89 x 67, just above the 30-pixel cell rule
HAMMING_K = (0, 49, 74, 75, 76, 99, 100)


def scale_table(nlevels):
    return np.cumprod(np.concatenate([[f32(1.0)], np.full(nlevels - 1, f32(1.2), f32)])).astype(f32)


def _rnd(v):
    v = np.float64(v)
    return int(np.sign(v) * np.floor(np.abs(v) + 0.5))


def level_dims(w, h, nlevels):
    isf = (f32(1.0) / scale_table(nlevels)).astype(f32)
    return [(int(np.rint(f32(f32(w) * s))), int(np.rint(f32(f32(h) * s)))) for s in isf]        # cvRound(width * inv), ORBextractor.cc:1156


# ------------------------------------------------------------------ images
def shifted_pair(w, h, d, seed, noise=True):
    import orbhip
    big = orbhip.synth_frames(w + 64, h, 1, seed=seed)[0]
    left = np.ascontiguousarray(big[:, 32:32 + w])
    right = big[:, 32 + d:32 + d + w].astype(np.int16)
    if noise:
        right = right + np.random.default_rng(seed + 1).integers(-2, 3, right.shape)
    return left, np.ascontiguousarray(np.clip(right, 0, 255).astype(np.uint8))


MIRROR_AXIS, MIRROR_ROWS = 160, (96, 157)
FLAT_BOX, STRIPE_BOX = (20, 141, 170, 236), (180, 301, 170, 236)          # x0, x1, y0, y1


def mirror_pair(seed):
    import orbhip
    left = orbhip.synth_frames(320, 240, 1, seed=seed)[0].copy()
    r0, r1 = MIRROR_ROWS
    for k in range(1, 41):
        left[r0:r1, MIRROR_AXIS + k] = left[r0:r1, MIRROR_AXIS - k]
    x0, x1, y0, y1 = FLAT_BOX
    left[y0:y1, x0:x1] = 90
    x0, x1, y0, y1 = STRIPE_BOX
    left[y0:y1, x0:x1] = np.array([60, 140, 200, 100], np.uint8)[np.arange(x0, x1) % 4][None, :]
    right = left.astype(np.int16)
    right[:90] += np.random.default_rng(seed + 1).integers(-2, 3, right[:90].shape)
    return left, np.clip(right, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ one frame's lists
class _Lists:
    def __init__(self, geom, seed, d_cand):
        self.w, self.h, self.nlevels = GEOMS[geom]
        self.sf = scale_table(self.nlevels)
        self.rng = np.random.default_rng(seed)
        self.d_cand = d_cand
        self.L, self.R, self.pins = [], [], {}
        ystep = 12 if self.h >= 240 else 10
        self.cols = list(range(24, self.w - 23, 24))
        self.slots = [(cx, cy) for cy in range(18, self.h - 17, ystep) for cx in self.cols]
        self.slots.reverse()                                        # pop() hands them out top-left first

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flip(self, d, k):
        bits = np.unpackbits(d)
        bits[self.rng.choice(256, k, replace=False)] ^= 1
        return np.packbits(bits)

    def addL(self, x, y, o, d):
        self.L.append((f32(x), f32(y), int(o), d)); return len(self.L) - 1

    def addR(self, x, y, o, d, pin=None):
        if pin is None:
            self.R.append((f32(x), f32(y), int(o), d))
        else:
            assert pin not in self.pins
            self.pins[pin] = (f32(x), f32(y), int(o), d)

    def slot(self, max_y=None):
        while True:
            cx, cy = self.slots.pop()
            if max_y is None or cy <= max_y:
                return cx, cy

    def octave(self):
        return int(self.rng.integers(0, 4))

    # ---- blocks
    def ham(self, k, o=None, d_cand=None, frac=0.0, max_y=None):
        """a left descriptor = its right one with k bits flipped; the right keypoint d_cand pixels to the left"""
        cx, cy = self.slot(max_y); o = self.octave() if o is None else o
        rd = self.desc()
        self.addR(cx + frac - (self.d_cand if d_cand is None else d_cand), cy, o, rd)
        return self.addL(cx + frac, cy, o, self.flip(rd, k))

    def tie(self, pins=None, k=30):
        """two right keypoints at equal distance in one band, the first d_cand to the left (the true match), the second at the far
        end of the window (no true match there): first-best-wins decides the result"""
        cx, cy = self.slot(); rd = self.desc(); ld = self.flip(rd, k)
        rd2 = self.flip(ld, k)
        pa, pb = pins if pins else (None, None)
        self.addR(cx - self.d_cand, cy, 0, rd, pa); self.addR(cx - 8, cy, 0, rd2, pb)
        return self.addL(cx, cy, 0, ld)

    def rowband(self, edge, inside, frac, o):
        cx, cy = self.slot(); rd = self.desc()
        yR = f32(cy + (0.37 if frac else 0.0)); r = f32(f32(2.0) * self.sf[o])
        lo, hi = int(np.floor(f32(yR - r))), int(np.ceil(f32(yR + r)))
        vL = {("lo", True): lo, ("lo", False): lo - 0.25, ("hi", True): hi + 0.75, ("hi", False): hi + 1}[(edge, inside)]
        self.addR(cx - self.d_cand, yR, o, rd)
        return self.addL(cx, vL, o, self.flip(rd, 20))

    def octave_gate(self, delta):
        cx, cy = self.slot(); rd = self.desc(); oL = 2 if delta < 0 else 1
        self.addR(cx - self.d_cand, cy, oL + delta, rd)
        return self.addL(cx, cy, oL, self.flip(rd, 20))

    def window(self, kind):
        cx, cy = self.slot(); rd = self.desc(); uL = f32(cx)
        x = {"at_uL": uL, "above_uL": np.nextafter(uL, f32(np.inf)), "at_min": f32(uL - f32(MAXD)),
             "below_min": np.nextafter(f32(uL - f32(MAXD)), f32(-np.inf))}[kind]
        self.addR(x, cy, 0, rd)
        return self.addL(uL, cy, 0, self.flip(rd, 20))

    def strip_left(self, cr, o):
        """right keypoint with round(x inv) == cr at the left keypoint's level: the strip starts at column cr - 10"""
        _, cy = self.slot(); rd = self.desc(); inv = f32(1.0) / self.sf[o]
        x = f32(cr * self.sf[o])
        assert _rnd(f32(x * inv)) == cr
        uL = f32(max(float(x) + 2.0, 5.5 * float(self.sf[o])))
        assert x >= uL - MAXD and _rnd(f32(uL * inv)) >= 5
        self.addR(x, cy, o, rd)
        return self.addL(uL, cy, o, self.flip(rd, 20))

    def strip_negative(self):
        _, cy = self.slot(); rd = self.desc()
        self.addR(-0.75, cy, 0, rd)                                  # round(-0.75) = -1: iniu < 0
        return self.addL(5.0, cy, 0, self.flip(rd, 20))

    def strip_right(self, off, o=0):
        _, cy = self.slot(); rd = self.desc(); inv = f32(1.0) / self.sf[o]
        wl = level_dims(self.w, self.h, self.nlevels)[o][0]
        x, uL = f32((wl - off) * self.sf[o]), f32((wl - off + 2) * self.sf[o])
        assert _rnd(f32(x * inv)) == wl - off and _rnd(f32(uL * inv)) == wl - off + 2      # endu = wl - off + 11 >= wl  <=>  off <= 11
        self.addR(x, cy, o, rd)
        return self.addL(uL, cy, o, self.flip(rd, 20))

    def no_window(self, x_off, y):
        """a left keypoint outside the patch bounds, in the column gap where no right keypoint lies in its disparity window"""
        cx, _ = self.slot()
        return self.addL(cx + x_off, y, 0, self.desc())

    def filler_left(self):
        return self.addL(int(self.rng.integers(24, self.w - 23)) + float(self.rng.choice([0.0, 0.25, 0.5])),
                         int(self.rng.integers(12, self.h - 11)) + float(self.rng.choice([0.0, 0.5])), self.octave(), self.desc())

    def filler_right(self):
        self.addR(int(self.rng.choice(self.cols)) + 14, float(self.rng.integers(0, self.h)) + float(self.rng.choice([0.0, 0.3])),
                  int(self.rng.integers(0, self.nlevels)), self.desc())

    def finish(self, nL, nR, left_order=None):
        assert len(self.L) <= nL and len(self.R) + len(self.pins) <= nR, (len(self.L), nL, len(self.R), len(self.pins), nR)
        while len(self.L) < nL:
            self.filler_left()
        while len(self.R) + len(self.pins) < nR:
            self.filler_right()
        L = self.L if left_order is None else [self.L[i] for i in left_order]
        rest = list(self.R)
        order = list(self.rng.permutation(len(rest)))                # right order is free: shuffle, then put the pinned ones in place
        R = []
        for i in range(nR):
            R.append(self.pins[i] if i in self.pins else rest[order.pop()])
        return _pack(L), _pack(R)


def _pack(items):
    import orbhip
    kp = np.zeros(len(items), orbhip.KP_DTYPE); desc = np.zeros((len(items), 32), np.uint8)
    for i, (x, y, o, d) in enumerate(items):
        kp[i] = (x, y, 31.0 * 1.2 ** o, 0.0, 50.0, o, -1); desc[i] = d
    return kp, desc


GOOD_K = (0, 10, 30, 49)


def _goods(b, n, **kw):
    return [b.ham(GOOD_K[i % 4], frac=(0.0, 0.5, 0.25)[i % 3], **kw) for i in range(n)]


# ------------------------------------------------------------------ the frames
def _frame(name, geom, pair, lists):
    (kpL, dL), (kpR, dR) = lists
    return dict(name=name, geom=geom, left=pair[0], right=pair[1], kpL=kpL, dL=dL, kpR=kpR, dR=dR)


def _mix(geom, seed, nL, nR, full):
    """every gate block on a disparity-2 pair (candidates 2 to the left: the true place; 8 to the left: none)"""
    b = _Lists(geom, seed, 2)
    w, h, nlev = GEOMS[geom]
    for k in HAMMING_K:
        for o in ((0, 2) if full else (1,)):
            b.ham(k, o=o)
    b.tie(); b.tie(k=60)
    b.tie(pins=(63, 64))
    if nR > 128:
        b.tie(pins=(127, 128))
    for edge in ("lo", "hi"):
        for inside in (True, False):
            for frac in ((False, True) if full else (True,)):
                for o in ((0, 1, 2, 3) if full else (0, 3)):
                    b.rowband(edge, inside, frac, o)
    for delta in (-2, -1, 1, 2):
        b.octave_gate(delta)
    for kind in ("at_uL", "above_uL", "at_min", "below_min"):
        b.window(kind)
    for cr in (0, 4, 9, 10):
        for o in ((0, 1) if full else (0,)):
            b.strip_left(cr, o)
    b.strip_negative(); b.strip_negative()
    for off in (12, 11):
        for o in ((0, 1) if full else (0,)):
            b.strip_right(off, o)
    for _ in range(3):
        b.ham(0, o=0, d_cand=7)                                      # the true place 5 to the right of the candidate: shift +5
    _goods(b, min(nL - len(b.L), nR - len(b.R) - len(b.pins), len(b.slots)) - 2)
    return _frame("mix%d_%s" % (nL, geom), geom, shifted_pair(w, h, 2, seed), b.finish(nL, nR))


@functools.lru_cache(maxsize=None)
def frames(geom):
    w, h, nlev = GEOMS[geom]
    out = []
    if geom == "qvga8":
        out.append(_mix(geom, 101, 200, 129, True))
        b = _Lists(geom, 102, 0); _goods(b, 60); b.tie(pins=(63, 64))                        # the scene 3 px further right: disparity < 0
        out.append(_frame("neg65", geom, shifted_pair(w, h, -3, 102), b.finish(65, 65)))
        b = _Lists(geom, 103, 8); _goods(b, 50)                                              # true disparity 10 >= maxD
        for _ in range(4):
            b.ham(0, o=0, d_cand=5)                                                          # ... and 5 to the left of the candidate: shift -5
        out.append(_frame("far63", geom, shifted_pair(w, h, 10, 103), b.finish(63, 64)))
        b = _Lists(geom, 104, 0)
        for y in (102, 113, 124, 135, 146, 150):                                             # on the mirror axis: the clamp
            rd = b.desc(); b.addR(MIRROR_AXIS, y, 0, rd); b.addL(MIRROR_AXIS, y, 0, b.flip(rd, 10))
        for i in range(6):                                                                   # flat: all SADs equal
            rd = b.desc(); x, y = 40 + 14 * i, 178 + 9 * i; b.addR(x, y, 0, rd); b.addL(x, y, 0, b.flip(rd, 10))
        for i in range(6):                                                                   # stripes of period 4: equal SADs at -4, 0, +4
            rd = b.desc(); x, y = 200 + 13 * i, 226 - 9 * i; b.addR(x, y, 0, rd); b.addL(x, y, 0, b.flip(rd, 10))
        _goods(b, 70, max_y=80)
        out.append(_frame("mirror128", geom, mirror_pair(104), b.finish(128, 129)))
        b = _Lists(geom, 105, 0); _goods(b, 64)                                              # median 0: everything removed
        out.append(_frame("same64", geom, shifted_pair(w, h, 0, 105, noise=False), b.finish(64, 64)))
        b = _Lists(geom, 106, 3)                                                             # only the last lane of the wave matches
        b.no_window(12, h + 0.5); b.no_window(12, -1.5); b.no_window(12, h); b.no_window(12, 2 * h)      # rows outside the image
        b.no_window(12, h - 1); b.no_window(12, h - 0.25)                                                  # the last row
        for _ in range(4):                                                                                 # maxU < 0, with a right keypoint in its row
            cx, cy = b.slot(); b.addR(cx + 14, cy, 0, b.desc()); b.addL(-1.0, cy, 0, b.desc())
        while len(b.L) < 63:
            b.filler_left()
        b.ham(0, o=1)
        out.append(_frame("lane63", geom, shifted_pair(w, h, 3, 106), b.finish(64, 65)))
        b = _Lists(geom, 107, 3); b.ham(10, o=0)                                             # V = 1 through the counts
        out.append(_frame("one", geom, shifted_pair(w, h, 3, 107), b.finish(1, 1)))
        b = _Lists(geom, 108, 3)
        out.append(_frame("noleft", geom, shifted_pair(w, h, 3, 108), b.finish(0, 64)))
        b = _Lists(geom, 109, 3)
        out.append(_frame("noright", geom, shifted_pair(w, h, 3, 109), b.finish(65, 0)))
        b = _Lists(geom, 110, 0)                                                             # V = 2: SADs 0 (mirror axis) and > 0 (noise): the rank of the median decides
        rd = b.desc(); b.addR(MIRROR_AXIS, 124, 0, rd); b.addL(MIRROR_AXIS, 124, 0, b.flip(rd, 10)); b.ham(30, o=0, max_y=70)
        out.append(_frame("two63", geom, mirror_pair(110), b.finish(63, 64, left_order=[2 + i for i in range(5)] + [0] +
                                                                              [7 + i for i in range(34)] + [1] + [41 + i for i in range(22)])))
        b = _Lists(geom, 111, 3); _goods(b, 128)                                             # two full ballots
        out.append(_frame("full128", geom, shifted_pair(w, h, 3, 111), b.finish(128, 129)))
        b = _Lists(geom, 112, 4); _goods(b, 65)                                              # a full ballot, then lane 0 alone
        out.append(_frame("full65", geom, shifted_pair(w, h, 4, 112), b.finish(65, 65)))
    else:
        out.append(_mix(geom, 201, 65, 65, False))
        b = _Lists(geom, 202, 0); _goods(b, 40)
        out.append(_frame("s_neg63", geom, shifted_pair(w, h, -3, 202), b.finish(63, 64)))
        b = _Lists(geom, 203, 0); _goods(b, 45)
        out.append(_frame("s_same64", geom, shifted_pair(w, h, 0, 203, noise=False), b.finish(64, 64)))
        b = _Lists(geom, 204, 3); b.ham(49, o=3)
        out.append(_frame("s_one", geom, shifted_pair(w, h, 3, 204), b.finish(1, 1)))
        b = _Lists(geom, 205, 3)
        out.append(_frame("s_noleft", geom, shifted_pair(w, h, 3, 205), b.finish(0, 1)))
        b = _Lists(geom, 206, 3)
        out.append(_frame("s_noright", geom, shifted_pair(w, h, 3, 206), b.finish(64, 0)))
        b = _Lists(geom, 207, 3); _goods(b, 45)
        out.append(_frame("s_full", geom, shifted_pair(w, h, 3, 207), b.finish(50, 129)))
    for fr in out:
        check_safe(fr, NFEAT)
    return tuple(out)


def batches(geom):
    """the frames in batches of 6 - 7: frames of differing counts side by side, a zero-left and a zero-right one in each"""
    fr = {f["name"]: f for f in frames(geom)}
    if geom == "qvga8":
        names = [["mix200_qvga8", "noleft", "neg65", "noright", "far63", "one", "lane63"],
                 ["mirror128", "noright", "same64", "two63", "noleft", "full128", "full65"]]
    else:
        names = [["mix65_qqvga4", "s_noleft", "s_neg63", "s_noright", "s_same64", "s_one", "s_full"]]
    return [[fr[n] for n in b] for b in names]


# ------------------------------------------------------------------ safety
def check_safe(fr, max_kp):
    w, h, nlev = GEOMS[fr["geom"]]
    sf = scale_table(nlev); isf = (f32(1.0) / sf).astype(f32); dims = level_dims(w, h, nlev)
    kpL, kpR = fr["kpL"], fr["kpR"]
    assert len(kpL) <= max_kp and len(kpR) <= max_kp, (fr["name"], len(kpL), len(kpR), max_kp)
    assert len(fr["dL"]) == len(kpL) and len(fr["dR"]) == len(kpR)
    for k in (kpL, kpR):
        assert np.isfinite(k["x"]).all() and np.isfinite(k["y"]).all() and ((k["octave"] >= 0) & (k["octave"] < nlev)).all(), fr["name"]
    assert (kpR["x"] > -5).all(), fr["name"]
    assert ((kpR["x"] >= 0) | (kpR["octave"] == 0)).all(), fr["name"]
    for i in range(len(kpL)):
        x, y, o = kpL["x"][i], kpL["y"][i], int(kpL["octave"][i])
        cu, cv = _rnd(f32(x * isf[o])), _rnd(f32(y * isf[o]))
        if 5 <= cu <= dims[o][0] - 6 and 5 <= cv <= dims[o][1] - 6:
            continue
        # outside the patch bounds: no right keypoint may lie in (a generous superset of) its disparity window
        assert not ((kpR["x"] >= x - f32(MAXD) - 1) & (kpR["x"] <= x + 1)).any(), (fr["name"], i, x, y, o)


# ------------------------------------------------------------------ the two sides
def oracle_frame(fr):
    """the oracle's extractors after extracting the pair (their pyramids are what its stereo call reads), the expected result of
    the CRAFTED lists, and the padded pyramids for the model"""
    import oracle_bind as ob
    w, h, nlev = GEOMS[fr["geom"]]
    eL = ob.OracleExtractor(NFEAT, 1.2, nlev, 20, 7); eR = ob.OracleExtractor(NFEAT, 1.2, nlev, 20, 7)
    realL = eL.extract(fr["left"], (0, 0)); realR = eR.extract(fr["right"], (0, 0))
    kept, ur, dp, sad = ob.compute_stereo_matches(eL, eR, fr["kpL"], fr["dL"], fr["kpR"], fr["dR"], MB, MBF)
    pyrL = [eL.pyramid_level(l, padded=True) for l in range(nlev)]; pyrR = [eR.pyramid_level(l, padded=True) for l in range(nlev)]
    return dict(kept=kept, ur=ur, dp=dp, sad=sad, pyrL=pyrL, pyrR=pyrR, realL=realL, realR=realR, eL=eL, eR=eR)


@functools.lru_cache(maxsize=None)
def oracle_results(geom):
    """oracle_frame of every frame of the geometry, by name: computed once, shared by the tests, never changed"""
    return {fr["name"]: oracle_frame(fr) for fr in frames(geom)}


_hip = None


def hip_runtime():
    global _hip
    if _hip is None:
        import ctypes as C
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def upload_lists(ext, side, batch):
    """overwrite keypoints, descriptors and counts of the extractor's latest extraction (frame f <- batch[f]) through the device
    pointers of results_device(); the caller has synchronised the extractor's context.  Entries beyond a frame's new count stay
    what the extraction left there."""
    hip = hip_runtime()
    kp_p, desc_p, cnt_p, _ = ext.results_device()
    mk = ext.max_keypoints
    for f, fr in enumerate(batch):
        check_safe(fr, mk)
        kp = np.ascontiguousarray(fr["kp" + side]); d = np.ascontiguousarray(fr["d" + side])
        if len(kp):
            assert hip.hipMemcpy(kp_p + f * mk * kp.dtype.itemsize, kp.ctypes.data, kp.nbytes, 1) == 0
            assert hip.hipMemcpy(desc_p + f * mk * 32, d.ctypes.data, d.nbytes, 1) == 0
    cnt = np.array([len(fr["kp" + side]) for fr in batch], np.int32)
    assert hip.hipMemcpy(cnt_p, cnt.ctypes.data, cnt.nbytes, 1) == 0
