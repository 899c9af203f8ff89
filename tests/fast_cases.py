"""Crafted images for the per-cell FAST stage: blocks on a flat background, each declaring for named pixels exactly one outcome.

A block is a ring (radius 3) drawn around a centre pixel, or a stored 9 x 9 patch holding two adjacent corners.  What a block changes
lies within 3 (patch: 4) pixels of its centre, so a pixel further than 6 (7) away scores as on the flat background; blocks are spaced so
that no declared pixel, and none of its eight neighbours, has another block's pixels on its ring.  The eight neighbours of a ring block's
centre are never corners (a ring shifted by one pixel shares at most two adjacent pixels with the ring), so an isolated centre always
survives the NMS.  By-product corners (ring pixels that are isolated bright dots themselves, ...) are left to the model.

Coordinates are candidate coordinates throughout: relative to the detection origin, image pixel (x + 16, y + 16).

Outcomes:
  KEPT(score)        in the list with that score
  NMS_LOST           a corner at the cell's threshold, not in the list: a neighbour of the same cell scores at least as much
  ARC_SHORT          not a corner at any threshold: its longest arc has 8 pixels
  AT_THRESHOLD       its arc score equals the threshold of the pass (meta th): not a corner
  OUT_OF_BAND        a strong corner outside every cell's band (apron of a clipped cell, a skipped cell, the image margin)
  WEAK_KEPT(score)   score + 1 <= iniThFAST: kept only because its cell was empty at iniThFAST
  WEAK_DROPPED       a corner at minThFAST only, in a cell that is not empty at iniThFAST
"""
import functools
import numpy as np

BG = 100
OUTCOMES = ("KEPT", "NMS_LOST", "ARC_SHORT", "AT_THRESHOLD", "OUT_OF_BAND", "WEAK_KEPT", "WEAK_DROPPED")
# ring in cv::makeOffsets order (restated; tests check it against the model's)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

# Geometries: image size, the cell grid (ncols, nrows, wcell, hcell) it must give, the instance k_fast_cells must select (0 large cells,
# 1 small cells: every cell at most 40 x 36) and the one ORBHIP_FAST_KERNEL=runs must select (2 k_fast_runs<4>, 3 k_fast_runs<6>: cells of
# more than 45 rows), cells per run (2 while 2 * wcell <= 64), and the rows run on it.
ALL_ROWS = ("arcs", "thresholds", "nms", "seams", "retry", "load")
GEOMS = {
    # 2 x 2 cells of 32: one run of two cells per cell row; last column / row clipped to 26
    "g96": dict(w=96, h=96, grid=(2, 2, 32, 32), inst=1, runs=2, rpc=2, rows=ALL_ROWS),
    # 3 x 2 cells, wcell 31: a two-cell run followed by a one-cell run; the last column's band is odd (dw 23); last row dh 26
    "g123": dict(w=123, h=97, grid=(3, 2, 31, 33), inst=1, runs=2, rpc=2, rows=ALL_ROWS),
    # 2 x 2 cells of 43 x 34: one cell per run; dw 37 (odd) in the last column
    "g118": dict(w=118, h=100, grid=(2, 2, 43, 34), inst=0, runs=2, rpc=1, rows=ALL_ROWS),
    # one 58 x 58 cell (band 52 x 52), the widest the library accepts: k_fast_runs<6>
    "g90": dict(w=90, h=90, grid=(1, 1, 58, 58), inst=0, runs=3, rpc=1, rows=ALL_ROWS),
    # 30 columns of 31, the last one skipped (ini_x = 915 >= max_bx - 6 = 911), column 28 clipped to dw 27; one cell row of 43 (band 37):
    # 43 > 36 rows, so the LARGE instance (the small one takes cells of at most 36 rows)
    "g933": dict(w=933, h=75, grid=(30, 1, 31, 43), inst=0, runs=2, rpc=2, rows=ALL_ROWS),
    # the same columns with two cell rows of 33: the skipped column under the small instance
    "g933s": dict(w=933, h=97, grid=(30, 2, 31, 33), inst=1, runs=2, rpc=2, rows=ALL_ROWS),
    # ... and with one cell row of 49 (band 43: the two half waves of k_fast_runs get 22 and 21 rows): the skipped column, clipped and odd
    # bands and two-cell runs under k_fast_runs<6>
    "g933t": dict(w=933, h=81, grid=(30, 1, 31, 49), inst=0, runs=3, rpc=2, rows=ALL_ROWS),
    # 903 is the smallest height (75 .. 1100, found by search over the cell grid: test_fast_cases.py repeats the search) whose last cell row
    # is skipped: 29 rows of 31, ini_y = 16 + 28 * 31 = 884 >= max_by - 3 = 884.  512 wide, since the octree behind FAST is undefined below
    # nIni = round(width / height) = 1.  435 cells a frame, so only the frames that bear on the skipped row: the band edges of every cell
    # and the strong corners outside the bands (every cell otherwise empty); the other rows have the small instance's geometries above
    "g903": dict(w=512, h=903, grid=(16, 29, 30, 31), inst=1, runs=2, rpc=2, rows=("outside",)),
    # 30 x 3 cells of 31 x 31 whose second pyramid level (778 x 104: 24 x 2 cells of 32 x 36) keeps the small instance: the batch of the chunk test
    "g933c": dict(w=933, h=125, grid=(30, 3, 31, 31), inst=1, runs=2, rpc=2, rows=("outside", "retry")),
}
PARAMS = ((20, 7), (7, 7), (7, 20))        # (iniThFAST, minThFAST); the last one has ini below min

# Adjacent corners with chosen scores, found by search_nms_patches(seed 1) below and stored: 9 x 9 bytes, A = the centre pixel (4, 4),
# B = A + direction, (score of A, score of B) at any threshold below them.  'gt': A is the strict maximum of its 3 x 3 and B would be kept
# were A masked off; 'eq': equal scores, each below nobody else.  np.rot90 gives the other directions (FAST is invariant under it).
NMS_PATCHES = {
    ("E", "gt"): ((1, 0), 74, 73, b'ddddddddddddddddddddddddddddddddddddd\x19\x1a\x1b\x19\x1addddd\x18\x1b\x1b\x1bdddddd\x1a\x19\x19ddddddd\x19\x18dddddddd\x19ddd'),
    ("E", "eq"): ((1, 0), 68, 68, b'%\x1f%\x1f%!ddd#!!!%!ddd###%%\x1fddd!!%%##ddd%#%!\x1f\x1fddddddddddddddddddddddddddddddddddddddd'),
    ("SE", "gt"): ((1, 1), 39, 31, b'ddddddddddddddddddddddddddd@<@DH@ddd<<DH<Hddd<<@DHDdddDH<@@HdddH<<D@@ddd<HHH@Hddd'),
    ("SE", "eq"): ((1, 1), 115, 115, b'\xc9\xd3\xce\xd8\xce\xd3ddd\xce\xc9\xce\xce\xce\xceddd\xd3\xc9\xce\xce\xd3\xd3ddd\xce\xc9\xd3\xce\xd8\xc9ddd\xce\xc9\xce\xce\xd8\xc9ddd\xd3\xd3\xd8\xce\xce\xd8dddddddddddddddddddddddddddddd'),
}


def search_nms_patches(score_map, seed=1, tries=200000):
    """How NMS_PATCHES was found (not run by the tests): random wedges on the background until the two named pixels have the wanted
    relation.  score_map(img, th) -> per-pixel cornerScore (0 where not a corner), e.g. from the model."""
    out = {}
    for name, (dx, dy) in (("E", (1, 0)), ("SE", (1, 1))):
        for rel in ("gt", "eq"):
            rng = np.random.default_rng(seed)
            C = 12
            for _ in range(tries):
                img = np.full((25, 25), BG, np.uint8)
                p = np.full((9, 9), BG, np.int32)
                ax, ay = rng.integers(2, 7, 2)
                sx, sy = rng.choice([-1, 1], 2)
                amp = int(rng.integers(40, 120)) * int(rng.choice([-1, 1]))
                yy, xx = np.mgrid[0:9, 0:9]
                m = ((xx - ax) * sx >= 0) & ((yy - ay) * sy >= 0)
                if rng.random() < 0.5:
                    m &= ((xx - ax) * sx + (yy - ay) * sy) <= rng.integers(2, 8)
                p[m] = BG + amp + rng.integers(0, 4, m.sum()) * rng.integers(0, 6)
                img[C - 4:C + 5, C - 4:C + 5] = np.clip(p, 0, 255)
                sc = score_map(img, 20)
                a, b = sc[C, C], sc[C + dy, C + dx]
                if a <= 0 or b <= 0 or (rel == "gt" and not a > b) or (rel == "eq" and a != b):
                    continue
                nb_a = [sc[C + j, C + i] for j in (-1, 0, 1) for i in (-1, 0, 1) if (i or j) and (rel == "gt" or (i, j) != (dx, dy))]
                nb_b = [sc[C + dy + j, C + dx + i] for j in (-1, 0, 1) for i in (-1, 0, 1) if (i or j) and (i + dx, j + dy) != (0, 0)]
                if all(v < a for v in nb_a) and all(v < b for v in nb_b):
                    out[(name, rel)] = ((dx, dy), int(a), int(b), np.clip(p, 0, 255).astype(np.uint8).tobytes())
                    break
    return out


def nms_patch(base, rel, k):
    """(direction, score A, score B, 9 x 9 array) of a stored patch turned k times by 90 degrees (counter-clockwise on the image, y down:
    direction (dx, dy) -> (dy, -dx))"""
    (dx, dy), a, b, raw = NMS_PATCHES[(base, rel)]
    p = np.frombuffer(raw, np.uint8).reshape(9, 9)
    for _ in range(k):
        dx, dy = dy, -dx
    return (dx, dy), a, b, np.rot90(p, k)


# ---------------------------------------------------------------------------------- geometry (restated from the grid literals above)
def band(g, ci, cj):
    """(x0, y0, dw, dh) of cell (ci, cj) in candidate coordinates; dw = dh = 0: skipped"""
    ncols, nrows, wcell, hcell = g["grid"]
    aw, ah = g["w"] - 32, g["h"] - 32                     # detection area
    if cj * wcell >= aw - 6 or ci * hcell >= ah - 3:
        return cj * wcell + 3, ci * hcell + 3, 0, 0
    dw, dh = min(wcell, aw - cj * wcell - 6), min(hcell, ah - ci * hcell - 6)
    if dw <= 0 or dh <= 0:
        dw = dh = 0
    return cj * wcell + 3, ci * hcell + 3, dw, dh


def live_cells(g):
    return [(ci, cj) for ci in range(g["grid"][1]) for cj in range(g["grid"][0]) if band(g, ci, cj)[2] > 0]


def cell_of(g, x, y):
    """(ci, cj) of the cell whose band holds candidate pixel (x, y), or None"""
    for ci, cj in live_cells(g):
        x0, y0, dw, dh = band(g, ci, cj)
        if x0 <= x < x0 + dw and y0 <= y < y0 + dh:
            return ci, cj
    return None


class Frame:
    def __init__(self, geom, name, ini=20, mn=7):
        self.geom, self.g, self.name, self.ini, self.mn = geom, GEOMS[geom], name, ini, mn
        self.img = np.full((self.g["h"], self.g["w"]), BG, np.uint8)
        self.decl = []                                    # (x, y, outcome, score or None, meta dict)

    def set(self, x, y, v):
        assert 0 <= x + 16 < self.g["w"] and 0 <= y + 16 < self.g["h"] and 0 <= v <= 255, (self.name, x, y, v)
        self.img[y + 16, x + 16] = v

    def put(self, cx, cy, block):
        for dx, dy, v in block["pixels"]:
            self.set(cx + dx, cy + dy, v)
        for dx, dy, outcome, score, meta in block["decl"]:
            assert outcome in OUTCOMES
            self.decl.append((cx + dx, cy + dy, outcome, score, dict(meta, th=meta.get("th", self.ini))))


# ---------------------------------------------------------------------------------- blocks
def arc_block(pol, L, s, wi, wd, step=2, outcome=None, centre=BG):
    """Ring pixels (s + i) % 16, i < L, differ from the centre by wd + step * ((i - wi) % L) (distinct levels, the weakest at arc index
    wi), brighter for pol = +1, darker for -1; the other ring pixels equal the centre.  Declared score: the best 9-window of the arc,
    min |diff| - 1; no window: ARC_SHORT."""
    d = [wd + step * ((i - wi) % L) for i in range(L)]
    pixels = [(RING[(s + i) % 16][0], RING[(s + i) % 16][1], centre + pol * d[i]) for i in range(L)]
    if centre != BG:
        pixels.append((0, 0, centre))
    starts = range(16) if L == 16 else range(L - 8)
    best, weakest = None, None
    for t in starts:
        win = [(d[(t + j) % L], (t + j) % L) for j in range(9)] if L >= 9 else []
        if win and (best is None or min(win)[0] > best):
            best, weakest = min(win)[0], (s + min(win)[1]) % 16
    meta = dict(kind="arc", pol=pol, L=L, start=s, weakest=weakest)
    if best is None:
        return dict(pixels=pixels, decl=[(0, 0, "ARC_SHORT", None, meta)])
    return dict(pixels=pixels, decl=[(0, 0, outcome or "KEPT", best - 1, meta)])


def redeclare(block, outcome, score="same", **meta):
    dx, dy, _, sc, m = block["decl"][0]
    return dict(pixels=block["pixels"], decl=[(dx, dy, outcome, sc if score == "same" else score, dict(m, **meta))])


def pair_block(base, rel, k, across=False):
    """The stored patch as a block centred on A.  Inside one cell: 'gt' -> A KEPT, B NMS_LOST; 'eq' -> both NMS_LOST.  With a cell seam
    between A and B (across): both KEPT, NMS never crosses cells."""
    (dx, dy), a, b, p = nms_patch(base, rel, k)
    pixels = [(i - 4, j - 4, int(p[j, i])) for j in range(9) for i in range(9) if p[j, i] != BG]
    mA, mB = dict(kind="pair", rel=rel, dir=(dx, dy), who="A"), dict(kind="pair", rel=rel, dir=(dx, dy), who="B")
    if across:
        decl = [(0, 0, "KEPT", a, mA), (dx, dy, "KEPT", b, mB)]
    elif rel == "gt":
        decl = [(0, 0, "KEPT", a, mA), (dx, dy, "NMS_LOST", None, mB)]
    else:
        decl = [(0, 0, "NMS_LOST", None, mA), (dx, dy, "NMS_LOST", None, mB)]
    return dict(pixels=pixels, decl=decl, dir=(dx, dy))


def all_pair_blocks(across=False):
    return [pair_block(base, rel, k, across) for base in ("E", "SE") for rel in ("gt", "eq") for k in range(4)]


# ---------------------------------------------------------------------------------- layouts
def pool_frames(geom, name, blocks, ini, mn, spacing=8, offsets=((0, 0),), whole=0):
    """Blocks on a grid of that spacing over the bands of all cells, frame after frame; frame n shifts the grid by offsets[n % ..] (so that
    the blocks meet the pixel pairs and seams at different phases).  whole > 0: only slots whose (2 whole + 1)^2 surrounding lies in one
    cell's band (pairs that must meet in the NMS)."""
    g = GEOMS[geom]
    frames, todo = [], list(blocks)
    lives = live_cells(g)
    xs_end = max(band(g, ci, cj)[0] + band(g, ci, cj)[2] for ci, cj in lives)
    ys_end = max(band(g, ci, cj)[1] + band(g, ci, cj)[3] for ci, cj in lives)
    while todo:
        ox, oy = offsets[len(frames) % len(offsets)]
        fr = Frame(geom, "%s%d" % (name, len(frames)), ini, mn)
        for y in range(3 + whole + oy, ys_end - whole, spacing):
            for x in range(3 + whole + ox, xs_end - whole, spacing):
                if not todo:
                    break
                c = cell_of(g, x, y)
                if c is None or (whole and any(cell_of(g, x + i, y + j) != c for i in (-whole, whole) for j in (-whole, whole))):
                    continue
                fr.put(x, y, todo.pop(0))
        assert fr.decl, (geom, name)
        frames.append(fr)
    return frames


def cell_slots(g, ci, cj):
    """slots of a cell for blocks that must keep every by-product inside the cell's own band: 6 pixels from its edges, 8 apart"""
    x0, y0, dw, dh = band(g, ci, cj)
    return [(x0 + i, y0 + j) for j in range(6, dh - 6, 8) for i in range(6, dw - 6, 8)]


def group_frames(geom, name, groups, ini, mn):
    """every group (at most 4 blocks) alone in a cell of its own; cells left over stay flat (empty after both passes)"""
    g = GEOMS[geom]
    frames, todo = [], list(groups)
    while todo:
        fr = Frame(geom, "%s%d" % (name, len(frames)), ini, mn)
        for ci, cj in live_cells(g):
            if not todo:
                break
            slots = cell_slots(g, ci, cj)
            assert len(slots) >= 4, (geom, ci, cj)
            for blk, (x, y) in zip(todo.pop(0), slots):
                fr.put(x, y, blk)
        frames.append(fr)
    return frames


# ---------------------------------------------------------------------------------- rows
def row_arcs(geom):
    """bright and dark arcs of 8, 9, 10, 15, 16 pixels at every start; the weakest pixel of a 9-arc at every ring position"""
    blocks = []
    for pol in (1, -1):
        for L in (8, 9, 10, 15, 16):
            for s in range(16):
                blocks.append(arc_block(pol, L, s, (s * 5 + L) % L, 30))
        for p in range(16):                                # weakest pixel at ring position p, at arc index p % 9
            blocks.append(arc_block(pol, 9, (p - p % 9) % 16, p % 9, 26 + p, step=3))
    return pool_frames(geom, "arcs", blocks, 20, 7, offsets=((0, 0), (1, 3), (4, 1), (5, 6)))


def row_thresholds(geom):
    frames = []
    for ini, mn in PARAMS:
        groups = []
        for rep, pol in enumerate((1, -1)):
            s = 3 + 8 * rep
            # a cell that is not empty at ini: weakest difference exactly ini (no corner) and ini + 1 (score ini); both saturations
            groups.append([redeclare(arc_block(pol, 9, s, 4, ini), "AT_THRESHOLD", None, th=ini),
                           arc_block(pol, 9, s + 2, 2, ini + 1),
                           arc_block(1, 16, 0, 0, 255, step=0, centre=0), arc_block(-1, 16, 0, 0, 255, step=0, centre=255)])
            if mn < ini:
                # an otherwise empty cell (every difference <= ini): weakest difference exactly min, and min + 1 (kept at score min)
                groups.append([redeclare(arc_block(pol, 9, s + 5, 7, mn, step=1), "AT_THRESHOLD", None, th=mn),
                               arc_block(pol, 9, s + 7, 0, mn + 1, step=1, outcome="WEAK_KEPT")])
            else:
                # (min >= ini: whatever the pass at ini does not find, the pass at min cannot find either)
                groups.append([redeclare(arc_block(pol, 9, s + 5, 7, ini, step=1), "AT_THRESHOLD", None, th=ini)])
        frames += group_frames(geom, "th_%d_%d_" % (ini, mn), groups, ini, mn)
    return frames


def row_nms(geom):
    """all eight directions, A above B and A equal to B (B above A is the opposite direction), A at both phases of the pixel pairs"""
    return pool_frames(geom, "nms_even", all_pair_blocks(), 20, 7, spacing=12, offsets=((0, 0),), whole=2) + \
           pool_frames(geom, "nms_odd", all_pair_blocks(), 20, 7, spacing=12, offsets=((1, 0),), whole=2)


def _strong(i):
    return arc_block((1, -1)[i % 2], 9 + i % 2, (3 * i) % 16, i % 9, 30)


def _weak(i, outcome):
    return arc_block((1, -1)[i % 2], 9, (5 * i + 1) % 16, (2 * i) % 9, 9 + i % 3, step=1, outcome=outcome)      # differences 9 .. 19 <= ini


def row_retry(geom):
    """frame 0: cells of even columns hold only weak corners, odd ones a strong corner and three weak ones; frame 1: the other way round;
    frame 2: every cell weak only; frame 3: every cell mixed.  In a two-cell run: left empty at ini, right empty, both, neither."""
    g = GEOMS[geom]
    frames = []
    for n in range(4):
        fr = Frame(geom, "retry%d" % n)
        for ci, cj in live_cells(g):
            weak_only = n == 2 or (n < 2 and cj % 2 == n)
            slots = cell_slots(g, ci, cj)
            blocks = [_weak(ci + cj + i, "WEAK_KEPT") for i in range(3)] if weak_only else \
                     [_strong(ci + cj)] + [_weak(ci + cj + i, "WEAK_DROPPED") for i in range(3)]
            for blk, (x, y) in zip(blocks, slots):
                fr.put(x, y, blk)
        frames.append(fr)
    return frames


def row_seams(geom, only_outside=False):
    g = GEOMS[geom]
    ncols, nrows, wcell, hcell = g["grid"]
    lives = live_cells(g)
    frames = []
    # first and last band column and row of every cell
    fr = Frame(geom, "edges")
    for n, (ci, cj) in enumerate(lives):
        x0, y0, dw, dh = band(g, ci, cj)
        for m, (x, y) in enumerate(((0, 8), (dw - 1, 16), (8, 0), (16, dh - 1))):
            fr.put(x0 + x, y0 + y, arc_block((1, -1)[(n + m) % 2], 9 + (n + m) % 3, (n * 4 + m * 5) % 16, (n + m) % 9, 30))
    frames.append(fr)
    # strong corners where no cell reports: just past the last band column / row (apron of the clipped cells), left of the first column, in
    # the band a skipped cell would have had.  Every cell is otherwise empty: the second pass must not bring them in either
    fr = Frame(geom, "outside")
    out = lambda i: redeclare(arc_block((1, -1)[i % 2], 9 + i % 4, (7 * i) % 16, i % 9, 30), "OUT_OF_BAND", None)
    for n, (ci, cj) in enumerate(lives):
        x0, y0, dw, dh = band(g, ci, cj)
        if (ci, cj + 1) not in lives:
            fr.put(x0 + dw, y0 + 8, out(n))
        if (ci + 1, cj) not in lives and cj % 2 == 0:
            fr.put(x0 + 16, y0 + dh, out(n + 1))
        if cj == 0:
            fr.put(x0 - 1, y0 + 16, out(n + 2))
    for ci in range(nrows):
        for cj in range(ncols):
            if (ci, cj) not in lives and (cj % 2 == 0 or cj == ncols - 1):
                fr.put(cj * wcell + 3 + 5, ci * hcell + 3 + 5, out(ci + cj))
    frames.append(fr)
    if only_outside:
        return frames
    # adjacent corners with a seam between them: both kept whatever their scores (horizontal pairs on vertical seams, ...)
    for rel in ("gt", "eq"):
        for k in range(4):
            blk = pair_block("E", rel, k, across=True)
            dx, dy = blk["dir"]
            fr = Frame(geom, "seam_%s_%d" % (rel, k))
            for ci, cj in lives:
                x0, y0, dw, dh = band(g, ci, cj)
                if dx and (ci, cj + 1) in lives:
                    fr.put(x0 + dw - (1 if dx > 0 else 0), y0 + 8, blk)
                if dy and (ci + 1, cj) in lives:
                    fr.put(x0 + 20, y0 + dh - (1 if dy > 0 else 0), blk)
            if fr.decl:
                frames.append(fr)
            blk = pair_block("SE", rel, k, across=True)
            dx, dy = blk["dir"]
            fr = Frame(geom, "corner_%s_%d" % (rel, k))
            for ci, cj in lives:
                x0, y0, dw, dh = band(g, ci, cj)
                if (ci, cj + 1) in lives and (ci + 1, cj) in lives and (ci + 1, cj + 1) in lives:
                    fr.put(x0 + dw - (1 if dx > 0 else 0), y0 + dh - (1 if dy > 0 else 0), blk)
            if fr.decl:
                frames.append(fr)
    return frames


def row_load(geom):
    """Undeclared frames, compared as whole lists: 0 / 255 salt and pepper, and isolated dots on a few lattices (the densest candidate
    patterns: test_fast_cases.py says which the model finds densest and how full the queues get)"""
    g = GEOMS[geom]
    frames = []
    fr = Frame(geom, "salt")
    fr.img[:] = np.where(np.random.default_rng(12345).random(fr.img.shape) < 0.5, 0, 255).astype(np.uint8)
    frames.append(fr)
    for px, py in ((2, 2), (3, 2), (3, 3), (4, 4)):
        fr = Frame(geom, "dots%d%d" % (px, py))
        fr.img[py // 2::py, px // 2::px] = 255
        frames.append(fr)
    # a steep triangle-wave ramp, 43 x + 24 y: every pixel differs from one end of each compass pair by more than 20, so every pixel pair
    # passes the necessary test and the queue of every cell is filled to its capacity dh * npb (the model counts it)
    fr = Frame(geom, "ramp")
    yy, xx = np.mgrid[0:g["h"], 0:g["w"]]
    fr.img[:] = np.abs((43 * xx + 24 * yy) % 510 - 255).astype(np.uint8)
    frames.append(fr)
    # a shallow one, 100 .. 120: no difference above 20, so every cell is empty at iniThFAST, and the second pass at 7 queues most pairs
    fr = Frame(geom, "weakramp")
    fr.img[:] = (BG + np.abs((7 * xx + 3 * yy) % 40 - 20)).astype(np.uint8)
    frames.append(fr)
    fr = Frame(geom, "checker")
    yy, xx = np.mgrid[0:g["h"], 0:g["w"]]
    fr.img[:] = np.where((xx // 2 + yy // 2) % 2 == 0, 40, 220).astype(np.uint8)
    frames.append(fr)
    return frames


ROWS = dict(outside=lambda geom: row_seams(geom, True), arcs=row_arcs, thresholds=row_thresholds, nms=row_nms, seams=row_seams, retry=row_retry, load=row_load)


@functools.lru_cache(maxsize=None)
def frames(geom):
    """every frame of a geometry, row after row (computed once, never changed)"""
    out = []
    for row in GEOMS[geom]["rows"]:
        for fr in ROWS[row](geom):
            fr.row = row
            fr.img.setflags(write=False)
            out.append(fr)
    return tuple(out)


def batches(geom, size=16):
    """the frames of a geometry grouped by parameter set, in batches of at most 16: [((ini, min), [frames])]"""
    out = []
    for prm in PARAMS:
        sel = [fr for fr in frames(geom) if (fr.ini, fr.mn) == prm]
        out += [(prm, sel[i:i + size]) for i in range(0, len(sel), size)]
    return out


def chunk_batch():
    """3 frames for a two-level extractor (20, 7): skipped cells, cells empty after both passes, weak and mixed cells side by side"""
    fr = {f.name: f for f in frames("g933c")}
    return np.stack([fr[n].img for n in ("outside", "edges", "retry0")])


@functools.lru_cache(maxsize=None)
def model_results(geom):
    """{frame name: (xs, ys, scores, facts)} from the plain model"""
    import fast_model as fm
    return {fr.name: fm.cells(fr.img, fr.ini, fr.mn) for fr in frames(geom)}


@functools.lru_cache(maxsize=None)
def oracle_results(geom):
    """{frame name: (xs, ys, scores)} from the C oracle (one-level extractor)"""
    import oracle_bind as ob
    out = {}
    for fr in frames(geom):
        ora = ob.OracleExtractor(1000, 1.2, 1, fr.ini, fr.mn)
        ora.extract(np.ascontiguousarray(fr.img))
        out[fr.name] = ora.fast_candidates(0)
    return out
