"""Plain model of the per-cell FAST stage (ORBextractor.cc:763-856): FAST-9/16 + cornerScore + 3x3 strict NMS per cell sub-image at
iniThFAST, again at minThFAST where that left the cell empty.  Integers only, numpy only; shares no code with oracle/ or csrc/.

np_fast(img, th)            one cv::FAST call with NMS on a whole image (the arc-score identity)
arc_score(img, x, y)        the arc score of one pixel, plain loops
grid(w, h)                  the cell grid of a w x h level
cells(img, ini_th, min_th)  the level's candidate list in reference order + per-cell facts
"""
import numpy as np

EDGE = 19                    # EDGE_THRESHOLD
MINB = EDGE - 3              # detection origin: candidate (x, y) is image pixel (x + MINB, y + MINB)
# cv::makeOffsets order, k = 0..15
DX = [0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1]
DY = [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]


def np_fast(img, th):
    """FAST-9/16 + cornerScore + 3x3 strict NMS from the arc-score identity (independent shape)."""
    h, w = img.shape
    dx, dy = DX, DY
    I = img.astype(np.int32)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([c - I[3 + dy[k]:h - 3 + dy[k], 3 + dx[k]:w - 3 + dx[k]] for k in range(16)])
    best = np.full(c.shape, -999, np.int32)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    score = np.zeros((h, w), np.int32)
    score[3:h - 3, 3:w - 3] = np.where(best > th, best - 1, 0)
    keep = score > 0
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            if oy or ox:
                sh_ = np.zeros_like(score)
                ys = slice(max(0, oy), h + min(0, oy)); yd = slice(max(0, -oy), h + min(0, -oy))
                xs = slice(max(0, ox), w + min(0, ox)); xd = slice(max(0, -ox), w + min(0, -ox))
                sh_[yd, xd] = score[ys, xs]
                keep &= score > sh_
    ys, xs = np.nonzero(keep)
    return xs, ys, score[ys, xs]


def arc_score(img, x, y):
    """the threshold-independent arc score S of image pixel (x, y), from its definition: the pixel is a corner at threshold t iff S > t,
    and its cornerScore is then S - 1"""
    v = int(img[y, x])
    d = [v - int(img[y + DY[k], x + DX[k]]) for k in range(16)]
    return max(max(min(d[(s + j) % 16] for j in range(9)), min(-d[(s + j) % 16] for j in range(9))) for s in range(16))


def grid(w, h):
    """(ncols, nrows, wcell, hcell) of a w x h level: cells of about 30 pixels over the detection area (ORBextractor.cc:767-775)"""
    width, height = w - 2 * MINB, h - 2 * MINB
    ncols, nrows = width // 30, height // 30
    return ncols, nrows, -(-width // ncols), -(-height // nrows)


def cell_band(w, h, ci, cj):
    """(ini_x, ini_y, dw, dh) of cell (row ci, column cj); dw = dh = 0 for a cell the reference skips.  The sub-image is
    [ini, ini + d + 6), its band (the pixels FAST can report) starts 3 pixels in."""
    ncols, nrows, wcell, hcell = grid(w, h)
    max_bx, max_by = w - MINB, h - MINB
    ini_x, ini_y = MINB + cj * wcell, MINB + ci * hcell
    if ini_y >= max_by - 3 or ini_x >= max_bx - 6:
        return ini_x, ini_y, 0, 0
    dw = min(ini_x + wcell + 6, max_bx) - ini_x - 6
    dh = min(ini_y + hcell + 6, max_by) - ini_y - 6
    if dw <= 0 or dh <= 0:
        return ini_x, ini_y, 0, 0
    return ini_x, ini_y, dw, dh


def compass_map(img):
    """M of every pixel at least 3 from the border (0 elsewhere): max(v - max_j min(a_j, b_j), min_j max(a_j, b_j) - v) over the four
    diametral pairs (a_j, b_j) of the compass points of the ring (k = 0/8, 2/10, 4/12, 6/14).  A corner at threshold t has M > t."""
    h, w = img.shape
    I = img.astype(np.int64)
    v = I[3:h - 3, 3:w - 3]
    ring = lambda k: I[3 + DY[k]:h - 3 + DY[k], 3 + DX[k]:w - 3 + DX[k]]
    lo = np.max(np.stack([np.minimum(ring(k), ring(k + 8)) for k in (0, 2, 4, 6)]), 0)
    hi = np.min(np.stack([np.maximum(ring(k), ring(k + 8)) for k in (0, 2, 4, 6)]), 0)
    M = np.zeros((h, w), np.int64)
    M[3:h - 3, 3:w - 3] = np.maximum(v - lo, hi - v)
    return M


def compass_pairs(M, x0, y0, dw, dh, th):
    """pixel pairs (2p, 2p + 1), p < (dw + 1) / 2, of the dh band rows starting at image pixel (x0, y0) with M > th in either pixel (the
    second pixel of an odd band's last pair lies past the band and counts: the pair is tested as a whole)"""
    npb = (dw + 1) // 2
    m = M[y0:y0 + dh, x0:x0 + 2 * npb].reshape(dh, npb, 2).max(2)
    return int((m > th).sum())


def cells(img, ini_th, min_th):
    """(xs, ys, scores, facts): the candidate list of the level in reference order (cells row-major, raster order inside a cell,
    coordinates relative to the detection origin) and one dict per cell, row-major: ci, cj, dw, dh, skipped, second_pass (the cell was
    empty at ini_th and min_th differs from it), n (candidates), nq (compass-test survivors per pass that ran), npb (pairs per band row)."""
    h, w = img.shape
    ncols, nrows, wcell, hcell = grid(w, h)
    M = compass_map(img)
    xs, ys, ss, facts = [], [], [], []
    for ci in range(nrows):
        for cj in range(ncols):
            ini_x, ini_y, dw, dh = cell_band(w, h, ci, cj)
            f = dict(ci=ci, cj=cj, dw=dw, dh=dh, skipped=dw == 0, second_pass=False, n=0, nq=[], npb=(dw + 1) // 2)
            facts.append(f)
            if f["skipped"]:
                continue
            sub = img[ini_y:ini_y + dh + 6, ini_x:ini_x + dw + 6]
            x, y, s = np_fast(sub, ini_th)
            f["nq"].append(compass_pairs(M, ini_x + 3, ini_y + 3, dw, dh, ini_th))
            if len(x) == 0:
                x, y, s = np_fast(sub, min_th)
                if min_th != ini_th:
                    f["second_pass"] = True
                    f["nq"].append(compass_pairs(M, ini_x + 3, ini_y + 3, dw, dh, min_th))
            f["n"] = len(x)
            xs.append(x + cj * wcell); ys.append(y + ci * hcell); ss.append(s)
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)
    return cat(xs), cat(ys), cat(ss), facts
