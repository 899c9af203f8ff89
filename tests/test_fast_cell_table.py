"""k_fast_cells reads a cell's geometry from a table that orb_plan_fast builds once per image size (one 16-byte record per cell of a frame).
orbhip_fast_cell_table returns that table decoded, without a device.  Here every field of every record is compared with an independent
restatement of the reference's cell loop (ORBextractor.cc:771-806) and of the project's cell-list layout, over a sweep of image sizes
that is asserted to contain clipped last columns / rows and skipped cells."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))

import orbhip  # noqa: E402

EDGE = 19                 # EDGE_THRESHOLD (ORBextractor.cc:72)
NLEVELS = 8
SCALE = np.float32(1.2)
FIELDS = ["level", "x0", "y0", "dw", "dh", "key_x0", "key_y0", "list", "tpr", "rpt", "magic", "cell_cap"]


def level_sizes(w, h, nlevels=NLEVELS):
    """ComputePyramid's sizes (ORBextractor.cc:1156-1157): cvRound of float32 products with the inverse scale factors (:413-429)"""
    s, ws, hs = np.float32(1.0), [], []
    for _ in range(nlevels):
        inv = np.float32(1.0) / s
        ws.append(int(np.rint(np.float32(w) * inv)))
        hs.append(int(np.rint(np.float32(h) * inv)))
        s = np.float32(s * SCALE)
    return ws, hs


def reference_cells(ws, hs):
    """The cells of a frame in level, then row-major order, from ORBextractor.cc:771-806 restated line by line; None where the extractor
    refuses the geometry (a level without a cell, or a cell beyond the kernel's 64 x 64 tile).  Returns (rows [cells][12], facts)."""
    levels = []
    for cols, rows_ in zip(ws, hs):
        min_b = EDGE - 3                                           # :771-772
        max_bx, max_by = cols - EDGE + 3, rows_ - EDGE + 3         # :773-774
        width, height = np.float32(max_bx - min_b), np.float32(max_by - min_b)      # :779-780
        if width < 30 or height < 30:
            return None, None
        ncols, nrows = int(width / np.float32(30)), int(height / np.float32(30))     # :782-783
        wcell, hcell = int(math.ceil(width / np.float32(ncols))), int(math.ceil(height / np.float32(nrows)))     # :784-785
        if wcell + 6 > 64 or hcell + 6 > 64:
            return None, None
        levels.append((min_b, max_bx, max_by, ncols, nrows, wcell, hcell))
    cell_cap = max(((wc + 1) // 2) * ((hc + 1) // 2) for *_, wc, hc in levels)      # 3x3 strict NMS: one keypoint per 2x2 block at the most
    out, cell = [], 0
    facts = {"clipped": 0, "skipped": 0, "empty": 0}
    for level, (min_b, max_bx, max_by, ncols, nrows, wcell, hcell) in enumerate(levels):
        npb = (wcell + 1) // 2                                     # pixel pairs per band row; the necessary test gives two pairs to a lane
        tpr = (npb + 1) // 2
        for i in range(nrows):                                     # :787
            ini_y = min_b + i * hcell
            max_y = ini_y + hcell + 6
            skip_row = ini_y >= max_by - 3                         # :791
            max_y = min(max_y, max_by)                             # :793
            for j in range(ncols):                                 # :796
                ini_x = min_b + j * wcell
                max_x = ini_x + wcell + 6
                skip = skip_row or ini_x >= max_bx - 6             # :799
                max_x = min(max_x, max_bx)                         # :801
                # cv::FAST on the max_x - ini_x by max_y - ini_y sub-image detects nothing within 3 pixels of its border
                dw, dh = max_x - ini_x - 6, max_y - ini_y - 6
                if skip:                                           # the reference's `continue`
                    dw = dh = 0
                    facts["skipped"] += 1
                elif dw <= 0 or dh <= 0:                           # a sub-image of 6 rows or fewer: cv::FAST finds nothing
                    dw = dh = 0
                    facts["empty"] += 1
                elif dw < wcell or dh < hcell:
                    facts["clipped"] += 1
                # keypoints come back relative to the sub-image and are moved by (j wCell, i hCell) (:836-837): band pixel (0, 0) is (3, 3) there
                out.append([level, ini_x - 1, ini_y, dw, dh, 3 + j * wcell, 3 + i * hcell, cell * cell_cap, tpr, 64 // tpr, 65536 // tpr + 1, cell_cap])
                cell += 1
    return np.array(out, np.int64), facts


def check(w, h, totals):
    ws, hs = level_sizes(w, h)
    want, facts = reference_cells(ws, hs)
    if want is None:
        with pytest.raises(orbhip.OrbHipError):
            orbhip.fast_cell_table(ws, hs)
        totals["refused"] += 1
        return
    got = orbhip.fast_cell_table(ws, hs).astype(np.int64)
    assert got.shape == want.shape, (w, h, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d x %d: cell %d field %s is %d, expected %d" % (w, h, bad[0][0], FIELDS[bad[0][1]], got[tuple(bad[0])], want[tuple(bad[0])])
    for k in facts:
        totals[k] += facts[k]
    totals["cells"] += len(want)
    totals["sizes"] += 1


def test_vga_table():
    """the flagship size: 815 cells, and the division by magic is exact for every lane"""
    totals = {"refused": 0, "clipped": 0, "skipped": 0, "empty": 0, "cells": 0, "sizes": 0}
    check(640, 480, totals)
    assert totals["cells"] == 815 and totals["refused"] == 0
    t = orbhip.fast_cell_table(*level_sizes(640, 480))
    for tpr, rpt, magic in {tuple(r) for r in t[:, 8:11].tolist()}:
        assert 8 <= tpr <= 15 and rpt == 64 // tpr
        assert all((i * magic) >> 16 == i // tpr for i in range(64))


@pytest.mark.parametrize("axis", ["width", "height"])
def test_sweep(axis):
    """every width (height) from below the smallest size the extractor accepts to 1000, the other axis held at a few values"""
    totals = {"refused": 0, "clipped": 0, "skipped": 0, "empty": 0, "cells": 0, "sizes": 0}
    for other in (224, 487, 811):
        for v in range(218, 1001):
            check(*((v, other) if axis == "width" else (other, v)), totals)
    print(axis, totals)
    assert totals["sizes"] > 2000 and totals["refused"] > 0, totals
    # the sweep cannot pass by missing the border cases: last columns / rows narrower than the nominal cell, cells the reference skips
    # (:791 / :799) and cells whose sub-image is too low for a band
    assert totals["clipped"] > 0 and totals["skipped"] > 0, totals
    assert axis == "width" or totals["empty"] > 0, totals          # (a column that is not skipped always keeps a band: :799 leaves 7 pixels)


def test_two_level_and_single_row():
    """fewer levels, and a level with one cell row (the large-cell kernel instance's geometry)"""
    totals = {"refused": 0, "clipped": 0, "skipped": 0, "empty": 0, "cells": 0, "sizes": 0}
    for ws, hs in (([933, 778], [122, 102]), ([300, 250], [90, 75]), ([1920, 1600], [1080, 900])):
        want, facts = reference_cells(ws, hs)
        got = orbhip.fast_cell_table(ws, hs).astype(np.int64)
        np.testing.assert_array_equal(got, want)
