"""The tiled descriptor kernel fetches, per patch row, only the 16-byte chunks that intersect the disc the rBRIEF pattern can sample
(orbhip_blur_half_widths).  Here every pattern point is rotated through a dense sweep of angles with the kernel's own float32
expressions (products, one add / subtract, round-half-even by the 1.5 * 2^23 trick): every sampled (row, column) must lie inside the
table, and rows and columns +-19 of the 39 x 39 patch must never be hit.  No GPU needed."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pattern():
    txt = open(os.path.join(ROOT, "orb-slam3-mac_amd", "csrc", "orb_pattern.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    v = np.array([int(t) for t in re.findall(r"-?\d+", txt)], np.int32)
    assert v.size == 1024
    return v.reshape(512, 2)                       # 512 points (x, y): two per test


def _half_widths():
    import orbhip
    return orbhip.blur_half_widths()


def test_table_is_the_rounded_chord_of_the_largest_norm():
    pts = _pattern()
    r2 = int((pts.astype(np.int64) ** 2).sum(1).max())
    assert r2 == 338 and abs(math.sqrt(r2) - 18.385) < 1e-3          # (13, 13): the norm the layout was sized for
    want = [min(int(math.floor(math.sqrt(r2 - max(d - 0.5, 0.0) ** 2) + 0.5)), 18) for d in range(19)]
    hw = _half_widths()
    assert hw.tolist() == want
    # |dy| = 18 .. 7, then 18 for |dy| <= 6
    assert hw[::-1][:12].tolist() == [6, 8, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17] and (hw[:7] == 18).all()


def test_every_sample_of_a_dense_angle_sweep_lies_inside_the_table():
    pts = _pattern().astype(np.float32)
    hw = _half_widths()
    px, py = pts[:, 0][None, :], pts[:, 1][None, :]
    magic = np.float32(12582912.0)
    factor_pi = np.float32(3.1415926535897932384626433832795 / 180.0)
    worst_row = worst_col = 0
    slack = np.full(19, 99, np.int64)               # table minus the largest |column| seen, per |row|
    # angles: every 1/128 degree of [0, 360] as float32 (cv::fastAtan2's range), plus the float32 neighbours of the multiples of 45 degrees
    base = (np.arange(0, 360 * 128 + 1, dtype=np.float64) / 128.0).astype(np.float32)
    near = np.concatenate([np.nextafter(np.float32(45.0 * k), np.float32(s)) for k in range(9) for s in (-1e9, 1e9)] +
                          [np.float32([45.0 * k]) for k in range(9)], axis=None).astype(np.float32)
    angles = np.unique(np.clip(np.concatenate([base, near]), np.float32(0), np.float32(360)))
    for chunk in np.array_split(angles, 64):
        rad = (chunk * factor_pi).astype(np.float32).astype(np.float64)      # __fmul_rn(angle, factor_pi), then double sin / cos, then float
        a = np.cos(rad).astype(np.float32)[:, None]
        b = np.sin(rad).astype(np.float32)[:, None]
        for da, db in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):            # one float32 ulp either way: the device's own sincos may round differently
            aa = np.nextafter(a, np.float32(np.inf) * da) if da else a
            bb = np.nextafter(b, np.float32(np.inf) * db) if db else b
            rowf = ((px * bb).astype(np.float32) + (py * aa).astype(np.float32)).astype(np.float32)
            colf = ((px * aa).astype(np.float32) - (py * bb).astype(np.float32)).astype(np.float32)
            row = ((rowf + magic).astype(np.float32) - magic).astype(np.int64)    # exact: fl(r + M) - M = round-half-even(r)
            col = ((colf + magic).astype(np.float32) - magic).astype(np.int64)
            ar, ac = np.abs(row), np.abs(col)
            worst_row = max(worst_row, int(ar.max())); worst_col = max(worst_col, int(ac.max()))
            assert worst_row <= 18 and worst_col <= 18, (worst_row, worst_col)
            assert (ac <= hw[ar]).all(), "a sample outside the half-width table"
            np.minimum.at(slack, ar.ravel(), (hw[ar] - ac).ravel())
    print("largest |row| %d, |col| %d; table minus largest |col| per |row|: %s" % (worst_row, worst_col, slack.tolist()))
    assert worst_row == 18 and worst_col == 18      # the sweep does reach the rim, so the bound is not vacuous
