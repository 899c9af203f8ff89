"""The trips of k_fast_cells' necessary test, from the plan's cell table (orbhip_fast_cell_table, no device): a cell of dh band rows takes
ceil(dh / rpt) trips of rpt rows, two flags per lane and trip.  A form of the kernel that keeps a lane's flags in one 32-bit mask
 needs 2 ceil(dh / rpt) <= 32 for every record; the LDS tile (cells of at most 58 x 58, so dh <= 58, and at least 4 rows per
trip) keeps every geometry the extractor accepts below that, and what lies beyond the tile is refused, never cut short."""
import numpy as np
import pytest

import orbhip
from test_fast_cell_table import FIELDS, level_sizes

DW, DH, RPT, TPR = FIELDS.index("dw"), FIELDS.index("dh"), FIELDS.index("rpt"), FIELDS.index("tpr")


def mask_bits(table):
    live = table[table[:, DW] > 0].astype(np.int64)
    return 2 * -(-live[:, DH] // live[:, RPT])


@pytest.mark.parametrize("w,h", [(640, 480), (752, 480), (1280, 720), (1920, 1080), (3840, 2160)])
def test_every_record_fits_a_32_bit_mask(w, h):
    t = orbhip.fast_cell_table(*level_sizes(w, h, 8))
    bits = mask_bits(t)
    assert len(bits) > 0 and bits.max() <= 32, (w, h, int(bits.max()))
    assert (t[:, RPT] == 64 // t[:, TPR]).all() and t[:, RPT].min() >= 4


def test_largest_accepted_cells_and_the_first_refused():
    """one-level geometries with a single cell row of 30 .. 59 rows (the tallest cells a grid can have: two rows give at most 45) under
    the widest cells (58 columns: 4 rows per trip): the tallest accepted one takes 13 trips = 26 bits; a cell of 59 rows would still fit
    the mask (28 bits) but not the 64-row tile, and is refused"""
    most = 0
    for hcell in range(30, 60):
        for wcell in (30, 45, 58):
            ws, hs = [wcell + 32], [hcell + 32]
            if hcell + 6 > 64:
                with pytest.raises(orbhip.OrbHipError):
                    orbhip.fast_cell_table(ws, hs)
                continue
            t = orbhip.fast_cell_table(ws, hs)
            assert len(t) == 1 and t[0, DH] == hcell - 6 and t[0, DW] == wcell - 6
            most = max(most, int(mask_bits(t).max()))
    assert most == 26
    with pytest.raises(orbhip.OrbHipError):
        orbhip.fast_cell_table([59 + 32], [58 + 32])           # 59 columns: beyond the tile as well
