"""Shared by test_gpu_fast_cell_table.py and its child process: ORBHIP_TUNE_FAST_CHUNK is read once per process, so a chunk size other than
the default needs a process of its own.  Extracts a batch of synthetic frames and returns every (frame, level) candidate list and the
FAST instance; as a program, writes them to the .npz named on the command line for the case named after it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (width, height, levels, frames): see test_gpu_fast_cell_table.py
CASES = {
    "min8": (224, 224, 8, 3),          # the smallest size with 8 levels (level 7 is 63 x 63: one cell)
    "odd": (331, 453, 8, 3),           # odd, not square, every level within the small-cell instance: clipped last column and row on most levels
    "skip": (813, 100, 2, 2),          # level 0: 26 columns of 31 px, the last one skipped (ORBextractor.cc:799)
    "large": (300, 90, 2, 3),          # one cell row of 58 and 43 px: the large-cell instance
    "batch16": (224, 224, 8, 16),      # a batch that forks (level-range launches under ORBHIP_TUNE_L0_EARLY)
}


def frames(case):
    import orbhip
    w, h, _, n = CASES[case]
    return orbhip.synth_frames(w, h, n, seed=20260101 + sorted(CASES).index(case))


def lists(ctx, case):
    import orbhip
    w, h, nlevels, n = CASES[case]
    ext = orbhip.Extractor(ctx, 1000, 1.2, nlevels, 20, 7)
    ext.extract_host(frames(case))
    out = {"kernel": np.int32(ext.fast_kernel())}
    for f in range(n):
        for l in range(nlevels):
            out["f%d_l%d" % (f, l)] = np.stack(ext.fast_candidates(f, l))
    ext.close()
    return out


if __name__ == "__main__":
    import orbhip
    ctx = orbhip.Context(0)
    np.savez(sys.argv[1], **lists(ctx, sys.argv[2]))
    ctx.close()
