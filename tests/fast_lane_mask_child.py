"""Child process of test_gpu_fast_lane_masks.py::test_skipped_cell_inside_a_chunk: ORBHIP_TUNE_FAST_CHUNK is read once per process, so a
chunk size other than the default needs a process of its own.  Extracts three crafted frames of the geometry named on the command line
(fast_cases.py: a skipped cell column) with a one-level extractor and writes every frame's candidate list and the FAST instance to the
.npz named first."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = ("outside", "edges", "retry0")


def batch(geom):
    import fast_cases as fc
    fr = {f.name: f for f in fc.frames(geom)}
    return [fr[n] for n in FRAMES]


def lists(ctx, geom):
    import orbhip
    frames = batch(geom)
    ext = orbhip.Extractor(ctx, 1000, 1.2, 1, 20, 7)
    ext.extract_host(np.stack([f.img for f in frames]))
    out = {"kernel": np.int32(ext.fast_kernel())}
    for f in range(len(frames)):
        out["f%d" % f] = np.stack(ext.fast_candidates(f, 0))
    ext.close()
    return out


if __name__ == "__main__":
    import orbhip
    ctx = orbhip.Context(0)
    np.savez(sys.argv[1], **lists(ctx, sys.argv[2]))
    ctx.close()
