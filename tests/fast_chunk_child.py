"""Child process of test_gpu_fast_cases.py::test_chunks_of_several_cells: ORBHIP_TUNE_FAST_CHUNK is read once per process, so a chunk size
other than the default needs a process of its own.  Extracts fast_cases.chunk_batch() with a two-level extractor and writes every
(frame, level) candidate list and the FAST instance to the .npz named on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def lists(ctx):
    import orbhip
    import fast_cases as fc
    imgs = fc.chunk_batch()
    ext = orbhip.Extractor(ctx, 1000, 1.2, 2, 20, 7)
    ext.extract_host(imgs)
    out = {"kernel": np.int32(ext.fast_kernel())}
    for f in range(len(imgs)):
        for l in range(2):
            out["f%d_l%d" % (f, l)] = np.stack(ext.fast_candidates(f, l))
    ext.close()
    return out


if __name__ == "__main__":
    import orbhip
    ctx = orbhip.Context(0)
    np.savez(sys.argv[1], **lists(ctx))
    ctx.close()
