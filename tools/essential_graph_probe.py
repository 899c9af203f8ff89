"""Times the essential-graph optimisation on the GPU: per call and per LM trial at 10 / 69 / 150 / 585 free vertices, split into
linearise / assemble / factor (fill + LDL^T + solve) / update (trial estimates, errors, reductions, the read-back).
The per-call figure is the host's wall time of an unprofiled call (what a caller waits for).  The split is DEVICE time: with
ORBHIP_PG_PROF=1 every stage is bracketed by two events on the stream (hipEventElapsedTime); an event pair around a single small kernel
still includes its launch gap, so the 10-vertex figures are mostly that.
Usage: python tools/essential_graph_probe.py [out.json]   (default profiles/r09_essential_graph.json)"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import orbhip               # noqa: E402
import synth_essential_graph as sg   # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_essential_graph.json")
    ctx = orbhip.Context(0)
    prof = orbhip.lib.orbhip_debug_pose_graph_prof
    prof.argtypes = [C.c_void_p, C.c_int]
    rows = []
    for n_free in (10, 69, 150, 585):
        g = sg.make_graph(1, n_free, True, rot_drift=2e-4, trans_drift=1e-2)
        p = orbhip.pose_graph_default_params(6, True)
        orbhip.optimize_essential_graph(ctx, [g], [g["sim3"]], p)                      # warm-up: arenas, LDS opt-in
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            _, st, _ = orbhip.optimize_essential_graph(ctx, [g], [g["sim3"]], p, trace=False)
            ts.append((time.perf_counter() - t) * 1e3)
        os.environ["ORBHIP_PG_PROF"] = "1"
        prof(None, 1)
        orbhip.optimize_essential_graph(ctx, [g], [g["sim3"]], p, trace=False)
        del os.environ["ORBHIP_PG_PROF"]
        v = (C.c_double * 7)()
        prof(C.cast(v, C.c_void_p), 1)
        its, trials = max(v[5], 1), max(v[4], 1)
        rows.append(dict(free_vertices=n_free, unknowns=7 * n_free, edges=int(len(g["edge_v0"])), iterations=st[0]["iterations"], trials=st[0]["trials"],
                         call_ms_median=float(np.median(ts)), call_ms_min=float(min(ts)), trial_ms=float(np.median(ts)) / st[0]["trials"],
                         device_us=dict(linearise_per_iteration=v[0] / its, assemble_per_iteration=v[1] / its, factor_per_trial=v[2] / trials,
                                          update_per_trial=v[3] / trials)))
        print(rows[-1], flush=True)
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(dict(what="Optimizer::OptimizeEssentialGraph on the device, fix_scale, 6 iterations; host wall time of the whole call "
                            "(median of 5) and, with ORBHIP_PG_PROF=1, device time per stage between two stream events (microseconds)", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
