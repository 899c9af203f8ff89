"""Times the 4-DoF essential-graph optimisation on the GPU against the 7-DoF one at the same keyframe counts, in one process: per call
and per LM trial at 10 / 69 / 150 / 585 free keyframes for both, and at 1024 (the largest admitted) for the 4-DoF one.
The per-call figure is the host's wall time of a synchronous call (it ends in the read-back of the estimates, after a stream
synchronise): what a caller waits for.  Per size: one warm-up call (arenas, LDS opt-in, code objects), then REPEATS timed calls of each
solver, alternating the two; median, minimum, maximum and the spread (max - min) / median are recorded.  The two solvers run different
graphs of the same keyframe count (their own generators), and past the decisive prefix the number of trials is decided by rounding, so
the per-trial figure is the one to compare; the per-call figure goes with its trial count.
Usage: python tools/essential_graph4dof_probe.py [out.json]   (default profiles/r10_essential_graph4dof.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import orbhip               # noqa: E402
import synth_essential_graph as sg7      # noqa: E402
import synth_essential_graph4dof as sg4  # noqa: E402

REPEATS = 9
ITERATIONS = 6


def stats(ts, trials):
    ts = np.asarray(ts)
    med = float(np.median(ts))
    return dict(call_ms_median=med, call_ms_min=float(ts.min()), call_ms_max=float(ts.max()), spread=float((ts.max() - ts.min()) / med), trials=int(trials),
                trial_ms=med / max(trials, 1))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_essential_graph4dof.json")
    ctx = orbhip.Context(0)
    rows = []
    for n_free in (10, 69, 150, 585, 1024):
        g4 = sg4.make_graph(1, n_free, yaw_drift=3e-4, trans_drift=3e-3, extra_fixed=False)
        p4 = orbhip.pose_graph4dof_default_params(ITERATIONS)
        run4 = lambda: orbhip.optimize_essential_graph4dof(ctx, [g4], [g4["state"]], p4, trace=False)[1][0]
        run7 = None
        if 7 * n_free <= 4096:
            g7 = sg7.make_graph(1, n_free, True, rot_drift=2e-4, trans_drift=1e-2)
            p7 = orbhip.pose_graph_default_params(ITERATIONS, True)
            run7 = lambda: orbhip.optimize_essential_graph(ctx, [g7], [g7["sim3"]], p7, trace=False)[1][0]
        run4()
        if run7:
            run7()
        t4, t7, st4, st7 = [], [], None, None
        for _ in range(REPEATS):                             # alternating, as the two are compared
            t = time.perf_counter(); st4 = run4(); t4.append((time.perf_counter() - t) * 1e3)
            if run7:
                t = time.perf_counter(); st7 = run7(); t7.append((time.perf_counter() - t) * 1e3)
        row = dict(free_keyframes=n_free, dof4=dict(unknowns=4 * n_free, edges=int(len(g4["edge_v0"])), iterations=st4["iterations"], **stats(t4, st4["trials"])))
        if run7:
            row["dof7"] = dict(unknowns=7 * n_free, edges=int(len(g7["edge_v0"])), iterations=st7["iterations"], **stats(t7, st7["trials"]))
            row["trial_ms_ratio_4_over_7"] = row["dof4"]["trial_ms"] / row["dof7"]["trial_ms"]
        rows.append(row)
        print(row, flush=True)
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(dict(what="Optimizer::OptimizeEssentialGraph4DoF on the device against OptimizeEssentialGraph (fix_scale) at equal keyframe counts, %d iterations; "
                            "host wall time of the whole synchronous call, one warm-up then %d alternating repeats: median / min / max, spread = (max - min) / median"
                            % (ITERATIONS, REPEATS), rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
