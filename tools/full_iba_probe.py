#!/usr/bin/env python3
"""Times orbhip_full_inertial_ba_solve_batch: one map per call (the synchronous host entry point: packing, upload, the persistent
kernel, download), median wall time of 20 calls after 3 warm-up calls.  Shared-bias mode at 10 / 20 / 30 / 52 keyframes, per-keyframe
mode at 10 / 20 / 32, about 100 points per keyframe, 4 iterations.  Beside each: orbhip_inertial_ba_solve_batch (LocalInertialBA's
path, one workgroup per window) on a window with the same number of reduced unknowns, per LM trial, for scale.
    python tools/full_iba_probe.py [out.json]      (default profiles/r08_full_iba.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import orbhip               # noqa: E402
import synth_full_iba as sf  # noqa: E402
import synth_iba            # noqa: E402

REPS, WARM, ITS = 20, 3, 4


def median_ms(call):
    ms = []
    for r in range(WARM + REPS):
        t0 = time.perf_counter()
        st = call()
        if r >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), st


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_full_iba.json")
    os.environ["ORBHIP_IBA_TEAM"] = "1"                     # the local path's yardstick with one workgroup per window, as the full BA runs
    ctx = orbhip.Context(0)
    res = []
    for shared, Ks in ((True, (10, 20, 30, 52)), (False, (10, 20, 32))):
        for K in Ks:
            win, sb = sf.make_map(1, K, pts_per_kf=100, bias0_sigma=1e-3)
            s = win.struct(orbhip.IbaWindow)
            p = orbhip.fiba_default_params(ITS, shared, 0.0, 0.0)
            ms, st = median_ms(lambda: orbhip.full_inertial_ba_solve_batch(ctx, [s], [win.kf0], [win.pts0], sb[None], p)[3][0])
            n = st["n_unknowns"]
            # LocalInertialBA at equal unknowns: n / 15 optimizable keyframes (its fixed previous keyframe and no other fixed ones)
            nl = max(2, min(32, int(round(n / 15.0))))
            lw = synth_iba.make_window(1, n_opt=nl, n_fixed_vis=0, n_points=100 * nl)
            ls = lw.struct(orbhip.IbaWindow)
            lp = orbhip.iba_default_params(False); lp.iterations = ITS
            lms, lst = median_ms(lambda: orbhip.inertial_ba_solve_batch(ctx, [ls], [lw.kf0], [lw.pts0], lp)[3][0])
            row = dict(shared_bias=shared, keyframes=K, points=win.n_points, edges=win.n_edges, unknowns=n, ms_per_call=ms, iterations=st["iterations_run"],
                       lm_trials=st["lm_trials"], ms_per_trial=ms / max(st["lm_trials"], 1),
                       local=dict(keyframes=nl, unknowns=15 * nl, edges=lw.n_edges, ms_per_call=lms, lm_trials=lst["lm_trials"], ms_per_trial=lms / max(lst["lm_trials"], 1)))
            res.append(row)
            print("%-12s K %2d  n %3d  %6d edges  %8.3f ms per call, %2d trials, %7.3f ms per trial | LocalInertialBA n %3d %6d edges %8.3f ms per call, %2d trials, %7.3f ms per trial"
                  % ("shared" if shared else "per-keyframe", K, n, win.n_edges, ms, st["lm_trials"], row["ms_per_trial"], 15 * nl, lw.n_edges, lms, lst["lm_trials"],
                     row["local"]["ms_per_trial"]), flush=True)
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:
        device = "unknown"
    with open(out, "w") as f:
        json.dump(dict(device=device, reps=REPS, warm=WARM, iterations=ITS, results=res), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
