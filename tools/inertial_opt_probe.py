#!/usr/bin/env python3
"""Times orbhip_inertial_optimization_device: one map and 64 maps of N in {10, 50, 200} keyframes, overloads (a) (monocular, the
reference's priors) and (d); median wall time of launch + synchronise over 20 calls after 3 warm-up calls, on fresh device copies of
the inputs each call.  With ORBHIP_IO_PROF=1 the kernel reports, per map, the share of its cycles (thread 0's clock) in the chain
elimination and in the border solve + back substitution; the probe prints their means.  Also (a) with fixed velocities on the same maps: what the velocity chain adds to a trial (build of the chain
blocks, elimination, Schur complement, back substitution) is the difference per LM trial -- an upper bound of the elimination's share.
    python tools/inertial_opt_probe.py [out.json]      (default profiles/r07_inertial_opt.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import torch                # noqa: E402
import orbhip               # noqa: E402
import inertial_opt_cases as ic      # noqa: E402
import synth_inertial_opt as sio     # noqa: E402


def time_call(ctx, maps, p, reps=20, warm=3):
    off, kf, link, preint, info, glob = sio.pack(maps)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    t_off, t_link, t_pre, t_info = dev(off), dev(link), dev(preint), dev(info)
    st = torch.zeros((len(maps), 8), dtype=torch.float64, device="cuda")
    ms = []
    for r in range(warm + reps):
        t_kf, t_glob = dev(kf), dev(glob)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        orbhip.inertial_optimization_device(ctx, p, len(maps), t_off.data_ptr(), t_kf.data_ptr(), t_link.data_ptr(), t_pre.data_ptr(),
                                            t_info.data_ptr(), t_glob.data_ptr(), st.data_ptr(), None)
        ctx.synchronize()
        if r >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    s = st.cpu().numpy()
    os.environ["ORBHIP_IO_PROF"] = "1"                       # one more call for the in-kernel cycle shares (stats [6], [7])
    t_kf, t_glob = dev(kf), dev(glob)
    orbhip.inertial_optimization_device(ctx, p, len(maps), t_off.data_ptr(), t_kf.data_ptr(), t_link.data_ptr(), t_pre.data_ptr(),
                                        t_info.data_ptr(), t_glob.data_ptr(), st.data_ptr(), None)
    ctx.synchronize()
    del os.environ["ORBHIP_IO_PROF"]
    sp = st.cpu().numpy()
    return dict(share_elimination=float(sp[:, 7].mean()), share_border_backsubst=float(sp[:, 6].mean()), ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), iterations=float(s[:, 0].mean()),
                trials=float(s[:, 1].mean()), trials_max=float(s[:, 1].max()))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_inertial_opt.json")
    ctx = orbhip.Context(0)
    res, shares = [], []
    for fam in ("a_mono_prior", "a_fixed", "d"):
        ov, mono, fixed, pg, pa = ic.FAMILIES[fam]
        p = orbhip.inertial_opt_params(ov, mono, fixed, pg, pa)
        for n in (10, 50, 200, 1000):
            one = time_call(ctx, [ic.make(fam, n, 1)], p)
            many = time_call(ctx, [ic.make(fam, n, 1 + i) for i in range(64)], p)
            row = dict(family=fam, n_kf=n, one_map=one, maps64=many, ratio_64_to_1=many["ms_median"] / one["ms_median"])
            res.append(row)
            print("%-13s n %3d  1 map %8.3f ms (%5.1f it, %5.1f trials; elimination %4.1f %%, border + back substitution %4.1f %% of the cycles)  "
                  "64 maps %8.3f ms (trials mean %5.1f max %3.0f)  ratio %.2f"
                  % (fam, n, one["ms_median"], one["iterations"], one["trials"], 100 * one["share_elimination"], 100 * one["share_border_backsubst"],
                     many["ms_median"], many["trials"], many["trials_max"], row["ratio_64_to_1"]), flush=True)
    for n in (10, 50, 200):
        a = [r for r in res if r["family"] == "a_mono_prior" and r["n_kf"] == n][0]["one_map"]
        f = [r for r in res if r["family"] == "a_fixed" and r["n_kf"] == n][0]["one_map"]
        share = 1.0 - (f["ms_median"] / max(f["trials"], 1)) / (a["ms_median"] / max(a["trials"], 1))
        shares.append(dict(n_kf=n, ms_per_trial_free=a["ms_median"] / max(a["trials"], 1), ms_per_trial_fixed_vel=f["ms_median"] / max(f["trials"], 1),
                           chain_side_share_upper_bound=share))
        print("n %3d  per trial: free %.4f ms, fixed velocities %.4f ms -> the chain side is at most %.0f %% of a trial" %
              (n, shares[-1]["ms_per_trial_free"], shares[-1]["ms_per_trial_fixed_vel"], 100 * share), flush=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=res, chain_share=shares), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
