#!/usr/bin/env python3
"""Times of orbhip_preintegrate_device on the device next to the host IntegrateNewMeasurement loop (host_preint_smoke, one thread):
    python tools/preint_probe.py [out.json]
Shapes: 2 chains x 10 measurements (the per-frame call of Tracking::PreintegrateIMU), 1 x 400, 50 x 100 and 500 x 100 (a map-wide
Reintegrate), each in both forms, and a sweep over the number of chains (x 100 measurements) around the forms' crossing.  A time is
the median over REPS calls of a host clock around the call and a synchronise of the context's stream, after WARM calls; the arrays are on
the device already (what the device entry costs a caller that keeps its records there).  want_info = 0; the information kernel is timed
on its own line."""
import json
import os
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orbhip                  # noqa: E402
import preint_cases as pc      # noqa: E402
import synth_inertial_opt as sio   # noqa: E402

WARM, REPS = 20, 200
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_preint_smoke")


def device_us(ctx, chains, length, form, want_info=False):
    import torch
    meas = np.concatenate([pc.chain(length, c) for c in range(chains)])
    off = (np.arange(chains + 1) * length).astype(np.int32)
    rec = np.zeros((chains, 67)); rec[:, 61:67] = np.stack([pc.bias(c) for c in range(chains)])
    t = [torch.from_numpy(a).cuda() for a in (off, meas, rec, np.zeros((chains, 225), np.float32), np.zeros((chains, 6), np.float32),
                                              np.zeros((chains, 99)))]
    p = orbhip.preint_params(force_form=form, want_info=want_info)
    ip = t[5].data_ptr()
    args = (ctx, p, chains, t[0].data_ptr(), t[1].data_ptr(), None, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), ip, ip + 8 * 81 * chains,
            ip + 8 * 90 * chains)
    torch.cuda.synchronize()
    times = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        orbhip.preintegrate_device(*args)
        ctx.synchronize()
        if i >= WARM:
            times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times)), float(np.percentile(times, 10)), float(np.percentile(times, 90))


def host_us(chains, length):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "a.in"), os.path.join(d, "a.out")
        sio.write_flat(fin, {"mode": np.array([-2], np.int32), "reps": np.array([30], np.int32),
                             "noise": np.array([pc.NG, pc.NA, pc.NGW, pc.NAW], np.float32),
                             "meas_off": (np.arange(chains + 1) * length).astype(np.int32),
                             "meas": np.concatenate([pc.chain(length, c) for c in range(chains)]),
                             "bias": np.stack([pc.bias(c) for c in range(chains)]), "bias_new": np.zeros((chains, 6), np.float32)})
        subprocess.run([EXE, fin, fout], check=True)
        return float(sio.read_flat(fout)["host_us"][0])


def main():
    ctx = orbhip.Context(0)
    res = {"warm": WARM, "reps": REPS, "shapes": [], "sweep": []}
    for chains, length in ((2, 10), (1, 400), (50, 100), (500, 100)):
        row = {"chains": chains, "length": length, "host_loop_us": host_us(chains, length)}
        for name, form in (("lane", orbhip.PREINT_FORM_LANE), ("wave", orbhip.PREINT_FORM_WAVE)):
            row[name + "_us_median_p10_p90"] = device_us(ctx, chains, length, form)
        row["auto_with_info_us_median_p10_p90"] = device_us(ctx, chains, length, orbhip.PREINT_FORM_AUTO, True)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    for chains in (1, 8, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        row = {"chains": chains, "length": 100, "lane_us": device_us(ctx, chains, 100, orbhip.PREINT_FORM_LANE)[0],
               "wave_us": device_us(ctx, chains, 100, orbhip.PREINT_FORM_WAVE)[0]}
        res["sweep"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
