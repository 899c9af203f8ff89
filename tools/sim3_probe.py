#!/usr/bin/env python3
"""Timing of the Sim3 refinement: one call of the class method (lib/host_sim3_smoke, ~100 edges), the host form for one pair
of 100 edges, device batches of 64 and 1024 pairs x 200 edges, and the numpy model's single-thread time on the same inputs.
    timeout -k 10 300 python tools/sim3_probe.py [out.json]
Every GPU step is a bounded number of calls; the child process runs under its own timeout."""
import json
import os
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import sim3_opt_model as m  # noqa: E402
import synth_sim3 as s  # noqa: E402


def med(f, reps, warm=3):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return dict(median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1], reps=reps)


def main():
    import torch
    import orbhip
    out = {}
    ctx = orbhip.Context(0)
    # ---- one pair of 100 edges: host form and model
    p = s.make_pair(7700, 100, outliers=10, no_kp2=0.1)
    c = orbhip.sim3_camera(p["cam1"]["K"])
    args = (ctx, p["P1c"], p["P2c"], p["obs1"], p["obs2"], p["w1"], p["w2"], c, c, p["th2"], False, p["sim3"])
    out["host_form_100_edges"] = med(lambda: orbhip.optimize_sim3_host(*args), 50)
    out["model_100_edges"] = med(lambda: m.solve(p), 5, warm=1)
    # ---- 64 and 1024 pairs x 200 edges, device form (inputs resident; the 1024 are the 64 repeated)
    probs = [s.make_pair(7800 + k, 200, outliers=20, no_kp2=0.1) for k in range(64)]
    E = 200
    for P in (64, 1024):
        A = {k: torch.from_numpy(np.stack([probs[f % 64][k] for f in range(P)])).cuda() for k in ("P1c", "P2c", "obs1", "obs2", "w1", "w2")}
        n = torch.full((P,), E, dtype=torch.int32, device="cuda")
        s0 = torch.from_numpy(np.stack([probs[f % 64]["sim3"] for f in range(P)])).cuda()
        sim3 = s0.clone(); flag = torch.zeros((P, E), dtype=torch.uint8, device="cuda"); nin = torch.zeros(P, dtype=torch.int32, device="cuda")
        st = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def batch():
            sim3.copy_(s0); torch.cuda.synchronize()
            t0 = time.perf_counter()
            orbhip.optimize_sim3_device(ctx, A["P1c"].data_ptr(), A["P2c"].data_ptr(), A["obs1"].data_ptr(), A["obs2"].data_ptr(), A["w1"].data_ptr(),
                                        A["w2"].data_ptr(), n.data_ptr(), P, E, c, c, 10.0, False, sim3.data_ptr(), flag.data_ptr(), nin.data_ptr(), st.data_ptr())
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(3):
            batch()
        t = sorted(batch() for _ in range(30))
        out["device_batch_%dx200" % P] = dict(median_ms=t[15], min_ms=t[0], max_ms=t[-1], reps=30, lm_trials_mean=float(st[:, 3].float().mean()))
    t0 = time.perf_counter()
    for q in probs:
        m.solve(q)
    out["model_64x200"] = dict(total_ms=(time.perf_counter() - t0) * 1e3)
    ctx.close()
    # ---- the class method (its own process: packing + one host-form call)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "a.in"), os.path.join(d, "a.out")
        s.write_flat(fin, s.make_keyframes(9210, n=130))
        r = subprocess.run([os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_sim3_smoke"), fin, fout, "50"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        out["class_method"] = [ln for ln in r.stdout.splitlines() if "median" in ln or "matches given" in ln]
    txt = json.dumps(out, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
