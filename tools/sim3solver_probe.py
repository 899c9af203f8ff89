#!/usr/bin/env python3
"""Timing of the batched Sim3Solver: one device call for 3 candidates x 300 iterations x 200 correspondences (what
LoopClosing's three best BoW candidates cost), the same for 64 candidates, the host form for one candidate, and the numpy model's
single-thread time on one candidate.  Host clock around a call that ends in a synchronise, inputs resident, warmed up, median of 50.
    timeout -k 10 300 python tools/sim3solver_probe.py [out.json]
Every GPU step is a bounded number of calls."""
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import sim3_solver_model as m  # noqa: E402
import synth_sim3_solver as sy  # noqa: E402

N, ITS, MIN_INL = 200, 300, 15


def main():
    import torch
    import orbhip
    out = {}
    ctx = orbhip.Context(0)
    pbs = [sy.make_pair(7900 + k, N, outlier_share=0.4) for k in range(64)]
    sets = [sy.host_sets(7990 + k, N, ITS) for k in range(64)]
    c = orbhip.sim3_camera(pbs[0]["cam1"]["K"])
    p = orbhip.sim3_solver_params(0.99, MIN_INL, ITS, False, False)
    for P in (3, 64):
        A = [torch.from_numpy(np.stack([pbs[f][k] for f in range(P)])).cuda() for k in ("X1c", "X2c", "max1", "max2")]
        n = torch.full((P,), N, dtype=torch.int32, device="cuda"); S = torch.from_numpy(np.stack(sets[:P])).cuda()
        conv = torch.zeros(P, dtype=torch.uint8, device="cuda"); R = torch.zeros(P, 9, device="cuda"); t = torch.zeros(P, 3, device="cuda")
        s = torch.zeros(P, device="cuda"); nin = torch.zeros(P, dtype=torch.int32, device="cuda"); inl = torch.zeros(P, N, dtype=torch.uint8, device="cuda")
        st = torch.zeros(P, 3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def batch():
            t0 = time.perf_counter()
            orbhip.sim3_solver_device(ctx, A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), A[3].data_ptr(), n.data_ptr(), P, N, c, c, p, S.data_ptr(),
                                      conv.data_ptr(), R.data_ptr(), t.data_ptr(), s.data_ptr(), nin.data_ptr(), inl.data_ptr(), st.data_ptr())
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(5):
            batch()
        ts = sorted(batch() for _ in range(50))
        out["device_batch_%dx%dx%d" % (P, ITS, N)] = dict(median_ms=ts[25], min_ms=ts[0], max_ms=ts[-1], reps=50, converged=int(conv.sum()),
                                                          budget=st[:, 0].tolist()[:3], winner=st[:, 1].tolist()[:3])
    args = (ctx, pbs[0]["X1c"], pbs[0]["X2c"], pbs[0]["max1"], pbs[0]["max2"], c, c, p, sets[0])
    for _ in range(5):
        orbhip.sim3_solver_host(*args)
    ts = []
    for _ in range(50):
        t0 = time.perf_counter(); orbhip.sim3_solver_host(*args); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    out["host_form_1x%dx%d" % (ITS, N)] = dict(median_ms=ts[25], min_ms=ts[0], max_ms=ts[-1], reps=50)
    ctx.close()
    t0 = time.perf_counter()
    m.solve(pbs[0], sets[0], 0.99, MIN_INL, ITS)
    out["model_1x%dx%d" % (ITS, N)] = dict(total_ms=(time.perf_counter() - t0) * 1e3)
    txt = json.dumps(out, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
