#!/usr/bin/env python3
"""Timing of the batched MLPnPsolver: one device call for 3 candidates x 300 iterations x 200 matches (what a lost tracker's
three best BoW candidates cost; first_call_iterations = 300 so that every iteration is run, 40 % outliers), the same for 64 candidates,
the host form for one candidate, and beside them orbhip_sim3_solver_device on the same candidates x iterations x n in the same process.
Host clock around a call that ends in a synchronise, inputs resident, warmed up, median of 50.  No threshold: the reference solver
cannot be built here, so there is nothing to compare against.
    timeout -k 10 300 python tools/mlpnp_probe.py [out.json]
Every GPU step is a bounded number of calls."""
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import synth_mlpnp as sy  # noqa: E402
import synth_sim3_solver as s3s  # noqa: E402

N, ITS = 200, 300


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    ts = sorted(fn() for _ in range(reps))
    return dict(median_ms=ts[reps // 2], min_ms=ts[0], max_ms=ts[-1], reps=reps)


def main():
    import torch
    import orbhip
    out = {}
    ctx = orbhip.Context(0)
    pbs = [sy.make_candidate(9900 + k, N, outlier_share=0.4) for k in range(64)]
    sets = [sy.host_sets(9990 + k, N, ITS) for k in range(64)]
    cam = orbhip.sim3_camera(pbs[0]["cam"]["K"])
    p = orbhip.mlpnp_params(max_iterations=ITS, first_call_iterations=ITS, draw_sets=False)
    for C in (3, 64):
        A = [torch.from_numpy(np.stack([pbs[f][k] for f in range(C)])).cuda() for k in ("Xw", "p2d", "sigma2")]
        n = torch.full((C,), N, dtype=torch.int32, device="cuda"); S = torch.from_numpy(np.stack(sets[:C])).cuda()
        oc = torch.zeros(C, dtype=torch.uint8, device="cuda"); T = torch.zeros(C, 12, device="cuda")
        nin = torch.zeros(C, dtype=torch.int32, device="cuda"); inl = torch.zeros(C, N, dtype=torch.uint8, device="cuda")
        st = torch.zeros(C, 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def batch():
            t0 = time.perf_counter()
            orbhip.mlpnp_solver_device(ctx, A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), n.data_ptr(), C, N, cam, p, S.data_ptr(), oc.data_ptr(),
                                       T.data_ptr(), nin.data_ptr(), inl.data_ptr(), st.data_ptr())
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        out["mlpnp_device_batch_%dx%dx%d" % (C, ITS, N)] = dict(timed(batch), outcomes=oc.tolist()[:3], budget=st[:, 0].tolist()[:3],
                                                                 returned_at=st[:, 1].tolist()[:3], refine_runs=st[:, 3].tolist()[:3])
    ts = timed(lambda: _host(orbhip, ctx, pbs[0], cam, p, sets[0]))
    out["mlpnp_host_form_1x%dx%d" % (ITS, N)] = ts
    # the sibling solver on the same candidates x iterations x n
    pairs = [s3s.make_pair(7900 + k, N, outlier_share=0.4) for k in range(64)]
    psets = [s3s.host_sets(7990 + k, N, ITS) for k in range(64)]
    c1 = orbhip.sim3_camera(pairs[0]["cam1"]["K"])
    q = orbhip.sim3_solver_params(0.99, 15, ITS, False, False)
    for C in (3, 64):
        A = [torch.from_numpy(np.stack([pairs[f][k] for f in range(C)])).cuda() for k in ("X1c", "X2c", "max1", "max2")]
        n = torch.full((C,), N, dtype=torch.int32, device="cuda"); S = torch.from_numpy(np.stack(psets[:C])).cuda()
        conv = torch.zeros(C, dtype=torch.uint8, device="cuda"); R = torch.zeros(C, 9, device="cuda"); t = torch.zeros(C, 3, device="cuda")
        s = torch.zeros(C, device="cuda"); nin = torch.zeros(C, dtype=torch.int32, device="cuda"); inl = torch.zeros(C, N, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def sbatch():
            t0 = time.perf_counter()
            orbhip.sim3_solver_device(ctx, A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), A[3].data_ptr(), n.data_ptr(), C, N, c1, c1, q, S.data_ptr(),
                                      conv.data_ptr(), R.data_ptr(), t.data_ptr(), s.data_ptr(), nin.data_ptr(), inl.data_ptr())
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        out["sim3solver_device_batch_%dx%dx%d" % (C, ITS, N)] = timed(sbatch)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")


def _host(orbhip, ctx, pb, cam, p, sets):
    t0 = time.perf_counter()
    orbhip.mlpnp_solver_host(ctx, pb["Xw"], pb["p2d"], pb["sigma2"], cam, p, sets)
    return (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    main()
