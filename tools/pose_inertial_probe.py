#!/usr/bin/env python3
"""Latency / throughput of the inertial pose-only optimisations (orbhip_pose_inertial_optimization_host / _device) on one GPU:
one TUM-VI rig frame (~600 edges) through the host form in each mode, and a device-resident batch of 1024 stereo frames.
    python tools/pose_inertial_probe.py  ->  one JSON line"""
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import orbhip
    import synth_pose_inertial as sp
    ctx = orbhip.Context(0)
    res = {}
    rig = sp.rig("rig")
    for mode in (0, 1):
        fr, _ = sp.make_frame(1, "rig", mode, n_points=480)
        for _ in range(5):
            orbhip.pose_inertial_optimization_host(ctx, mode, False, rig, fr)
        ts = []
        for _ in range(50):
            t0 = time.perf_counter()
            orbhip.pose_inertial_optimization_host(ctx, mode, False, rig, fr)
            ts.append(time.perf_counter() - t0)
        res["host_call_ms_mode%d" % mode] = float(np.median(ts) * 1e3)
        res["edges_mode%d" % mode] = len(fr["Xw"])
    F, M = 1024, 400
    srig = sp.rig("stereo")
    frames = [sp.make_frame(1000 + (i % 64), "stereo", 1, n_points=300)[0] for i in range(F)]
    n = np.array([len(f["Xw"]) for f in frames], np.int32)
    z = lambda *s: np.zeros(s)
    Xw, obs, is2, knd, cl = z(F, M, 3), z(F, M, 3), z(F, M), np.zeros((F, M), np.uint8), np.zeros((F, M), np.uint8)
    for f, fr in enumerate(frames):
        k = n[f]; Xw[f, :k] = fr["Xw"]; obs[f, :k] = fr["obs"]; is2[f, :k] = fr["inv_sigma2"]; knd[f, :k] = fr["kind"]; cl[f, :k] = fr["close"]
    st = lambda key: np.stack([np.asarray(fr[key], np.float64).reshape(-1) for fr in frames])
    prior = np.stack([np.concatenate([fr["prior"], fr["prior_H"]]) for fr in frames])
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Xw, obs, is2, knd, cl, n, st("prev"), st("preint"), st("info"),
                                                                     st("info_g"), st("info_a"), prior)]
    s0 = torch.from_numpy(st("state")).cuda()
    state = s0.clone(); out = torch.zeros((F, M), dtype=torch.uint8, device="cuda")
    ret = torch.zeros(F, dtype=torch.int32, device="cuda"); H = torch.zeros((F, 225), dtype=torch.float64, device="cuda")

    def run():
        state.copy_(s0)
        orbhip.pose_inertial_optimization_device(ctx, 1, False, srig, F, M, *[x.data_ptr() for x in t], state.data_ptr(), out.data_ptr(),
                                                 ret.data_ptr(), H.data_ptr())
    for _ in range(3):
        run()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        run()
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / 10
    res.update(batch_frames=F, batch_edges_mean=float(n.mean()), batch_ms=dt * 1e3, batch_frames_per_s=F / dt)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
