#!/usr/bin/env python3
"""Time of the two-view reconstruction (orbhip_two_view_reconstruct_device / _host) on one GPU:
  * one device call on 1024 pairs x 200 iterations x ~300 matches (synthetic pairs of tests/synth_two_view.py, 64 distinct ones tiled),
    host clock around calls that end in a synchronise; per-stage kernel times come from a separate run of this script under
    `rocprofv3 --kernel-trace --stats` (tools/tvr_stage_summary.py reads its kernel_stats csv);
  * extract -> match -> reconstruct (device-drawn sets) on the benchmark's VGA batch next to extract -> match alone;
  * one pair through the host form (what the TwoViewReconstruction class calls);
  * the float32 numpy model's single-thread time per pair, labelled "model": the only CPU figure available, NOT the reference.
    python tools/tvr_probe.py [--pairs 1024] [--batch 1024]  ->  one JSON line"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, sync, warm=3, reps=10):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3), float(np.max(ts) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1024, help="frames of the extract -> match -> reconstruct chain (VGA)")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--device-call-only", action="store_true", help="only the batched device call (the run to put under rocprofv3 for per-stage times)")
    a = ap.parse_args()
    import torch
    import orbhip
    import synth_two_view as sy
    import two_view_model as tv
    ctx = orbhip.Context(0)
    res = {}
    # ---- one call on `pairs` synthetic pairs
    P, IT, max_n = a.pairs, a.iterations, 2048
    kinds = ["general", "plane_a", "plane_b", "lowpar"]
    scenes = [sy.scene(kinds[i % 4], 100 + i) for i in range(64)]
    kp1 = np.zeros((P, max_n), orbhip.KP_DTYPE); kp2 = np.zeros((P, max_n), orbhip.KP_DTYPE)
    n1 = np.zeros(P, np.int32); n2 = np.zeros(P, np.int32); m12 = np.full((P, max_n), -1, np.int32)
    for p in range(P):
        s = scenes[p % 64]
        n1[p], n2[p] = len(s["kp1"]), len(s["kp2"])
        kp1[p, :n1[p]]["x"] = s["kp1"][:, 0]; kp1[p, :n1[p]]["y"] = s["kp1"][:, 1]
        kp2[p, :n2[p]]["x"] = s["kp2"][:, 0]; kp2[p, :n2[p]]["y"] = s["kp2"][:, 1]
        m12[p, :n1[p]] = s["matches12"]
    res["pairs"], res["iterations"] = P, IT
    res["matches_per_pair_mean"] = float(np.mean([(s["matches12"] >= 0).sum() for s in scenes]))
    t = [torch.from_numpy(x.view(np.uint8) if x.dtype == orbhip.KP_DTYPE else x).cuda() for x in (kp1, n1, kp2, n2, m12)]
    sets = torch.zeros((P, IT, 8), dtype=torch.int32, device="cuda")
    ok = torch.zeros(P, dtype=torch.uint8, device="cuda"); R = torch.zeros((P, 9), device="cuda"); tt = torch.zeros((P, 3), device="cuda")
    P3D = torch.zeros((P, max_n, 3), device="cuda"); tri = torch.zeros((P, max_n), dtype=torch.uint8, device="cuda")
    prm = orbhip.tvr_params(IT, 1.0, 0.5, True, 1)

    def call():
        orbhip.two_view_reconstruct_device(ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), max_n, t[4].data_ptr(), P, max_n,
                                           sy.K4, prm, sets.data_ptr(), ok.data_ptr(), R.data_ptr(), tt.data_ptr(), P3D.data_ptr(), tri.data_ptr())
    res["device_call_ms_median_min_max"] = timed(call, ctx.synchronize)
    res["pairs_ok"] = int(ok.sum().item())
    if a.device_call_only:
        ctx.close()
        print(json.dumps(res))
        return
    # ---- the chain on the benchmark's VGA batch
    B, W, H = a.batch, 640, 480
    imgs = orbhip.synth_frames(W, H, B, seed=20241004)
    d = torch.from_numpy(imgs).cuda()
    ext = orbhip.Extractor(ctx, 1000, 1.2, 8, 20, 7); ext.reserve(W, H, B)
    mk = ext.max_keypoints
    kp, desc, cnt, _ = ext.results_device()
    prev = torch.zeros((B, mk, 2), dtype=torch.float32, device="cuda")
    cm12 = torch.full((B, mk), -1, dtype=torch.int32, device="cuda"); nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    Q = B - 1
    csets = torch.zeros((Q, IT, 8), dtype=torch.int32, device="cuda")
    cok = torch.zeros(Q, dtype=torch.uint8, device="cuda"); cR = torch.zeros((Q, 9), device="cuda"); ct = torch.zeros((Q, 3), device="cuda")
    cP = torch.zeros((Q, mk, 3), device="cuda"); ctri = torch.zeros((Q, mk), dtype=torch.uint8, device="cuda")
    Kvga = (458.654, 457.296, 320.0, 240.0)

    def front():
        ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
        orbhip.prev_matched_init_device(ctx, kp, mk, Q, mk, prev.data_ptr())
        orbhip.search_for_initialization_device(ctx, kp, desc, cnt, kp + mk * 28, desc + mk * 32, cnt + 4, Q, mk, mk, (0.0, 0.0, float(W), float(H)), 100, 0.9,
                                                True, prev.data_ptr(), cm12.data_ptr(), nm.data_ptr())

    def chain():
        front()
        orbhip.two_view_reconstruct_device(ctx, kp, cnt, kp + mk * 28, cnt + 4, mk, cm12.data_ptr(), Q, mk, Kvga, prm, csets.data_ptr(), cok.data_ptr(),
                                           cR.data_ptr(), ct.data_ptr(), cP.data_ptr(), ctri.data_ptr())
    res["chain_frames"] = B
    res["extract_match_ms_median_min_max"] = timed(front, ctx.synchronize)
    res["extract_match_reconstruct_ms_median_min_max"] = timed(chain, ctx.synchronize)
    res["chain_matches_per_pair_mean"] = float(nm[:Q].float().mean().item())
    ext.close()
    # ---- one pair through the host form
    s = scenes[0]
    hk1 = kp1[0, :n1[0]].copy(); hk2 = kp2[0, :n2[0]].copy()
    hp = orbhip.tvr_params(IT, 1.0, 0.5, False)
    hsets = sy.model_sets("probe", int((s["matches12"] >= 0).sum()), IT)
    res["host_call_one_pair_ms_median_min_max"] = timed(lambda: orbhip.two_view_reconstruct_host(ctx, hk1, hk2, s["matches12"], sy.K4, hp, hsets), lambda: None,
                                                        warm=5, reps=50)
    # ---- the numpy model, one thread (the only CPU figure there is: a model, not the reference)
    t0 = time.perf_counter()
    for i in range(4):
        tv.reconstruct(scenes[i]["kp1"], scenes[i]["kp2"], scenes[i]["matches12"], sy.K4, hsets if i == 0 else sy.model_sets("probe%d" % i, int((scenes[i]["matches12"] >= 0).sum()), IT), np.float32)
    res["model_float32_numpy_ms_per_pair"] = float((time.perf_counter() - t0) / 4 * 1e3)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
