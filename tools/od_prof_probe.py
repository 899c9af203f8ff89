#!/usr/bin/env python3
"""Phase split of the descriptor kernel (k_orient_desc_tiled, or k_orient_desc with ORBHIP_BLUR_TILED=0) on the bench's default workload
(1024 VGA frames), from the cycle counters of a DEBUG build:
     make -C orb-slam3-mac_amd EXTRA=-DOD_PROF -B build/desc_kernels.o lib/liborbhip.so && python tools/od_prof_probe.py
Prints wave-cycles per phase (summed over the waves) as shares of the kernel's wave time, and cycles per trip (one wave, four keypoints).
OD_B sets the batch, ORBHIP_TUNE_DESC_BLOCKS the workgroups per XCD."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import torch
import orbhip
import bench

B, W, H = int(os.environ.get("OD_B", 1024)), 640, 480
imgs = bench.synth_frames_parallel(orbhip, W, H, B, 20241004, 0)
d = torch.from_numpy(imgs).cuda()
ctx = orbhip.Context(0)
ext = orbhip.Extractor(ctx, 1000, 1.2, 8, 20, 7)
ext.reserve(W, H, B)
fn = orbhip.lib.orbhip_debug_od_prof
fn.argtypes = [C.c_void_p, C.c_int]
for _ in range(2):
    ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
ctx.synchronize()
out = (C.c_ulonglong * 12)()
assert fn(out, 1) == 0
N = 3
for _ in range(N):
    ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
ctx.synchronize()
assert fn(out, 0) == 0
v = [int(x) for x in out]
names = ["head: top of trip -> header known", "issue of the patch loads", "wait for the patch data", "lds + moments", "lds + angle, sine, cosine",
         "BRIEF + stores", "skipped trips"]
tot, trips = v[9], max(v[7], 1)
res = {"frames": B, "launches": N, "trips_per_launch": v[7] // N, "skipped_trips_per_launch": v[8] // N, "wave_cycles_per_launch": tot // N,
       "cycles_per_trip": round(sum(v[:6]) / trips, 1),
       "share": {n: round(v[i] / tot, 4) for i, n in enumerate(names)}, "cycles_per_trip_by_phase": {n: round(v[i] / trips, 1) for i, n in enumerate(names[:6])},
       "prologue_share": round(v[10] / tot, 4), "unaccounted_share": round(1 - (sum(v[:7]) + v[10]) / tot, 4)}
print(json.dumps(res))
