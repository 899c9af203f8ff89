#!/usr/bin/env python3
"""Times of the SearchLocalPoints stage (orbhip_frustum_queries_device / orbhip_search_local_points_device and the class method) on one GPU:
  * the frustum kernel's call on 1 frame x 4096 points and on 1024 frames x 1000 points (scenes of tests/synth_frustum.py, 8 distinct ones
    tiled): host clock around `--queue` queued calls that end in one synchronise, divided by their number.  The kernel's own duration comes
    from a separate run of this script under `rocprofv3 --kernel-trace --stats` with --kernels-only;
  * the composed call (frustum -> matcher) on 1024 frames x 1000 points beside the matcher alone on the queries the first call left;
  * the call latency of the class method Tracking::SearchLocalPoints (lib/host_frustum_smoke track) beside what a caller had before for the
    same inputs -- the host member Frame::isInFrustum in a loop, then ORBmatcher::SearchByProjection(F, vpMapPoints, ...) (`today`) --
    1000 local points and a frame of a few hundred keypoints built from their projections, 30 runs each (every process's first run is
    left out), the two programs alternating;
  * the scenes' outcome histograms.
    python tools/frustum_probe.py [--out profiles/frustum_probe.json]  ->  one JSON line"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, sync, queue, warm=3, reps=10):
    """median / min / max over reps of (queue calls + one synchronise) / queue, in ms"""
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(queue):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / queue)
    return dict(median_ms=float(np.median(ts) * 1e3), min_ms=float(np.min(ts) * 1e3), max_ms=float(np.max(ts) * 1e3), queue=queue, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--queue", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="only the device calls, a few times each (the run to put under rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import orbhip
    import frustum_model as fm
    import synth_frustum as sf
    import test_gpu_frustum as tg
    ctx = orbhip.Context(0)
    res = dict(frames=a.frames, points=a.points)

    # ---- the frustum kernel alone
    fr1, pts1 = sf.make_scene("mono", 4096, 40)
    t1, recs1 = tg._upload([(fr1, pts1)], 4096, 4096)

    def frustum(t, recs, fr, max_points, max_q):
        orbhip.frustum_queries_device(ctx, recs, max_points, t["Xw"].data_ptr(), t["normal"].data_ptr(), t["min_dist"].data_ptr(), t["max_dist"].data_ptr(),
                                      t["flags"].data_ptr(), t["desc"].data_ptr(), t["track_depth"].data_ptr(), fr["bounds"], max_q, t["track"].data_ptr(),
                                      t["ntm"].data_ptr(), t["q"].data_ptr(), t["dq"].data_ptr(), t["owner"].data_ptr(), t["nq"].data_ptr())
    cases = [tg._chain_case("mono", a.points, 50 + k) for k in range(8)]
    hist = sf.histogram(cases[0][0], cases[0][2])
    res["scene_outcomes_left"] = hist["left"].tolist(); res["scene_levels"] = hist["levels"].tolist()
    tiled = [cases[f % 8] for f in range(a.frames)]
    max_n = max(len(c[4]["kp"]) for c in cases)
    res["keypoints_per_frame"] = int(np.mean([len(c[4]["kp"]) for c in cases])); res["queries_per_frame"] = int(np.mean([len(c[5]) for c in cases]))
    tN, recsN = tg._upload([(c[0], c[1]) for c in tiled], a.points, a.points)
    kp = np.zeros((a.frames, max_n), orbhip.KP_DTYPE); desc = np.zeros((a.frames, max_n, 32), np.uint8); nn = np.zeros(a.frames, np.int32)
    tm0 = np.full((a.frames, max_n), -1, np.int32)
    for f, c in enumerate(tiled):
        n = len(c[4]["kp"]); kp[f, :n] = c[4]["kp"]; desc[f, :n] = c[4]["desc"]; nn[f] = n; tm0[f, :n] = c[4]["train_match"]
    d = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in dict(kp=kp, desc=desc, n=nn, tm0=tm0).items()}
    d["tm"] = d["tm0"].clone(); d["nm"] = torch.zeros(a.frames, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b = cases[0][0]["bounds"]

    def chain():
        d["tm"].copy_(d["tm0"]); torch.cuda.current_stream().synchronize()
        orbhip.search_local_points_device(ctx, recsN, a.points, tN["Xw"].data_ptr(), tN["normal"].data_ptr(), tN["min_dist"].data_ptr(), tN["max_dist"].data_ptr(),
                                          tN["flags"].data_ptr(), tN["desc"].data_ptr(), tN["track_depth"].data_ptr(), a.points, d["kp"].data_ptr(),
                                          d["desc"].data_ptr(), None, d["n"].data_ptr(), None, None, max_n, max_n, b, 100, 0.8, tN["track"].data_ptr(),
                                          tN["ntm"].data_ptr(), tN["q"].data_ptr(), tN["dq"].data_ptr(), tN["owner"].data_ptr(), tN["nq"].data_ptr(),
                                          d["tm"].data_ptr(), d["nm"].data_ptr())

    def matcher():
        d["tm"].copy_(d["tm0"]); torch.cuda.current_stream().synchronize()
        orbhip.search_local_map_device(ctx, tN["q"].data_ptr(), tN["dq"].data_ptr(), tN["nq"].data_ptr(), a.points, d["kp"].data_ptr(), d["desc"].data_ptr(), None,
                                       d["n"].data_ptr(), max_n, max_n, a.frames, b, 100, 0.8, d["tm"].data_ptr(), d["nm"].data_ptr())
    if a.kernels_only:
        for _ in range(5):
            frustum(t1, recs1, fr1, 4096, 4096); ctx.synchronize()
            frustum(tN, recsN, cases[0][0], a.points, a.points); ctx.synchronize()
            chain(); ctx.synchronize()
        print(json.dumps(dict(kernels_only=True)))
        return
    res["frustum_1x4096"] = timed(lambda: frustum(t1, recs1, fr1, 4096, 4096), ctx.synchronize, a.queue)
    res["frustum_%dx%d" % (a.frames, a.points)] = timed(lambda: frustum(tN, recsN, cases[0][0], a.points, a.points), ctx.synchronize, a.queue)
    res["frustum_1x4096_single_call"] = timed(lambda: frustum(t1, recs1, fr1, 4096, 4096), ctx.synchronize, 1, reps=30)
    chain(); ctx.synchronize(); ctx.check_status()
    res["matches_per_frame"] = float(d["nm"].cpu().numpy().mean())
    # (each timed call resets the claims first: a device-to-device copy that both sides pay)
    res["chain_%dx%d" % (a.frames, a.points)] = timed(chain, ctx.synchronize, 1, reps=15)
    res["matcher_alone_%dx%d" % (a.frames, a.points)] = timed(matcher, ctx.synchronize, 1, reps=15)
    res["chain_again"] = timed(chain, ctx.synchronize, 1, reps=15)
    ctx.check_status()

    # ---- the class method beside what a caller had before, one frame of 1000 local points
    smoke = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_frustum_smoke")
    inp, want = tg._drop_in_case("mono", 60, n_points=1000, n_target=1000)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "in.bin")
    sf.write_flat(path, inp)
    lat = {"track": [], "today": []}
    for rnd in range(3):                                                        # the two programs alternate: other work shares the host
        for mode in ("track", "today"):
            out = subprocess.run([smoke, mode, path, os.path.join(tmp, "out.bin"), "10"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if out.returncode != 0:
                raise RuntimeError(out.stdout[-2000:])
            lat[mode] += [float(x) for x in re.findall(r"run \d+: ([0-9.]+) ms", out.stdout)]
    for mode, name in (("track", "class_SearchLocalPoints"), ("today", "host_isInFrustum_loop_then_SearchByProjection")):
        v = np.array(lat[mode])
        res[name] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), p10_ms=float(np.percentile(v, 10)),
                         p90_ms=float(np.percentile(v, 90)), runs=len(v))
    res["class_case"] = dict(points=len(inp["min_dist"]), keypoints=len(inp["oct"]), matches=int(want["ret"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
