#!/usr/bin/env python3
"""Wall time of one LocalMapping::CreateNewMapPoints call (the class drop-in, lib/host_newpoints_smoke in `time` mode) on a synthetic
stereo keyframe with NEIGH neighbours of N keypoints each (tests/synth_new_points.py scenes; default 20 x 1000).
    python tools/newpoints_probe.py [N] [NEIGH]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import synth_new_points as sy                      # noqa: E402
from synth_sim3 import write_flat                  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    neigh = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    pairs = sy.make_world("stereo", 5, n1=n, n2s=(n,) * neigh)["pairs"]
    T44 = lambda r: np.concatenate([np.asarray(r, np.float32).reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)])
    a = dict(cam_type=np.array([0]), cam=sy.PIN, cam2=sy.PIN, monocular=np.array([0]), inertial=np.array([0]), far_points=np.array([0]),
             th_far=np.array([0], np.float32), scale=sy.SCALE, sigma2=sy.SIGMA2, check_true_at=np.array([-1]), tlr=np.eye(4, dtype=np.float32),
             nkf=np.array([neigh + 1]), nleft=np.full(neigh + 1, -1))

    def put(k, Tcw, mb, kp, raw, ur, dp, desc, nid):
        a["Tcw%d" % k] = Tcw; a["mb%d" % k] = np.array([mb], np.float32)
        a["kp%d" % k] = np.stack([kp["x"], kp["y"]], 1); a["raw%d" % k] = np.stack([raw["x"], raw["y"]], 1); a["oct%d" % k] = kp["octave"]
        a["ur%d" % k] = ur; a["dp%d" % k] = dp; a["desc%d" % k] = desc; a["nid%d" % k] = nid
        a["mp%d" % k] = np.zeros(len(kp), np.int32); a["mpx%d" % k] = np.zeros((len(kp), 3), np.float32)
    p0 = pairs[0]
    put(0, T44(p0["P"]["Tcw1"][0]), p0["P"]["mb1"], p0["kp1"], p0["kp1_raw"], p0["ur1"], p0["depth1"], p0["d1"], p0["nid1"])
    for k, pr in enumerate(pairs, start=1):
        put(k, T44(pr["P"]["Tcw2"][0]), pr["P"]["mb2"], pr["kp2"], pr["kp2_raw"], pr["ur2"], pr["depth2"], pr["d2"], pr["nid2"])
    with tempfile.TemporaryDirectory() as d:
        fin = os.path.join(d, "np.in")
        write_flat(fin, a)
        exe = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_newpoints_smoke")
        sys.exit(subprocess.run([exe, fin, os.path.join(d, "np.out"), "time"]).returncode)


if __name__ == "__main__":
    main()
