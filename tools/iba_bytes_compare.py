#!/usr/bin/env python3
"""Does a change to csrc/iba_kernels.hip or to the headers its kernels are made of (iba_edges.h, so3_f64.h, imu_layout.h, geom3.h,
ba_camera.h, ba_ldlt.h) leave Optimizer::LocalInertialBA's device path alone?  Solves tests/golden's windows
(synth_iba.load_golden_windows()) and two synthetic ones through orbhip_inertial_ba_solve_batch with two builds of liborbhip.so -- one
child process per library, each with its own HIP runtime -- and compares every output byte (keyframe states, points, outlier flags,
stats), with one workgroup per window and with the team grid.
    python tools/iba_bytes_compare.py <parent liborbhip.so> [<new liborbhip.so>]      (default: the tree's own build)
Exit status 0: byte-identical."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import synth_iba            # noqa: E402

vp, cd = C.c_void_p, C.c_double


class IbaWindow(C.Structure):           # orbhip_iba_window (include/orbhip.h)
    _fields_ = [("n_kf", C.c_int32), ("kf_fixed", vp), ("kf_imu", vp), ("Rcb", cd * 9), ("tcb", cd * 3),
                ("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("bf", cd),
                ("camera_model", C.c_int32), ("kb", cd * 4), ("has_cam2", C.c_int32), ("Trl", cd * 12),
                ("fx2", cd), ("fy2", cd), ("cx2", cd), ("cy2", cd), ("camera2_model", C.c_int32), ("kb2", cd * 4),
                ("n_points", C.c_int32), ("n_edges", C.c_int32), ("edge_kf", vp), ("edge_point", vp), ("edge_obs", vp),
                ("edge_stereo", vp), ("edge_inv_sigma2", vp), ("edge_close", vp),
                ("n_inertial", C.c_int32), ("in_kf1", vp), ("in_kf2", vp), ("in_preint", vp), ("in_info", vp),
                ("in_info_g", vp), ("in_info_a", vp), ("in_robust", vp)]


class IbaParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lambda_init", cd), ("large", C.c_int32), ("max_trials", C.c_int32)]


class IbaStats(C.Structure):
    _fields_ = [("iterations_run", C.c_int32), ("lm_trials", C.c_int32), ("n_outliers", C.c_int32), ("failed", C.c_int32), ("err", cd), ("err_end", cd)]


def windows():
    wins = [w for w, _ in synth_iba.load_golden_windows()]
    wins.append(synth_iba.make_window(21, n_opt=8, n_fixed_vis=10, n_points=300))
    wins.append(synth_iba.make_window(25, n_opt=8, n_fixed_vis=10, n_points=400, fisheye_rig=True))
    return wins


def solve(lib_path, out_path):
    lib = C.CDLL(lib_path)
    lib.orbhip_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.orbhip_ctx_destroy.argtypes = [vp]
    lib.orbhip_iba_default_params.argtypes = [C.POINTER(IbaParams), C.c_int]
    lib.orbhip_inertial_ba_solve_batch.argtypes = [vp, vp, C.c_int, C.POINTER(IbaParams), vp, vp, vp, vp]
    h = vp()
    assert lib.orbhip_ctx_create(0, None, C.byref(h)) == 0
    wins = windows()
    res = {}
    for team in ("1", "8"):
        os.environ["ORBHIP_IBA_TEAM"] = team
        for large in (0, 1):
            n = len(wins)
            p = IbaParams()
            lib.orbhip_iba_default_params(C.byref(p), large)
            arr = (IbaWindow * n)(*[w.struct(IbaWindow) for w in wins])
            kfs = [w.kf0.copy() for w in wins]; pts = [w.pts0.copy() for w in wins]
            outl = [np.zeros(max(w.n_edges, 1), np.uint8) for w in wins]
            stats = (IbaStats * n)()
            pk = (vp * n)(*[a.ctypes.data for a in kfs]); pq = (vp * n)(*[a.ctypes.data for a in pts]); po = (vp * n)(*[a.ctypes.data for a in outl])
            rc = lib.orbhip_inertial_ba_solve_batch(h, C.cast(arr, vp), n, C.byref(p), C.cast(pk, vp), C.cast(pq, vp), C.cast(po, vp), C.cast(stats, vp))
            assert rc == 0, rc
            for i in range(n):
                key = "t%s_l%d_w%d_" % (team, large, i)
                res[key + "kf"], res[key + "pts"], res[key + "out"] = kfs[i], pts[i], outl[i]
                res[key + "stats"] = np.frombuffer(bytes(stats[i]), np.uint8).copy()
    lib.orbhip_ctx_destroy(h)
    np.savez(out_path, **res)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--solve":
        return solve(sys.argv[2], sys.argv[3])
    parent = os.path.abspath(sys.argv[1])
    new = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "liborbhip.so")
    with tempfile.TemporaryDirectory() as tmp:
        outs = []
        for name, lib in (("parent", parent), ("new", new)):
            out = os.path.join(tmp, name + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--solve", lib, out], check=True, timeout=300)
            outs.append(np.load(out))
        a, b = outs
        assert sorted(a.files) == sorted(b.files)
        diff = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
        print("orbhip_inertial_ba_solve_batch, %d outputs (4 windows x bLarge 0 / 1 x team 1 / 8): %s" %
              (len(a.files), "byte-identical" if not diff else "DIFFERENT: " + ", ".join(diff)))
        for k in diff:
            if a[k].dtype == np.float64:
                print("  %s max |difference| %.3g" % (k, np.abs(a[k] - b[k]).max()))
        return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
