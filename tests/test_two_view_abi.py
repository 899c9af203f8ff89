"""CPU tests of the two-view reconstruction's interface: the C ABI symbols, the reference's own call lines (src/Tracking.cc:1506-1538)
compiled against the host headers, TwoViewReconstruction::Reconstruct without a usable GPU (false, empty R21 / t21, a message, no CPU
fallback) and the host RANSAC set generator (DUtils::Random's scheme: 8 distinct indices < N per iteration, the same in every process)."""
import os
import re
import subprocess
import numpy as np
import synth_two_view as sy
import two_view_model as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_smoke")


def test_symbols_declared_and_exported():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for s in ("orbhip_tvr_default_params", "orbhip_two_view_reconstruct_device", "orbhip_two_view_reconstruct_host"):
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(orbhip.lib, s), s
    assert "orbhip_tvr_params" in txt and "orbhip_tvr_stats" in txt
    p = orbhip.tvr_params()
    assert (p.sigma, p.iterations, p.min_parallax, p.min_triangulated, p.draw_sets) == (1.0, 200, 1.0, 50, 1) and abs(p.rh_threshold - 0.5) < 1e-7


def test_tracking_initialization_lines_compile_against_the_host_classes(tmp_path):
    obj = str(tmp_path / "init.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(HOST, "compile_callers_init.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    src = open(os.path.join(HOST, "compile_callers_init.cc")).read()
    for line in ("if(mpCamera->ReconstructWithTwoViews(mInitialFrame.mvKeysUn,mCurrentFrame.mvKeysUn,mvIniMatches,Rcw,tcw,mvIniP3D,vbTriangulated))",
                 "Rcw.copyTo(Tcw.rowRange(0,3).colRange(0,3));", "tcw.copyTo(Tcw.rowRange(0,3).col(3));"):
        assert line in src
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines()
              if "ORB_SLAM3::TwoViewReconstruction::" in ln or "ORB_SLAM3::GeometricCamera::ReconstructWithTwoViews" in ln]
    assert any("ReconstructWithTwoViews" in w for w in wanted), undefined
    o = str(tmp_path / "tvr.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "TwoViewReconstruction.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined]
    assert "ORB_SLAM3::TwoViewReconstruction::Reconstruct(" in defined and "ORB_SLAM3::TwoViewReconstruction::TwoViewReconstruction(cv::Mat&, float, int)" in defined


def _smoke(tmp_path, tag, sc, cam=sy.K4, cam_type=0, env=None):
    fin, fout = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    sy.write_flat(fin, dict(kp1=sc["kp1"], kp2=sc["kp2"], matches=sc["matches12"], cam_type=np.array([cam_type]), cam=np.array(cam, np.float32)))
    r = subprocess.run([EXE, "tvr", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = sy.read_flat(fout)
    out["_stderr"] = r.stderr
    return out


def test_no_usable_gpu_returns_false_and_the_sets_are_the_same_in_every_process(tmp_path):
    sc = sy.scene("general", 1)
    N = len(tv.match_list(sc["matches12"], len(sc["kp2"]))[0])
    nogpu = {"ORBHIP_DEVICE": "4096"}                      # no such device: the calling thread gets no context, here and on a GPU machine
    a = _smoke(tmp_path, "a", sc, env=nogpu)
    b = _smoke(tmp_path, "b", sc, env=nogpu)
    assert a["ok"][0] == 0 and a["R21"].size == 0 and a["t21"].size == 0
    assert "no usable GPU" in a["_stderr"] and "no CPU fallback" in a["_stderr"]
    assert a["sizes"].tolist() == [len(sc["kp1"])] * 3 and not a["P3D"].any() and not a["tri"].any()
    sets = a["sets"].reshape(200, 8)
    s = np.sort(sets, axis=1)
    assert s.min() >= 0 and s.max() < N and np.all(s[:, 1:] != s[:, :-1])
    assert np.array_equal(a["sets"], b["sets"])
    assert len(np.unique(sets, axis=0)) > 190             # 200 draws, not one repeated
    # the reference's scheme (:81-96) replayed on the same rand() stream: srand(0), int(rand() / (RAND_MAX + 1.0) * d)
    import ctypes
    libc = ctypes.CDLL(None)
    libc.srand(0)
    expect = tv.draw_sets_reference(N, 200, lambda d: int((libc.rand() / (2147483647 + 1.0)) * d))
    assert np.array_equal(sets, expect)


def test_fisheye_keys_round_trip_to_the_pinhole_camera(tmp_path):
    """KannalaBrandt8::ReconstructWithTwoViews first undistorts both key sets to the pinhole K (a Newton inversion in double): keys
    distorted with the camera's own polynomial come back within 1e-3 px (~16 ulp of a float pixel coordinate)"""
    sc = sy.scene("general", 1)
    fe = dict(sc, kp1=sy.kb8_distort(sc["kp1"].astype(np.float64), sy.KB8_CAM).astype(np.float32),
              kp2=sy.kb8_distort(sc["kp2"].astype(np.float64), sy.KB8_CAM).astype(np.float32))
    out = _smoke(tmp_path, "fe", fe, cam=sy.KB8_CAM, cam_type=1, env={"ORBHIP_DEVICE": "4096"})
    err = np.abs(out["un1"].reshape(-1, 2) - sc["kp1"]).max()
    print("round trip: %.3g px" % err)
    assert err <= 1e-3
