"""CPU tests of the Sim3 refinement's interface: the C ABI symbols and the Python binding, LoopClosing's own call lines
(src/LoopClosing.cc:523-532, :736-742) compiled against the host headers, and Optimizer::OptimizeSim3 without a usable GPU (one
message, 0, nothing touched, no CPU fallback)."""
import os
import re
import subprocess
import numpy as np
import synth_sim3 as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_sim3_smoke")


def test_symbols_declared_exported_and_bound():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for name in ("orbhip_optimize_sim3_device", "orbhip_optimize_sim3_host"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name), name
    assert "orbhip_sim3_camera" in txt
    assert callable(orbhip.optimize_sim3_device) and callable(orbhip.optimize_sim3_host)
    c = orbhip.sim3_camera((1.0, 2.0, 3.0, 4.0), kb8=(5.0, 6.0, 7.0, 8.0))
    assert (c.fx, c.fy, c.cx, c.cy, c.camera_model, list(c.kb)) == (1.0, 2.0, 3.0, 4.0, 1, [5.0, 6.0, 7.0, 8.0])
    assert orbhip.sim3_camera((1, 2, 3, 4)).camera_model == 0


def test_loop_closing_lines_compile_against_the_host_classes(tmp_path):
    obj = str(tmp_path / "loop.o")
    src_path = os.path.join(HOST, "compile_callers_loop.cc")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, src_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    src = open(src_path).read()
    for line in ("int numOptMatches = Optimizer::OptimizeSim3(mpCurrentKF, pMatchedKF, vpMatchedMPs, gScm, 10, bFixedScale, mHessian7x7, true);",
                 "int numOptMatches = Optimizer::OptimizeSim3(mpCurrentKF, pKFi, vpMatchedMP, gScm, 10, mbFixScale, mHessian7x7, true);",
                 "g2o::Sim3 gSwm(Converter::toMatrix3d(mTwm.rowRange(0, 3).colRange(0, 3)),Converter::toVector3d(mTwm.rowRange(0, 3).col(3)),1.0);",
                 "g2o::Sim3 gScm = gScw * gSwm;", "Eigen::Matrix<double, 7, 7> mHessian7x7;"):
        assert line in src, line
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::Optimizer::OptimizeSim3" in ln]
    assert wanted, undefined
    o = str(tmp_path / "opt.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "Optimizer_OptimizeSim3.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined], (wanted, defined)


def test_no_usable_gpu_returns_zero_and_touches_nothing(tmp_path):
    sc = s.make_keyframes(9100)
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    s.write_flat(fin, sc)
    # no such device: the calling thread gets no context, here and on a GPU machine
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, ORBHIP_DEVICE="4096"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = s.read_flat(fout)
    assert out["ret"][0] == 0
    msgs = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(msgs) == 1 and "no CPU fallback" in msgs[0], r.stderr
    assert np.array_equal(out["matches_null"], (sc["matches"] < 0).astype(np.int32))          # vpMatches1 as given
    assert out["sim3"].tobytes() == sc["sim3"].tobytes()                                        # g2oS12 as given
    assert np.array_equal(out["hessian"].view(np.float64), np.full(49, 7.0))                    # mAcumHessian as given
