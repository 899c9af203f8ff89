"""CPU tests of the Sim3Solver interface: the C ABI symbols and defaults, the header as C99 and C++11, the reference's own lines
(src/LoopClosing.cc:669-684, :720) and host/Sim3Solver.cc compiled -Wall -Werror against the stand-ins, and the class without a usable
GPU (one message, bNoMore, an empty matrix, no inliers, no CPU fallback) -- with the sets it drew from rand()'s unseeded stream."""
import ctypes
import os
import re
import subprocess
import numpy as np
import sim3_solver_model as m
import synth_sim3_solver as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_sim3solver_smoke")
SYMBOLS = ("orbhip_sim3solver_default_params", "orbhip_sim3_solver_device", "orbhip_sim3_solver_host")


def test_symbols_declared_and_exported():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(orbhip.lib, s), s
    assert "orbhip_sim3solver_params" in txt
    p = orbhip.sim3_solver_params()
    assert (p.probability, p.min_inliers, p.max_iterations, p.fix_scale, p.draw_sets, p.seed) == (0.99, 6, 300, 0, 1, 0)
    assert ctypes.sizeof(orbhip.Sim3SolverParams) == 32
    # the kernels are in the library: without csrc/sim3solver_kernels.hip there is nothing to launch
    names = subprocess.run(["strings", "-a", os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    for k in ("k_s3s_prepare", "k_s3s_hyp", "k_s3s_score", "k_s3s_decide"):
        assert k in names, k


def test_header_compiles_as_c99_and_cxx11(tmp_path):
    src = '#include "orbhip.h"\nint f(void) { orbhip_sim3solver_params p; orbhip_sim3solver_default_params(&p); return (int)sizeof(p) + p.max_iterations; }\n'
    for name, cmd in (("a.c", ["gcc", "-std=c99", "-pedantic"]), ("a.cc", ["g++", "-std=c++11", "-pedantic"])):
        f = tmp_path / name
        f.write_text(src)
        r = subprocess.run(cmd + ["-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / (name + ".o")), str(f)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]


def test_loop_closing_lines_compile_against_the_host_class(tmp_path):
    obj = str(tmp_path / "loop.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(HOST, "compile_callers_loop_sim3.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    src = open(os.path.join(HOST, "compile_callers_loop_sim3.cc")).read()
    for line in ("Sim3Solver solver = Sim3Solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);",
                 "solver.SetRansacParameters(0.99, nBoWInliers, 300); // at least 15 inliers",
                 "mTcm = solver.iterate(20,bNoMore, vbInliers, nInliers, bConverge);",
                 "g2o::Sim3 gScm(Converter::toMatrix3d(solver.GetEstimatedRotation()),Converter::toVector3d(solver.GetEstimatedTranslation()),solver.GetEstimatedScale());"):
        assert line in src
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::Sim3Solver::" in ln]
    assert len(wanted) >= 6, undefined
    o = str(tmp_path / "solver.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "Sim3Solver.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined]
    assert "ORB_SLAM3::Sim3Solver::find(" in defined and "ORB_SLAM3::Sim3Solver::iterate(int, bool&, std::vector<bool" in defined
    # the library entry point the class calls is what the library exports
    assert "orbhip_sim3_solver_host" in subprocess.run(["nm", "-u", o], stdout=subprocess.PIPE, text=True).stdout


def test_no_usable_gpu_says_no_more_and_returns_nothing(tmp_path):
    spec = sy.CLASS_SCENES["own_keyframe"]
    sc = sy.make_scene(**spec)
    pb, index, n1 = sy.class_problem(sc)
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    sy.s3.write_flat(fin, sc)
    budget = m.iteration_budget(len(index), 0.99, int(sc["min_inliers"][0]), int(sc["max_iterations"][0]))
    assert budget == 300
    for mode, pre in (("loop", ""), ("find", "find_")):
        r = subprocess.run([EXE, fin, fout, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                           env=dict(os.environ, ORBHIP_DEVICE="4096"))    # no such device: the calling thread gets no context, here and on a GPU machine
        assert r.returncode == 0, (r.stdout, r.stderr)
        out = sy.s3.read_flat(fout)
        assert r.stderr.count("no device context") == 1 and "no CPU fallback" in r.stderr and len(r.stderr.splitlines()) == 1
        if mode == "loop":
            assert (out["converged"][0], out["no_more"][0], out["calls"][0]) == (0, 1, 1)
        assert out[pre + "T"].size == 0 and out[pre + "n_inliers"][0] == 0 and out[pre + "R"].size == 0
        assert len(out[pre + "inliers"]) == n1 and not out[pre + "inliers"].any()
        # the sets were drawn before the device was asked for: RandomInt's formula on rand() as a process starts it, 3 * mRansacMaxIts at once
        libc = ctypes.CDLL(None)
        libc.srand(1)
        randint = lambda d: int((libc.rand() / (2147483647 + 1.0)) * d)
        assert np.array_equal(out[pre + "sets"].reshape(-1, 3), m.draw_sets_reference(len(index), budget, randint))
