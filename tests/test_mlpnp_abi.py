"""CPU tests of the MLPnPsolver interface: the C ABI symbols, defaults and sizes, the kernels in the library, the header as C99 and C++11,
the reference's own lines (src/Tracking.cc:2673-2674, :2697-2698) and host/MLPnPsolver.cc compiled -Wall -Werror against the stand-ins,
the class without a usable GPU (one message, bNoMore, an empty matrix, no CPU fallback) with the sets it drew from rand()'s unseeded
stream, and csrc/mlpnp_core.h in a stand-alone program under the address and undefined-behaviour sanitizers against the model."""
import ctypes
import os
import re
import subprocess
import numpy as np

import mlpnp_model as m
import synth_mlpnp as sy
import synth_sim3 as s3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_mlpnp_smoke")
SYMBOLS = ("orbhip_mlpnp_default_params", "orbhip_mlpnp_solver_device", "orbhip_mlpnp_solver_host")
F32 = np.float32


def test_symbols_declared_and_exported():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(orbhip.lib, s), s
    assert "orbhip_mlpnp_params" in txt
    p = orbhip.mlpnp_params()
    assert (p.probability, p.min_inliers, p.max_iterations, p.min_set, p.first_call_iterations, p.resume_at, p.draw_sets, p.seed) == \
        (0.99, 8, 300, 6, 0, 0, 1, 0)
    assert (F32(p.epsilon), F32(p.th2)) == (F32(0.4), F32(5.991))
    assert ctypes.sizeof(orbhip.MlpnpParams) == 48
    # the kernels are in the library: without csrc/mlpnp_kernels.hip there is nothing to launch
    names = subprocess.run(["strings", "-a", os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    for k in ("k_pnp_prepare", "k_pnp_hyp", "k_pnp_score", "k_pnp_decide"):
        assert k in names, k


def test_header_compiles_as_c99_and_cxx11(tmp_path):
    src = ('#include "orbhip.h"\nint f(void) { orbhip_mlpnp_params p; orbhip_mlpnp_default_params(&p); '
           'return (int)sizeof(p) + p.max_iterations + (sizeof(p) == 48 ? 0 : 1); }\n')
    for name, cmd in (("a.c", ["gcc", "-std=c99", "-pedantic"]), ("a.cc", ["g++", "-std=c++11", "-pedantic"])):
        f = tmp_path / name
        f.write_text(src)
        r = subprocess.run(cmd + ["-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / (name + ".o")), str(f)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]


def test_relocalization_lines_compile_against_the_host_class(tmp_path):
    obj = str(tmp_path / "reloc.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(HOST, "compile_callers_reloc.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    src = open(os.path.join(HOST, "compile_callers_reloc.cc")).read()
    for line in ("MLPnPsolver* pSolver = new MLPnPsolver(mCurrentFrame,vvpMapPointMatches[i]);",
                 "pSolver->SetRansacParameters(0.99,10,300,6,0.5,5.991);  //This solver needs at least 6 points",
                 "MLPnPsolver* pSolver = vpMLPnPsolvers[i];",
                 "cv::Mat Tcw = pSolver->iterate(5,bNoMore,vbInliers,nInliers);"):
        assert line in src
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::MLPnPsolver::" in ln]
    assert len(wanted) >= 3, undefined
    o = str(tmp_path / "solver.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "MLPnPsolver.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined]
    assert "ORB_SLAM3::MLPnPsolver::iterate(int, bool&, std::vector<bool" in defined
    assert "ORB_SLAM3::MLPnPsolver::SetRansacParameters(double, int, int, int, float, float)" in defined
    # the library entry point the class calls is what the library exports
    assert "orbhip_mlpnp_solver_host" in subprocess.run(["nm", "-u", o], stdout=subprocess.PIPE, text=True).stdout


def test_no_usable_gpu_says_no_more_and_returns_nothing(tmp_path):
    pb = sy.make_candidate(9777, 30)
    n = len(pb["Xw"])
    level = {float(v): k for k, v in enumerate(sy.SIGMA2)}
    arrays = dict(cam_type=np.array([0]), cam=np.array(list(pb["cam"]["K"]) + [0, 0, 0, 0], F32), sigma2=sy.SIGMA2, kp=pb["p2d"],
                  oct=np.array([level[float(v)] for v in pb["sigma2"]]), mp_pos=pb["Xw"], mp_bad=np.zeros(n, np.int32), matches=np.arange(n),
                  probability=np.array([0.99], F32), min_inliers=np.array([10]), max_iterations=np.array([300]), epsilon=np.array([0.5], F32),
                  th2=np.array([5.991], F32), n_iterations=np.array([5]))
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    s3.write_flat(fin, arrays)
    nmin, budget = m.ransac_parameters(n, 0.99, 10, 300, 6, 0.5)
    assert (nmin, budget) == (15, 35)
    r = subprocess.run([EXE, fin, fout, "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                       env=dict(os.environ, ORBHIP_DEVICE="4096"))    # no such device: the calling thread gets no context, here and on a GPU machine
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = s3.read_flat(fout)
    assert r.stderr.count("no device context") == 1 and "no CPU fallback" in r.stderr and len(r.stderr.splitlines()) == 1
    assert (out["calls"][0], out["ret_empty"].tolist(), out["no_more"].tolist(), out["n_inliers"].tolist()) == (1, [1], [1], [0])
    assert out["T"].size == 0 and out["inliers"].tolist() == [0]
    # the sets were drawn before the device was asked for: RandomInt's formula on rand() as a process starts it, 6 * max(budget, 5) at once
    libc = ctypes.CDLL(None)
    libc.srand(1)
    randint = lambda d: int((libc.rand() / (2147483647 + 1.0)) * d)
    assert np.array_equal(out["sets"].reshape(-1, 6), m.draw_sets_reference(n, budget, randint))


def test_core_header_under_sanitizers_against_the_model(tmp_path):
    """csrc/mlpnp_core.h in a stand-alone program (its own main) built with g++ -fsanitize=address,undefined: the 6-point and the N-point
    solve, planar and not, on candidates of the committed batch; the poses against the model, after rounding to float, within 4 x the
    model's own variant distance and at least one float ulp of the largest entry.  Only this program runs under the sanitizers."""
    exe = str(tmp_path / "core_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(ROOT, "orb-slam3-mac_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "mlpnp_core_check.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    problems, want = [], []
    grp, cands, ress = sy.gpu_batch_model(False)[0]
    for k in (0, 2, 5, 6):                                                      # n = 15, 64, and the two planar candidates
        (pb, sets), res = cands[k], ress[k]
        f = res["f"].astype(np.float64); X = pb["Xw"].astype(np.float64)
        good = np.nonzero(~pb["outlier_true"])[0]
        for idx in (good[:6], good[3:9], good):                                # two 6-point sets and all true inliers
            problems.append(np.c_[f[idx], X[idx]]); want.append(m.compute_pose(f[idx], X[idx]))
    text = "%d\n" % len(problems) + "".join("%d\n%s\n" % (len(p), "\n".join(" ".join(repr(float(v)) for v in row) for row in p)) for p in problems)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    got = np.array([[float(v) for v in ln.split()] for ln in r.stdout.splitlines()])
    assert got.shape == (len(problems), 12)
    measured = sy.measured_variant_distance(False)
    worst = 0.0
    for g, w in zip(got, want):
        a, b = g.astype(F32).astype(np.float64), w.astype(F32).astype(np.float64)
        d = float(np.abs(a - b).max())
        assert d <= max(4 * measured, float(np.spacing(F32(np.abs(b).max())))), (d, g, w)
        worst = max(worst, float(np.abs(g - w).max()))
    print("largest distance between the header and the model, in double: %.3e" % worst)
