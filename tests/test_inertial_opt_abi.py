"""CPU tests of the inertial initialisation's interface: the C ABI symbols, the kernel in the library, the header as C99 / C++11, the
default parameters of the four overloads, the reference's own call lines (src/LocalMapping.cc:1306, :1428, src/LoopClosing.cc:2026)
compiled against the host headers, the host-side packing under AddressSanitizer / UBSan in a stand-alone program, and the class without
a usable GPU (one message, everything unchanged, no CPU fallback)."""
import os
import re
import subprocess
import numpy as np
import inertial_opt_cases as ic
import inertial_opt_model as iom
import synth_inertial_opt as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
HOST = os.path.join(PKG, "host")
EXE = os.path.join(PKG, "lib", "host_inertial_opt_smoke")
NAMES = ("orbhip_inertial_opt_default_params", "orbhip_inertial_opt_lds_keyframes", "orbhip_inertial_optimization_device",
         "orbhip_inertial_optimization_host")


def test_symbols_declared_exported_and_bound():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name), name
    assert "orbhip_inertial_opt_params" in txt and "ORBHIP_IO_GLOBAL 16" in txt
    assert orbhip.inertial_opt_lds_keyframes() == int(re.search(r"#define ORBHIP_IO_LDS_KEYFRAMES (\d+)", txt).group(1))
    so = os.path.join(PKG, "lib", "liborbhip.so")
    strings = subprocess.run(["strings", so], stdout=subprocess.PIPE, text=True).stdout
    assert "k_inertial_opt" in strings
    for f in (orbhip.inertial_opt_params, orbhip.inertial_optimization_device, orbhip.inertial_optimization_host):
        assert callable(f)


def test_header_compiles_as_c99_and_cxx11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "orbhip.h"\nint f(void) { orbhip_inertial_opt_params p; orbhip_inertial_opt_default_params(&p, 0, 1, 0, 1e2f, 1e6f); '
                   'return p.iterations + ORBHIP_IO_GLOBAL + ORBHIP_IO_LDS_KEYFRAMES; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-x", "c"], ["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++"]):
        r = subprocess.run(cmd + ["-I", inc, "-c", "-o", str(tmp_path / "t.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]


def test_default_parameters_of_the_four_overloads():
    import orbhip
    fields = ("free_vel_bias", "free_gdir", "free_scale", "gauss_newton", "iterations", "max_trials", "lambda_init", "prior_g", "prior_a")
    table = {   # (overload, mono, fixed_vel, priorG, priorA) -> the issue's table
        (0, 1, 0, 1e2, 1e6): (1, 1, 1, 0, 200, 100, 1e3, 1e2, 1e6),
        (0, 0, 0, 1e2, 1e6): (1, 1, 0, 0, 200, 100, 1e3, 1e2, 1e6),
        (0, 1, 1, 1e2, 1e6): (0, 1, 1, 0, 200, 100, 1e3, 1e2, 1e6),
        (0, 1, 0, 0.0, 1e6): (1, 1, 1, 0, 200, 100, 0.0, 0.0, 1e6),
        (1, 0, 0, 1e2, 1e6): (1, 0, 0, 0, 200, 100, 1e3, 1e2, 1e6),
        (2, 0, 0, 1e2, 1e6): (1, 0, 0, 0, 200, 100, 1e3, 1e2, 1e6),
        (3, 0, 0, 1e2, 1e6): (0, 1, 1, 1, 10, 100, 0.0, 0.0, 0.0),
    }
    for args, want in table.items():
        p = orbhip.inertial_opt_params(*args)
        assert tuple(getattr(p, f) for f in fields) == want, (args, [getattr(p, f) for f in fields])
        m = iom.default_params(min(args[0], 1) if args[0] != 3 else 3, *args[1:])
        assert tuple(m[f] for f in fields) == want, args


def test_call_lines_compile_and_the_overloads_are_defined(tmp_path):
    obj = str(tmp_path / "callers.o")
    src_path = os.path.join(HOST, "compile_callers_imu_init.cc")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, src_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    src = open(src_path).read()
    for line in ("Optimizer::InertialOptimization(mpAtlas->GetCurrentMap(), mRwg, mScale, mbg, mba, mbMonocular, infoInertial, false, false, priorG, priorA);",
                 "Optimizer::InertialOptimization(mpAtlas->GetCurrentMap(), mRwg, mScale);", "Optimizer::InertialOptimization(pCurrentMap,bg,ba);",
                 "bg << 0., 0., 0.;", "mRwg = Eigen::Matrix3d::Identity();"):
        assert line in src, line
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = sorted({ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::Optimizer::InertialOptimization" in ln})
    assert len(wanted) == 4, undefined
    o = str(tmp_path / "opt.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "Optimizer_InertialOptimization.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    assert not [w for w in wanted if w not in defined], (wanted, defined)
    und = subprocess.run(["nm", "-C", "-u", o], stdout=subprocess.PIPE, text=True).stdout
    assert "orbhip_inertial_optimization_host" in und and "inertial_information" in und


def _scene(overload, **kw):
    mp = ic.make("a_mono_prior" if overload != 3 else "d", 8, 5)
    return mp, sio.class_scene(mp, overload, mono=True, seed=3, bad_kf=5, far_bias=(2, 6), **kw)


def test_no_usable_gpu_leaves_everything_unchanged(tmp_path):
    for overload in range(4):
        mp, (arrays, _) = _scene(overload)
        fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
        sio.write_flat(fin, arrays)
        # no such device: the calling thread gets no context, here and on a GPU machine
        r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, ORBHIP_DEVICE="4096"))
        assert r.returncode == 0, (r.stdout, r.stderr)
        msgs = [ln for ln in r.stderr.splitlines() if ln.strip()]
        assert len(msgs) == 1 and "no device context" in msgs[0] and "no CPU fallback" in msgs[0], r.stderr
        out = sio.read_flat(fout)
        for k in ("Rwg", "scale", "bg", "ba"):
            assert out[k].tobytes() == arrays[k].tobytes(), k
        assert out["vel"].tobytes() == arrays["vel"].astype(np.float32).tobytes()
        assert out["bias"].tobytes() == arrays["bias"].astype(np.float32).tobytes()
        assert out["pre_bu"].tobytes() == (arrays["pre_b"].astype(np.float32) * arrays["has_preint"][:, None]).astype(np.float32).tobytes()
        assert not out["reint"].any()


STUB = r"""
// stand-alone check of the host-side packing of Optimizer::InertialOptimization under AddressSanitizer / UBSan: the class file, its
// helpers and a stub of the library's entry points that reads every input byte and writes every output byte the real ones may.
#include <cstdio>
#include <cstring>
#include "../include/orbhip.h"
static int g_calls = 0, g_edges = 0, g_n = 0;
extern "C" {
void orbhip_inertial_opt_default_params(orbhip_inertial_opt_params *p, int, int, int, float, float) { memset(p, 0, sizeof(*p)); p->iterations = 3; p->free_vel_bias = 1; }
int orbhip_inertial_optimization_host(orbhip_ctx *, const orbhip_inertial_opt_params *p, int n_kf, double *kf, const uint8_t *link, const double *preint,
                                      const double *info, double *glob, double *stats, double *trace)
{
    double s = 0;
    for (int k = 0; k < n_kf; k++) {
        for (int i = 0; i < ORBHIP_IBA_KF; i++) s += kf[k * ORBHIP_IBA_KF + i];
        if (link[k]) { g_edges++; for (int i = 0; i < ORBHIP_IBA_PREINT; i++) s += preint[k * ORBHIP_IBA_PREINT + i]; for (int i = 0; i < 81; i++) s += info[k * 81 + i]; }
        for (int i = 12; i < 21; i++) kf[k * ORBHIP_IBA_KF + i] += 0.5;
    }
    for (int i = 0; i < ORBHIP_IO_GLOBAL; i++) { s += glob[i]; glob[i] += 0.25; }
    if (stats) for (int i = 0; i < 8; i++) stats[i] = s;
    if (trace) for (int i = 0; i < 2 * p->iterations; i++) trace[i] = s;
    g_calls++; g_n = n_kf;
    return s != s ? -3 : 0;
}
const char *orbhip_last_error(void) { return ""; }
}
namespace ORB_SLAM3 { namespace hip { orbhip_ctx *ThreadContext() { return (orbhip_ctx *)&g_calls; } int GetDevice() { return 0; } } }
"""


def test_host_packing_under_sanitizers(tmp_path):
    """ordering, filters and blob layout of the class under -fsanitize=address,undefined: a stand-alone program (the smoke driver's
    main, the class file, a stub of the one library entry point), run on the CPU."""
    stub = tmp_path / "stub.cc"
    stub.write_text(STUB.replace("../include/orbhip.h", os.path.join(ROOT, "include", "orbhip.h")))
    exe = str(tmp_path / "io_asan")
    srcs = [os.path.join(HOST, f) for f in ("host_inertial_opt_smoke.cc", "Optimizer_InertialOptimization.cc", "Optimizer_LocalInertialBA.cc")]
    # Optimizer_LocalInertialBA.cc (the shared edge information) refers to further library entry points that this program never calls
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", HOST, "-o", exe] + srcs +
                       [str(stub), "-Wl,--unresolved-symbols=ignore-all"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    for overload in range(4):
        mp, (arrays, chain) = _scene(overload)
        fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
        sio.write_flat(fin, arrays)
        r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
        out = sio.read_flat(fout)
        # the stub added 0.25 to the globals and 0.5 to velocities and biases: what comes back shows which fields the class writes back
        g = np.concatenate([out["Rwg"].view(np.float64), out["scale"].view(np.float64), out["bg"].view(np.float64), out["ba"].view(np.float64)])
        if overload in (0, 3):
            np.testing.assert_array_equal(g[:10], np.concatenate([mp["glob"][:9], mp["glob"][9:10]]) + 0.25)
        else:
            np.testing.assert_array_equal(g[:10], np.concatenate([mp["glob"][:9], mp["glob"][9:10]]))
        inside = arrays["kf_id"] <= arrays["max_kf_id"][0]
        vel_in = arrays["vel"].astype(np.float32)
        if overload == 3:
            assert out["vel"].tobytes() == vel_in.tobytes() and g[10:].tolist() == [7.0, 8.0, 9.0, -7.0, -8.0, -9.0]
        else:
            want = np.where(inside[:, None], (vel_in.astype(np.float64) + 0.5).astype(np.float32), vel_in)
            np.testing.assert_array_equal(out["vel"].reshape(-1, 3), want)
