"""CPU tests of the 4-DoF essential-graph interface: the C ABI symbols and kernels in the library, the header as C99 / C++11 with the
struct sizes, the default parameters, every BADARG / CAPACITY answer with its message, the reference's own call line
(src/LoopClosing.cc:1218) compiled against the host headers, the class method's packing and write-back under AddressSanitizer / UBSan in
a stand-alone program linked against a stub of the entry points, and the class without a usable GPU (one message, everything unchanged).
The entry point checks every graph before it touches the device, so the refusals are exercised here without a GPU (the context handle is
never dereferenced on these paths)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import synth_essential_graph4dof as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
NAMES = ("orbhip_pose_graph4dof_default_params", "orbhip_optimize_essential_graph4dof_host", "orbhip_debug_pose_graph4dof_last_path")
HOST = os.path.join(PKG, "host")
EXE = os.path.join(PKG, "lib", "host_essential_graph4dof_smoke")
E_BADARG, E_CAPACITY = -1, -4


def test_symbols_declared_exported_and_bound():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name), name
    strings = subprocess.run(["strings", os.path.join(PKG, "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    for k in ("k_pg4_linearize", "k_pg4_assemble", "k_pg4_maxdiag", "k_pg4_fill", "k_pg4_ldlt", "k_pg4_big_diag", "k_pg4_big_rows", "k_pg4_big_trail",
              "k_pg4_big_backsub", "k_pg4_update", "k_pg4_errors", "k_pg4_reduce"):
        assert k in strings, k
    assert callable(orbhip.optimize_essential_graph4dof) and orbhip.PG4_STATE == 36


def test_header_compiles_as_c99_and_cxx11_and_struct_sizes(tmp_path):
    import orbhip
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "orbhip.h"\nint main(void) { orbhip_pose_graph4dof_params p; orbhip_pose_graph_stats s; s.end_reason = ORBHIP_PG_END_NBAD; p.iterations = 1;\n'
                   'printf("%d %d %d %d\\n", (int)sizeof(orbhip_pose_graph4dof), (int)sizeof(p), ORBHIP_PG4_STATE, ORBHIP_PG_TRACE + s.end_reason - 2 + p.iterations - 1); return 0; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-x", "c"], ["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++"]):
        exe = str(tmp_path / "t")
        r = subprocess.run(cmd + ["-I", inc, "-o", exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split()
        assert [int(v) for v in out] == [C.sizeof(orbhip.PoseGraph4DoF), C.sizeof(orbhip.PoseGraph4DoFParams), 36, 4]
    assert (C.sizeof(orbhip.PoseGraph4DoF), C.sizeof(orbhip.PoseGraph4DoFParams)) == (48, 80)


def test_default_parameters():
    import orbhip
    p = orbhip.pose_graph4dof_default_params()
    assert (p.iterations, p.lambda_init, p.tau, p.max_trials) == (20, 0.0, 1e-50, 100)
    assert list(p.info_diag) == [1e3, 1e3, 1.0, 1.0, 1.0, 1.0]      # (2, 2) is never set in the reference: yaw keeps weight 1
    assert orbhip.pose_graph4dof_default_params(7, lambda_init=2.0).lambda_init == 2.0


class _Ctx:
    """A handle that is not NULL: the refusals below return before the context is used."""
    h = C.cast(C.pointer(C.c_int(0)), C.c_void_p)


def _refused(graph, state=None, **params):
    import orbhip
    p = orbhip.pose_graph4dof_default_params()
    for k, v in params.items():
        if k == "info_diag":
            p.info_diag[v[0]] = v[1]
        else:
            setattr(p, k, v)
    state = graph["state"] if state is None else state
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph4dof(_Ctx, [graph], [state], p)
    return ei.value.code, str(ei.value)


def test_every_refusal_names_its_field():
    import orbhip
    g = sg.make_graph(1, 5)
    V = len(g["fixed"])
    for field, idx, val, what in (("edge_v0", 2, V, "edge_v0[2] = %d is outside the vertices" % V), ("edge_v1", 4, -1, "edge_v1[4] = -1 is outside the vertices")):
        bad = dict(g, **{field: g[field].copy()})
        bad[field][idx] = val
        code, msg = _refused(bad)
        assert code == E_BADARG and what in msg, msg
    bad = dict(g, edge_v1=g["edge_v1"].copy()); bad["edge_v1"][1] = bad["edge_v0"][1]
    code, msg = _refused(bad)
    assert code == E_BADARG and "an edge from a vertex to itself" in msg, msg
    for v in (np.nan, np.inf):
        bad = dict(g, edge_meas=g["edge_meas"].copy()); bad["edge_meas"][6, 11] = v
        code, msg = _refused(bad)
        assert code == E_BADARG and "edge_meas[6][11] is not finite" in msg, msg
    s = g["state"].copy(); s[2, 35] = np.nan
    code, msg = _refused(g, state=s)
    assert code == E_BADARG and "state_inout[2][35] is not finite" in msg, msg
    for kw, what in ((dict(iterations=0), "iterations < 1"), (dict(max_trials=0), "max_trials < 1"), (dict(lambda_init=np.nan), "lambda_init is not finite"),
                     (dict(tau=0.0), "tau is not finite and positive"), (dict(tau=np.inf), "tau is not finite and positive"),
                     (dict(tau=np.nan, lambda_init=-1.0), "tau is not finite and positive"), (dict(info_diag=(4, np.inf)), "info_diag[4] is not finite")):
        code, msg = _refused(g, **kw)
        assert code == E_BADARG and what in msg and "orbhip_optimize_essential_graph4dof_host" in msg, msg
    for field in ("n_vertices", "n_edges"):
        arr = (orbhip.PoseGraph4DoF * 1)()
        setattr(arr[0], field, -1)
        pe = (C.c_void_p * 1)(g["state"].ctypes.data)
        rc = orbhip.lib.orbhip_optimize_essential_graph4dof_host(_Ctx.h, C.cast(arr, C.c_void_p), 1, C.byref(orbhip.pose_graph4dof_default_params()), C.cast(pe, C.c_void_p), None, None)
        assert rc == E_BADARG and ("%s < 0" % field).encode() in orbhip.lib.orbhip_last_error()
    rc = orbhip.lib.orbhip_optimize_essential_graph4dof_host(None, None, 0, None, None, None, None)
    assert rc == E_BADARG and b"NULL" in orbhip.lib.orbhip_last_error()
    # a bad tau does not matter when the user gives the start lambda: such a call gets past the checks (and here to the NULL fixed of an empty struct)
    arr = (orbhip.PoseGraph4DoF * 1)(); arr[0].n_vertices = 1
    p = orbhip.pose_graph4dof_default_params(lambda_init=1.0); p.tau = np.nan
    pe = (C.c_void_p * 1)(g["state"].ctypes.data)
    rc = orbhip.lib.orbhip_optimize_essential_graph4dof_host(_Ctx.h, C.cast(arr, C.c_void_p), 1, C.byref(p), C.cast(pe, C.c_void_p), None, None)
    assert rc == E_BADARG and b"fixed is NULL" in orbhip.lib.orbhip_last_error()


def test_capacity_refusal_names_the_count_and_writes_nothing():
    g = sg.make_graph(1, 1025, consistent=True)
    before = g["state"].copy()
    code, msg = _refused(g)
    assert code == E_CAPACITY and "4100 unknowns" in msg and "1025 free keyframes" in msg and "4096" in msg and "(1024)" in msg and "no CPU fallback" in msg, msg
    assert g["state"].tobytes() == before.tobytes()


def test_call_line_compiles_and_the_method_is_defined(tmp_path):
    obj = str(tmp_path / "callers.o")
    src_path = os.path.join(HOST, "compile_callers_essential_graph4dof.cc")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, src_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "Optimizer::OptimizeEssentialGraph4DoF(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections);" in open(src_path).read()
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = sorted({ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::Optimizer::OptimizeEssentialGraph4DoF" in ln})
    assert len(wanted) == 1, undefined
    o = str(tmp_path / "opt.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "Optimizer_OptimizeEssentialGraph4DoF.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert wanted[0] in subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    und = subprocess.run(["nm", "-C", "-u", o], stdout=subprocess.PIPE, text=True).stdout
    assert "orbhip_optimize_essential_graph4dof_host" in und and "orbhip_pose_graph_correct_points_host" in und


def test_no_usable_gpu_leaves_everything_unchanged(tmp_path):
    from synth_inertial_opt import read_flat, write_flat
    sc = sg.class_scene(n_kf=12, n_points=40)
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    write_flat(fin, sc["arrays"])
    # no such device: the calling thread gets no context, here and on a GPU machine
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, ORBHIP_DEVICE="4096"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    msgs = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(msgs) == 1 and "no device context" in msgs[0] and "no CPU fallback" in msgs[0], r.stderr
    out = read_flat(fout)
    assert out["Tcw"].tobytes() == sc["Tcw"].tobytes() and out["mp_pos"].tobytes() == sc["mp_pos"].tobytes()
    assert not out["mp_updates"].any() and out["change"][0] == 0


STUB = r"""
// stand-alone check of the host-side packing and write-back of Optimizer::OptimizeEssentialGraph4DoF under AddressSanitizer / UBSan: the
// class file, the flat-file driver and a stub of the library's entry points that reads every input byte and writes every output byte
// the real ones may.
#include <cstdio>
#include <cstring>
#include "../include/orbhip.h"
static int g_dummy = 0;
extern "C" {
void orbhip_pose_graph4dof_default_params(orbhip_pose_graph4dof_params *p)
{
    memset(p, 0, sizeof(*p)); p->iterations = 20; p->tau = 1e-50; p->max_trials = 100;
    for (int k = 0; k < 6; k++) p->info_diag[k] = k < 2 ? 1e3 : 1.0;
}
int orbhip_optimize_essential_graph4dof_host(orbhip_ctx *, const orbhip_pose_graph4dof *g, int n, const orbhip_pose_graph4dof_params *p, double *const *state,
                                             orbhip_pose_graph_stats *st, double *trace)
{
    double s = 0, orth = 0; int n_fixed = 0, in_range = 1, fixed_at = -1;
    for (int v = 0; v < g->n_vertices; v++) {
        if (g->fixed[v]) { n_fixed++; fixed_at = v; }
        const double *a = state[0] + ORBHIP_PG4_STATE * v;
        for (int k = 0; k < ORBHIP_PG4_STATE; k++) s += a[k];
        // Rcw = Rcb Rwb^T up to the float storage: the rows are where the ABI says they are
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
            double d = -a[12 + 3 * i + j];
            for (int k = 0; k < 3; k++) d += a[24 + 3 * i + k] * a[3 * j + k];
            if (d < 0) d = -d;
            if (d > orth) orth = d;
        }
    }
    for (int e = 0; e < g->n_edges; e++) {
        if (g->edge_v0[e] < 0 || g->edge_v0[e] >= g->n_vertices || g->edge_v1[e] < 0 || g->edge_v1[e] >= g->n_vertices) in_range = 0;
        for (int k = 0; k < 12; k++) s += g->edge_meas[12 * e + k];
    }
    for (int v = 0; v < g->n_vertices; v++) if (!g->fixed[v]) state[0][ORBHIP_PG4_STATE * v + 21] += 0.5;
    if (st) { memset(st, 0, sizeof(*st)); st->chi2_initial = s; }
    printf("STUB graphs %d n_vertices %d n_fixed %d fixed_at %d n_edges %d in_range %d its %d trace %d derived %d yaw_weight_is_one %d\n", n, g->n_vertices, n_fixed, fixed_at,
           g->n_edges, in_range, p->iterations, trace != nullptr, orth < 1e-5, p->info_diag[2] == 1.0 && p->info_diag[0] == 1e3);
    return s != s ? -3 : 0;
}
int orbhip_pose_graph_correct_points_host(orbhip_ctx *, const float *Xw, const int32_t *ref, int n, const double *Scw, const double *Swc, int nv, float *out)
{
    double s = 0;
    for (int i = 0; i < 8 * nv; i++) s += Scw[i] + Swc[i];
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) out[3 * i + k] = Xw[3 * i + k] + ((ref[i] >= 0 && ref[i] < nv) ? 0.25f : 0.f);
    return s != s ? -3 : 0;
}
const char *orbhip_last_error(void) { return ""; }
}
namespace ORB_SLAM3 { namespace hip { orbhip_ctx *ThreadContext() { return (orbhip_ctx *)&g_dummy; } int GetDevice() { return 0; } } }
"""


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eg4_asan")
    stub = tmp / "stub.cc"
    stub.write_text(STUB.replace("../include/orbhip.h", os.path.join(ROOT, "include", "orbhip.h")))
    exe = str(tmp / "eg4_asan")
    srcs = [os.path.join(HOST, f) for f in ("host_essential_graph4dof_smoke.cc", "Optimizer_OptimizeEssentialGraph4DoF.cc")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", HOST, "-o", exe] + srcs + [str(stub)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe, tmp


@pytest.mark.parametrize("bad_kf", [None, 9])
def test_packing_and_write_back_under_sanitizers(asan_exe, bad_kf):
    from synth_inertial_opt import read_flat, write_flat
    exe, tmp = asan_exe
    sc = sg.class_scene(bad_kf=bad_kf)
    g, vertex, left, _ = sg.gather(sc)
    fin, fout = str(tmp / "a.in"), str(tmp / "a.out")
    write_flat(fin, sc["arrays"])
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STUB")][0].split()
    st = dict(zip(line[1::2], [int(v) for v in line[2::2]]))
    assert st == dict(graphs=1, n_vertices=len(g["fixed"]), n_fixed=1, fixed_at=int(vertex[sc["loop"]]), n_edges=len(g["edge_v0"]), in_range=1, its=20, trace=0, derived=1,
                      yaw_weight_is_one=1)
    assert ("%d edges with a bad keyframe" % left in r.stdout) == (left > 0)
    out = read_flat(fout)
    T = out["Tcw"].reshape(-1, 4, 4)
    for k in range(sc["K"]):
        if vertex[k] < 0 or k == sc["loop"]:
            assert T[k].tobytes() == sc["Tcw"][k].tobytes()                    # a bad keyframe and the fixed one keep their pose
        else:
            row = g["state"][vertex[k]]
            np.testing.assert_allclose(T[k][:3, 3], (row[21:24] + np.array([0.5, 0, 0])).astype(np.float32), rtol=0, atol=1e-6)
            np.testing.assert_allclose(T[k][:3, :3], row[12:21].reshape(3, 3).astype(np.float32), rtol=0, atol=1e-6)
    moved = ~sc["mp_bad"] & (vertex[sc["mp_ref"]] >= 0)
    np.testing.assert_array_equal(out["mp_pos"].reshape(-1, 3), np.where(moved[:, None], sc["mp_pos"] + np.float32(0.25), sc["mp_pos"]))
    np.testing.assert_array_equal(out["mp_updates"], (~sc["mp_bad"]).astype(np.int32))
    assert out["change"][0] == 1
