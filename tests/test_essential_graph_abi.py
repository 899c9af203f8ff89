"""CPU tests of the essential-graph interface: the C ABI symbols and kernels in the library, the header as C99 / C++11 with the struct
sizes, the default parameters, every BADARG / CAPACITY answer with its message, the reference's own call line (src/LoopClosing.cc:1223)
compiled against the host headers, the class method's packing and write-back under AddressSanitizer / UBSan in a stand-alone program
linked against a stub of the entry points, and the class without a usable GPU (one message, everything unchanged).  The entry point checks every graph before it
touches the device, so the refusals are exercised here without a GPU (the context handle is never dereferenced on these paths)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import synth_essential_graph as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
NAMES = ("orbhip_pose_graph_default_params", "orbhip_optimize_essential_graph_host", "orbhip_pose_graph_correct_points_device",
         "orbhip_pose_graph_correct_points_host")
HOST = os.path.join(PKG, "host")
EXE = os.path.join(PKG, "lib", "host_essential_graph_smoke")
E_BADARG, E_CAPACITY = -1, -4


def test_symbols_declared_exported_and_bound():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name), name
    strings = subprocess.run(["strings", os.path.join(PKG, "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    for k in ("k_pg_linearize", "k_pg_assemble", "k_pg_fill", "k_pg_ldlt", "k_pg_big_diag", "k_pg_big_rows", "k_pg_big_trail", "k_pg_big_backsub",
              "k_pg_update", "k_pg_errors", "k_pg_reduce", "k_pg_points"):
        assert k in strings, k
    assert callable(orbhip.optimize_essential_graph) and callable(orbhip.pose_graph_correct_points_device)


def test_header_compiles_as_c99_and_cxx11_and_struct_sizes(tmp_path):
    import orbhip
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "orbhip.h"\nint main(void) { orbhip_pose_graph_params p; orbhip_pose_graph_stats s; s.end_reason = ORBHIP_PG_END_NBAD; p.iterations = 1;\n'
                   'printf("%d %d %d %d\\n", (int)sizeof(orbhip_pose_graph), (int)sizeof(p), (int)sizeof(s), ORBHIP_PG_TRACE + s.end_reason - 2 + p.iterations - 1); return 0; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-x", "c"], ["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++"]):
        exe = str(tmp_path / "t")
        r = subprocess.run(cmd + ["-I", inc, "-o", exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split()
        assert [int(v) for v in out] == [C.sizeof(orbhip.PoseGraph), C.sizeof(orbhip.PoseGraphParams), C.sizeof(orbhip.PoseGraphStats), 4]
    assert (C.sizeof(orbhip.PoseGraph), C.sizeof(orbhip.PoseGraphParams), C.sizeof(orbhip.PoseGraphStats)) == (48, 24, 48)


def test_default_parameters():
    import orbhip
    p = orbhip.pose_graph_default_params()
    assert (p.iterations, p.lambda_init, p.fix_scale, p.max_trials) == (20, 1e-16, 0, 100)
    assert orbhip.pose_graph_default_params(7, True).fix_scale == 1


class _Ctx:
    """A handle that is not NULL: the refusals below return before the context is used."""
    h = C.cast(C.pointer(C.c_int(0)), C.c_void_p)


def _refused(graph, sim3=None, **params):
    import orbhip
    p = orbhip.pose_graph_default_params()
    for k, v in params.items():
        setattr(p, k, v)
    sim3 = graph["sim3"] if sim3 is None else sim3
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph(_Ctx, [graph], [sim3], p)
    return ei.value.code, str(ei.value)


def test_every_refusal_names_its_field():
    import orbhip
    g = sg.make_graph(1, 5, False)
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
        bad = dict(g, edge_meas=g["edge_meas"].copy()); bad["edge_meas"][6, 7] = v
        code, msg = _refused(bad)
        assert code == E_BADARG and "edge_meas[6][7] is not finite" in msg, msg
    s = g["sim3"].copy(); s[2, 4] = np.nan
    code, msg = _refused(g, sim3=s)
    assert code == E_BADARG and "sim3_inout[2][4] is not finite" in msg, msg
    for kw, what in ((dict(iterations=0), "iterations < 1"), (dict(max_trials=0), "max_trials < 1"), (dict(lambda_init=0.0), "lambda_init"), (dict(lambda_init=np.nan), "lambda_init")):
        code, msg = _refused(g, **kw)
        assert code == E_BADARG and what in msg, msg
    rc = orbhip.lib.orbhip_optimize_essential_graph_host(None, None, 0, None, None, None, None)
    assert rc == E_BADARG and b"NULL" in orbhip.lib.orbhip_last_error()


def test_capacity_refusal_names_the_count_and_writes_nothing():
    g = sg.make_graph(1, 586, True, consistent=True)
    before = g["sim3"].copy()
    code, msg = _refused(g)
    assert code == E_CAPACITY and "4102 unknowns" in msg and "586 free keyframes" in msg and "4096" in msg and "no CPU fallback" in msg, msg
    assert g["sim3"].tobytes() == before.tobytes()


def test_call_line_compiles_and_the_method_is_defined(tmp_path):
    obj = str(tmp_path / "callers.o")
    src_path = os.path.join(HOST, "compile_callers_essential_graph.cc")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, src_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "Optimizer::OptimizeEssentialGraph(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixedScale);" in open(src_path).read()
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = sorted({ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if "ORB_SLAM3::Optimizer::OptimizeEssentialGraph" in ln})
    assert len(wanted) == 1, undefined
    o = str(tmp_path / "opt.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", o, os.path.join(HOST, "Optimizer_OptimizeEssentialGraph.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert wanted[0] in subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    und = subprocess.run(["nm", "-C", "-u", o], stdout=subprocess.PIPE, text=True).stdout
    assert "orbhip_optimize_essential_graph_host" in und and "orbhip_pose_graph_correct_points_host" in und


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
// stand-alone check of the host-side packing and write-back of Optimizer::OptimizeEssentialGraph under AddressSanitizer / UBSan: the
// class file, the flat-file driver and a stub of the library's entry points that reads every input byte and writes every output byte
// the real ones may.
#include <cstdio>
#include <cstring>
#include "../include/orbhip.h"
static int g_dummy = 0;
extern "C" {
void orbhip_pose_graph_default_params(orbhip_pose_graph_params *p) { memset(p, 0, sizeof(*p)); p->iterations = 20; p->lambda_init = 1e-16; p->max_trials = 100; }
int orbhip_optimize_essential_graph_host(orbhip_ctx *, const orbhip_pose_graph *g, int n, const orbhip_pose_graph_params *p, double *const *sim3,
                                         orbhip_pose_graph_stats *st, double *trace)
{
    double s = 0; int n_fixed = 0, in_range = 1;
    for (int v = 0; v < g->n_vertices; v++) { n_fixed += g->fixed[v]; for (int k = 0; k < 8; k++) s += sim3[0][8 * v + k]; }
    for (int e = 0; e < g->n_edges; e++) {
        if (g->edge_v0[e] < 0 || g->edge_v0[e] >= g->n_vertices || g->edge_v1[e] < 0 || g->edge_v1[e] >= g->n_vertices) in_range = 0;
        for (int k = 0; k < 8; k++) s += g->edge_meas[8 * e + k];
    }
    for (int v = 0; v < g->n_vertices; v++) if (!g->fixed[v]) { sim3[0][8 * v + 4] += 0.5; sim3[0][8 * v + 7] = 2.0; }
    if (st) { memset(st, 0, sizeof(*st)); st->chi2_initial = s; }
    printf("STUB graphs %d n_vertices %d n_fixed %d n_edges %d in_range %d fix_scale %d its %d trace %d\n", n, g->n_vertices, n_fixed, g->n_edges, in_range,
           p->fix_scale, p->iterations, trace != nullptr);
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
    tmp = tmp_path_factory.mktemp("eg_asan")
    stub = tmp / "stub.cc"
    stub.write_text(STUB.replace("../include/orbhip.h", os.path.join(ROOT, "include", "orbhip.h")))
    exe = str(tmp / "eg_asan")
    srcs = [os.path.join(HOST, f) for f in ("host_essential_graph_smoke.cc", "Optimizer_OptimizeEssentialGraph.cc")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", HOST, "-o", exe] + srcs + [str(stub)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe, tmp


@pytest.mark.parametrize("bad_kf", [None, 9])
def test_packing_and_write_back_under_sanitizers(asan_exe, bad_kf):
    from synth_inertial_opt import read_flat, write_flat
    exe, tmp = asan_exe
    sc = sg.class_scene(bad_kf=bad_kf, fix_scale=bad_kf is not None)
    g, vertex, left = sg.gather(sc)
    fin, fout = str(tmp / "a.in"), str(tmp / "a.out")
    write_flat(fin, sc["arrays"])
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STUB")][0].split()
    st = dict(zip(line[1::2], [int(v) for v in line[2::2]]))
    assert st == dict(graphs=1, n_vertices=len(g["fixed"]), n_fixed=1, n_edges=len(g["edge_v0"]), in_range=1, fix_scale=int(bad_kf is not None), its=20, trace=0)
    assert ("%d edges with a bad keyframe" % left in r.stdout) == (left > 0)
    out = read_flat(fout)
    T = out["Tcw"].reshape(-1, 4, 4)
    for k in range(sc["K"]):
        if vertex[k] < 0 or k == 0:
            assert T[k].tobytes() == sc["Tcw"][k].tobytes()                    # a bad keyframe and the fixed one keep their pose
        else:
            want = (sc["nc"][k][4:7] + np.array([0.5, 0, 0])) / 2.0                # [R | t / s]
            if k in sc["corr"]:
                want = (sc["g"]["sim3"][k][4:7] + np.array([0.5, 0, 0])) / 2.0
            np.testing.assert_allclose(T[k][:3, 3], want.astype(np.float32), rtol=0, atol=1e-6)
    index_of_id = {int(i): k for k, i in enumerate(sc["ids"])}
    ref_kf = np.where(sc["by_cur"], [index_of_id[int(i)] for i in sc["mp_cref"]], sc["mp_ref"])
    moved = ~sc["mp_bad"] & (vertex[ref_kf] >= 0)
    np.testing.assert_array_equal(out["mp_pos"].reshape(-1, 3), np.where(moved[:, None], sc["mp_pos"] + np.float32(0.25), sc["mp_pos"]))
    np.testing.assert_array_equal(out["mp_updates"], (~sc["mp_bad"]).astype(np.int32))
    assert out["change"][0] == 1
