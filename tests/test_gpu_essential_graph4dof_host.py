"""GPU test of the class method Optimizer::OptimizeEssentialGraph4DoF (host/Optimizer_OptimizeEssentialGraph4DoF.cc) through
lib/host_essential_graph4dof_smoke on a 40-keyframe stand-in inertial map against the model: the poses as the float Tiw = [R | t] the
reference stores, the corrected map points, the change index, a bad keyframe in the map.
The class walks std::set<KeyFrame*> in pointer order, the restatement (synth_essential_graph4dof.gather) in index order: the edge set is
the same, the summation order is not, and the 20 iterations run past the decisive prefix.  Poses and points are therefore held to the
project's K rule (ba_step_model.within_bound, K = 128) on what is stored: e_class <= K (e_float64_model + 2^-24 max|value|), both errors
against the extended-precision model of the same graph, the floor being the float storage of the result."""
import os
import subprocess
import numpy as np
import pytest
import essential_graph_model as em7
import essential_graph4dof_model as em
import synth_essential_graph4dof as sg
from ba_step_model import K as K_RULE, within_bound
from synth_inertial_opt import read_flat, write_flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_essential_graph4dof_smoke")


def expected(sc, dt=np.float64):
    g, vertex, left, vS = sg.gather(sc)
    r = em.optimize(g, g["state"], em.default_params(20), dt)
    est = np.asarray(r["est"], np.float64)
    Tcw = sc["Tcw"].copy()
    for k in range(sc["K"]):
        if vertex[k] >= 0:
            Tcw[k, :3, :3] = est[vertex[k], 12:21].reshape(3, 3).astype(np.float32); Tcw[k, :3, 3] = est[vertex[k], 21:24].astype(np.float32)
    ref = np.where(sc["mp_bad"], -1, vertex[sc["mp_ref"]])
    Siw = np.stack([np.concatenate([em7.R_to_quat(e[12:21].reshape(3, 3)), e[21:24], [1.0]]) for e in est])      # g2o::Sim3(Ri, ti, 1.)
    pos = em7.correct_points(sc["mp_pos"], ref, vS[~sc["bad"]], em7.s3_inverse(Siw))
    return Tcw, pos, ref, left, r


def run(sc, tmp_path):
    fin, fout = str(tmp_path / "eg4.in"), str(tmp_path / "eg4.out")
    write_flat(fin, sc["arrays"])
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return read_flat(fout), r.stderr


@pytest.mark.parametrize("bad_kf", [None, 9])
def test_class_method_against_the_model(tmp_path, bad_kf):
    sc = sg.class_scene(bad_kf=bad_kf)
    Tcw, pos, ref, left, r = expected(sc, np.longdouble)
    Tcw64, pos64, _, _, _ = expected(sc)
    out, err = run(sc, tmp_path)
    got, gpos = out["Tcw"].reshape(-1, 4, 4), out["mp_pos"].reshape(-1, 3)
    e = dict(Tcw=(np.abs(got - Tcw).max(), np.abs(Tcw64 - Tcw).max(), 2.0 ** -24 * np.abs(Tcw).max()),
             X=(np.abs(gpos - pos).max(), np.abs(pos64 - pos).max(), 2.0 ** -24 * np.abs(pos).max()))
    print("[essential-graph4dof] class   bad %s: %s, model its %d chi2 %.4g -> %.4g" % (
        bad_kf, " ".join("%s %.2g (f64 %.2g, ratio %.2g)" % (k, v[0], v[1], v[0] / (v[1] + v[2])) for k, v in e.items()), r["iterations"],
        r["chi_first"], r["chi_last"]))
    for k, v in e.items():
        assert within_bound(v[0], v[1], v[2], K_RULE), (k, v)
    assert np.abs(Tcw - sc["Tcw"]).max() > 1e-2, "the scene is to move its keyframes"
    assert got[sc["loop"]].tobytes() == sc["Tcw"][sc["loop"]].tobytes()      # the loop keyframe is fixed
    moved = ref >= 0
    assert moved.sum() > 100 and np.abs(pos - sc["mp_pos"])[moved].max() > 1e-3
    # bad points, and points whose keyframe has no vertex, keep their bytes; only bad points miss UpdateNormalAndDepth
    keep = ref < 0
    assert keep.any() and gpos[keep].tobytes() == sc["mp_pos"][keep].tobytes()
    np.testing.assert_array_equal(out["mp_updates"], (~sc["mp_bad"]).astype(np.int32))
    assert out["change"][0] == 1
    msgs = [ln for ln in err.splitlines() if ln.strip()]
    if bad_kf is None:
        assert left == 0 and not msgs, err
    else:
        assert left > 0 and len(msgs) == 1 and ("%d edges with a bad keyframe" % left) in msgs[0], err
        assert got[bad_kf].tobytes() == sc["Tcw"][bad_kf].tobytes()
