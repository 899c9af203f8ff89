"""GPU tests of the drop-in class method Optimizer::FullInertialBA (host/Optimizer_FullInertialBA.cc) through the flat-file driver
lib/host_full_iba_smoke: what the class writes back equals what the C ABI returns for the map the class packs (same float inputs, the
body poses and edge informations as the driver reports them), in both modes and both nLoopId branches; a map beyond the capacity is
refused with one message and left untouched.  The observations of a point reach the solver in std::map<KeyFrame*> order, which is
the allocator's, so sums over a point's edges may associate differently from the array order used here: values are compared to 1e-5
(they are floats in the classes), not by bytes."""
import os
import subprocess
import numpy as np
import pytest
import synth_full_iba as sf
import synth_inertial_opt as sio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_full_iba_smoke")
TOL = 1e-5


def _drive(tmp_path, sc):
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    sio.write_flat(fin, sc)
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return sio.read_flat(fout), r.stderr


def _tcw(kf, Rcb, tcb):
    Rwb, twb = kf[:9].reshape(3, 3), kf[9:12]
    T = np.eye(4); T[:3, :3] = Rcb @ Rwb.T; T[:3, 3] = -T[:3, :3] @ twb + tcb
    return T.reshape(-1)


@pytest.mark.parametrize("b_init,loop_id", [(True, 0), (False, 0), (True, 5), (False, 5)])
def test_class_method_equals_the_abi_on_the_same_map(tmp_path, gpu_ctx, b_init, loop_id):
    import orbhip
    win, _ = sf.make_map(4, 6, pts_per_kf=15, bias0_sigma=1e-3)
    K, bad = win.n_kf, 3
    priors = (1.0, 1e5)
    sc = sf.class_scene(win, 4, b_init, priors, loop_id=loop_id, bad_kf=bad, stop=0)
    out, err = _drive(tmp_path, sc)
    assert not err.strip(), err
    w2, sb = sf.abi_map_of_scene(win, sc, out, b_init, bad_kf=bad)
    p = orbhip.fiba_default_params(4, b_init, *priors)
    kf, X, sbo, st = orbhip.full_inertial_ba_solve_batch(gpu_ctx, [w2.struct(orbhip.IbaWindow)], [w2.kf0], [w2.pts0], sb[None], p)
    kf, X, sbo = kf[0], X[0], sbo[0]
    assert st[0]["iterations_run"] >= 1
    G = "GBA" if loop_id else ""
    Tcw = np.stack([_tcw(kf[k], w2.Rcb.reshape(3, 3), w2.tcb) for k in range(K)])
    assert np.abs(out["Tcw" + G].reshape(-1, 16)[:K] - Tcw).max() < TOL
    assert np.abs(out["vel" + G].reshape(-1, 3)[:K] - kf[:, 12:15]).max() < TOL
    bias = np.tile(sbo, (K, 1)) if b_init else kf[:, 15:21]
    assert np.abs(out["bias" + G].reshape(-1, 6)[:K] - bias).max() < TOL
    seen = np.zeros(w2.n_points, bool); seen[w2.arrays["edge_point"]] = True
    pos = out["mp_gba_pos" if loop_id else "mp_pos"].reshape(-1, 3)
    assert np.abs(pos[seen] - X[seen]).max() < TOL
    assert np.abs(kf[:, 9:12] - w2.kf0[:, 9:12]).max() > 1e-4          # (the solve moved something)
    assert out["change"][0] == 1
    if loop_id:
        np.testing.assert_array_equal(out["kf_gba"], [loop_id] * K + [0])
        np.testing.assert_array_equal(out["mp_gba"], np.where(seen, loop_id, 0))
        assert out["Tcw"].tobytes() == sc["Tcw"].tobytes() and out["mp_pos"].tobytes() == sc["mp_pos"].tobytes() and not out["mp_updates"].any()
    else:
        assert not out["kf_gba"].any() and not out["TcwGBA"].any()
        np.testing.assert_array_equal(out["mp_updates"], seen.astype(np.int32))
        assert out["mp_pos"].reshape(-1, 3)[~seen].tobytes() == sc["mp_pos"][~seen].tobytes()
    # the keyframe beyond maxKFid keeps every byte
    assert out["Tcw"].reshape(-1, 16)[K].tobytes() == sc["Tcw"][K].tobytes() and out["vel"].reshape(-1, 3)[K].tobytes() == sc["vel"][K].tobytes()


@pytest.mark.parametrize("b_init,K", [(True, 53), (False, 33)])
def test_class_method_refuses_a_map_beyond_the_capacity(tmp_path, b_init, K):
    win, _ = sf.make_map(2, K, pts_per_kf=2, bias0_sigma=1e-3)
    sc = sf.class_scene(win, 3, b_init, (1.0, 1e5), extra_kf=False)
    out, err = _drive(tmp_path, sc)
    msgs = [ln for ln in err.splitlines() if ln.strip()]
    assert len(msgs) == 1 and "%d reduced unknowns" % (9 * K + 6 if b_init else 15 * K) in msgs[0] and "no CPU fallback" in msgs[0], err
    assert out["Tcw"].tobytes() == sc["Tcw"].tobytes() and out["vel"].tobytes() == sc["vel"].tobytes() and out["bias"].tobytes() == sc["bias"].tobytes()
    assert out["mp_pos"].tobytes() == sc["mp_pos"].tobytes() and out["change"][0] == 0 and not out["mp_updates"].any()
