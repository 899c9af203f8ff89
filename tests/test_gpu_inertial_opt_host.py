"""Optimizer::InertialOptimization (the four class methods, host/Optimizer_InertialOptimization.cc) through the flat-file driver against
the C ABI on the same numbers: the keyframes reach the class in a shuffled order with one beyond maxKFid and one bad (a gap); the test
orders them itself, feeds orbhip_inertial_optimization_host the class's own pose / information values (dumped by the driver) and holds
Rwg, scale and biases to the ABI's bytes, velocities and keyframe biases to their float roundings, the preintegrations' bias to the
new one (KeyFrame::SetNewBias hands it on), and Reintegrate() to exactly the keyframes whose gyro bias moved by more than 0.01: a second
pass puts the keyframes' gyro biases 0.02 and 0.005 away from the solved one, a case on each side of the threshold."""
import os
import subprocess
import numpy as np
import pytest
import inertial_opt_cases as ic
import synth_inertial_opt as sio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_inertial_opt_smoke")
CASES = {"a_mono": (0, dict(mono=True)), "a_stereo": (0, dict(mono=False)), "a_fixed": (0, dict(mono=True, fixed_vel=True)), "b": (1, {}),
         "c_list": (2, {}), "d": (3, {})}


@pytest.mark.parametrize("name", list(CASES))
def test_class_agrees_with_the_abi(gpu_ctx, tmp_path, name):
    import orbhip
    overload, kw = CASES[name]
    mp = ic.make({"a_mono": "a_mono_prior", "a_stereo": "a_stereo", "a_fixed": "a_fixed", "b": "b", "c_list": "b", "d": "d"}[name], 9, 6)
    arrays, chain = sio.class_scene(mp, overload, seed=4, bad_kf=5, **kw)
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    front = int(arrays["list"][0]) if overload == 2 else 0       # vpKFs.front(): scene row 0, or the list's first entry
    for both_sides in (False, True):
        # only the front keyframe's bias enters the solve.  The second pass puts the others' gyro biases around the solved one: 0.02 away
        # (keyframes 2 and 6 of the chain) or 0.005 away (the rest), one case on each side of the 0.01 that calls Reintegrate()
        if both_sides:
            solved = out["bg"].view(np.float64)
            for i, row in enumerate(chain):
                if row != front:
                    arrays["bias"][row, 0:3] = solved + np.array([0.02 if i in (2, 6) else 0.005, 0, 0])
        sio.write_flat(fin, arrays)
        r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0 and "done" in r.stdout, r.stdout[-2000:]
        out = sio.read_flat(fout)
        if overload == 3:
            break
    # the same numbers for the ABI, in chain order: heads by id, then along the links; keyframe 5 is bad, so its edge is absent
    n = len(chain)
    f32 = lambda k, w: arrays[k].astype(np.float32).astype(np.float64).reshape(-1, w)       # noqa: E731
    kf = np.zeros((n, 21)); link = np.zeros(n, np.uint8); pre = np.zeros((n, 67)); info = np.zeros((n, 81))
    dinfo = out["info"].view(np.float64).reshape(-1, 81)
    for i, row in enumerate(chain):
        kf[i, 0:9] = out["Rwb"].reshape(-1, 9)[row]; kf[i, 9:12] = out["twb"].reshape(-1, 3)[row]
        kf[i, 12:15] = f32("vel", 3)[row]; kf[i, 15:21] = f32("bias", 6)[row]
        if i >= 1 and mp["link"][i] and i != 5:
            link[i] = 1
            pre[i] = np.concatenate([f32("pre_dT", 1)[row], f32("pre_dR", 9)[row], f32("pre_dV", 3)[row], f32("pre_dP", 3)[row], f32("pre_JRg", 9)[row],
                                     f32("pre_JVg", 9)[row], f32("pre_JVa", 9)[row], f32("pre_JPg", 9)[row], f32("pre_JPa", 9)[row], f32("pre_b", 6)[row]])
            info[i] = dinfo[row]
    assert link.sum() == n - 2
    glob = np.zeros(16)
    glob[0:10] = mp["glob"][0:10] if overload in (0, 3) else np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0])
    glob[10:16] = f32("bias", 6)[front]
    p = orbhip.inertial_opt_params(overload, kw.get("mono", False), kw.get("fixed_vel", False), 1e2, 1e6)
    akf, aglob, ast, _ = orbhip.inertial_optimization_host(gpu_ctx, p, dict(kf=kf, link=link, preint=pre, info=info, glob=glob))
    assert ast[0] >= 1
    got = {k: out[k].view(np.float64) for k in ("Rwg", "scale", "bg", "ba")}
    if overload in (0, 3):
        assert got["Rwg"].tobytes() == aglob[0:9].tobytes() and got["scale"].tobytes() == aglob[9:10].tobytes()
    else:
        assert got["Rwg"].tobytes() == sio.raw(mp["glob"][0:9]).tobytes()
    if overload == 3:
        assert got["bg"].tolist() == [7.0, 8.0, 9.0] and out["vel"].tobytes() == arrays["vel"].astype(np.float32).tobytes()
        assert not out["reint"].any()
        return
    assert got["bg"].tobytes() == aglob[10:13].tobytes() and got["ba"].tobytes() == aglob[13:16].tobytes()
    new_b = aglob[10:16].astype(np.float32)
    old_g = arrays["bias"].astype(np.float32).reshape(-1, 6)[:, 0:3]
    moved = np.sqrt(((old_g - new_b[0:3]).astype(np.float64) ** 2).sum(1)) > 0.01
    want_reint = np.zeros(len(old_g), np.int32)
    for i, row in enumerate(chain):
        np.testing.assert_array_equal(out["vel"].reshape(-1, 3)[row], akf[i, 12:15].astype(np.float32))
        np.testing.assert_array_equal(out["bias"].reshape(-1, 6)[row], new_b)
        want_reint[row] = 1 if (moved[row] and arrays["has_preint"][row]) else 0
    np.testing.assert_array_equal(out["reint"], want_reint)
    for i, row in enumerate(chain):
        if row != front and arrays["has_preint"][row]:
            assert out["reint"][row] == (1 if i in (2, 6) else 0), (i, out["reint"], moved)
    assert out["reint"].sum() >= 2 and (out["reint"][[int(r_) for r_ in chain]] == 0).sum() >= 3
    extra = [r_ for r_ in range(len(old_g)) if r_ not in set(int(c) for c in chain)][0]     # beyond maxKFid: untouched
    assert out["bias"].reshape(-1, 6)[extra].tobytes() == arrays["bias"].astype(np.float32).reshape(-1, 6)[extra].tobytes()
    # KeyFrame::SetNewBias hands the new bias on to the keyframe's preintegration
    for row in chain:
        if arrays["has_preint"][row]:
            np.testing.assert_array_equal(out["pre_bu"].reshape(-1, 6)[row], new_b)
