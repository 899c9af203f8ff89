"""IMU::Preintegrated (host/ImuTypes.cc) through host_preint_smoke on the GPU: Reintegrate(), ReintegrateBatch and MergePrevious
reproduce the C ABI's output for the same measurements byte for byte; IntegrateNewMeasurement on the host and Reintegrate() on the
device agree under the K rule (both within K of the longdouble model, tests/test_gpu_preint.py's rule); Optimizer::InertialOptimization
on keyframes that carry measurements re-integrates exactly the keyframes beyond the 0.01 threshold, in one device call, and leaves the
fields of the others untouched."""
import os
import subprocess
import numpy as np
import pytest
import ba_step_model as bsm
import preint_cases as pc
import preint_model as pm
import synth_inertial_opt as sio
from test_preint_model import _host_fields, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_preint_smoke")
NGA, WALK = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)


def _run(tmp_path, arrays):
    fin, fout = str(tmp_path / "p.in"), str(tmp_path / "p.out")
    sio.write_flat(fin, arrays)
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    return sio.read_flat(fout)


def _abi(ctx, bias, meas):
    import orbhip
    rec, cov, avg, _, _, _ = orbhip.preintegrate_host(ctx, orbhip.preint_params(pc.NG, pc.NA, pc.NGW, pc.NAW, want_info=False), bias, meas)
    return pm.record_fields(rec, cov, avg)


def _same_bytes(a, b, rows):
    for k in pm.FIELDS:
        assert np.asarray(a[k], np.float32)[rows].tobytes() == np.asarray(b[k], np.float32)[rows].tobytes(), k


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_class_reproduces_the_abi(gpu_ctx, tmp_path, mode):
    arrays, meas, bias, bias_new = _scene(mode)
    n = len(meas)
    out = _run(tmp_path, arrays)
    dev, host = _host_fields(out, "dev_", n), _host_fields(out, "host_", n)
    if mode in (0, 1):
        want = _abi(gpu_ctx, bias_new, meas)
        _same_bytes(dev, want, slice(None))
        assert out["dev_b"].reshape(n, 6).tobytes() == bias_new.tobytes()
        assert out["device_calls"][0] == (n if mode == 0 else 1) and out["reint"].tolist() == ([1] * n if mode == 0 else [0] * n)
    else:
        merged = [np.concatenate([meas[k - 1], meas[k]]) if k % 2 else meas[k] for k in range(n)]
        want = _abi(gpu_ctx, bias, merged)
        _same_bytes(dev, want, slice(1, None, 2))
        _same_bytes(dev, host, slice(0, None, 2))
        assert out["nmeas"].tolist() == [len(m) for m in merged] and out["device_calls"][0] == n // 2


def test_host_loop_and_device_agree_under_the_k_rule(gpu_ctx, tmp_path):
    """The same chains at the same bias: IntegrateNewMeasurement (host) and Reintegrate() (device) are each within K of the longdouble
    model, so of one another."""
    arrays, meas, bias, _ = _scene(0)
    arrays["bias_new"] = bias
    n = len(meas)
    out = _run(tmp_path, arrays)
    ref, f32 = pc.models(bias, meas, NGA, WALK)
    for prefix in ("host_", "dev_"):
        for g, (ed, ef, fl) in pc.k_rule_ratios(_host_fields(out, prefix, n), ref, f32).items():
            print("%s%-8s e %.3e e_f32 %.3e floor %.3e ratio %.2f" % (prefix, g, ed, ef, fl, ed / (ef + fl) if ed else 0.0))
            assert bsm.within_bound(ed, ef, fl), (prefix, g, ed, ef, fl)


def test_inertial_optimization_reintegrates_in_one_call(gpu_ctx, tmp_path):
    n = 8
    b0 = pc.bias(70)
    meas = [pc.chain(30, 70 + k) for k in range(n)]
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(m) for m in meas])
    # strong priors keep the solved biases near zero: keyframes with a small gyro bias stay within 0.01 of it, those 0.05 off do not
    kf_bias = np.tile(np.array([0.001, -0.002, 0.0015, 0.01, -0.02, 0.03], np.float32), (n + 1, 1))
    far = [2, 3, 6]
    kf_bias[far, 0] += np.float32(0.05)
    arrays = {"mode": np.array([3], np.int32), "noise": np.array([pc.NG, pc.NA, pc.NGW, pc.NAW], np.float32), "meas_off": off,
              "meas": np.concatenate(meas), "bias": np.tile(b0, (n, 1)), "bias_new": np.tile(b0, (n, 1)), "kf_bias": kf_bias,
              "prior": np.array([1e15, 1e15], np.float32)}
    out = _run(tmp_path, arrays)
    bg = out["bg"].view(np.float64)
    assert np.isfinite(bg).all()
    moved = np.sqrt((((kf_bias[:, :3] - bg.astype(np.float32)[None, :]).astype(np.float32).astype(np.float64)) ** 2).sum(axis=1)) > 0.01
    want = moved[1:]                                      # object k hangs on keyframe k + 1
    assert want.any() and not want.all()
    assert out["reint"].tolist() == [int(w) for w in want]
    assert out["device_calls"][0] == 1
    dev, host = _host_fields(out, "dev_", n), _host_fields(out, "host_", n)
    _same_bytes(dev, host, ~want)
    # the re-integrated ones now sit at the solved bias, re-integrated from their own measurements
    bnew = np.concatenate([out["bg"].view(np.float64), out["ba"].view(np.float64)]).astype(np.float32)
    rows = np.flatnonzero(want)
    fresh = _abi(gpu_ctx, [bnew] * len(rows), [meas[k] for k in rows])
    for k in pm.FIELDS:
        assert np.asarray(dev[k], np.float32)[rows].tobytes() == np.asarray(fresh[k], np.float32).tobytes(), k
    assert (out["dev_b"].reshape(n, 6)[rows] == bnew[None, :]).all()
