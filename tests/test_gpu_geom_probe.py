"""The shared SO(3) / Sim(3) / SE(3) / camera primitives, each ALONE on the device (orbhip.debug_geom_probe, csrc/geom_probe_kernels.hip),
at the inputs of geom_probe_cases.py: every branch of R_to_quat, of the Sim3 exponential and logarithm with every pivot outcome of its 3x3
solve, LogSO3 at cosines of exactly +-1 and an ulp outside, both sides of every small-angle threshold, rotations up to pi.

Double ops, per item: e_dev = max |device - expected|, e_64 = max |float64 model - expected|, floor = 2^-52 max |expected|, expected = the
faithful model at 50 digits (geom_probe_model.py); asserted: ba_step_model.within_bound(e_dev, e_64, floor), the project's K = 128 rule as
it stands, and equal NaN / Inf patterns.  The truth checks use the same rule with the closed-form-free truth as the expected value (the
reference's own truncation is then in e_64 too).  Float ops: bit for bit against the op-by-op float32 models.

Largest e_dev / (e_64 + floor) per op, measured on an MI355X (-s prints them; K = 128 is not tuned to them, every op would hold K = 16):
  quat_to_R 0.83   R_to_quat 0.52   quat_rot 0.93   quat_mul 0.59   quat_norm_rot 0.72   huber 0.52   se3_oplus 2.1   se3_mul 0.98
  so3_exp 0.77   so3_exp_imu 1.01   so3_log 1.0   so3_right_jac 1.0   so3_inv_right_jac 1.0   so3_normalize 0.41
  s3_exp 1.01   s3_log 10.8 (a large-sigma, large-theta item with row exchanges: e_dev 3.9e-14)   s3_mul 0.72   s3_inverse 0.92   s3_map 0.98
  cam_project 0.71   cam_project_jac 1.17
  truth checks: se3_oplus 1.0   so3_exp 0.65   so3_exp_imu 1.0   so3_log round trip 1.0   Jr Jr^-1 1.0   so3_normalize against the polar
  factor 0.41   s3_exp 1.0   s3_log round trip 3.2   cam_project_jac against mp.diff 1.17
  (a ratio of 1.0 with a large e_64 is the reference's own truncation or quirk, which device and float64 model share: I + Omega + Omega^2
  below 1e-5, B of the large-sigma small-theta branch, the unscaled LogSO3 near pi.)
  float ops: tri_project 49 + 98, tri_unproject 32 + 111, tri_svd4_null 50 items bit for bit, no atan2 left out; null vector on the
  clear-gap matrices: angle / (4 numpy angle + 2^-23) <= 0.87.
  so3_normalize, |R^T R - I| before -> after two steps (distance to the polar factor): delta 1e-15: 1.4e-15 -> 2.0e-16 (9.6e-17);
  6e-8: 7.6e-8 -> 2.8e-16 (1.4e-16); 1e-5: 1.3e-5 -> 2.0e-16 (1.2e-16); 1e-3: 1.7e-3 -> 1.5e-13 (7.4e-14), within delta^4 + floor."""
import numpy as np
import pytest
from mpmath import mp

import ba_step_model as bsm
import geom_probe_cases as gc
import geom_probe_model as gm
import orbhip

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def model():
    cache = {}

    def get(op):
        if op not in cache:
            cache[op] = gm.run_faithful(op, gc.CASES[op].inputs)
        return cache[op]
    return get


def run_device(ctx, op):
    """the op on its case table: twice (same bytes), into a buffer with three sentinel rows past n"""
    x = gc.CASES[op].inputs
    n, w = len(x), orbhip.GEOM_OPS[op][2]
    out = np.full((n + 3, w), SENTINEL)
    orbhip.debug_geom_probe(ctx, op, x, out=out, n=n)
    assert np.all(out[n:] == SENTINEL), op
    again = orbhip.debug_geom_probe(ctx, op, x)
    assert again.tobytes() == out[:n].tobytes(), op
    return out[:n].copy()


def hold(name, cand, y64, expected):
    """the K = 128 rule per item, NaN / Inf patterns equal; prints the largest ratio"""
    e_dev, fl, same_dev = gm.errors(cand, expected)
    e_64, _, same_64 = gm.errors(y64, expected)
    assert same_dev.all() and same_64.all(), (name, np.flatnonzero(~same_dev), np.flatnonzero(~same_64))
    ratio = e_dev / np.where(e_64 + fl > 0, e_64 + fl, 2.0 ** -1074)
    worst = int(ratio.argmax())
    print("%-22s largest e_dev / (e_64 + floor) = %-9.3g (item %d: e_dev %.3g, e_64 %.3g, floor %.3g)"
          % (name, ratio[worst], worst, e_dev[worst], e_64[worst], fl[worst]))
    bad = [i for i in range(len(e_dev)) if not bsm.within_bound(e_dev[i], e_64[i], fl[i])]
    assert not bad, (name, bad[:8], [(e_dev[i], e_64[i], fl[i]) for i in bad[:8]])
    return ratio[worst]


def faithful(ctx, model, op):
    dev = run_device(ctx, op)
    expected, y64 = model(op)[:2]
    hold(op, dev, y64, expected)
    return dev, y64


def test_quaternions_and_huber(gpu_ctx, model):
    for op in ("quat_to_R", "R_to_quat", "quat_rot", "quat_mul", "quat_norm_rot", "huber"):
        faithful(gpu_ctx, model, op)


def test_se3(gpu_ctx, model):
    dev, y64 = faithful(gpu_ctx, model, "se3_oplus")
    faithful(gpu_ctx, model, "se3_mul")
    c = gc.CASES["se3_oplus"]
    truth = [gm.truth_se3_oplus(c.inputs[i][:6], c.inputs[i][6:]) for i in c.truth]
    hold("se3_oplus truth", [[float(v) for v in gm.se3_as_matrix(dev[i])] for i in c.truth],
         [[float(v) for v in gm.se3_as_matrix(y64[i])] for i in c.truth], truth)


def test_so3(gpu_ctx, model):
    out = {}
    for op in ("so3_exp", "so3_exp_imu", "so3_log", "so3_right_jac", "so3_inv_right_jac"):
        out[op] = faithful(gpu_ctx, model, op)
    for op in ("so3_exp", "so3_exp_imu"):
        c = gc.CASES[op]
        hold(op + " truth", out[op][0][c.truth], out[op][1][c.truth], [gm.truth_so3_exp(c.inputs[i]) for i in c.truth])
    c = gc.CASES["so3_log"]                                      # expm([log_dev(R)]x) against R
    hold("so3_log round trip", [[float(v) for v in gm.roundtrip_so3_log(out["so3_log"][0][i])] for i in c.truth],
         [[float(v) for v in gm.roundtrip_so3_log(out["so3_log"][1][i])] for i in c.truth], [list(c.inputs[i]) for i in c.truth])
    c = gc.CASES["so3_right_jac"]                                # Jr Jr^-1 against I
    eye = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]

    def prod(a, b):
        return [float(v) for v in gm._mm([mp.mpf(float(x)) for x in a], [mp.mpf(float(x)) for x in b])]
    idx = [i for i in c.truth if np.isfinite(out["so3_inv_right_jac"][1][i]).all()]
    hold("Jr Jr^-1", [prod(out["so3_right_jac"][0][i], out["so3_inv_right_jac"][0][i]) for i in idx],
         [prod(out["so3_right_jac"][1][i], out["so3_inv_right_jac"][1][i]) for i in idx], [eye for _ in idx])


def test_so3_normalize(gpu_ctx, model):
    """Two Newton steps of the polar iteration in place of the reference's U V^T: against the polar factor for delta <= 1e-5, and what
    they leave of an orthogonality error of 1e-3 (printed: the header's 'a rounding error away' as numbers)."""
    dev, y64 = faithful(gpu_ctx, model, "so3_normalize")
    c = gc.CASES["so3_normalize"]
    polar = [gm.truth_polar(r) for r in c.inputs]
    near = [i for i, l in enumerate(c.labels) if l != "0.001"]
    hold("so3_normalize polar", dev[near], y64[near], [polar[i] for i in near])

    def ortho(R):
        M = gm._M3([mp.mpf(float(v)) for v in R])
        E = M.T * M - mp.eye(3)
        return float(max(abs(v) for v in gm._flat(E)))
    for delta in ("1e-15", "6e-08", "1e-05", "0.001"):
        idx = [i for i, l in enumerate(c.labels) if l == delta]
        e_in, e_out = max(ortho(c.inputs[i]) for i in idx), max(ortho(dev[i]) for i in idx)
        to_polar = max(float(max(abs(mp.mpf(float(a)) - b) for a, b in zip(dev[i], polar[i]))) for i in idx)
        print("so3_normalize delta %-6s |R^T R - I| in %.3g -> out %.3g, distance to the polar factor %.3g" % (delta, e_in, e_out, to_polar))
        if delta == "0.001":
            assert e_out <= float(delta) ** 4 + 2.0 ** -52, (e_out, delta)


def test_sim3(gpu_ctx, model):
    out = {}
    for op in ("s3_exp", "s3_log", "s3_mul", "s3_inverse", "s3_map"):
        out[op] = faithful(gpu_ctx, model, op)
    # the exact pivot tie: only the last bit of upsilon_0 tells Eigen's "first of equal magnitudes" from the other order
    # (test_geom_probe_model.py::test_pivot_tie_is_exact: contraction does not change this item's bits)
    assert out["s3_log"][0][gc.TIE_ITEM].tobytes() == out["s3_log"][1][gc.TIE_ITEM].tobytes(), (out["s3_log"][0][gc.TIE_ITEM], out["s3_log"][1][gc.TIE_ITEM])
    c = gc.CASES["s3_exp"]
    hold("s3_exp truth", [[float(v) for v in gm.s3_as_matrix(out["s3_exp"][0][i])] for i in c.truth],
         [[float(v) for v in gm.s3_as_matrix(out["s3_exp"][1][i])] for i in c.truth], [gm.truth_s3_exp(c.inputs[i]) for i in c.truth])
    c = gc.CASES["s3_log"]                                       # expm(generator(log_dev(S))) against S
    hold("s3_log round trip", [[float(v) for v in gm.roundtrip_s3_log(out["s3_log"][0][i])] for i in c.truth],
         [[float(v) for v in gm.roundtrip_s3_log(out["s3_log"][1][i])] for i in c.truth], [gm.s3_as_matrix(c.inputs[i]) for i in c.truth])


def test_cameras_double(gpu_ctx, model):
    faithful(gpu_ctx, model, "cam_project")
    dev, y64 = faithful(gpu_ctx, model, "cam_project_jac")
    c = gc.CASES["cam_project_jac"]
    assert np.isnan(dev[[i for i, r in enumerate(c.inputs) if r[4] == 1 and r[9] == 0 and r[10] == 0]]).any()      # the optical axis, KB8
    hold("cam_project_jac truth", dev[c.truth], y64[c.truth], [gm.truth_cam_jac(c.inputs[i]) for i in c.truth])


def _same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _float_exact(dev):
    assert np.all((dev == dev.astype(f32).astype(f64)) | np.isnan(dev))
    return dev.astype(f32)


def test_cameras_float(gpu_ctx):
    for op, t in (("tri_project_pinhole", 0), ("tri_project_kb8", 1)):
        x = gc.CASES[op].inputs
        dev = _float_exact(run_device(gpu_ctx, op))
        skip = np.zeros(len(x), bool)
        if t == 1:                                               # the one licence: an atan2 within 2^-50 of a float32 rounding boundary
            for i, r in enumerate(x):
                P = f32(r[8:])
                skip[i] = min(gm.atan2f_boundary_distance(np.sqrt(P[0] * P[0] + P[1] * P[1]), P[2]), gm.atan2f_boundary_distance(P[1], P[0])) <= 2.0 ** -50
            assert skip.sum() <= 0.01 * len(x)
        bad = [i for i, r in enumerate(x) if not skip[i] and not _same_bits(dev[i], gm.tri_project(t, r[:8], r[8:]))]
        print("%-22s %d items bit for bit, %d left out" % (op, len(x) - int(skip.sum()), int(skip.sum())))
        assert not bad, (op, bad, [(dev[i], gm.tri_project(t, x[i][:8], x[i][8:])) for i in bad[:4]])
    for op, t in (("tri_unproject_pinhole", 0), ("tri_unproject_kb8", 1)):
        x = gc.CASES[op].inputs
        dev = _float_exact(run_device(gpu_ctx, op))
        bad = [i for i, r in enumerate(x) if not _same_bits(dev[i], gm.tri_unproject(t, r[:8], r[8], r[9]))]
        print("%-22s %d items bit for bit" % (op, len(x)))
        assert not bad, (op, bad, [(dev[i], gm.tri_unproject(t, x[i][:8], x[i][8], x[i][9])) for i in bad[:4]])


def test_svd4_null(gpu_ctx):
    c = gc.CASES["tri_svd4_null"]
    dev = _float_exact(run_device(gpu_ctx, "tri_svd4_null"))
    bad = [i for i, a in enumerate(c.inputs) if not _same_bits(dev[i], gm.tri_svd4_null(a))]
    assert not bad, (bad, [(c.labels[i], dev[i], gm.tri_svd4_null(c.inputs[i])) for i in bad[:4]])
    worst = 0.0
    for i in c.truth:                                            # clear gap: the yardstick is the float32 numpy SVD's own angle
        null, _ = gm.truth_null4(c.inputs[i])
        A = c.inputs[i].reshape(4, 4).T.astype(f32)
        a_np = gm.angle_to(np.linalg.svd(A)[2][3], null)
        a_dev = gm.angle_to(dev[i], null)
        worst = max(worst, a_dev / (4 * a_np + 2.0 ** -23))
        assert a_dev <= 4 * a_np + 2.0 ** -23, (i, a_dev, a_np)
    print("tri_svd4_null          %d items bit for bit; clear gap: largest angle / (4 numpy angle + 2^-23) = %.3g" % (len(c.inputs), worst))


def test_sizes_and_argument_errors(gpu_ctx, model):
    x = np.tile(gc.CASES["quat_rot"].inputs, (5, 1))[:1000]
    full = orbhip.debug_geom_probe(gpu_ctx, "quat_rot", x)
    for n in (1, 63, 64, 65, 1000):
        out = np.full((n + 2, 3), SENTINEL)
        orbhip.debug_geom_probe(gpu_ctx, "quat_rot", x, out=out, n=n)
        assert out[:n].tobytes() == full[:n].tobytes() and np.all(out[n:] == SENTINEL), n
    hold("quat_rot n = 1000", full[:len(gc.CASES["quat_rot"].inputs)], model("quat_rot")[1], model("quat_rot")[0])
    f = orbhip.lib.orbhip_debug_geom_probe_host
    big = np.zeros((65537, 7))
    out = np.full((65537, 3), SENTINEL)
    op = orbhip.GEOM_OPS["quat_rot"][0]
    for args, code in (((-1, 4, 7, 3), orbhip.E_BADARG), ((len(orbhip.GEOM_OPS), 4, 7, 3), orbhip.E_BADARG), ((op, 4, 8, 3), orbhip.E_BADARG),
                       ((op, 4, 7, 4), orbhip.E_BADARG), ((op, -1, 7, 3), orbhip.E_BADARG), ((op, 65537, 7, 3), orbhip.E_CAPACITY),
                       ((op, 0, 7, 3), orbhip.OK)):
        rc = f(gpu_ctx.h, args[0], big.ctypes.data, args[1], args[2], out.ctypes.data, args[3])
        assert rc == code and np.all(out == SENTINEL), (args, rc)
        assert code == orbhip.OK or b"orbhip_debug_geom_probe_host" in orbhip.lib.orbhip_last_error()
    assert f(gpu_ctx.h, op, big.ctypes.data, 65536, 7, out.ctypes.data, 3) == orbhip.OK and np.all(out[65536:] == SENTINEL) and np.all(out[:65536] == 0)
    assert sorted(v[0] for v in orbhip.GEOM_OPS.values()) == list(range(len(orbhip.GEOM_OPS)))
