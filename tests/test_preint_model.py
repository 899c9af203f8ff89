"""CPU tests of IMU preintegration: the numpy model (tests/preint_model.py) against independent facts -- bias Jacobians against central
differences of the longdouble recursion, dR orthogonality, continuing against the concatenated list, both sides of IntegratedRotation's
branch, the information against a pseudo-inverse -- and the host class (host/ImuTypes.cc) in a stand-alone program under
AddressSanitizer / UBSan against a stub of the one device entry: IntegrateNewMeasurement held to the longdouble model by the K rule
the device is held to (tests/test_gpu_preint.py), Reintegrate's packing, MergePrevious's concatenation, Calib::Set.  No GPU.

Measured here, IntegrateNewMeasurement on the host, e_host / (e_float32_model + 2^-24 max|group|), worst group over the cases of
test_host_class_under_sanitizers: 2.7 (JPg; K = 128)."""
import os
import re
import subprocess
import numpy as np
import pytest
import ba_step_model as bsm
import preint_cases as pc
import preint_model as pm
import synth_inertial_opt as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
HOST = os.path.join(PKG, "host")
LD = pm.LD
NAMES = ("orbhip_preint_default_params", "orbhip_preint_wave_max_chains", "orbhip_preintegrate_device", "orbhip_preintegrate_host")


def test_symbols_declared_exported_and_bound():
    import orbhip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name), name
    assert orbhip.preint_wave_max_chains() == int(re.search(r"#define ORBHIP_PREINT_WAVE_MAX_CHAINS (\d+)", txt).group(1))
    strings = subprocess.run(["strings", os.path.join(PKG, "lib", "liborbhip.so")], stdout=subprocess.PIPE, text=True).stdout
    for k in ("k_preint_lane", "k_preint_wave", "k_preint_info"):
        assert k in strings, k
    p = orbhip.preint_params(ng=2.0, na=3.0, ngw=4.0, naw=5.0)
    assert np.array_equal(np.array(p.nga[:]).reshape(6, 6), np.diag([4.0] * 3 + [9.0] * 3))
    assert np.array_equal(np.array(p.nga_walk[:]).reshape(6, 6), np.diag([16.0] * 3 + [25.0] * 3))
    assert p.force_form == orbhip.PREINT_FORM_AUTO and p.want_info == 1


def _log_so3(R):
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD) / 2
    s = np.sqrt(w @ w)
    return w if s < 1e-30 else w * (np.arcsin(s) / s)


def test_bias_jacobians_match_central_differences():
    """J* are d(dR, dV, dP) / d(bias): the longdouble recursion re-run at b +- h.  Central differences leave O(h^2) (1e-10 here, times
    the third derivative, which grows with the chain's duration: the tolerance is 1e-7 relative to the Jacobian's largest entry)."""
    nga, walk = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)
    b = pc.bias(3).astype(np.float64)
    m = [pc.chain(80, 3)]
    h = 1e-5

    S0 = _integrate_ld(np.asarray(b, LD)[None, :], m, nga, walk)
    for j in range(6):
        e = np.zeros(6); e[j] = h
        Sp, Sm = _integrate_ld(np.asarray(b + e, LD)[None, :], m, nga, walk), _integrate_ld(np.asarray(b - e, LD)[None, :], m, nga, walk)
        dV = (Sp["dV"][0] - Sm["dV"][0]) / (2 * h); dP = (Sp["dP"][0] - Sm["dP"][0]) / (2 * h)
        dR = _log_so3(Sm["dR"][0].T @ Sp["dR"][0]) / (2 * h)
        if j < 3:
            JR, JV, JP = S0["JRg"][0][:, j], S0["JVg"][0][:, j], S0["JPg"][0][:, j]
        else:
            JR, JV, JP = np.zeros(3, LD), S0["JVa"][0][:, j - 3], S0["JPa"][0][:, j - 3]
        for got, want, scale in ((dR, JR, np.max(np.abs(S0["JRg"]))), (dV, JV, np.max(np.abs(S0["JVg"]))), (dP, JP, np.max(np.abs(S0["JPg"])))):
            assert float(np.max(np.abs(got - want))) <= 1e-7 * float(scale), (j, got, want)


def _integrate_ld(bias_ld, meas, nga, walk):
    return pm.integrate(bias_ld, meas, nga, walk, LD, exact_bias=True)


def test_dR_stays_orthogonal():
    b, m = pc.single(257)
    nga, walk = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)
    for dtype, tol in ((np.float32, 8 * 2.0 ** -24), (LD, 1e-17)):
        R = pm.integrate(b, m, nga, walk, dtype)["dR"][0].astype(LD)
        assert float(np.max(np.abs(R.T @ R - np.eye(3)))) <= tol
        assert abs(float(np.linalg.det(R.astype(np.float64))) - 1) < 1e-6


@pytest.mark.parametrize("split", [1, 64, 65])
def test_continuing_equals_the_concatenated_list(split):
    """MergePrevious / Tracking's appending: the recursion on the concatenation, to the last bit in the model's own arithmetic."""
    b, m = pc.single(129)
    nga, walk = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)
    for dtype in (np.float32, LD):
        whole = pm.integrate(b, m, nga, walk, dtype)
        first = pm.integrate(b, [m[0][:split]], nga, walk, dtype)
        both = pm.integrate(b, [m[0][split:]], nga, walk, dtype, start=first)
        for k in pm.FIELDS:
            assert np.array_equal(whole[k], both[k]), (k, dtype)     # (longdouble has padding bytes: values, not bytes)
        assert pm.concat([m[0][:split]], [m[0][split:]])[0].tobytes() == m[0].tobytes()


def test_cases_reach_both_sides_of_the_small_angle_branch():
    b, m = pc.branch_chain()
    accW = (m[:, 3:6] - b[None, 0:3]).astype(np.float32)
    v = accW * m[:, 6:7]
    d = np.sqrt((v * v).sum(axis=1, dtype=np.float32))
    assert d[3] == 0 and 0.85e-4 < d[6] < pm.EPS and pm.EPS < d[9] < 1.15e-4
    assert (d[[0, 1, 2, 4, 5, 7, 8, 10, 11]] > pm.EPS).all()
    dR, rJ = pm.integrated_rotation(accW, m[:, 6])
    for k in (3, 6):
        assert np.array_equal(dR[k], np.eye(3, dtype=np.float32) + pm.skew(v[k])) and np.array_equal(rJ[k], np.eye(3, dtype=np.float32))
    # the 0.5 W^2 term the small branch leaves out is below the float32 resolution of 1: the two branches meet.  (In float32 the other
    # branch returns rightJ = I at 1.1e-4 too, 1 - cos(d) being 0 there; in longdouble it is I - W / 2 + ...)
    ld, ldJ = pm.integrated_rotation(accW.astype(LD), m[:, 6].astype(LD))
    assert float(np.max(np.abs(ld[6] - dR[6].astype(LD)))) < 2.0 ** -24
    assert np.array_equal(ldJ[6], np.eye(3)) and float(np.max(np.abs(ldJ[9] - np.eye(3)))) > 5e-5


def test_information_is_the_pseudo_inverse():
    b, m = pc.single(65)
    C = pm.integrate(b, m, pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW), np.float32)["C"][0]
    info, ig, ia, w = pm.information(C, LD)
    A = ((C[:9, :9].astype(np.float64) + C[:9, :9].T.astype(np.float64)) / 2)
    assert (w > 8 * 9e-7 * np.max(np.abs(w))).all()            # full rank here: the plain inverse
    np.testing.assert_allclose((info.astype(np.float64) @ A), np.eye(9), atol=1e-6)
    np.testing.assert_allclose(ig.astype(np.float64) @ C[9:12, 9:12].astype(np.float64), np.eye(3), atol=1e-6)
    i64 = pm.information(C, np.float64)[0]
    assert float(np.max(np.abs(i64 - info))) <= 1e-9 * float(np.max(np.abs(info)))
    # a length-1 chain: three exactly singular directions are dropped, not inverted
    C1 = pm.integrate(*pc.single(1), pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW), np.float32)["C"][0]
    info1, _, _, w1 = pm.information(C1, LD)
    assert int((w1 <= 9e-7 * np.max(np.abs(w1))).sum()) == 3 and np.isfinite(info1.astype(np.float64)).all()
    assert np.linalg.matrix_rank(info1.astype(np.float64), tol=1e-6 * float(np.max(np.abs(info1)))) == 6


def test_information_cases_keep_clear_of_the_cut():
    """The condition the information check sets on its inputs, on the float32 model's covariances: every named length (preint_cases.
    info_lengths) and every chain of the batch and full-Nga cases the GPU test runs."""
    sets = [pc.info_lengths() + (pc.calib_nga(),), pc.batch(65) + (pc.calib_nga(),), pc.batch(5, seed=3) + (pc.full_nga(),)]
    sets[2][1][1] = pc.chain(1, 91); sets[2][1][3] = pc.chain(66, 92)
    for bias, meas, nga in sets:
        S = pm.integrate(bias, meas, nga, pc.calib_nga(pc.NGW, pc.NAW), np.float32)
        for c, m in enumerate(meas):
            if len(m) == 0:
                continue
            w = np.abs(pm.information(S["C"][c], LD)[3])
            thr = 9e-7 * float(np.max(w))
            assert not ((w > thr / 8) & (w < thr * 8)).any(), (len(m), w / thr)


def test_compile_callers_preint(tmp_path):
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "c.o"), os.path.join(HOST, "compile_callers_preint.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


STUB = r"""
// stand-alone check of IMU::Preintegrated's host side under AddressSanitizer / UBSan: the class file, the smoke driver's main and a stub
// of the one device entry that reads every input byte and writes every output byte the real one may, recognisably.
#include <cstdio>
#include <cstring>
#include "../include/orbhip.h"
static int g_calls = 0;
extern "C" {
void orbhip_preint_default_params(orbhip_preint_params *p, float, float, float, float) { memset(p, 0, sizeof(*p)); p->want_info = 1; }
int orbhip_preintegrate_host(orbhip_ctx *, const orbhip_preint_params *p, int chains, const int32_t *off, const float *meas, const uint8_t *cont,
                             double *rec, float *cov, float *avg, double *info, double *info_g, double *info_a)
{
    if (cont || p->want_info || info || info_g || info_a) return -1;
    for (int c = 0; c < chains; c++) {
        double *r = rec + ORBHIP_IBA_PREINT * c;
        double sa[3] = {0, 0, 0}, sw[3] = {0, 0, 0}, st = 0;
        for (int i = off[c]; i < off[c + 1]; i++) { for (int k = 0; k < 3; k++) { sa[k] += meas[7 * i + k]; sw[k] += meas[7 * i + 3 + k]; } st += meas[7 * i + 6]; }
        for (int i = 0; i < 61; i++) r[i] = 0;
        r[0] = off[c + 1] - off[c]; r[1] = st;
        for (int k = 0; k < 3; k++) { r[10 + k] = sa[k]; r[13 + k] = sw[k]; }
        for (int i = 0; i < 225; i++) cov[225 * c + i] = (float)(c + 1) + p->nga[i % 36] + p->nga_walk[i % 36];
        for (int i = 0; i < 6; i++) avg[6 * c + i] = (float)r[61 + i];
    }
    g_calls++;
    return 0;
}
const char *orbhip_last_error(void) { return ""; }
}
namespace ORB_SLAM3 { namespace hip { orbhip_ctx *ThreadContext() { return (orbhip_ctx *)&g_calls; } int GetDevice() { return 0; } } }
"""


def _scene(mode, n=6, seed=0):
    lens = [0, 1, 2, 40, 65, 130][:n]
    meas = [pc.chain(k, 50 + seed + i) for i, k in enumerate(lens)]
    bias = np.stack([pc.bias(60 + seed + i) for i in range(n)])
    m_b, m_m = pc.branch_chain()
    meas[3] = m_m; bias[3] = m_b
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(m) for m in meas])
    bias_new = (bias + np.float32(0.02)).astype(np.float32)
    return {"mode": np.array([mode], np.int32), "noise": np.array([pc.NG, pc.NA, pc.NGW, pc.NAW], np.float32), "meas_off": off,
            "meas": np.concatenate(meas).astype(np.float32), "bias": bias, "bias_new": bias_new}, meas, bias, bias_new


def _host_fields(out, prefix, n):
    r = lambda k, *s: out[prefix + k].reshape((n,) + s)
    return {"dT": r("dT"), "dR": r("dR", 3, 3), "dV": r("dV", 3), "dP": r("dP", 3), "JRg": r("JRg", 3, 3), "JVg": r("JVg", 3, 3),
            "JVa": r("JVa", 3, 3), "JPg": r("JPg", 3, 3), "JPa": r("JPa", 3, 3), "avgA": r("avgA", 3), "avgW": r("avgW", 3), "C": r("C", 15, 15)}


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    """host_preint_smoke's main, the class file and Tracking::PreintegrateIMU with the stub, under -fsanitize=address,undefined."""
    d = tmp_path_factory.mktemp("preint_asan")
    stub = d / "stub.cc"
    stub.write_text(STUB.replace("../include/orbhip.h", os.path.join(ROOT, "include", "orbhip.h")))
    exe = str(d / "preint_asan")
    srcs = [os.path.join(HOST, f) for f in ("host_preint_smoke.cc", "ImuTypes.cc", "Tracking_PreintegrateIMU.cc")]
    # the driver's mode 3 (Optimizer::InertialOptimization) and GetInformationMatrix refer to files this program leaves out and never calls
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", HOST, "-o", exe] + srcs +
                       [str(stub), "-Wl,--unresolved-symbols=ignore-all"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _run_exe(exe, tmp_path, arrays):
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    sio.write_flat(fin, arrays)
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-3000:]
    return sio.read_flat(fout), r.stdout


def test_host_class_under_sanitizers(asan_exe, tmp_path):
    exe = asan_exe
    worst = 0.0
    for mode in (0, 1, 2):
        arrays, meas, bias, bias_new = _scene(mode)
        n = len(meas)
        out, _ = _run_exe(exe, tmp_path, arrays)
        # Calib::Set
        assert out["calib"][:36].tobytes() == pc.calib_nga().tobytes() and out["calib"][36:].tobytes() == pc.calib_nga(pc.NGW, pc.NAW).tobytes()
        # IntegrateNewMeasurement: the K rule against the longdouble model
        nga, walk = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)
        ref, f32 = pc.models(bias, meas, nga, walk)
        for name, (ed, ef, fl) in pc.k_rule_ratios(_host_fields(out, "host_", n), ref, f32).items():
            print("host %-8s e_host %.3e e_f32 %.3e floor %.3e ratio %.2f" % (name, ed, ef, fl, ed / (ef + fl) if ed else 0.0))
            worst = max(worst, ed / (ef + fl) if ed else 0.0)
            assert bsm.within_bound(ed, ef, fl), (name, ed, ef, fl)
        assert out["host_b"].reshape(n, 6).tobytes() == bias.tobytes()
        # what the stub saw: the chain's own measurements at the updated bias (modes 0, 1), the previous chain's then the own (mode 2)
        dev = _host_fields(out, "dev_", n)
        if mode in (0, 1):
            assert out["device_calls"][0] == (n if mode == 0 else 1)
            assert out["reint"].tolist() == ([1] * n if mode == 0 else [0] * n)
            chains, want_b, who = meas, bias_new, range(n)
        else:
            assert out["device_calls"][0] == n // 2
            chains = list(meas)
            for k in range(0, n - 1, 2):
                chains[k + 1] = np.concatenate([meas[k], meas[k + 1]])
            want_b, who = bias, range(1, n, 2)
            assert out["nmeas"].tolist() == [len(c) for c in chains]
        for c in who:
            mm = chains[c].astype(np.float64)
            assert dev["dT"][c] == np.float32(len(mm))
            np.testing.assert_array_equal(dev["dV"][c], mm[:, 0:3].sum(axis=0).astype(np.float32))
            np.testing.assert_array_equal(dev["dP"][c], mm[:, 3:6].sum(axis=0).astype(np.float32))
            assert dev["dR"][c][0, 0] == np.float32(mm[:, 6].sum())
            np.testing.assert_array_equal(np.concatenate([dev["avgA"][c], dev["avgW"][c]]), want_b[c])
            assert out["dev_b"].reshape(n, 6)[c].tobytes() == want_b[c].tobytes()
        if mode == 2:
            for c in range(0, n, 2):                     # the previous objects are left as the host loop made them
                for k in pm.FIELDS:
                    assert dev[k][c].tobytes() == _host_fields(out, "host_", n)[k][c].tobytes()
    print("worst host ratio %.2f" % worst)


def test_batch_integrates_a_repeated_object_once(asan_exe, tmp_path):
    """ReintegrateBatch with every object listed twice: one call, every chain once (the stub counts the chains of a call)."""
    arrays, meas, bias, bias_new = _scene(1)
    arrays["dup"] = np.array([1], np.int32)
    out, _ = _run_exe(asan_exe, tmp_path, arrays)
    n = len(meas)
    assert out["device_calls"][0] == 1
    dev = _host_fields(out, "dev_", n)
    for c in range(n):
        assert dev["dT"][c] == np.float32(len(meas[c]))
        assert dev["C"][c][0, 0] == np.float32(np.float32(c + 1) + pc.calib_nga()[0, 0] + pc.calib_nga(pc.NGW, pc.NAW)[0, 0])       # chain c of n, not of 2 n


# ---------------------------------------------------------------------------------------------- Tracking::PreintegrateIMU
def _steps_model(ts, imu, t_prev, t_cur):
    """src/Tracking.cc:574-647 restated: the queue walk -> (points taken, points left in the queue), then the four interpolation cases in
    float32 as the C++ evaluates them (differences of double stamps rounded to float, Point3f arithmetic in float)."""
    f = np.float32
    taken, queue = [], list(range(len(ts)))
    while queue:
        i = queue[0]
        if ts[i] < t_prev - 0.001:
            queue.pop(0)
        elif ts[i] < t_cur - 0.001:
            taken.append(i); queue.pop(0)
        else:
            taken.append(i)
            break
    n = len(taken) - 1
    steps = []
    for i in range(n):
        p, q = taken[i], taken[i + 1]
        a0, a1 = imu[p].astype(f), imu[q].astype(f)
        if i == 0 and i < n - 1:
            tab, tini = f(ts[q] - ts[p]), f(ts[p] - t_prev)
            v = ((a0 + a1) - (a1 - a0) * f(tini / tab)) * f(0.5); dt = f(ts[q] - t_prev)
        elif i < n - 1:
            v = (a0 + a1) * f(0.5); dt = f(ts[q] - ts[p])
        elif i > 0 and i == n - 1:
            tab, tend = f(ts[q] - ts[p]), f(ts[q] - t_cur)
            v = ((a0 + a1) - (a1 - a0) * f(tend / tab)) * f(0.5); dt = f(t_cur - ts[p])
        else:
            v = a0; dt = f(t_cur - t_prev)
        steps.append(np.concatenate([v.astype(f), [dt]]).astype(f))
    return np.array(steps, f).reshape(-1, 7), len(taken), len(queue)


@pytest.mark.parametrize("k_inside", [1, 2, 3, 9])
def test_tracking_preintegrate_imu_interpolation(asan_exe, tmp_path, k_inside):
    """The four cases of src/Tracking.cc:609-647: one step (n = 1: the single case), two (first and last), three and more (first, middle,
    last); points before the previous frame are dropped, the first point at or after the current frame closes the list and stays
    queued; both chains take every step, the keyframe chain on top of what it held."""
    rng = np.random.default_rng(k_inside)
    t_prev, t_cur = 1403636580.763555527, 1403636580.813555527
    inside = t_prev + 0.0007 + (t_cur - t_prev) * (np.arange(k_inside) / k_inside)
    ts = np.concatenate([[t_prev - 0.012, t_prev - 0.007], inside, [t_cur + 0.0031, t_cur + 0.0081]])
    imu = np.concatenate([np.array([0.3, 9.7, -0.8]) + 0.5 * rng.standard_normal((len(ts), 3)), 0.3 * rng.standard_normal((len(ts), 3))], axis=1).astype(np.float32)
    pre = pc.chain(5, 31)
    arrays = {"mode": np.array([-3], np.int32), "noise": np.array([pc.NG, pc.NA, pc.NGW, pc.NAW], np.float32), "meas_off": np.array([0, 5], np.int32),
              "meas": pre, "bias": pc.bias(31)[None, :], "bias_new": pc.bias(31)[None, :], "kf_pre": np.array([5], np.int32), "imu": imu,
              "imu_t": sio.raw(ts), "t_prev": sio.raw([t_prev]), "t_cur": sio.raw([t_cur])}
    out, _ = _run_exe(asan_exe, tmp_path, arrays)
    want, n_taken, n_left = _steps_model(ts, imu, t_prev, t_cur)
    assert len(want) == k_inside and n_taken == k_inside + 1 and n_left == 2         # the closing point stays queued, one more behind it
    assert out["steps"].reshape(-1, 7).tobytes() == want.tobytes()
    assert out["frame_n"][0] == k_inside and out["kf_n"][0] == 5 + k_inside
    assert out["from_last_frame"][0] == n_taken and out["queue_left"][0] == n_left
    assert out["integrated"][0] == 1 and out["kf_is_current"][0] == 1
    # both chains hold the recursion on those steps: the frame chain fresh, the keyframe chain continuing (K rule, as the host loop)
    nga, walk = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)
    meas = [np.concatenate([pre, want]), want]
    bias = [pc.bias(31)] * 2
    ref, f32 = pc.models(bias, meas, nga, walk)
    for name, (ed, ef, fl) in pc.k_rule_ratios(_host_fields(out, "host_", 2), ref, f32).items():
        assert bsm.within_bound(ed, ef, fl), (name, ed, ef, fl)


def test_tracking_preintegrate_imu_without_work(asan_exe, tmp_path):
    """No previous frame, or an empty queue: the frame is marked integrated and nothing else happens."""
    base = {"mode": np.array([-3], np.int32), "noise": np.array([pc.NG, pc.NA, pc.NGW, pc.NAW], np.float32), "meas_off": np.array([0, 0], np.int32),
            "meas": np.zeros((1, 7), np.float32), "bias": pc.bias(31)[None, :], "bias_new": pc.bias(31)[None, :], "kf_pre": np.array([0], np.int32),
            "t_cur": sio.raw([10.05])}
    imu = np.ones((3, 6), np.float32)
    for arrays in (dict(base, imu=imu, imu_t=sio.raw([10.0, 10.02, 10.06])),                               # no t_prev: no previous frame
                   dict(base, imu=np.zeros((0, 6), np.float32), imu_t=sio.raw([]), t_prev=sio.raw([10.0]))):
        out, _ = _run_exe(asan_exe, tmp_path, arrays)
        assert out["integrated"][0] == 1 and out["kf_n"][0] == 0 and "frame_n" not in out and out["kf_is_current"][0] == 0
        assert out["queue_left"][0] == len(arrays["imu"])
