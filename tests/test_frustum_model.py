"""CPU tests of the Frame::isInFrustum model (tests/frustum_model.py): against a float64 restatement written separately, on crafted boundary
rows with hand-written outcomes, the level thresholds against the expression of MapPoint::PredictScale, the C++ host member
(lib/host_frustum_smoke frustum) bit for bit, and the guards: wrong comparison rules are told from right ones, the new symbols are declared,
exported and bound, the reference's call lines compile against the host classes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frustum_model as fm
import synth_frustum as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_frustum_smoke")
EPS = 2.0 ** -24            # half an ulp of a float32 in [1, 2): the relative error of one rounding
_SCENES = {}


def _scene(kind):
    """the three seeded scenes and the model's answer (computed once, shared, not modified)"""
    if kind not in _SCENES:
        fr, pts = sf.make_scene(kind, 1000, {"mono": 1, "stereo": 2, "rig": 3}[kind])
        rec, ntm, und = fm.frustum(fr, pts)
        assert not und.any()
        _SCENES[kind] = (fr, pts, rec, ntm, sf.assert_covers(fr, rec))
    return _SCENES[kind]


# ---------------------------------------------------------------- the float64 restatement (no helper shared with the model)
def _project64(cam_type, p, P):
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        if cam_type == 0:
            return p[0] * x / z + p[2], p[1] * y / z + p[3]
        theta = np.arctan2(np.hypot(x, y), z); psi = np.arctan2(y, x)
        r = theta + p[4] * theta ** 3 + p[5] * theta ** 5 + p[6] * theta ** 7 + p[7] * theta ** 9
        return p[0] * r * np.cos(psi) + p[2], p[1] * r * np.sin(psi) + p[3]


def _frustum64(fr, pts, right):
    """codes, levels, u, v, depth, viewCos in float64, the margin of every point's deciding quantity (relative distance to the nearest
    threshold it was compared with, up to and including the test that decided), and a per-point tolerance for u, v, depth, viewCos."""
    R = np.asarray(fr["Rrw" if right else "Rcw"], np.float64).reshape(3, 3); t = np.asarray(fr["trw" if right else "tcw"], np.float64)
    O = np.asarray(fr["Orw" if right else "Ow"], np.float64)
    cam = np.asarray(fr["cam"][1 if right else 0], np.float64); ctype = int(fr["cam_type"][1 if right else 0])
    X = pts["Xw"].astype(np.float64); Nn = pts["normal"].astype(np.float64)
    min_x, min_y, max_x, max_y = [float(v) for v in fr["bounds"]]
    Pc = X @ R.T + t
    depth = np.linalg.norm(Pc, axis=1)
    u, v = _project64(ctype, cam, Pc)
    PO = X - O
    dist = np.linalg.norm(PO, axis=1)
    near = float(np.float32(0.8)) * pts["min_dist"].astype(np.float64); far = float(np.float32(1.2)) * pts["max_dist"].astype(np.float64)
    cos = np.einsum("ij,ij->i", PO, Nn) / dist
    lsf = float(fr["log_scale_factor"]); nl = int(fr["nlevels"])
    ratio = pts["max_dist"].astype(np.float64) / dist
    e = np.log(ratio) / lsf
    level = np.clip(np.ceil(e), 0, nl - 1).astype(int)
    n = len(X)
    code = np.zeros(n, int); margin = np.full(n, np.inf)
    W, H = max_x - min_x, max_y - min_y
    tests = [(2, Pc[:, 2] < 0, np.abs(Pc[:, 2]) / depth),
             (3, (u < min_x) | (u > max_x), np.minimum(np.abs(u - min_x), np.abs(u - max_x)) / W),
             (4, (v < min_y) | (v > max_y), np.minimum(np.abs(v - min_y), np.abs(v - max_y)) / H),
             (5, dist < near, np.abs(dist / np.maximum(near, 1e-300) - 1)), (6, dist > far, np.abs(dist / far - 1)),
             (7, cos < float(fr["viewing_cos_limit"]), np.abs(cos / float(fr["viewing_cos_limit"]) - 1))]
    live = np.ones(n, bool)
    for c, fails, m in tests:
        margin[live] = np.minimum(margin[live], m[live])
        code[live & fails] = c
        live &= ~fails
    # the level changes where e crosses an integer in [0, nl - 2]: the ratio's relative distance to scale^k is |e - k| * lsf
    k = np.clip(np.round(e), 0, nl - 2)
    margin[live] = np.minimum(margin[live], (np.abs(e - k) * lsf)[live])
    # tolerances from float32 rounding of the operands (EPS = 2^-24 per rounding).  Pc_i is three products and three sums: at most 6 roundings
    # of numbers no larger than sum_j |R_ij X_j| + |t_i|.  The projection moves by at most |dPc| * dproj/dP, plus the roundings of its own
    # few operations (pinhole: 4; KannalaBrandt8: the polynomial and the float roundings of the atan2 / sine / cosine results: 16) on |u - c| and one on u
    dP = 6 * EPS * (np.abs(X) @ np.abs(R).T + np.abs(t)).max(axis=1)
    rho = np.hypot(Pc[:, 0], Pc[:, 1])
    with np.errstate(all="ignore"):
        if ctype == 0:
            gain = (1 + np.maximum(np.abs(Pc[:, 0]), np.abs(Pc[:, 1])) / np.abs(Pc[:, 2])) / np.abs(Pc[:, 2])
            own = 4
        else:
            gain = 2 * (1 / depth + np.arctan2(rho, Pc[:, 2]) / np.maximum(rho, 1e-300))
            own = 16
    tol_u = cam[0] * dP * gain + own * EPS * np.abs(u - cam[2]) + EPS * np.abs(u)
    tol_v = cam[1] * dP * gain + own * EPS * np.abs(v - cam[3]) + EPS * np.abs(v)
    tol_depth = np.sqrt(3) * dP + 2 * EPS * depth
    # PO_i: one rounding of a float subtraction; the dot product and the norm are exact to double; one rounding of the quotient, one of dist
    tol_cos = EPS * (np.abs(PO) @ np.ones(3)) * np.linalg.norm(Nn, axis=1) / dist * 2 + 3 * EPS * np.abs(cos)
    return dict(code=code, level=level, u=u, v=v, depth=depth, cos=cos, margin=margin, tol=(tol_u, tol_v, tol_depth, tol_cos))


@pytest.mark.parametrize("kind", sf.KINDS)
def test_model_against_a_float64_restatement(kind):
    """Outcome codes and levels agree except on points whose deciding quantity lies within relative 1e-5 of its threshold in float64
    (exempt; at most 0.5 % of a scene), and the accepted points' u, v, depth and viewCos agree within the tolerance _frustum64 derives from
    float32 rounding of the operands.  Measured, 1000 points per scene (skipped points are not counted): mono 0 exempt, stereo 0, rig 0
    left / 0 right; every code and level of the others equal."""
    fr, pts, rec, ntm, hist = _scene(kind)
    print(kind, {k: v.tolist() for k, v in hist.items()})
    for right in ([False, True] if fr["rig"] else [False]):
        r = _frustum64(fr, pts, right)
        code = rec["code_r" if right else "code"].astype(int)
        live = code != 1
        exempt = live & (r["margin"] < 1e-5)
        print(kind, "right" if right else "left", "exempt", int(exempt.sum()), "of", int(live.sum()))
        assert exempt.sum() <= 0.005 * len(code)
        cmp = live & ~exempt
        assert np.array_equal(code[cmp], r["code"][cmp]), np.flatnonzero(cmp & (code != r["code"]))[:5]
        acc = cmp & (code == 0)
        assert acc.sum() > 200
        assert np.array_equal(rec["level_r" if right else "level"][acc], r["level"][acc])
        names = ("proj_xr", "proj_yr", "depth_r", "view_cos_r") if right else ("proj_x", "proj_y", "depth", "view_cos")
        for name, want, tol in zip(names, (r["u"], r["v"], r["depth"], r["cos"]), r["tol"]):
            err = np.abs(rec[name][acc].astype(np.float64) - want[acc])
            assert np.all(err <= tol[acc]), (name, float(np.max(err / tol[acc])))


# ---------------------------------------------------------------- boundary rows
def test_boundary_rows_have_their_hand_written_outcomes():
    for fr, pts, names, codes, nq_row, radius in sf.boundary_rows():
        rec, ntm, und = fm.frustum(fr, pts)
        assert not und.any()
        assert np.array_equal(rec["code"], codes[:, 0]) and np.array_equal(rec["code_r"], codes[:, 1]), (names, rec["code"], rec["code_r"])
        q, dq, owner = fm.queries(fr, pts, rec)
        assert np.array_equal(np.bincount(owner, minlength=len(names)), nq_row), (names, owner)
        for name, want in radius.items():
            assert q["radius"][list(owner).index(names.index(name))] == want
        assert ntm == int(np.sum((rec["in_view"] | rec["in_view_r"]) != 0))
    # the rig point only the right camera sees: no query with a stale depth above thFarPoints, its right query (has_obs | 2) below it
    fr, pts, names, codes, nq_row, _ = sf.boundary_rows()[1]
    rec, _, _ = fm.frustum(fr, pts)
    q, _, owner = fm.queries(fr, pts, rec)
    k = list(owner).index(names.index("right_only_near"))
    assert names.index("right_only_far") not in owner and q["has_obs"][k] == 3 and q["ur"][k] == -1 and rec["depth"][names.index("right_only_near")] == 0


@pytest.mark.parametrize("rule,rows,code", [("bounds_strict", ("u_min", "u_max"), 3), ("bounds_strict", ("v_min", "v_max"), 4),
                                            ("distance_strict", ("near",), 5), ("distance_strict", ("far",), 6), ("angle_strict", ("cos_limit",), 7)])
def test_boundary_rows_tell_wrong_rules_from_right(rule, rows, code):
    """`<` replaced by `<=` in the bounds, distance or angle test changes the outcome of the rows that sit on that threshold, and of no other"""
    fr, pts, names, codes, _, _ = sf.boundary_rows()[0]
    rec, _, _ = fm.frustum(fr, pts, dict(fm.RIGHT_RULES, **{rule: False}))
    for name in rows:
        assert rec["code"][names.index(name)] == code and codes[names.index(name), 0] == 0
    on_threshold = {"bounds_strict": ("u_min", "u_max", "v_min", "v_max"), "distance_strict": ("near", "far"), "angle_strict": ("cos_limit",)}[rule]
    others = [i for i, nm in enumerate(names) if nm not in on_threshold]
    assert np.array_equal(rec["code"][others], codes[others, 0])


# ---------------------------------------------------------------- level thresholds
@pytest.mark.parametrize("scale,nlevels", [(1.2, 8), (2.0, 4)])
def test_level_thresholds_equal_the_predict_scale_expression(scale, nlevels):
    """Counting thresholds == ceil(logf(ratio) / mfLogScaleFactor) clamped, for every float within 4096 ulps of every threshold and on 10^6
    seeded ratios from 1e-3 to 1e3 -- which also shows the level never decreases with the ratio, what the bisection assumes."""
    import orbhip
    lsf = fm.logf(np.float32(scale))
    T = orbhip.predict_scale_thresholds(lsf, nlevels)
    assert len(T) == nlevels - 1 and np.all(np.diff(T) > 0) and T[0] == np.nextafter(np.float32(1), np.float32(2))
    logf = fm._libm.logf

    def levels(r):
        lg = np.array([logf(x) for x in r.tolist()], np.float32)
        return np.clip(np.ceil(lg / lsf), 0, nlevels - 1).astype(int)
    for n, t in enumerate(T):
        bits = int(np.float32(t).view(np.uint32)) + np.arange(-4096, 4097)
        r = bits.astype(np.uint32).view(np.float32)
        want = levels(r)
        got = np.count_nonzero(r[:, None] >= T[None, :], axis=1)
        assert np.array_equal(got, want), (n, t)
        assert want[4095] == n and want[4096] == n + 1                         # the threshold IS the first ratio of level n + 1
    rng = np.random.default_rng(12)
    r = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), 1000000)).astype(np.float32)
    want = levels(r)
    assert np.array_equal(np.count_nonzero(r[:, None] >= T[None, :], axis=1), want)
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff(want[order]) >= 0) and set(want.tolist()) == set(range(nlevels))
    assert all(fm.level_by_expression(x, lsf, nlevels) == w for x, w in zip(r[:200], want[:200]))       # the model's own spelling


def test_threshold_builder_refuses_bad_arguments():
    import orbhip
    for args in ((np.float32(0.18), 33), (np.float32(0.18), 0), (np.float32(0.0), 8), (np.float32(np.inf), 8)):
        with pytest.raises(orbhip.OrbHipError) as ei:
            orbhip.predict_scale_thresholds(*args)
        assert ei.value.code == orbhip.E_BADARG
    assert len(orbhip.predict_scale_thresholds(np.float32(0.18), 1)) == 0


# ---------------------------------------------------------------- the C++ host member against the model, no device
def _host_member(tmp_path, fr, pts, seed):
    n = len(pts["flags"])
    trk_f, trk_i = sf.initial_state(n, seed)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    sf.write_flat(inp, sf.smoke_input(fr, pts, trk_f, trk_i))
    r = subprocess.run([SMOKE, "frustum", inp, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    got = sf.read_flat(out)
    rec, _, und = fm.frustum(fr, pts)
    mps = sf.points_from_state(pts, trk_f, trk_i)
    want_ret = np.full(n, -1, np.int32)
    for p, rr in zip(mps, rec):
        if rr["code"] != 1:
            fm.apply_record(p, rr, bool(fr["rig"]))
            want_ret[p.idx] = int(rr["in_view"] or rr["in_view_r"])
    tf, ti, _, _ = sf.state_arrays(mps)
    return got, tf, ti, want_ret, rec, und


@pytest.mark.parametrize("kind", sf.KINDS)
def test_host_member_equals_the_model_bit_for_bit(tmp_path, kind):
    """Frame::isInFrustum of host/Frame.cc (lib/host_frustum_smoke frustum: the host member alone, no device) leaves every MapPoint field as
    the model's record and code say -- the ones it writes and the ones it leaves alone -- and returns the model's value, on the three scenes.
    (The member's signature shows no outcome code: which fields of a point changed, from a random earlier state, is what tells the codes
    apart -- 2..4, which leave the same trace, excepted.)"""
    fr, pts, _, _, _ = _scene(kind)
    got, tf, ti, want_ret, rec, und = _host_member(tmp_path, fr, pts, 1)
    assert np.array_equal(got["ret"], want_ret)
    assert np.array_equal(got["trk_i"].reshape(-1, 4), ti)
    assert np.array_equal(got["trk_f"].view(np.uint32).reshape(-1, 8), tf.view(np.uint32)), \
        np.flatnonzero(np.any(got["trk_f"].view(np.uint32).reshape(-1, 8) != tf.view(np.uint32), axis=1))[:10]


def test_host_member_on_the_boundary_rows(tmp_path):
    for k, (fr, pts, names, codes, _, _) in enumerate(sf.boundary_rows()):
        got, tf, ti, want_ret, rec, und = _host_member(tmp_path, fr, pts, 2 + k)
        assert np.array_equal(rec["code"], codes[:, 0])
        assert np.array_equal(got["ret"], want_ret), (names, got["ret"], want_ret)
        assert np.array_equal(got["trk_i"].reshape(-1, 4), ti) and np.array_equal(got["trk_f"].view(np.uint32).reshape(-1, 8), tf.view(np.uint32)), names


# ---------------------------------------------------------------- bookkeeping and guards
def test_th_choice_table():
    """Tracking.cc:2406-2426 row by row: (sensor, imu initialised, BA2, frame id, last reloc id, state) -> th"""
    MONO, STEREO, RGBD, IMU_MONO, IMU_STEREO, OK, RECENTLY_LOST, LOST = 0, 1, 2, 3, 4, 2, 3, 4
    table = [((MONO, 0, 0, 10, 0, OK), 1), ((STEREO, 0, 0, 10, 0, OK), 1), ((RGBD, 0, 0, 10, 0, OK), 3), ((IMU_MONO, 0, 0, 10, 0, OK), 10),
             ((IMU_STEREO, 0, 0, 10, 0, OK), 10), ((IMU_MONO, 1, 0, 10, 0, OK), 3), ((IMU_STEREO, 1, 1, 10, 0, OK), 2), ((RGBD, 1, 1, 10, 0, OK), 2),
             ((MONO, 0, 0, 10, 9, OK), 5), ((MONO, 0, 0, 11, 9, OK), 1), ((IMU_MONO, 1, 1, 10, 9, OK), 5), ((MONO, 0, 0, 10, 9, RECENTLY_LOST), 15),
             ((RGBD, 0, 0, 10, 0, LOST), 15)]
    for row, th in table:
        assert fm.choose_th(*row) == th, row


def test_new_symbols_are_declared_exported_and_bound():
    import orbhip
    txt = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("orbhip_frustum_queries_device", "orbhip_search_local_points_device", "orbhip_search_local_points_host",
                 "orbhip_search_local_points_host_resident", "orbhip_predict_scale_thresholds", "orbhip_frustum_chunk"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(orbhip.lib, name) and getattr(orbhip.lib, name).argtypes is not None, name
    for name in ("frustum_queries_device", "search_local_points_device", "search_local_points_host", "predict_scale_thresholds"):
        assert callable(getattr(orbhip, name))
    assert orbhip.FRUSTUM_CHUNK == int(re.search(r"#define ORBHIP_FRUSTUM_CHUNK (\d+)", txt).group(1))
    assert orbhip.TRACK_RECORD_DTYPE == fm.TRACK_RECORD_DTYPE
    # the record layouts the binding mirrors are the header's: a C program prints their sizes
    assert orbhip.FRUSTUM_FRAME_DTYPE.itemsize == 480 and orbhip.TRACK_RECORD_DTYPE.itemsize == 44 and C.sizeof(orbhip.LocalPoints) == 64


def test_record_sizes_match_the_header(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "orbhip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(orbhip_frustum_frame), sizeof(orbhip_track_record), '
                   'sizeof(orbhip_local_points)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    import orbhip
    assert subprocess.check_output([str(exe)], text=True).split() == [str(orbhip.FRUSTUM_FRAME_DTYPE.itemsize), str(orbhip.TRACK_RECORD_DTYPE.itemsize),
                                                                     str(C.sizeof(orbhip.LocalPoints))]


def test_tracking_call_lines_compile_against_the_host_classes(tmp_path):
    """host/compile_callers_tracking.cc (the reference's lines Tracking.cc:1981-1982, :2380-2401, :2428) builds -Wall -Werror against the host
    headers, and what it calls of Frame, Tracking and ORBmatcher is defined by host/Frame.cc, host/Tracking_SearchLocalPoints.cc and
    host/ORBmatcher.cc"""
    host = os.path.join(ROOT, "orb-slam3-mac_amd", "host")
    obj = str(tmp_path / "callers.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(host, "compile_callers_tracking.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    undefined = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True).stdout
    wanted = [ln.split("U ", 1)[1].strip() for ln in undefined.splitlines() if re.search(r"ORB_SLAM3::(Frame|Tracking|ORBmatcher)::", ln)]
    assert any("Frame::isInFrustum" in w for w in wanted) and any("Tracking::SearchLocalPoints" in w for w in wanted), wanted
    defined = ""
    for src in ("Frame.cc", "Tracking_SearchLocalPoints.cc", "ORBmatcher.cc"):
        o = str(tmp_path / (src + ".o"))
        r = subprocess.run(["g++", "-std=c++17", "-O0", "-c", "-o", o, os.path.join(host, src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        defined += subprocess.run(["nm", "-C", "--defined-only", o], stdout=subprocess.PIPE, text=True).stdout
    missing = [w for w in wanted if w not in defined]
    assert not missing, missing
