"""The case table and the models of the geometry probe, on the CPU: every item takes the branch its label names in the 50-digit and in the
float64 run, the branches the issue lists are all taken, every branch argument keeps its margin, the float64 faithful model stands at
float64's floor against the 50-digit one, it agrees with the models the solver tests already use, the faithful models meet the truth
where the reference's formula is exact, and the truth checks stay below 400 items.  Run with -s for the coverage table."""
import math
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp

import essential_graph_model as egm
import geom_probe_cases as gc
import geom_probe_model as gm
import oracle_match_bind as om
import pose_inertial_model as pim
import sim3_opt_model as s3m

f32, f64 = np.float32, np.float64
MARGIN = 1e-9
BRANCHY = [op for op, c in gc.CASES.items() if c.labels is not None and op in gm.FAITHFUL and op != "so3_normalize"]     # (its labels are the deltas)


@pytest.fixture(scope="module")
def runs():
    return {op: gm.run_faithful(op, gc.CASES[op].inputs, want_margins=True) for op in gm.FAITHFUL}


def test_labels_coverage_and_margins(runs):
    cover = {}
    for op in BRANCHY:
        _, _, br, br64, mg = runs[op]
        lab = gc.CASES[op].labels
        for i, (b, b64, l) in enumerate(zip(br, br64, lab)):
            assert b in l.split("|") and b64 == b, (op, i, b, b64, l)
            for name, v in mg[i]:
                assert v == 0.0 or v >= MARGIN, (op, i, name, v)
        cover[op] = Counter(br)
        print("%-18s %s" % (op, dict(sorted(cover[op].items()))))
    c = cover["R_to_quat"]
    assert all(c[b] >= 16 for b in ("trace", "i0", "i1", "i2")), c
    R = gc.CASES["R_to_quat"].inputs
    assert sum(1 for r, l in zip(R, gc.CASES["R_to_quat"].labels) if r[0] == r[4] and l != "trace") >= 8           # ties R[0] == R[4]
    assert all(cover["quat_norm_rot"][b] >= 3 for b in ("flip", "keep", "w0"))
    assert all(cover["huber"][b] >= 8 for b in ("below", "at", "above"))
    for op in ("so3_exp", "so3_exp_imu", "so3_right_jac", "so3_inv_right_jac"):
        assert cover[op]["small"] >= 16 and cover[op]["large"] >= 16
    assert all(cover["so3_log"][b] >= 2 for b in ("scaled", "unscaled", "out_of_range"))
    e = Counter(b.split("/")[0] for b in runs["s3_exp"][2])
    assert all(e[b] >= 16 for b in ("ssts", "sstl", "slts", "sltl")), e
    assert Counter(b.split("/")[1] for b in runs["s3_exp"][2])["i1"] >= 4          # the exponential reaches R_to_quat's other branches
    assert {b.split("/")[1] for b in runs["se3_oplus"][2]} == {"trace", "i0", "i1", "i2"}
    lg = Counter(runs["s3_log"][2])
    for pre in ("sstl", "sltl", "slts"):
        for piv in ("p01", "p11", "p21", "p02", "p12", "p22"):
            assert lg[pre + "/" + piv] >= 8, (pre, piv, lg)
    # no exchange is reachable with a small sigma AND a small theta (the search below)
    assert lg["ssts/p01"] >= 8 and lg["ssts/p02"] == 1 and all(k in ("ssts/p01", "ssts/p02") for k in lg if k.startswith("ssts")), lg     # (p02: the crafted zero pivot)
    assert cover["cam_project"]["kb8"] and cover["cam_project"]["pinhole"]


def test_s3_log_small_small_never_pivots():
    """the CPU search behind 'unreachable': with |sigma| < 1e-5 and d > 1 - 1e-5, W = I + O(theta) and no row is ever exchanged"""
    rng = np.random.default_rng(5)
    seen = Counter()
    for _ in range(2000):
        x = gc.s3_log_draw(rng, True, True)
        seen[gm.s3_log(gm.N64, [f64(v) for v in x])[1].split("/")[1]] += 1
    assert set(seen) == {"p01"}, seen


def test_pivot_tie_is_exact():
    """the crafted item's column 0 is (a, a, 0) bit for bit: Eigen keeps the first row"""
    S = gc.CASES["s3_log"].inputs[gc.TIE_ITEM]
    t = S[3] * 2.0 ** -9
    assert S[2] * 2 * S[3] == t                                                     # om2 = 2 z w exactly
    a = f64(1) + (f64(1) / f64(6)) * -(f64(t) * f64(t))
    assert a == 0.5 * t and a > 0
    m = []
    _, br = gm.s3_log(gm.N64, [f64(v) for v in S], m)
    assert br == "ssts/p01" and dict(m)["pivot0"] == 0.0
    # Both pivot orders solve [[a, -a, 0], [a, a, 0], [0, 0, 1]] x = T equally well: x1 = fl(fl(T1 - T0) / 2a) either way, and
    # x0 = (T0 + a x1) / a with the first row kept, (T1 - a x1) / a with the rows exchanged.  For this T the two differ in the last bit
    # with the product contracted (one rounding) or not (two), and the first-row order gives the same bits both ways: a device result
    # equal to the float64 model's bits can only come from Eigen's rule (the first of equal magnitudes).
    a, T0, T1 = Fraction(float(a)), gc.TIE_T0, gc.TIE_T1

    def rnd(fr):
        return fr.numerator / fr.denominator                                        # int / int is correctly rounded
    y = rnd(Fraction(T1 - T0) / (2 * a))
    keep_fma, keep_two = rnd(Fraction(T0) + a * Fraction(y)), T0 + rnd(a * Fraction(y))
    swap_fma, swap_two = rnd(Fraction(T1) - a * Fraction(y)), T1 - rnd(a * Fraction(y))
    x0 = rnd(Fraction(keep_fma) / a)
    assert keep_fma == keep_two and x0 != rnd(Fraction(swap_fma) / a) and x0 != rnd(Fraction(swap_two) / a)
    row = gm.run_faithful("s3_log", [S])[1][0]
    assert row.tolist() == [0.0, 0.0, t, x0, y, 2.25, 0.0]
    Z = gc.CASES["s3_log"].inputs[gc.TIE_ITEM - 1]                                  # and the crafted zero on column 1's diagonal
    t = f64(Z[3] * 2.0 ** -9)
    assert Z[0] * 2 * Z[3] == t == gc.ZERO_PIVOT_T and f64(1) + (f64(1) / f64(6)) * -(t * t) == 0
    assert gm.s3_log(gm.N64, [f64(v) for v in Z])[1] == "ssts/p02" and np.isfinite(gm.run_faithful("s3_log", [Z])[1]).all()


def test_f64_model_at_its_floor(runs):
    """A sanity check on the models: the float64 run of a formula against its 50-digit run.  Per op the largest e_64 / floor (floor =
    2^-52 max |expected| of the item) is printed and held to the op's conditioning: 1 / |sin theta| <= 1e7 for the logarithms and the
    inverse right Jacobian at pi - 1e-7, the 1e5 of dividing by a 1e-5 sine / angle, 2^10 elsewhere; s3_log with a large sigma and a small
    theta solves with cond(W) <= 1 + |B| theta^2 <= 1e10 (B <= 1 / sigma^3 at |sigma| >= 1.1e-5, theta <= 4e-3; geom_probe_cases.py)."""
    cap = dict(so3_log=2e8, s3_log=1e11, so3_inv_right_jac=2e8, so3_right_jac=1e6, s3_exp=1e6, se3_oplus=1e6, so3_exp=1e6, so3_exp_imu=1e6)
    for op, (exp, y64, _, _, _) in runs.items():
        e, fl, same = gm.errors(y64, exp)
        assert same.all(), (op, np.flatnonzero(~same))
        ratio = e / np.where(fl > 0, fl, 2.0 ** -52)
        print("%-18s e_64 / floor <= %.3g" % (op, ratio.max()))
        assert ratio.max() <= cap.get(op, 1024.0), (op, int(ratio.argmax()), ratio.max())


def _close(a, b, tol=1e-13):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return np.max(np.abs(a - b)[ok] / (1 + np.abs(b)[ok]), initial=0.0) <= tol


def test_other_models_agree(runs):
    """the float64 run against what the solver tests' models state for the same functions"""
    x = {op: gc.CASES[op].inputs for op in gc.CASES}
    y = {op: runs[op][1] for op in runs}
    assert _close(y["quat_to_R"], egm.quat_to_R(x["quat_to_R"]).reshape(-1, 9))
    assert _close(y["R_to_quat"], egm.R_to_quat(x["R_to_quat"].reshape(-1, 3, 3)))
    assert _close(y["quat_rot"], egm.quat_rot(x["quat_rot"][:, :4], x["quat_rot"][:, 4:]))
    assert _close(y["quat_mul"], egm.quat_mul(x["quat_mul"][:, :4], x["quat_mul"][:, 4:]))
    assert _close(y["s3_exp"], egm.s3_exp(x["s3_exp"]))
    assert _close(y["s3_mul"], egm.s3_mul(x["s3_mul"][:, :8], x["s3_mul"][:, 8:]))
    assert _close(y["s3_inverse"], egm.s3_inverse(x["s3_inverse"]))
    assert _close(y["s3_map"], egm.s3_map(x["s3_map"][:, :8], x["s3_map"][:, 8:]))
    keep = np.array([not l.startswith("slts") for l in gc.CASES["s3_log"].labels])     # (there W is ill-conditioned, cond <= 1e10: the order of operations shows)
    with np.errstate(all="ignore"):
        assert _close(y["s3_log"][keep], egm.s3_log(x["s3_log"])[keep], 1e-9) and keep.sum() > 100
    for i in range(0, len(x["s3_exp"]), 7):
        assert _close(y["s3_exp"][i], s3m.sim3_exp(x["s3_exp"][i]))
    for i, v in enumerate(x["so3_inv_right_jac"]):
        with np.errstate(all="ignore"):
            assert _close(y["so3_inv_right_jac"][i], pim.inv_right_jac(v).ravel(), 1e-12)
    for m in (0, 1):
        sel = x["cam_project"][:, 4] == m
        rows = x["cam_project"][sel]
        cam = dict(K=rows[0, :4], kb8=rows[0, 5:9] if m else None)
        with np.errstate(all="ignore"):
            for r0 in np.unique(rows[:, :9], axis=0):
                s2 = np.all(rows[:, :9] == r0, 1)
                cam = dict(K=r0[:4], kb8=r0[5:9] if m else None)
                assert _close(y["cam_project"][sel][s2], s3m.project(cam, rows[s2, 9:]))
                assert _close(y["cam_project_jac"][sel][s2], s3m.project_jac(cam, rows[s2, 9:]).reshape(-1, 6))
    # the float models against the oracle's exported camera functions, bit for bit
    for op, t in (("tri_project_pinhole", 0), ("tri_project_kb8", 1)):
        for r in x[op]:
            assert gm.tri_project(t, r[:8], r[8:]).tobytes() == om.camera_project_f(t, f32(r[:8]), f32(r[8:])).tobytes(), (op, r)
    for op, t in (("tri_unproject_pinhole", 0), ("tri_unproject_kb8", 1)):
        for r in x[op]:
            assert gm.tri_unproject(t, r[:8], r[8], r[9]).tobytes() == om.camera_unproject_f(t, f32(r[:8]), f32(r[8]), f32(r[9])).tobytes(), (op, r)


def test_faithful_meets_truth_where_exact(runs):
    """outside the small-angle bands the reference's closed forms ARE the exponential; exp(log S) = S and S S^-1 = 1"""
    c = gc.CASES["so3_exp_imu"]
    for i in c.truth:
        if c.labels[i] == "large":
            t = gm.truth_so3_exp(c.inputs[i])
            assert max(abs(a - b) for a, b in zip(runs["so3_exp_imu"][0][i], t)) < mp.mpf(10) ** -40
    c = gc.CASES["s3_exp"]
    for i in c.truth:
        if c.labels[i].startswith("sltl") or (c.labels[i].startswith("sstl") and c.inputs[i][6] == 0):      # (C = 1 drops O(sigma) below 1e-5)
            S = runs["s3_exp"][0][i]
            n = mp.sqrt(sum(v * v for v in S[:4]))                 # R_to_quat of a rotation: unit up to 1e-50
            assert max(abs(a - b) for a, b in zip(gm.s3_as_matrix(S), gm.truth_s3_exp(c.inputs[i]))) < mp.mpf(10) ** -38 and abs(n - 1) < mp.mpf(10) ** -40
    c = gc.CASES["s3_log"]
    for i in c.truth[::3]:
        if "tl/" in c.labels[i]:
            S = [mp.mpf(float(v)) for v in c.inputs[i]]
            u = runs["s3_log"][0][i]
            back = gm.s3_exp(gm.NMP, u)[0]
            sg = 1 if back[3] * S[3] >= 0 else -1
            nq = mp.sqrt(sum(v * v for v in S[:4]))               # the input quaternion is unit to 1e-16 only
            # (the 1e-16 by which the input misses a rotation, times the 1 / sin theta <= 1e2 of these items' logarithm)
            assert max(abs(sg * a - b / nq) for a, b in zip(back[:4], S[:4])) < 1e-12
            assert max(abs(a - b) for a, b in zip(back[4:], S[4:])) < 1e-12 * (1 + max(abs(v) for v in S[4:]))
    for S in gc.CASES["s3_inverse"].inputs[::25]:
        S = [mp.mpf(float(v)) for v in S]
        one = gm.s3_mul(gm.NMP, S, gm.s3_inverse(gm.NMP, S)[0])[0]
        nq = sum(v * v for v in S[:4])
        assert max(abs(a - b) for a, b in zip(one, [0, 0, 0, nq, 0, 0, 0, 1])) < mp.mpf(10) ** -14


def test_truth_items_at_most_400():
    assert gc.N_TRUTH <= 400, gc.N_TRUTH


def test_float_cases_leave_out_none():
    """no atan2 of the committed float inputs lies within 2^-50 of a float32 rounding boundary; the unproject labels; the Newton steps"""
    for r in gc.CASES["tri_project_kb8"].inputs:
        P = f32(r[8:])
        with np.errstate(all="ignore"):
            rr = np.sqrt(P[0] * P[0] + P[1] * P[1])
        assert gm.atan2f_boundary_distance(rr, P[2]) > 2.0 ** -50 and gm.atan2f_boundary_distance(P[1], P[0]) > 2.0 ** -50, r
    c = gc.CASES["tri_unproject_kb8"]
    steps = Counter()
    for r, l in zip(c.inputs, c.labels):
        info = {}
        gm.tri_unproject(1, r[:8], r[8], r[9], info)
        assert info["branch"] == l, (r, info, l)
        steps[info["steps"]] += 1
    print("tri_unproject Newton steps:", dict(sorted(steps.items())))
    assert steps[0] >= 3 and max(steps) == 10
    lab = Counter(c.labels)
    assert lab["tiny"] >= 3 and lab["newton/clamped"] >= 3
    sv = gc.CASES["tri_svd4_null"]
    beta = Counter()
    for a, l in zip(sv.inputs, sv.labels):                        # the first rotated pair sees both signs of beta = |col 0|^2 - |col 1|^2
        if l == "random":
            At = a.reshape(4, 4)
            beta[bool(At[0] @ At[0] < At[1] @ At[1])] += 1
    assert beta[True] >= 3 and beta[False] >= 3
    assert Counter(sv.labels)["rank2"] >= 4 and Counter(sv.labels)["diagonal"] >= 3
