"""CPU tests of the FullInertialBA model (tests/full_iba_model.py): its Jacobians against central differences (shared mode: the border
columns and the two prior edges too), the whole schedule in per-keyframe mode against the LocalInertialBA oracle on the golden
windows, float64 against extended precision over the decisive prefix of every committed case, g2o's activity rule."""
import numpy as np
import pytest
import full_iba_cases as fc
import full_iba_model as fm
import synth_full_iba as sf
import synth_iba

LD = np.longdouble


def _stacked_jacobians(P, S):
    """Dense d(error)/d(x) of every inertial edge [M,9,n] and every visual edge w.r.t. x [E,3,n] and its point [E,3,3] from the model's
    analytic blocks, placed by the model's own column maps."""
    _, Jx, Jp = fm.visual(P, S, True)
    _, J = fm.inertial(P, S, True)
    Ji = np.zeros((P.M, 9, P.n), P.dtype)
    for m in range(P.M):
        cols = fm.inertial_columns(P, m)
        keep = cols >= 0
        Ji[m][:, cols[keep]] = J[m][:, keep]
    Jv = np.zeros((P.E, 3, P.n), P.dtype)
    for e in range(P.E):
        o = P.xoff[P.ek[e]]
        if o >= 0:
            Jv[e][:, o:o + 6] = Jp[e]
    return Ji, Jv, Jx


@pytest.mark.parametrize("kw", [dict(K=3, bias0_sigma=1e-3), dict(K=4, no_imu=(1,), fixed=(3,), bias0_sigma=1e-3), dict(K=3, fisheye_rig=True, bias0_sigma=1e-3)])
def test_shared_mode_jacobians_match_central_differences(kw):
    win, sb = sf.make_map(5, state_noise=0.2, **kw)
    prm = fm.default_params(1, True, 1.0, 1e5)
    P = fm.Problem(win, prm, LD, smooth=True)
    S = P.initial_state(win, sb)
    Ji, Jv, Jx = _stacked_jacobians(P, S)
    assert P.shared and P.n == P.os + 6
    h = LD(1e-6)
    zl = np.zeros((P.L, 3), LD)
    for q in range(P.n):
        x = np.zeros(P.n, LD); x[q] = h
        ip, _ = fm.inertial(P, fm.apply_step(P, S, x, zl)); im, _ = fm.inertial(P, fm.apply_step(P, S, -x, zl))
        vp, _, _ = fm.visual(P, fm.apply_step(P, S, x, zl)); vm, _, _ = fm.visual(P, fm.apply_step(P, S, -x, zl))
        di, dv = (ip - im) / (2 * h), (vp - vm) / (2 * h)
        # the reference's analytic Jacobian drops second-order terms of the rotation residual (exact at er = 0): ~1e-2 there
        assert np.allclose(Ji[:, 3:, q], di[:, 3:], atol=2e-5), (q, float(np.abs(Ji[:, 3:, q] - di[:, 3:]).max()))
        assert np.allclose(Ji[:, :3, q], di[:, :3], atol=2e-2), (q, float(np.abs(Ji[:, :3, q] - di[:, :3]).max()))
        assert np.allclose(Jv[:, :, q], dv, rtol=1e-5, atol=1e-4), (q, float(np.abs(Jv[:, :, q] - dv).max()))
    # the border: every inertial edge has its bias columns in the shared block, wherever its keyframes are (fixed ones too)
    assert P.M and all(np.abs(Ji[m][:, P.os:]).max() > 0 for m in range(P.M))
    for l in np.flatnonzero(P.active_pt)[:12]:
        for c in range(3):
            d = zl.copy(); d[l, c] = h
            z = np.zeros(P.n, LD)
            vp, _, _ = fm.visual(P, fm.apply_step(P, S, z, d)); vm, _, _ = fm.visual(P, fm.apply_step(P, S, z, -d))
            sel = P.el == l
            assert np.allclose(Jx[sel][:, :, c], ((vp - vm) / (2 * h))[sel], rtol=1e-5, atol=1e-4)


def test_prior_edges_as_the_reference_writes_them():
    """EdgePriorGyro / EdgePriorAcc: error 0 - b (its derivative is -I), Jacobian WRITTEN as +I (G2oTypes.cc:971-983): H gets prior I and
    b = -J^T Omega e = +prior b.  chi2 gets prior |b|^2."""
    win, sb = sf.make_map(5, 3, bias0_sigma=1e-3)
    with_p, without = fm.default_params(1, True, 1.0, 1e5), fm.default_params(1, True, 0.0, 0.0)
    P1, P0 = fm.Problem(win, with_p, LD), fm.Problem(win, without, LD)
    S = P1.initial_state(win, sb)
    e1, e0 = fm.evaluate(P1, S), fm.evaluate(P0, S)
    pr = np.array([1.0] * 3 + [float(np.float32(1e5))] * 3, LD)
    assert abs(e1["chi"] - e0["chi"] - np.sum(pr * S["sb"] ** 2)) <= 1e-17 * abs(e1["chi"])
    b1, b0 = fm.build(P1, S, e1), fm.build(P0, S, e0)
    dH, db = b1["H"] - b0["H"], b1["b"] - b0["b"]
    o = P1.os
    assert np.abs(dH[o:, o:] - np.diag(pr)).max() <= 1e-12 * pr.max() and np.abs(dH[:o]).max() == 0 and np.abs(dH[:, :o]).max() == 0
    assert np.abs(db[o:] - pr * S["sb"]).max() <= 1e-12 * np.abs(pr * S["sb"]).max() and np.abs(db[:o]).max() == 0


def test_per_keyframe_mode_reproduces_the_local_inertial_ba_oracle():
    """The model in per-keyframe mode with LocalInertialBA's parameters, up to the end of optimize(), against oracle_iba_bind.solve on the
    golden windows: as closely as test_oracle_iba.py's own numpy model (same iterations and trials, err to 1e-9, err_end to 1e-5,
    keyframe states to 1e-5, points to 1e-4)."""
    import oracle_iba_bind as ib
    for win, _ in synth_iba.load_golden_windows():
        kf_o, pts_o, _, st = ib.solve(win)
        r = fm.optimize(win, fm.local_params(), np.float64)
        assert (r["iterations"], r["trials"]) == (st.iterations_run, st.lm_trials), (r["iterations"], r["trials"], st.iterations_run, st.lm_trials)
        assert abs(r["chi_first"] - st.err) <= 1e-9 * st.err
        assert abs(r["chi_eval"] - st.err_end) <= 1e-5 * st.err_end, (r["chi_eval"], st.err_end)
        if not st.failed:
            assert np.max(np.abs(r["kf"] - kf_o.reshape(-1, 21))) <= 1e-5 and np.max(np.abs(r["X"] - pts_o.reshape(-1, 3))) <= 1e-4


@pytest.mark.parametrize("name", list(fc.CASES))
def test_float64_and_extended_precision_decide_alike(name):
    """Every committed case: a decisive prefix of at least three iterations, the same iterations / trial decisions over it in both
    precisions, and a float64 end state within MODEL_RMSE of the extended one (full_iba_cases.py says why the seeds are chosen so)."""
    r64, rld, pre = fc.model_runs(name)
    assert pre >= fc.MIN_PREFIX, (name, pre)
    assert fm.prefix_totals(r64, pre)[:3] == fm.prefix_totals(rld, pre)[:3], (name, fm.prefix_totals(r64, pre)[:3], fm.prefix_totals(rld, pre)[:3])
    rmse = fc.gauge_rmse(r64["kf"], r64["X"], rld)
    print("[full-iba model] %-10s n %3d prefix %d its %d trials %d reason %d rmse(float64, extended) %.3g" %
          (name, rld["n"], pre, rld["iterations"], rld["trials"], rld["reason"], rmse))
    assert rmse <= fc.MODEL_RMSE, (name, rmse)


def test_activity_rule_on_an_inertial_edge_between_two_fixed_keyframes():
    """Keyframes 5 and 6 fixed, both with IMU states, an inertial edge between them.  Shared biases are never fixed, so the edge is active:
    it is in chi2 and in the shared block.  With biases per keyframe all six of its vertices are fixed: it is in nothing."""
    win, sb = sf.make_map(1, 7, fixed=(5, 6), bias0_sigma=1e-3)
    a = win.arrays
    ff = [m for m in range(win.n_inertial) if a["kf_fixed"][a["in_kf1"][m]] and a["kf_fixed"][a["in_kf2"][m]]]
    assert len(ff) == 1
    d = dict(win.d)
    keep = np.ones(win.n_inertial, bool); keep[ff] = False
    for k in ("in_kf1", "in_kf2", "in_robust", "in_preint", "in_info", "in_info_g", "in_info_a"):
        d[k] = np.asarray(d[k])[keep]
    cut = synth_iba.Window(d)
    for shared in (True, False):
        prm = fm.default_params(1, shared, 1.0, 1e5)
        P, Pc = fm.Problem(win, prm, np.float64), fm.Problem(cut, prm, np.float64)
        S, Sc = P.initial_state(win, sb), Pc.initial_state(cut, sb)
        e, ec = fm.evaluate(P, S), fm.evaluate(Pc, Sc)
        B, Bc = fm.build(P, S, e), fm.build(Pc, Sc, ec)
        if shared:
            assert P.M == Pc.M + 1
            m = int(np.flatnonzero(P.fixed[P.k1] & P.fixed[P.k2])[0])
            rho = float(fm._rho(e["chi_i"][m], P.delta_i, P.dsqr_i))
            assert rho > 0 and abs((e["chi"] - ec["chi"]) - rho) <= 1e-9 * e["chi"]
            dH = B["H"] - Bc["H"]
            assert np.abs(dH[P.os:, P.os:]).max() > 0 and np.abs(dH[:P.os]).max() == 0 and np.abs(dH[:, :P.os]).max() == 0
        else:
            assert P.M == Pc.M and e["chi"] == ec["chi"] and np.array_equal(B["H"], Bc["H"]) and np.array_equal(B["b"], Bc["b"])


def test_point_seen_by_fixed_keyframes_only_is_constant():
    win, sb, prm = fc.make("s_fixed")
    l = win.d["fixed_only_point"]
    r64, _, _ = fc.model_runs("s_fixed")
    assert not r64["active_pt"][l] and np.array_equal(r64["X"][l], win.pts0[l])
    d = dict(win.d)
    keep = np.asarray(d["edge_point"]) != l
    for k in ("edge_kf", "edge_point", "edge_stereo", "edge_inv_sigma2", "edge_close", "edge_obs"):
        d[k] = np.asarray(d[k])[keep]
    r = fm.optimize(synth_iba.Window(d), prm, np.float64, sb)
    assert r["chi_first"] == r64["chi_first"] and r["kf"].tobytes() == r64["kf"].tobytes()      # its edges add nothing to chi2
