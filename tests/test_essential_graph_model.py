"""CPU tests of the essential-graph model (tests/essential_graph_model.py): exp o log = id on all four branches, the numeric Jacobian
against the model's own finite difference at a larger step, a drift-free graph stays put, an injected drift is recovered, g2o's
activity rule, and the conditions every committed case has to meet (tests/essential_graph_cases.py): a decisive prefix of at least
three iterations over which float64 and longdouble decide alike, no evaluated branch argument within 1e-6 of its threshold."""
import numpy as np
import pytest
import essential_graph_cases as ec
import essential_graph_model as em
import synth_essential_graph as sg

LD = np.longdouble


@pytest.mark.parametrize("dt,tol", [(np.float64, 1e-13), (LD, 1e-16)])
@pytest.mark.parametrize("om,sig", [(1e-7, 1e-7), (0.5, 1e-7), (1e-7, 0.3), (0.5, 0.3)])
def test_exp_log_roundtrip_on_all_four_branches(dt, tol, om, sig):
    rng = np.random.default_rng(3)
    u = rng.standard_normal((64, 7)).astype(dt)
    u[:, :3] *= om; u[:, 6] *= sig
    mg = em.Margins()
    S = em.s3_exp(u, mg)
    back = em.s3_log(S, mg)
    # the small-angle exponential keeps R = I + Omega + Omega^2 and the logarithm reads omega = 1/2 deltaR(R): exact to O(theta^3)
    assert float(np.abs(back - u).max()) <= tol + (om ** 3 if om < 1e-5 else 0)
    assert mg.smallest() > 1e-6
    small_t, small_s = np.sqrt((u[:, :3] ** 2).sum(1)) < 1e-5, np.abs(u[:, 6]) < 1e-5
    assert small_t.all() == (om < 1e-5) and small_s.all() == (sig < 1e-5)
    # group laws
    T = em.s3_exp(rng.standard_normal((64, 7)).astype(dt) * dt(0.3))
    I = em.s3_mul(S, em.s3_inverse(S))
    assert float(np.abs(I - np.array([0, 0, 0, 1, 0, 0, 0, 1], dt)).max()) < 1e3 * tol
    X = rng.standard_normal((64, 3)).astype(dt)
    assert float(np.abs(em.s3_map(em.s3_mul(S, T), X) - em.s3_map(S, em.s3_map(T, X))).max()) < 1e3 * tol


@pytest.mark.parametrize("fix_scale", [False, True])
def test_numeric_jacobian_against_a_larger_step(fix_scale):
    """The reference's delta = 1e-9 differences in longdouble against the model's own central differences at 1e-4, beyond the exponential's
    small-angle branch (truncation error ~ 1e-8 |J'''|): the same derivative; under fix_scale column 6 is exactly zero; a fixed vertex gets zeros."""
    g = sg.make_graph(4, 10, fix_scale)
    p = em.prepare(g, fix_scale)
    est = g["sim3"].astype(LD)
    Ji, Jj = em.numeric_jacobians(est, p["a_v0"], p["a_v1"], p["a_meas"].astype(LD), p["free"], fix_scale)
    Ki, Kj = em.numeric_jacobians(est, p["a_v0"], p["a_v1"], p["a_meas"].astype(LD), p["free"], fix_scale, delta=1e-4)
    assert float(np.abs(Ji - Ki).max()) < 1e-6 and float(np.abs(Jj - Kj).max()) < 1e-6
    assert float(np.abs(Ji).max()) > 0.5
    if fix_scale:
        assert not Ji[:, :, 6].any() and not Jj[:, :, 6].any()
    else:
        assert np.abs(Ji[:, 6, 6]).min() > 0.5
    fixed_j = ~p["free"][p["a_v1"]]
    assert fixed_j.any() and not Jj[fixed_j].any() and Ji[fixed_j].any()
    # float64 carries the rounding of the 1e-9 step: eps / delta ~ 1e-7 per unit of error
    Fi, _ = em.numeric_jacobians(est.astype(np.float64), p["a_v0"], p["a_v1"], p["a_meas"], p["free"], fix_scale)
    assert 1e-12 < float(np.abs(Fi - Ji).max()) < 1e-4


def test_activity_rule_and_empty_graphs():
    g = sg.make_graph(1, 5, False)
    p = em.prepare(g, False)
    both_fixed = g["fixed"][g["edge_v0"]].astype(bool) & g["fixed"][g["edge_v1"]].astype(bool)
    assert both_fixed.sum() == 1 and np.array_equal(p["active"], ~both_fixed)
    pairs = list(zip(g["edge_v0"].tolist(), g["edge_v1"].tolist()))
    assert len(pairs) > len(set(pairs)), "the generator is to produce several edges between one pair"
    r = em.optimize(sg.empty_graph(), np.zeros((0, 8)), em.default_params())
    assert r["iterations"] == 0 and r["trials"] == 0
    allfixed = dict(g, fixed=np.ones_like(g["fixed"]))
    r = em.optimize(allfixed, g["sim3"], em.default_params())
    assert r["iterations"] == 0 and r["est"].tobytes() == g["sim3"].tobytes()


@pytest.mark.parametrize("fix_scale", [False, True])
def test_drift_free_graph_stays_put(fix_scale):
    g = sg.make_graph(2, 10, fix_scale, consistent=True)
    r = em.optimize(g, g["sim3"], em.default_params(5, fix_scale), LD)
    assert float(r["chi_first"]) < 1e-24                      # the measurements are float64 data
    assert float(np.abs(r["est"] - g["sim3"].astype(LD)).max()) < 1e-12


@pytest.mark.parametrize("fix_scale", [False, True])
def test_injected_drift_is_recovered(fix_scale):
    """Consistent measurements, estimates pushed off by a known Sim3 per free vertex: the optimum is the start of the drift."""
    g = sg.make_graph(2, 10, fix_scale, consistent=True)
    rng = np.random.default_rng(9)
    u = rng.standard_normal((len(g["fixed"]), 7)) * np.array([0.05] * 3 + [0.2] * 3 + [0.0 if fix_scale else 0.05])
    u[g["fixed"].astype(bool)] = 0
    start = em.s3_mul(em.s3_exp(u), g["sim3"])
    r = em.optimize(g, start, em.default_params(20, fix_scale), LD)
    assert float(r["chi_first"]) > 1e-3 and float(r["chi_last"]) < 1e-20 * float(r["chi_first"])
    got, want = ec._canon(r["est"]), ec._canon(g["sim3"])
    assert float(np.abs(got - want).max()) < 1e-9


@pytest.mark.parametrize("name", list(ec.CASES))
def test_case_conditions(name):
    r64, rld, pre = ec.model_runs(name)
    g, prm = ec.make(name)
    assert r64["n"] == 7 * ec.CASES[name][0]
    if name in ec.LARGE:
        m = r64["margins"].as_dict()
        print("[essential-graph] %-9s float64 only: its %d trials %d margins %s" % (name, r64["iterations"], r64["trials"], m))
        assert em.decisive_prefix(r64["trace"]) >= ec.MIN_PREFIX and r64["margins"].smallest() > ec.MIN_MARGIN, m
        return
    print("[essential-graph] %-9s prefix %d of %d iterations, trials %d / %d, margins f64 %s ld %s" % (
        name, pre, rld["iterations"], r64["trials"], rld["trials"], r64["margins"].as_dict(), rld["margins"].as_dict()))
    assert pre >= ec.MIN_PREFIX, pre
    assert em.prefix_totals(r64, pre)[:3] == em.prefix_totals(rld, pre)[:3]
    assert rld["margins"].smallest() > ec.MIN_MARGIN and r64["margins"].smallest() > ec.MIN_MARGIN, (rld["margins"].as_dict(), r64["margins"].as_dict())


def test_cases_cover_both_settings_and_both_sides_of_both_thresholds():
    fs = {ec.CASES[n][1] for n in ec.CASES}
    assert fs == {False, True}
    sides = dict(sigma=set(), d=set())
    for name in ("v2", "v5", "v10", "v10_fix"):
        g, prm = ec.make(name)
        p = em.prepare(g, prm["fix_scale"])
        r64, _, _ = ec.model_runs(name)
        for est in (g["sim3"], r64["trace"][0]["est"]):
            E = em.s3_mul(em.s3_mul(p["a_meas"], np.asarray(est, np.float64)[p["a_v0"]]), em.s3_inverse(np.asarray(est, np.float64)[p["a_v1"]]))
            R = em.quat_to_R(E[:, :4])
            d = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1)
            sides["sigma"] |= set((np.abs(np.log(E[:, 7])) < 1e-5).tolist())
            sides["d"] |= set((d > 1 - 1e-5).tolist())
    assert sides["sigma"] == {False, True} and sides["d"] == {False, True}


def test_point_correction_model():
    g, _ = ec.make("v10")
    r64, _, _ = ec.model_runs("v10")
    Xw, ref, Scw, Swc = sg.points_scene(g, r64["est"], 500)
    out = em.correct_points(Xw, ref, Scw, Swc)
    assert out.dtype == np.float32 and np.array_equal(out[ref < 0], Xw[ref < 0]) and (ref < 0).any()
    # a point keeps its place in its reference keyframe's camera up to the scale change: Scw_after.map(out) = Scw_before.map(Xw)
    ok = ref >= 0
    cam0 = em.s3_map(Scw[ref[ok]], Xw[ok].astype(np.float64))
    cam1 = em.s3_map(np.asarray(r64["est"], np.float64)[ref[ok]], out[ok].astype(np.float64))
    assert np.abs(cam1 - cam0).max() < 1e-4


@pytest.mark.parametrize("name", [n for n in ec.CASES if n not in ec.LARGE])
def test_recorded_slack_is_what_the_models_show(name):
    """The records the GPU test uses against the function that measured them: chi2 at the end of the prefix to 1e-9, the slack (a
    difference of nearly equal numbers: it moves with the libm's last bits) within a factor of 4."""
    ref, slack = ec.past_prefix_slack(name)
    rec_ref, rec_slack = ec.PAST_PREFIX_SLACK[name]
    assert abs(ref - rec_ref) <= 1e-9 * rec_ref and rec_slack / 4 <= slack <= 4 * rec_slack, (ref, slack, rec_ref, rec_slack)
