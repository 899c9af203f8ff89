"""GPU tests of the 4-DoF essential-graph optimisation (orbhip_optimize_essential_graph4dof_host; csrc/pose_graph4dof_kernels.hip) against
the extended-precision model (tests/essential_graph4dof_model.py) on the committed cases (tests/essential_graph4dof_cases.py).

Per case, over the decisive prefix: the same iterations, accepted / rejected trials and trace lambdas as the extended-precision model;
every solved quantity under the project's K rule (ba_step_model.within_bound, K = 128: e_device <= K (e_float64_model + 2^-52
max|value|), both errors against the extended-precision model).  Past the prefix decisions are rounding noise: the run ends as a model
run does and its final chi2 stays within essential_graph4dof_cases.past_prefix_slack of the chi2 at the end of the prefix.  Then: fixed
vertices keep their bytes, reruns are byte-identical, 120 / 121 free keyframes take the two factorisations, both factorisations agree
on one graph, ragged batches, the empty / all-fixed / edgeless graphs, the refused ones, the largest admitted graph.
Measured on an MI355X, e_device / (e_float64 + floor), largest per group over all cases: R 3.5, t 5.4, chi2 15 (the 2-vertex case: 7e-20
against 4.6e-21 on a chi2 of 2.9e-7), lambda 7.7."""
import os
import numpy as np
import pytest
import essential_graph4dof_cases as ec
import essential_graph4dof_model as em
import synth_essential_graph4dof as sg

pytestmark = pytest.mark.gpu
E_BADARG, E_CAPACITY = -1, -4
LD = np.longdouble


@pytest.fixture(scope="module")
def hip():
    import orbhip
    ctx = orbhip.Context(0)
    yield orbhip, ctx
    ctx.close()


def _params(orbhip, prm, iterations=None):
    return orbhip.pose_graph4dof_default_params(prm["iterations"] if iterations is None else iterations, prm["info_diag"], prm["lambda_init"])


def _solve(hip, name, iterations=None):
    orbhip, ctx = hip
    g, prm = ec.make(name)
    est, st, tr = orbhip.optimize_essential_graph4dof(ctx, [g], [g["state"]], _params(orbhip, prm, iterations))
    return est[0], st[0], tr[0]


def _report(tag, name, rep):
    print("[essential-graph4dof] %-7s %-10s %s" % (tag, name, " ".join("%s %.2g (f64 %.2g, ratio %.2g)" % (g, v[0], v[2], v[3]) for g, v in rep.items())))


@pytest.mark.parametrize("name", list(ec.CASES))
def test_decisions_and_state_over_the_decisive_prefix(hip, name):
    _, rld_full, pre = ec.model_runs(name)
    assert pre >= ec.min_prefix(name)
    r64, rld, _ = (ec.model_runs(name) if pre == rld_full["iterations"] else ec.model_runs(name, pre))
    est, st, tr = _solve(hip, name, iterations=pre)
    its, trials, flags, lam = em.prefix_totals(rld_full, pre)
    assert (st["iterations"], st["trials"], st["n_unknowns"]) == (its, trials, rld["n"]), (st, its, trials)
    assert [bool(x) for x in tr[:, 3]] == flags
    assert abs(st["chi2_initial"] - float(rld["chi_first"])) <= 1e-9 * float(rld["chi_first"])
    dev = ec.group_values(est, st["chi2_final"], st["lam"], rld["free"])
    ok, rep = ec.k_rule(dev, r64, rld)
    _report("prefix", name, rep)
    assert ok, rep
    # the trace's rows: the lambda every trial was solved with (the first one is tau * max |H(j, j)| or lambda_init), K rule
    want = [t for r in rld_full["trace"][:pre] for t in r["trials"]]
    want64 = [t for r in r64["trace"][:pre] for t in r["trials"]]
    for row, (chi, rho, lam_used, good), t64 in zip(tr, want, want64):
        assert ec.within_bound(abs(row[2] - float(lam_used)), abs(float(t64[2]) - float(lam_used)), 2.0 ** -52 * float(lam_used), ec.K_RULE), (row, lam_used, t64[2])
    # fixed vertices keep their bytes; a free vertex keeps its calibration
    g, _ = ec.make(name)
    fx = g["fixed"].astype(bool)
    assert est[fx].tobytes() == g["state"][fx].tobytes() and est[:, 24:].tobytes() == g["state"][:, 24:].tobytes()
    assert np.abs(est[~fx, :24] - g["state"][~fx, :24]).max() > 1e-6


@pytest.mark.parametrize("name", list(ec.CASES))
def test_whole_run_ends_like_the_model_and_reruns_identically(hip, name):
    r64, rld, pre = ec.model_runs(name)
    est, st, tr = _solve(hip, name)
    assert st["end_reason"] in (r64["reason"], rld["reason"]), (st, r64["reason"], rld["reason"])
    assert st["iterations"] >= pre
    ref, slack = ec.past_prefix_slack(name)
    print("[essential-graph4dof] whole   %-10s chi2 %.17g, end of prefix %.17g, slack %.3g, its %d trials %d reason %d" % (
        name, st["chi2_final"], ref, slack, st["iterations"], st["trials"], st["end_reason"]))
    assert st["chi2_final"] <= ref + slack
    est2, st2, tr2 = _solve(hip, name)
    assert est2.tobytes() == est.tobytes() and st2 == st and tr2.tobytes() == tr.tobytes()


def test_120_and_121_free_keyframes_take_the_two_factorisations(hip):
    last_path = hip[0].lib.orbhip_debug_pose_graph4dof_last_path
    _, st, _ = _solve(hip, "v120", iterations=1)
    p120 = last_path()
    _, st1, _ = _solve(hip, "v121", iterations=1)
    assert (st["n_unknowns"], p120, st1["n_unknowns"], last_path()) == (480, 0, 484, 1)


def test_both_factorisations_give_the_same_trace(hip):
    """v120 (480 unknowns) in one workgroup and, with ORBHIP_PG_FORCE_BIG=1, over many: the same decisions over the decisive prefix,
    chi2 per trial to 1e-9, and both under the K rule.  Not bit for bit: the two share the elimination order and the per-entry formula,
    but the single-workgroup path runs ba_ldlt.h's DPP / MFMA forms where the many-workgroup one runs plain fused multiply-adds."""
    last_path = hip[0].lib.orbhip_debug_pose_graph4dof_last_path
    r64, rld, pre = ec.model_runs("v120", ec.model_runs("v120")[2])
    est, st, tr = _solve(hip, "v120", iterations=pre)
    path = last_path()
    os.environ["ORBHIP_PG_FORCE_BIG"] = "1"                  # read at every call
    try:
        est_b, st_b, tr_b = _solve(hip, "v120", iterations=pre)
        path_b = last_path()
    finally:
        del os.environ["ORBHIP_PG_FORCE_BIG"]
    assert path == 0 and path_b == 1
    assert np.array_equal(tr_b[:, 3], tr[:, 3])
    np.testing.assert_allclose(tr_b[:, 0], tr[:, 0], rtol=1e-9)
    for e, s_ in ((est, st), (est_b, st_b)):
        ok, rep = ec.k_rule(ec.group_values(e, s_["chi2_final"], s_["lam"], rld["free"]), r64, rld)
        _report("paths", "v120", rep)
        assert ok, rep


def test_ragged_batch_equals_single_calls(hip):
    orbhip, ctx = hip
    gs = [ec.make(n)[0] for n in ec.RAGGED]
    gs.insert(1, sg.empty_graph())
    p = orbhip.pose_graph4dof_default_params(3)
    est, st, tr = orbhip.optimize_essential_graph4dof(ctx, gs, [g["state"] for g in gs], p)
    assert st[1]["iterations"] == 0 and st[1]["trials"] == 0 and st[1]["n_unknowns"] == 0 and est[1].size == 0
    for i in (0, 2, 3):
        e1, s1, t1 = orbhip.optimize_essential_graph4dof(ctx, [gs[i]], [gs[i]["state"]], p)
        assert s1[0] == st[i] and st[i]["iterations"] >= 1
        assert e1[0].tobytes() == est[i].tobytes() and t1[0].tobytes() == tr[i].tobytes()


def test_all_fixed_and_edgeless_graphs_answer_ok_with_zero_iterations(hip):
    orbhip, ctx = hip
    g, _ = ec.make("v10")
    allfixed = dict(g, fixed=np.ones_like(g["fixed"]))
    est, st, _ = orbhip.optimize_essential_graph4dof(ctx, [allfixed], [g["state"]])
    assert st[0]["iterations"] == 0 and st[0]["n_free"] == 0 and est[0].tobytes() == g["state"].tobytes()
    noedges = dict(g, edge_v0=g["edge_v0"][:0], edge_v1=g["edge_v1"][:0], edge_meas=g["edge_meas"][:0])
    est, st, _ = orbhip.optimize_essential_graph4dof(ctx, [noedges], [g["state"]])
    assert st[0]["iterations"] == 0 and st[0]["n_free"] == 10 and est[0].tobytes() == g["state"].tobytes()
    # only the edge between the two fixed vertices: not active
    k = np.flatnonzero(g["fixed"][g["edge_v0"]].astype(bool) & g["fixed"][g["edge_v1"]].astype(bool))
    one = dict(g, edge_v0=g["edge_v0"][k], edge_v1=g["edge_v1"][k], edge_meas=g["edge_meas"][k])
    est, st, _ = orbhip.optimize_essential_graph4dof(ctx, [one], [g["state"]])
    assert len(k) == 1 and st[0]["iterations"] == 0 and est[0].tobytes() == g["state"].tobytes()
    # and it adds nothing to chi2: with and without it the same run
    keep = np.ones(len(g["edge_v0"]), bool); keep[k] = False
    without = dict(g, edge_v0=g["edge_v0"][keep], edge_v1=g["edge_v1"][keep], edge_meas=g["edge_meas"][keep])
    a = orbhip.optimize_essential_graph4dof(ctx, [g], [g["state"]])
    b = orbhip.optimize_essential_graph4dof(ctx, [without], [g["state"]])
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[1] == b[1]


def test_a_user_lambda_overrides_the_computed_start(hip):
    orbhip, ctx = hip
    g, _ = ec.make("v10")
    _, st, tr = orbhip.optimize_essential_graph4dof(ctx, [g], [g["state"]], orbhip.pose_graph4dof_default_params(1, lambda_init=0.25))
    _, st0, tr0 = orbhip.optimize_essential_graph4dof(ctx, [g], [g["state"]], orbhip.pose_graph4dof_default_params(1))
    assert tr[0][0, 2] == 0.25 and 0 < tr0[0][0, 2] < 1e-40


def test_refusals_leave_the_state_untouched(hip):
    orbhip, ctx = hip
    g, _ = ec.make("v10")
    bad = dict(g, edge_meas=g["edge_meas"].copy())
    bad["edge_meas"][3, 10] = np.nan
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph4dof(ctx, [g, bad], [g["state"], g["state"]])
    assert ei.value.code == E_BADARG and "edge_meas[3][10]" in str(ei.value) and "graph 1" in str(ei.value)
    big = sg.make_graph(1, 1025, consistent=True, extra_fixed=False)
    before = big["state"].copy()
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph4dof(ctx, [big], [big["state"]])
    assert ei.value.code == E_CAPACITY and "4100 unknowns" in str(ei.value) and "1025 free keyframes" in str(ei.value)
    assert big["state"].tobytes() == before.tobytes()


def test_largest_graph_is_accepted(hip):
    """1024 free keyframes (4096 unknowns): one iteration on a consistent graph whose free vertices are pushed off in yaw and position.
    The residual is close to linear, so the Gauss-Newton step brings chi2 down by six decades, which a wrong entry anywhere in the
    many-workgroup factorisation would spoil."""
    orbhip, ctx = hip
    g = sg.make_graph(1, 1024, consistent=True, extra_fixed=False)
    rng = np.random.default_rng(2)
    S = em.load(g["state"], np.float64)
    fl = np.flatnonzero(g["fixed"] == 0)
    u = rng.standard_normal((len(fl), 4)) * 1e-3
    start = em.to_state36(em.oplus(S, fl, u), g["state"], g["fixed"] == 0)
    est, st, _ = orbhip.optimize_essential_graph4dof(ctx, [g], [start], orbhip.pose_graph4dof_default_params(1))
    assert st[0]["n_unknowns"] == 4096 and st[0]["iterations"] == 1 and st[0]["trials"] == 1
    assert hip[0].lib.orbhip_debug_pose_graph4dof_last_path() == 1
    print("[essential-graph4dof] largest chi2 %.3g -> %.3g" % (st[0]["chi2_initial"], st[0]["chi2_final"]))
    assert st[0]["chi2_final"] < 1e-6 * st[0]["chi2_initial"]
