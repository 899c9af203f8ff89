"""GPU tests of the essential-graph optimisation (orbhip_optimize_essential_graph_host, orbhip_pose_graph_correct_points_device;
csrc/pose_graph_kernels.hip) against the extended-precision model (tests/essential_graph_model.py) on the committed cases
(tests/essential_graph_cases.py).

Per case, over the decisive prefix: the same iterations, accepted / rejected trials and lambda as the extended-precision model; every
solved quantity under the project's K rule (ba_step_model.within_bound, K = 128: e_device <= K (e_float64_model + 2^-52 max|value|),
both errors against the extended-precision model).  Past the prefix decisions are rounding noise: the run ends as a model run does and
its final chi2 stays within essential_graph_cases.past_prefix_slack of the chi2 at the end of the prefix.  The 150-vertex case is held
to the float64 model, estimates and chi2, by K x the largest float64-vs-longdouble distance of the smaller cases of its scale setting.  Then: both factorisations on the
68-vertex cases, the largest graph with both scale settings, ragged batches, reruns, the empty / all-fixed / refused graphs, the point kernel."""
import os
import numpy as np
import pytest
import essential_graph_cases as ec
import essential_graph_model as em
import synth_essential_graph as sg

pytestmark = pytest.mark.gpu
E_BADARG, E_CAPACITY = -1, -4
LD = np.longdouble
SMALL = [n for n in ec.CASES if n not in ec.LARGE]


@pytest.fixture(scope="module")
def hip():
    import orbhip
    ctx = orbhip.Context(0)
    yield orbhip, ctx
    ctx.close()


def _solve(hip, name, iterations=None):
    orbhip, ctx = hip
    g, prm = ec.make(name)
    p = orbhip.pose_graph_default_params(prm["iterations"] if iterations is None else iterations, prm["fix_scale"])
    est, st, tr = orbhip.optimize_essential_graph(ctx, [g], [g["sim3"]], p)
    return est[0], st[0], tr[0]


def _report(tag, name, rep):
    print("[essential-graph] %-7s %-9s %s" % (tag, name, " ".join("%s %.2g (f64 %.2g, ratio %.2g)" % (g, v[0], v[2], v[3]) for g, v in rep.items())))


@pytest.mark.parametrize("name", SMALL)
def test_decisions_and_state_over_the_decisive_prefix(hip, name):
    _, rld_full, pre = ec.model_runs(name)
    assert pre >= ec.MIN_PREFIX
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
    # the trace's rows: the lambda every trial was solved with, under the K rule against the two models' (the good-step factor
    # 1 - (2 rho - 1)^3 carries rho's error wherever it is not clamped to 1/3)
    want = [t for r in rld_full["trace"][:pre] for t in r["trials"]]
    want64 = [t for r in r64["trace"][:pre] for t in r["trials"]]
    for row, (chi, rho, lam_used, good), t64 in zip(tr, want, want64):
        assert ec.within_bound(abs(row[2] - float(lam_used)), abs(float(t64[2]) - float(lam_used)), 2.0 ** -52 * float(lam_used), ec.K_RULE), (row, lam_used, t64[2])
    # fixed vertices keep their bytes
    g, _ = ec.make(name)
    fx = g["fixed"].astype(bool)
    assert est[fx].tobytes() == g["sim3"][fx].tobytes()


@pytest.mark.parametrize("name", SMALL)
def test_whole_run_ends_like_the_model_and_reruns_identically(hip, name):
    """The free-scale cases v68, v69 and v75 run three iterations, all of them decisive: they have NO part past the prefix, and for
    them this test repeats the chi2 bound the K-rule test holds already (plus the end reason and the rerun)."""
    r64, rld, pre = ec.model_runs(name)
    est, st, tr = _solve(hip, name)
    assert st["end_reason"] in (r64["reason"], rld["reason"]), (st, r64["reason"], rld["reason"])
    assert st["iterations"] >= pre
    ref, slack = ec.PAST_PREFIX_SLACK[name]
    print("[essential-graph] whole   %-9s chi2 %.17g, end of prefix %.17g, slack %.3g, its %d trials %d reason %d" % (
        name, st["chi2_final"], ref, slack, st["iterations"], st["trials"], st["end_reason"]))
    assert st["chi2_final"] <= ref + slack
    est2, st2, tr2 = _solve(hip, name)
    assert est2.tobytes() == est.tobytes() and st2 == st and tr2.tobytes() == tr.tobytes()


@pytest.mark.parametrize("name", ec.LARGE)
def test_large_case_against_the_float64_model(hip, name):
    """Estimates and chi2 of the 150-vertex case against the float64 model: K x the largest float64-vs-longdouble distance over the
    smaller cases of the SAME scale setting (fixed scale: t 3.8e-7 m, so about 5e-5 m here), plus the float64 storage floor."""
    r64, _, _ = ec.model_runs(name)
    est, st, tr = _solve(hip, name)
    flags = [a for r in r64["trace"] for a in r["accepted"]]
    pre = em.decisive_prefix(r64["trace"])
    k = em.prefix_totals(r64, pre)[1]
    assert st["n_unknowns"] == r64["n"] and st["iterations"] >= pre and [bool(x) for x in tr[:k, 3]] == flags[:k]
    ref = ec.run_groups(r64)
    d = ec.group_errors(ec.group_values(est, st["chi2_final"], st["lam"], r64["free"]), ref)
    d["chi_rel"] = d["chi"] / abs(float(r64["chi_last"]))
    bound = ec.largest_model_distance(ec.CASES[name][1])
    floor = dict(q=2.0 ** -52, t=2.0 ** -52 * float(np.abs(ref["t"]).max()), s=2.0 ** -52, chi_rel=2.0 ** -52)
    print("[essential-graph] large   %-9s %s" % (name, " ".join("%s %.2g (f64-vs-ld %.2g, ratio %.2g)" % (g, d[g], bound[g], d[g] / (bound[g] + floor[g])) for g in bound)))
    for g in bound:
        assert ec.within_bound(d[g], bound[g], floor[g], ec.K_RULE), (g, d[g], bound[g])


@pytest.mark.parametrize("name", ["v68_fix", "v68"])
def test_both_factorisations_give_the_same_trace(hip, name):
    """The 68-vertex cases (476 unknowns) in one workgroup and, with ORBHIP_PG_FORCE_BIG=1, over many: the same decisions over the
    decisive prefix, chi2 and lambda per trial to 1e-9 (fixed scale) / to the K rule's bound of the case (free scale), and estimates
    to 1e-9 when the whole runs decide alike.  Not bit for bit, and only over the prefix: the two paths share the elimination order
    and the per-entry formula, but the single-workgroup path runs ba_ldlt.h's DPP-broadcast diagonal block, four-lane rows and MFMA
    trailing update where the many-workgroup one runs plain fused multiply-adds, so they round differently and past the prefix
    decide differently."""
    last_path = hip[0].lib.orbhip_debug_pose_graph_last_path
    est, st, tr = _solve(hip, name)
    path = last_path()
    os.environ["ORBHIP_PG_FORCE_BIG"] = "1"                  # read at every call
    try:
        est_b, st_b, tr_b = _solve(hip, name)
        path_b = last_path()
    finally:
        del os.environ["ORBHIP_PG_FORCE_BIG"]
    _, rld, pre = ec.model_runs(name)
    k = em.prefix_totals(rld, pre)[1]
    assert st_b["iterations"] >= pre and np.array_equal(tr_b[:k, 3], tr[:k, 3])
    assert path == 0 and path_b == 1, "476 unknowns go to one workgroup unless the switch is set"
    if name == "v68_fix":
        np.testing.assert_allclose(tr_b[:k, [0, 2]], tr[:k, [0, 2]], rtol=1e-9)
        if (st_b["iterations"], st_b["trials"]) == (st["iterations"], st["trials"]):
            assert np.abs(est_b - est).max() <= 1e-9
    else:                                                    # free scale: conditioning makes the float64 model itself miss 1e-9; both paths under the K rule
        r64, rld, _ = ec.model_runs(name)
        for e, s_ in ((est, st), (est_b, st_b)):
            ok, rep = ec.k_rule(ec.group_values(e, s_["chi2_final"], s_["lam"], rld["free"]), r64, rld)
            _report("paths", name, rep)
            assert ok, rep


def test_ragged_batch_equals_single_calls(hip):
    orbhip, ctx = hip
    gs = [ec.make(n)[0] for n in ec.RAGGED]
    gs.insert(1, sg.empty_graph())
    p = orbhip.pose_graph_default_params(4, False)
    est, st, tr = orbhip.optimize_essential_graph(ctx, gs, [g["sim3"] for g in gs], p)
    assert st[1]["iterations"] == 0 and st[1]["trials"] == 0 and st[1]["n_unknowns"] == 0 and est[1].size == 0
    for i in (0, 2, 3):
        e1, s1, t1 = orbhip.optimize_essential_graph(ctx, [gs[i]], [gs[i]["sim3"]], p)
        assert s1[0] == st[i] and st[i]["iterations"] >= 1
        assert e1[0].tobytes() == est[i].tobytes() and t1[0].tobytes() == tr[i].tobytes()


def test_all_fixed_and_edgeless_graphs_answer_ok_with_zero_iterations(hip):
    orbhip, ctx = hip
    g, _ = ec.make("v5")
    allfixed = dict(g, fixed=np.ones_like(g["fixed"]))
    est, st, _ = orbhip.optimize_essential_graph(ctx, [allfixed], [g["sim3"]])
    assert st[0]["iterations"] == 0 and st[0]["n_free"] == 0 and est[0].tobytes() == g["sim3"].tobytes()
    noedges = dict(g, edge_v0=g["edge_v0"][:0], edge_v1=g["edge_v1"][:0], edge_meas=g["edge_meas"][:0])
    est, st, _ = orbhip.optimize_essential_graph(ctx, [noedges], [g["sim3"]])
    assert st[0]["iterations"] == 0 and st[0]["n_free"] == 5 and est[0].tobytes() == g["sim3"].tobytes()
    # only the edge between the two fixed vertices: not active
    k = np.flatnonzero(g["fixed"][g["edge_v0"]].astype(bool) & g["fixed"][g["edge_v1"]].astype(bool))
    one = dict(g, edge_v0=g["edge_v0"][k], edge_v1=g["edge_v1"][k], edge_meas=g["edge_meas"][k])
    est, st, _ = orbhip.optimize_essential_graph(ctx, [one], [g["sim3"]])
    assert len(k) == 1 and st[0]["iterations"] == 0 and est[0].tobytes() == g["sim3"].tobytes()


def test_refusals_leave_the_estimates_untouched(hip):
    orbhip, ctx = hip
    g, _ = ec.make("v5")
    bad = dict(g, edge_meas=g["edge_meas"].copy())
    bad["edge_meas"][3, 5] = np.nan
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph(ctx, [g, bad], [g["sim3"], g["sim3"]])
    assert ei.value.code == E_BADARG and "edge_meas[3][5]" in str(ei.value) and "graph 1" in str(ei.value)
    big = sg.make_graph(1, 586, True, consistent=True)
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.optimize_essential_graph(ctx, [big], [big["sim3"]])
    assert ei.value.code == E_CAPACITY and "4102 unknowns" in str(ei.value) and "586 free keyframes" in str(ei.value)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_largest_graph_is_accepted(hip, fix_scale):
    """585 free vertices (4095 unknowns), both scale settings: one iteration on a consistent graph pushed off by a small drift.  With
    fixed scale the problem is nearly linear and the Gauss-Newton step brings chi2 down by six decades, which a wrong entry anywhere
    in the many-workgroup factorisation would spoil.  With free scale the 1e-3 scale noise times the metres of translation makes the
    step nonlinear (the float64 model's one trial goes from 0.0205 to 0.0046): there the test asks for the capacity, one accepted
    trial and moved scales only; accuracy of that path with free scale is what the 69- and 75-vertex cases hold."""
    orbhip, ctx = hip
    g = sg.make_graph(1, 585, fix_scale, consistent=True)
    rng = np.random.default_rng(2)
    u = rng.standard_normal((len(g["fixed"]), 7)) * 1e-3
    if fix_scale:
        u[:, 6] = 0
    u[g["fixed"].astype(bool)] = 0
    est, st, _ = orbhip.optimize_essential_graph(ctx, [g], [em.s3_mul(em.s3_exp(u), g["sim3"])], orbhip.pose_graph_default_params(1, fix_scale))
    assert st[0]["n_unknowns"] == 4095 and st[0]["iterations"] == 1
    if fix_scale:
        assert st[0]["chi2_final"] < 1e-6 * st[0]["chi2_initial"]
    else:
        assert st[0]["trials"] == 1 and st[0]["chi2_final"] < st[0]["chi2_initial"] and np.abs(est[0][:, 7] - 1).max() > 0


def test_point_kernel_within_one_ulp_and_identical_on_a_rerun(hip):
    import torch
    orbhip, ctx = hip
    g, _ = ec.make("v10")
    r64, _, _ = ec.model_runs("v10")
    Xw, ref, Scw, Swc = sg.points_scene(g, r64["est"], 10000)
    assert (ref < 0).sum() > 100
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dX, dr, dS, dW = dev(Xw), dev(ref), dev(Scw), dev(Swc)
    outs = []
    for _ in range(2):
        out = torch.zeros_like(dX)
        torch.cuda.synchronize()
        orbhip.pose_graph_correct_points_device(ctx, dX.data_ptr(), dr.data_ptr(), len(ref), dS.data_ptr(), dW.data_ptr(), len(Scw), out.data_ptr())
        ctx.synchronize()
        outs.append(out.cpu().numpy())
    want = em.correct_points(Xw, ref, Scw, Swc)
    ulp = np.abs(outs[0].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
    assert ulp <= 1, ulp
    assert outs[0][ref < 0].tobytes() == Xw[ref < 0].tobytes() and outs[1].tobytes() == outs[0].tobytes()
    assert np.abs(outs[0] - Xw)[ref >= 0].max() > 1e-3
