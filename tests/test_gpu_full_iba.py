"""GPU tests of the full inertial BA (orbhip_full_inertial_ba_solve_batch, k_fiba_solve in csrc/iba_kernels.hip) against the
extended-precision model (tests/full_iba_model.py) on the committed cases (tests/full_iba_cases.py).

Per case: iterations, trial count and lambda after the decisive prefix equal the extended-precision model's (lambda under the K rule);
one LM iteration and the end state are held to the project's K rule (ba_step_model.within_bound, K = 128: e_device <=
K (e_float64_model + 2^-52 max|value|), truth = the extended-precision model); the end state, with the 4-DoF gauge taken out, to the
1e-4 RMSE parity bound; a run that goes past the decisive prefix gets the slack of full_iba_cases.past_prefix_slack; a second run is
byte-identical.  Then the capacity refusals, the stop flag, a ragged batch with an empty map."""
import ctypes as C
import numpy as np
import pytest
import full_iba_cases as fc
import full_iba_model as fm
import synth_full_iba as sf

pytestmark = pytest.mark.gpu
E_CAPACITY, E_ABORTED = -4, -5


@pytest.fixture(scope="module")
def hip():
    import orbhip
    ctx = orbhip.Context(0)
    yield orbhip, ctx
    ctx.close()


def _solve(hip, name, iterations=None, max_trials=None):
    orbhip, ctx = hip
    win, sb, prm = fc.make(name)
    p = orbhip.fiba_default_params(prm["iterations"] if iterations is None else iterations, prm["shared"], prm["prior_g"], prm["prior_a"])
    if max_trials is not None:
        p.max_trials = max_trials
    kf, X, sbo, st = orbhip.full_inertial_ba_solve_batch(ctx, [win.struct(orbhip.IbaWindow)], [win.kf0], [win.pts0], sb[None], p)
    return kf[0], X[0], sbo[0], st[0]


def _report(tag, name, rep, rmse):
    print("[full-iba] %-7s %-10s %s rmse %.3g" % (tag, name, " ".join("%s %.2g (f64 %.2g, ratio %.2g)" % (g, v[0], v[2], v[3]) for g, v in rep.items()), rmse))


def _prefix_runs(name):
    r64, rld, pre = fc.model_runs(name)
    if pre == rld["iterations"]:
        return r64, rld, pre                                 # the whole run is decisive: optimize(pre) is the same run
    return fc.model_runs(name, pre)[:2] + (pre,)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_decisions_and_state_over_the_decisive_prefix(hip, name):
    _, rld_full, pre = fc.model_runs(name)
    r64, rld, _ = _prefix_runs(name)
    assert pre >= fc.MIN_PREFIX and rld["iterations"] == pre
    kf, X, sb, st = _solve(hip, name, iterations=pre)
    want_its, want_trials, _, _ = fm.prefix_totals(rld_full, pre)
    assert (st["iterations_run"], st["lm_trials"]) == (want_its, want_trials), (st, want_its, want_trials)
    assert st["n_unknowns"] == rld["n"]
    assert abs(st["chi2_first"] - float(rld["chi_first"])) <= 1e-9 * float(rld["chi_first"])
    dev = fc.group_values(kf, X, sb, st["chi2_last"], st["lam"], rld)
    ok, rep = fc.k_rule(dev, r64, rld)
    rmse = fc.gauge_rmse(kf, X, rld)
    _report("prefix", name, rep, rmse)
    assert ok, rep
    assert rmse <= fc.PARITY_RMSE, rmse


@pytest.mark.parametrize("name", list(fc.CASES))
def test_one_iteration_within_the_k_rule(hip, name):
    r64, rld, _ = fc.model_runs(name, 1)
    kf, X, sb, st = _solve(hip, name, iterations=1)
    assert (st["iterations_run"], st["lm_trials"]) == (1, rld["trials"]), (st, rld["trials"])
    assert rld["trace"][0]["accepted"][-1], "the iteration of this case ends without an accepted step: nothing to compare"
    dev = fc.group_values(kf, X, sb, st["chi2_last"], st["lam"], rld)
    ok, rep = fc.k_rule(dev, r64, rld)
    _report("tick", name, rep, fc.gauge_rmse(kf, X, rld))
    assert ok, rep


@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in fc.LARGE])
def test_whole_run_end_state_and_rerun(hip, name):
    """The case's own iteration count.  Past the decisive prefix the accept / reject decisions are rounding noise: the end reason is one
    either model run gives, at most three further iterations run, and the end state gets past_prefix_slack()."""
    r64, rld, pre = fc.model_runs(name)
    kf, X, sb, st = _solve(hip, name)
    assert st["end_reason"] in (rld["reason"], r64["reason"]), (st, rld["reason"], r64["reason"])
    if pre == rld["iterations"]:
        assert (st["iterations_run"], st["lm_trials"]) == (rld["iterations"], rld["trials"]), (st, rld["iterations"], rld["trials"])
        slack = None
    else:
        assert pre <= st["iterations_run"] <= pre + fc.PAST_PREFIX_ITERATIONS, (st, pre)
        slack = fc.past_prefix_slack(r64, rld, pre)
    dev = fc.group_values(kf, X, sb, st["chi2_last"], st["lam"], rld)
    ok, rep = fc.k_rule(dev, r64, rld, slack)
    rmse = fc.gauge_rmse(kf, X, rld)
    _report("whole", name, rep, rmse)
    assert ok, rep
    assert rmse <= fc.PARITY_RMSE, rmse
    kf2, X2, sb2, st2 = _solve(hip, name)
    assert kf2.tobytes() == kf.tobytes() and X2.tobytes() == X.tobytes() and sb2.tobytes() == sb.tobytes() and st2 == st


def _raw(hip, wins, kfs, pts, sb, p, stop=None):
    """The C entry point on the caller's own buffers (the wrapper copies its inputs)."""
    orbhip, ctx = hip
    n = len(wins)
    arr = (orbhip.IbaWindow * n)(*[w.struct(orbhip.IbaWindow) for w in wins])
    pk = (C.c_void_p * n)(*[a.ctypes.data for a in kfs]); pq = (C.c_void_p * n)(*[a.ctypes.data for a in pts])
    stats = (orbhip.FibaStats * n)()
    rc = orbhip.lib.orbhip_full_inertial_ba_solve_batch(ctx.h, C.cast(arr, C.c_void_p), n, C.byref(p), stop.ctypes.data if stop is not None else None,
                                                        C.cast(pk, C.c_void_p), C.cast(pq, C.c_void_p), sb.ctypes.data, C.cast(stats, C.c_void_p))
    return rc, orbhip.lib.orbhip_last_error().decode(), stats


@pytest.mark.parametrize("shared,K,n", [(True, 53, 9 * 53 + 6), (False, 33, 15 * 33)])
def test_capacity_refusal_names_the_count_and_writes_nothing(hip, shared, K, n):
    orbhip, _ = hip
    win, sb0 = sf.make_map(2, K, pts_per_kf=2, bias0_sigma=1e-3)
    kf, X, sb = win.kf0.copy(), win.pts0.copy(), sb0.copy()
    rc, msg, _ = _raw(hip, [win], [kf], [X], sb, orbhip.fiba_default_params(3, shared, 1.0, 1e5))
    assert rc == E_CAPACITY, (rc, msg)
    assert "%d reduced unknowns" % n in msg and "%d free keyframes" % K in msg and "480" in msg, msg
    assert kf.tobytes() == win.kf0.tobytes() and X.tobytes() == win.pts0.tobytes() and sb.tobytes() == sb0.tobytes()


def test_largest_maps_are_accepted(hip):
    """52 free IMU keyframes with shared biases (474 unknowns), 32 with biases per keyframe (480)."""
    orbhip, ctx = hip
    for shared, K, n in ((True, 52, 474), (False, 32, 480)):
        win, sb = sf.make_map(2, K, pts_per_kf=2, bias0_sigma=1e-3)
        _, _, _, st = orbhip.full_inertial_ba_solve_batch(ctx, [win.struct(orbhip.IbaWindow)], [win.kf0], [win.pts0], sb[None],
                                                          orbhip.fiba_default_params(1, shared, 0.0, 0.0))
        assert st[0]["n_unknowns"] == n and st[0]["iterations_run"] == 1


def test_stop_flag_set_before_the_call(hip):
    orbhip, _ = hip
    win, sb0, prm = fc.make("s_k3")
    kf, X, sb = win.kf0.copy(), win.pts0.copy(), sb0.copy()
    p = orbhip.fiba_default_params(3, True, prm["prior_g"], prm["prior_a"])
    rc, _, _ = _raw(hip, [win], [kf], [X], sb, p, stop=np.array([1], np.uint8))
    assert rc == E_ABORTED
    assert kf.tobytes() == win.kf0.tobytes() and X.tobytes() == win.pts0.tobytes() and sb.tobytes() == sb0.tobytes()
    rc, _, stats = _raw(hip, [win], [kf], [X], sb, p, stop=np.array([0], np.uint8))
    assert rc == 0 and stats[0].iterations_run == 3 and kf.tobytes() != win.kf0.tobytes()


def test_ragged_batch_with_an_empty_map(hip):
    """Three maps of different size and an empty one in one call: every map's result is the bytes of its own call."""
    orbhip, ctx = hip
    maps = [fc.make(n)[:2] for n in fc.RAGGED]
    maps.insert(1, sf.empty_map())
    p = orbhip.fiba_default_params(4, True, 1.0, 1e5)
    call = lambda ms: orbhip.full_inertial_ba_solve_batch(ctx, [w.struct(orbhip.IbaWindow) for w, _ in ms], [w.kf0 for w, _ in ms],
                                                          [w.pts0 for w, _ in ms], np.stack([s for _, s in ms]), p)
    kf, X, sb, st = call(maps)
    assert st[1] == dict(iterations_run=0, lm_trials=0, end_reason=0, n_unknowns=0, chi2_first=0.0, chi2_last=0.0, lam=0.0)
    assert kf[1].size == 0 and not sb[1].any()
    for i in (0, 2, 3):
        kf1, X1, sb1, st1 = call([maps[i]])
        assert st1[0] == st[i] and st[i]["iterations_run"] >= 1
        assert kf1[0].tobytes() == kf[i].tobytes() and X1[0].tobytes() == X[i].tobytes() and sb1[0].tobytes() == sb[i].tobytes()


def test_shared_result_is_written_to_every_inertial_keyframe(hip):
    """With shared biases the bias slots of every keyframe with IMU states, fixed ones too, hold the shared estimate on return
    (Optimizer.cc:807-823); a keyframe without IMU states and a fixed keyframe's pose and velocity keep their bytes."""
    win, _, _ = fc.make("s_fixed")
    kf, X, sb, _ = _solve(hip, "s_fixed", iterations=2)
    assert (kf[:, 15:21] == sb[None]).all() and not (sb == win.kf0[0, 15:21]).all()
    assert kf[5:, :15].tobytes() == win.kf0[5:, :15].tobytes()
    l = win.d["fixed_only_point"]
    assert X[l].tobytes() == win.pts0[l].tobytes()
    winm, _, _ = fc.make("s_mixed")
    kfm, _, _, _ = _solve(hip, "s_mixed", iterations=2)
    assert kfm[2, 12:].tobytes() == winm.kf0[2, 12:].tobytes() and kfm[2, :12].tobytes() != winm.kf0[2, :12].tobytes()
