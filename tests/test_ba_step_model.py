"""CPU checks of the one-tick BA model (tests/ba_step_model.py): they keep the model and the bound of test_gpu_ba_step.py /
test_gpu_iba_step.py honest.

* the float64 oracle after ONE Levenberg-Marquardt tick against the extended-precision model, on every graph the GPU tests use: the
  oracle accepts the first trial (a condition of the case list, not a measurement) and its step error is <= 1e-10 + 64 floor (largest
  seen: 2e-12 in the generator's coordinates) -- this guards the model against its own mistakes, it is not the GPU bound;
* the model against the dense, Schur-free numpy model of test_oracle_match_ba.py (numeric Jacobians) on its 6 x 40 graph;
* teeth: against a model that leaves ONE off-diagonal block pair of ONE point out of the Schur complement, or one pose's W term out
  of one point's back-substitution, the oracle FAILS the bound the GPU tests apply to the device (same function, same K)."""
import numpy as np
import pytest
import ba_step_model as bm
import ba_step_cases as bc


def _oracle_model_bound(o):
    return 1e-10 + 64 * o["floor"]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_oracle_first_tick_matches_the_model(name):
    ref = bc.local_reference(name)
    st, t, o = ref["stats"], ref["tick"], ref["oracle"]
    spec = bc.CASES[name][1]
    if "nf" in spec:
        assert t["n"] == 6 * spec["nf"]
    print("[ba-step cpu] %-26s n %4d edges %6d lambda %.3g chi2 %.6g -> %.6g |dx| %.3g e_oracle %.3g floor %.3g backward %.3g growth %.3g max|L| %.3g"
          % (name, t["n"], t["n_edges"], float(t["lam"]), st["chi2_initial"], st["chi2_final"], o["norm"], o["e"], o["floor"], o["backward"],
             t["growth"], t["max_L"]))
    assert st["lm_trials"] == 1 and st["iterations_run"] == [1, 0] and st["discarded"] == 0
    assert st["chi2_final"] < st["chi2_initial"]
    assert abs(st["chi2_initial"] - t["chi2"]) <= t["n_edges"] * 2.0 ** -52 * t["chi2"]
    assert o["e"] <= _oracle_model_bound(o), (o, _oracle_model_bound(o))
    assert o["backward"] <= t["order"] * 2.0 ** -52


def test_model_against_the_dense_numpy_model():
    """_dense_numpy_ba_model: numeric Jacobians, the dense (6 nf + 3 L) system, numpy.linalg.solve, no Schur complement -- agreement to
    that model's finite-difference accuracy, the tolerances test_ba_first_lm_iteration_against_an_independent_dense_numpy_model states."""
    import synth_ba
    import oracle_ba_bind as ob
    from test_oracle_match_ba import _dense_numpy_ba_model
    g = synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=321, n_fixed=2, outlier_frac=0.1)
    p = ob.default_params()
    p.iters1, p.iters2 = 1, 0
    R1, t1, X1, chi0, chi1, trials, _, _, _ = _dense_numpy_ba_model(g, p, [1])
    t = bm.local_tick(g, p)
    assert trials == 1 and abs(chi0 - t["chi2"]) <= 1e-9 * chi0
    for i, k in enumerate(t["free"]):
        assert np.max(np.abs(np.asarray(t["R1"][i], np.float64) - R1[k])) <= 1e-6 and np.max(np.abs(np.asarray(t["t1"][i], np.float64) - t1[k])) <= 1e-6, k
    assert np.max(np.abs(np.asarray(t["X1"], np.float64) - X1)) <= 1e-5


@pytest.mark.parametrize("name", ["nf15", "pool0", "shift_mono"])
def test_exact_pinhole_edges_and_what_the_yardstick_does_not_see(name):
    """The model takes the oracle's float64 residuals and Jacobians, so e_oracle contains no edge-evaluation error.  With the monocular
    Pinhole edges evaluated in longdouble by the model itself: in the generator's coordinates nothing changes (the oracle stays within
    its CPU bound, which pins orc_ba_edge a second time); in the world shifted by (1000, -2000, 500) m, R X + t cancels 2000 m down
    to 5 m and a float64 evaluation -- the oracle's, the device's -- loses about eps |X| f / z = 3e-10 px per residual, which moves the
    step by 6.6e-10 of its size.  That is the level the device shows there (8.9e-10) and the reason for K, see ba_step_model.K.
    Bound for the shifted window: 2^-52 |X| f / z per residual against a residual scale of 1 px, times the 64 of the CPU bound."""
    g, p = bc.graph(name), bc.local_params(name)
    ref = bc.local_reference(name)
    t = bm.local_tick(g, p, edges=bm.exact_pinhole_mono_edges)
    o = bm.local_errors(t, ref["oracle_poses"], ref["oracle_points"])
    print("[ba-step exact edges] %-12s e_oracle with exact edges %.3g, with the oracle's own %.3g, floor %.3g" % (name, o["e"], ref["oracle"]["e"], o["floor"]))
    if bc.CASES[name][1].get("shifted"):
        assert o["e"] <= 64 * 2.0 ** -52 * 2300.0 * 458.0 / 2.0
    else:
        assert o["e"] <= _oracle_model_bound(o)


@pytest.mark.parametrize("leave_out", ["schur", "backsub"])
@pytest.mark.parametrize("name", ["stereo_0.4", "pool5"])
def test_bound_has_teeth(name, leave_out):
    """The committed form of the mutation experiment: the oracle measured against a model with one block (pair) missing must fail the
    device's bound, whose yardstick stays the oracle against the intact model.  stereo_0.4 is the 12 x 300 stereo graph, pool5 a
    20 x 200 one the batches use; the 20 x 500 graph is below."""
    ref = bc.local_reference(name)
    g, p = bc.graph(name), bc.local_params(name)
    bad = bm.local_tick(g, p, leave_out=leave_out)
    cand = bm.local_errors(bad, ref["oracle_poses"], ref["oracle_points"])
    print("[ba-step teeth] %-12s %-8s e against the mutated model %.3g, yardstick %.3g + floor %.3g" % (name, leave_out, cand["e"], ref["oracle"]["e"], ref["oracle"]["floor"]))
    assert bm.within_bound(ref["oracle"]["e"], ref["oracle"]["e"], ref["oracle"]["floor"])
    assert not bm.within_bound(cand["e"], ref["oracle"]["e"], ref["oracle"]["floor"])
    assert cand["e"] > 100 * bm.K * (ref["oracle"]["e"] + ref["oracle"]["floor"])          # not a near miss


@pytest.mark.parametrize("leave_out", ["schur", "backsub"])
def test_bound_has_teeth_20x500(leave_out):
    import synth_ba
    import oracle_ba_bind as ob
    g = synth_ba.make_graph(n_kf=20, n_pts=500, obs=8, seed=12)
    p = ob.default_params(); p.iters1, p.iters2, p.no_discard = 1, 0, 1
    rc, poses, pts, _, st = ob.solve(g, p)
    assert st["lm_trials"] == 1
    good = bm.local_errors(bm.local_tick(g, p), poses, pts)
    cand = bm.local_errors(bm.local_tick(g, p, leave_out=leave_out), poses, pts)
    print("[ba-step teeth] 20x500 %-8s e against the mutated model %.3g, yardstick %.3g + floor %.3g" % (leave_out, cand["e"], good["e"], good["floor"]))
    assert not bm.within_bound(cand["e"], good["e"], good["floor"])


# ---------------------------------------------------------------------------------------------- inertial local BA
@pytest.mark.parametrize("name", list(bc.IBA_CASES))
def test_inertial_oracle_first_tick_matches_the_model(name):
    ref = bc.iba_reference(name)
    st, t, o = ref["stats"], ref["tick"], ref["oracle"]
    w = bc.window(name)
    assert t["n"] == 15 * bc.IBA_CASES[name][0]["n_opt"]
    print("[iba-step cpu] %-20s n %4d edges %6d err %.6g -> %.6g |dx| %.3g e_oracle %.3g floor %.3g backward %.3g growth %.3g max|L| %.3g"
          % (name, t["n"], w.n_edges, st.err, st.err_end, o["norm"], o["e"], o["floor"], o["backward"], t["growth"], t["max_L"]))
    assert st.iterations_run == 1 and st.lm_trials == 1 and st.failed == 0
    assert st.err_end < st.err
    assert abs(st.err - t["chi2"]) <= t["n_edges"] * 2.0 ** -52 * t["chi2"]
    assert o["e"] <= _oracle_model_bound(o), (o, _oracle_model_bound(o))
    assert o["backward"] <= t["order"] * 2.0 ** -52


@pytest.mark.parametrize("leave_out", ["schur", "backsub"])
@pytest.mark.parametrize("name", ["opt8", "opt10_fisheye_rig"])
def test_inertial_bound_has_teeth(name, leave_out):
    ref = bc.iba_reference(name)
    bad = bm.inertial_tick(bc.window(name), bc.iba_params(name), leave_out=leave_out)
    cand = bm.inertial_errors(bad, ref["oracle_kf"], ref["oracle_points"])
    print("[iba-step teeth] %-18s %-8s e against the mutated model %.3g, yardstick %.3g + floor %.3g" % (name, leave_out, cand["e"], ref["oracle"]["e"], ref["oracle"]["floor"]))
    assert not bm.within_bound(cand["e"], ref["oracle"]["e"], ref["oracle"]["floor"])
