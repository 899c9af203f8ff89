"""HIP-vs-model parity of the batched MLPnPsolver (PnP RANSAC for relocalisation candidates), through the C ABI, the host form and the
class.  The yardstick is the numpy model (tests/mlpnp_model.py) on the committed batch (tests/synth_mlpnp.py): budget, outcome, returning
iteration, n_inliers, inlier flags and the number of Refine() calls identical on EVERY candidate, count[k] identical on every iteration whose
margin is >= delta = 1e-3, Tcw within a bound that is measured here, not fixed: 4 x the largest distance, after rounding to float, between
the model's decomposition variants (numpy.linalg versus its own Jacobi, closed-form versus randomly turned null-space bases) on the same
sets, and at least one float ulp of the candidate's largest entry.  The preconditions of that comparison are checked on the model in
tests/test_mlpnp_model.py."""
import os
import subprocess
import numpy as np
import pytest

import mlpnp_model as m
import ransac_sets_model as rs
import synth_mlpnp as sy
import synth_sim3 as s3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_mlpnp_smoke")
SENT_U8, SENT_F, SENT_I = 7, 123.0, -9                           # what the kernels must not touch keeps these values
F32 = np.float32
KB8 = pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])


def _params(grp_params, iterations, sets_given, seed=0, first_call=0, resume_at=0):
    import orbhip
    return orbhip.mlpnp_params(grp_params["probability"], grp_params["min_inliers"], iterations, 6, grp_params["epsilon"], grp_params["th2"],
                               first_call, resume_at, not sets_given, seed)


def _run(ctx, pbs, max_n, iterations, grp_params, sets=None, seed=0, n_override=None, stats=True, counts=True, first_call=0, resume_at=0):
    """device form -> dict of numpy arrays; sets = list of [iterations][6] (draw_sets = 0) or None (drawn on the device)"""
    import torch
    import orbhip
    C = len(pbs)
    X = np.zeros((C, max_n, 3), F32); P = np.zeros((C, max_n, 2), F32); S2 = np.ones((C, max_n), F32)
    n = np.array([len(pb["Xw"]) for pb in pbs], np.int32)
    for f, pb in enumerate(pbs):
        k = min(n[f], max_n)
        X[f, :k] = pb["Xw"][:k]; P[f, :k] = pb["p2d"][:k]; S2[f, :k] = pb["sigma2"][:k]
    if n_override is not None:
        n = np.asarray(n_override, np.int32)
    S = np.full((C, iterations, 6), SENT_I, np.int32)
    if sets is not None:
        for f, s in enumerate(sets):
            S[f] = s[:iterations]
    t = [torch.from_numpy(a).cuda() for a in (X, P, S2, n, S)]
    oc = torch.full((C,), SENT_U8, dtype=torch.uint8, device="cuda")
    T = torch.full((C, 12), SENT_F, dtype=torch.float32, device="cuda")
    nin = torch.full((C,), SENT_I, dtype=torch.int32, device="cuda")
    inl = torch.full((C, max_n), SENT_U8, dtype=torch.uint8, device="cuda")
    st = torch.full((C, 4), SENT_I, dtype=torch.int32, device="cuda")
    cnt = torch.full((C, iterations), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cam = orbhip.sim3_camera(pbs[0]["cam"]["K"], pbs[0]["cam"]["kb8"])
    p = _params(grp_params, iterations, sets is not None, seed, first_call, resume_at)
    orbhip.mlpnp_solver_device(ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), C, max_n, cam, p, t[4].data_ptr(),
                               oc.data_ptr(), T.data_ptr(), nin.data_ptr(), inl.data_ptr(), st.data_ptr() if stats else None,
                               cnt.data_ptr() if counts else None)
    ctx.synchronize()
    return dict(outcome=oc.cpu().numpy(), Tcw=T.cpu().numpy(), n_inliers=nin.cpu().numpy(), inlier=inl.cpu().numpy(), stats=st.cpu().numpy(),
                counts=cnt.cpu().numpy(), sets=t[4].cpu().numpy())


def _check_pose(got, ref, measured, tag):
    """got / ref = Tcw [12] float; -> distance"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, F32).astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), tag
    d = float(np.abs(got - ref).max())
    bound = max(4 * measured, float(np.spacing(F32(np.abs(ref).max()))))
    assert d <= bound, (tag, d, bound)
    return d


def _compare(out, f, pb, r, measured, tag, sets=None):
    """one candidate of a device result against its model result -> (distance, counts compared, counts left to the flags)"""
    n, E = len(pb["Xw"]), r["executed"]
    assert out["stats"][f][0] == r["budget"], (tag, out["stats"][f], r["budget"])
    assert (out["inlier"][f, n:] == SENT_U8).all(), tag                         # rows at n and above are untouched
    assert (out["counts"][f, E:] == -1).all(), tag                              # iterations the call does not run
    if sets is not None:
        assert np.array_equal(out["sets"][f], sets[:len(out["sets"][f])]), tag                        # draw_sets = 0: the caller's sets are read only
    far = r["margins"] >= sy.DELTA
    np.testing.assert_array_equal(out["counts"][f, :E][far], r["counts"][:E][far], err_msg=str(tag))
    assert (out["outcome"][f], out["stats"][f][1], out["n_inliers"][f], out["stats"][f][3]) == (r["outcome"], r["ret"], r["n_inliers"], r["nref"]), \
        (tag, out["outcome"][f], out["stats"][f], out["n_inliers"][f], r["outcome"], r["ret"], r["n_inliers"], r["nref"])
    np.testing.assert_array_equal(out["inlier"][f, :n], r["inlier"].astype(np.uint8), err_msg=str(tag))
    assert out["n_inliers"][f] == int(out["inlier"][f, :n].sum()), tag
    if r["outcome"] == 0:
        assert (out["Tcw"][f] == SENT_F).all() and out["stats"][f].tolist() == [r["budget"], -1, 0, 0], tag      # the pose is untouched
        return 0.0, int(far.sum()), int((~far).sum())
    assert out["stats"][f][2] == out["counts"][f, r["ret"]] == r["ret_count"], tag
    if r["outcome"] == 2:
        assert out["n_inliers"][f] == out["counts"][f, r["ret"]], tag            # the same device function counted and flagged
    return _check_pose(out["Tcw"][f], r["Tcw"], measured, tag), int(far.sum()), int((~far).sum())


@KB8
def test_batch_matches_the_model(gpu_ctx, kb8):
    """n = 15, 63, 64, 65, 200, two planar candidates (world z exactly 0), a scripted scan, 4097 (one above the LDS-resident limit); n = 6
    with min_inliers 6 (budget 1); n = 9 with min_inliers 10 (bNoMore at once) and n = 20 with exactly 10 inliers under (0.99, 10, 300, 6,
    0.5, 5.991): a return needs MORE than 10, outcome 2.  Sets from the host.  No candidate is left out of any comparison."""
    measured = sy.measured_variant_distance(kb8)
    worst, compared, skipped, outcomes = 0.0, 0, 0, []
    for grp, cands, ress in sy.gpu_batch_model(kb8):
        pbs, sets = [c[0] for c in cands], [c[1] for c in cands]
        max_n = max(len(pb["Xw"]) for pb in pbs) + 3
        out = _run(gpu_ctx, pbs, max_n, sy.ITERATIONS, grp["params"], sets)
        gpu_ctx.check_status()
        for f, (pb, r) in enumerate(zip(pbs, ress)):
            d, c, s = _compare(out, f, pb, r, measured, (grp["name"], f), sets[f])
            worst = max(worst, d); compared += c; skipped += s; outcomes.append(r["outcome"])
            print("%-18s n = %4d: budget %3d, outcome %d at iteration %3d, %4d inliers, %d Refine() calls, distance to the model %.3e" %
                  (grp["name"], len(pb["Xw"]), r["budget"], r["outcome"], r["ret"], r["n_inliers"], r["nref"], d))
    assert set(outcomes) == {0, 1, 2}
    print("model variants after rounding to float (measured): %.3e; largest distance to the model in Tcw: %.3e; counts compared on %d "
          "iterations, %d within delta left to the flags" % (measured, worst, compared, skipped))


def test_null_stats_and_counts(gpu_ctx):
    """the optional outputs left out: everything else is the same"""
    grp, cands, ress = sy.gpu_batch_model(False)[2]
    pbs, sets = [c[0] for c in cands], [c[1] for c in cands]
    a = _run(gpu_ctx, pbs, 24, sy.ITERATIONS, grp["params"], sets)
    b = _run(gpu_ctx, pbs, 24, sy.ITERATIONS, grp["params"], sets, stats=False, counts=False)
    assert (b["stats"] == SENT_I).all() and (b["counts"] == SENT_I).all()
    for k in ("outcome", "Tcw", "n_inliers", "inlier"):
        assert np.array_equal(a[k], b[k]), k


@KB8
def test_host_form(gpu_ctx, kb8):
    import orbhip
    measured = sy.measured_variant_distance(kb8)
    for grp, cands, ress in sy.gpu_batch_model(kb8):
        for f, ((pb, sets), r) in enumerate(zip(cands, ress)):
            cam = orbhip.sim3_camera(pb["cam"]["K"], pb["cam"]["kb8"])
            h = orbhip.mlpnp_solver_host(gpu_ctx, pb["Xw"], pb["p2d"], pb["sigma2"], cam, _params(grp["params"], sy.ITERATIONS, True), sets,
                                         np.full(12, SENT_F, F32))
            out = dict(outcome=[h["outcome"]], Tcw=h["Tcw"][None], n_inliers=[h["n_inliers"]], inlier=h["inlier"][None], stats=h["stats"][None],
                       counts=h["counts"][None], sets=h["sets"][None])
            _compare(out, 0, pb, r, measured, (grp["name"], f, "host"), sets)


def _class_file(path, pb, params, n_iterations, extra_null=3):
    """a stand-in frame: every match has a keypoint; extra NULL matches, one bad map point and one match beyond mvKeysUn are skipped by the
    constructor (:65-70) -> (the flat arrays written, indices of the gathered matches)"""
    n = len(pb["Xw"])
    r = np.random.RandomState(4)
    slots = n + extra_null + 1
    order = r.permutation(n + extra_null)                                      # keypoint slot of every match (NULL slots in between)
    kp = np.zeros((n + extra_null, 2), F32); octv = np.zeros(n + extra_null, np.int32); matches = np.full(slots, -1, np.int32)
    level = {float(v): k for k, v in enumerate(sy.SIGMA2)}
    mp_pos = np.r_[pb["Xw"], np.zeros((2, 3), F32)]; mp_bad = np.zeros(n + 2, np.int32); mp_bad[n] = 1
    for i in range(n):
        kp[order[i]] = pb["p2d"][i]; octv[order[i]] = level[float(pb["sigma2"][i])]; matches[order[i]] = i
    matches[order[n]] = n                                                      # a bad map point
    matches[slots - 1] = n + 1                                                 # a match at an index beyond mvKeysUn
    cam = pb["cam"]
    arrays = dict(cam_type=np.array([0 if cam["kb8"] is None else 1]), cam=np.array(list(cam["K"]) + list(cam["kb8"] or (0, 0, 0, 0)), F32),
                  sigma2=sy.SIGMA2, kp=kp, oct=octv, mp_pos=mp_pos, mp_bad=mp_bad, matches=matches,
                  probability=np.array([params["probability"]], F32), min_inliers=np.array([params["min_inliers"]]),
                  max_iterations=np.array([300]), epsilon=np.array([params["epsilon"]], F32), th2=np.array([params["th2"]], F32),
                  n_iterations=np.array([n_iterations]))
    s3.write_flat(path, arrays)
    gathered = np.array([i for i in range(n + extra_null) if matches[i] >= 0 and matches[i] < n])
    return arrays, gathered, slots


@KB8
def test_class_drop_in(gpu_ctx, kb8, tmp_path):
    """lib/host_mlpnp_smoke: the constructor's gathering, Relocalization's parameters, iterate(40, ...) and a second call that resumes
    (40 > the budget of 35, so the second call draws further sets, and the first returns on the sets of srand(1)); against the model on
    the sets the class drew"""
    pb = sy.make_candidate(9150, 50, kb8=kb8, outlier_share=0.2)
    params = dict(probability=0.99, min_inliers=10, epsilon=0.5, th2=5.991)    # src/Tracking.cc:2674
    NIT = 40
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    arrays, gathered, slots = _class_file(fin, pb, params, NIT)
    r = subprocess.run([EXE, fin, fout, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = s3.read_flat(fout)
    # the class's correspondences, in the order of the match vector
    q = dict(Xw=pb["Xw"][arrays["matches"][gathered]], p2d=arrays["kp"][gathered], sigma2=sy.SIGMA2[arrays["oct"][gathered]], cam=pb["cam"])
    sets = out["sets"].reshape(-1, 6)
    nmin, budget = m.ransac_parameters(len(gathered), max_iterations=300, **{k: params[k] for k in ("probability", "min_inliers", "epsilon")})
    assert budget == 35 and len(sets) > NIT                                     # further sets were drawn by the second call
    pos, ipos, first = 0, 0, 0
    measured = sy.measured_variant_distance(kb8)
    for call in range(int(out["calls"][0])):
        K = max(budget, first + NIT)
        assert K <= len(sets)
        ref = m.solve(q, sets[:K], max_iterations=K, first_call_iterations=K, resume_at=first, delta=sy.DELTA, **params)
        assert m.decision_is_stable(ref, sy.DELTA)
        assert out["stats"][4 * call + 1] == ref["ret"] and out["stats"][4 * call + 3] == ref["nref"], (call, out["stats"], ref["ret"], ref["nref"])
        assert out["ret_empty"][call] == int(ref["outcome"] == 0) and out["no_more"][call] == int(ref["outcome"] != 1)
        assert out["n_inliers"][call] == ref["n_inliers"]
        nflags = int(out["inliers"][ipos]); flags = out["inliers"][ipos + 1: ipos + 1 + nflags]; ipos += 1 + nflags
        if ref["outcome"]:
            assert nflags == slots
            want = np.zeros(slots, np.int32); want[gathered[ref["inlier"]]] = 1
            assert np.array_equal(flags, want)
            T = out["T"][pos: pos + 16].reshape(4, 4); pos += 16
            assert T[3].tolist() == [0, 0, 0, 1]
            _check_pose(np.r_[T[:3, :3].reshape(9), T[:3, 3]], ref["Tcw"], measured, ("class", call))
        else:
            assert nflags == 0
        if call == 0:
            assert ref["outcome"] == 1                                         # so that the second call resumes: further sets, resume_at, mnIterations
        first = ref["ret"] + 1 if ref["outcome"] == 1 else K
    assert int(out["calls"][0]) == 2 and first > 1


@KB8
def test_device_drawn_sets(gpu_ctx, kb8):
    """sets drawn on the device: 6 distinct indices in [0, n), the generator of csrc/ransac_common.h as tests/ransac_sets_model.py restates it, keyed
    by (seed, the candidate's INDEX in the call, iteration, draw): the same index gives the same sets, alone or inside a batch, twice; a
    candidate moved to another index, or another seed, gets other sets; the result on them is the model's"""
    grp, cands, _ = sy.gpu_batch_model(kb8)[0]
    pbs = [cands[k][0] for k in (0, 1, 4)]                                     # n = 15, 63, 200
    a = _run(gpu_ctx, pbs, 200, 64, grp["params"], None, seed=5)
    for f, pb in enumerate(pbs):
        n = len(pb["Xw"]); s = a["sets"][f]
        assert (s >= 0).all() and (s < n).all() and all(len(set(row)) == 6 for row in s.tolist()), f
    b = _run(gpu_ctx, pbs, 200, 64, grp["params"], None, seed=5)
    c = _run(gpu_ctx, pbs, 200, 64, grp["params"], None, seed=6)
    assert np.array_equal(a["sets"], b["sets"]) and not np.array_equal(a["sets"], c["sets"])
    for k in ("outcome", "Tcw", "n_inliers", "inlier", "stats", "counts"):
        assert np.array_equal(a[k], b[k]), k
    alone = _run(gpu_ctx, pbs[:1], 200, 64, grp["params"], None, seed=5)       # candidate 0 keeps its index: the same sets
    assert np.array_equal(alone["sets"][0], a["sets"][0]) and np.array_equal(alone["Tcw"][0], a["Tcw"][0])
    moved = _run(gpu_ctx, pbs[::-1], 200, 64, grp["params"], None, seed=5)     # the 200-point candidate at index 0: index 0's draws, scaled to its n
    assert np.array_equal(moved["sets"][0], rs.device_sets(5, 0, 200, 64, 6)) and not np.array_equal(moved["sets"][0], a["sets"][2])
    cut = lambda n: dict(pbs[0], Xw=pbs[0]["Xw"][:n], p2d=pbs[0]["p2d"][:n], sigma2=pbs[0]["sigma2"][:n])
    small = _run(gpu_ctx, [cut(4)], 8, 16, grp["params"], None)
    assert (small["sets"] == -1).all() and small["outcome"][0] == 0             # n < 6: no set can be drawn
    edge = _run(gpu_ctx, [cut(6), cut(7)], 8, 300, grp["params"], None, seed=5)  # every draw meets a moved slot or the last one
    for f, n in enumerate((6, 7)):
        assert np.array_equal(edge["sets"][f], rs.device_sets(5, f, n, 300, 6)), n
    measured = sy.measured_variant_distance(kb8)
    for f, pb in enumerate(pbs):
        assert np.array_equal(a["sets"][f], rs.device_sets(5, f, len(pb["Xw"]), 64, 6)), f
        ref = m.solve(pb, a["sets"][f], max_iterations=64, delta=sy.DELTA, **grp["params"])
        assert m.decision_is_stable(ref, sy.DELTA), f                          # a seed that breaks it is replaced, not skipped
        _compare(a, f, pb, ref, measured, ("drawn", f))


@KB8
def test_resume_at(gpu_ctx, kb8):
    """resume_at = returning iteration + 1 gives the model's next return: earlier iterations rebuild the best, they cannot return"""
    grp, cands, ress = sy.gpu_batch_model(kb8)[0]
    (pb, sets), r0 = cands[7], ress[7]                                         # the scripted scan: returns at 5, a better set at 6
    assert (r0["outcome"], r0["ret"]) == (1, 5)
    measured = sy.measured_variant_distance(kb8)
    resume = 6
    for _ in range(2):
        ref = m.solve(pb, sets, max_iterations=sy.ITERATIONS, resume_at=resume, delta=sy.DELTA, **grp["params"])
        assert ref["outcome"] == 1 and ref["ret"] >= resume and m.decision_is_stable(ref, sy.DELTA)
        out = _run(gpu_ctx, [pb], 64, sy.ITERATIONS, grp["params"], [sets], resume_at=resume)
        _compare(out, 0, pb, ref, measured, ("resume", resume), sets)
        resume = ref["ret"] + 1
    assert ref["nref"] >= 3 and ref["ret"] > 6                                 # the third return: Refine() was called at 5, at 6 and there


def test_first_call_iterations(gpu_ctx):
    """the loop's `|| nCurrentIterations < nIterations`: a call runs max(budget, first_call_iterations) iterations, never more than K"""
    grp, cands, ress = sy.gpu_batch_model(False)[2]
    (pb, sets), r = cands[1], ress[1]                                          # n = 20: budget 35, outcome 2
    for first_call, K, E in ((0, 300, 35), (50, 300, 50), (50, 40, 40), (10, 20, 20)):
        ref = m.solve(pb, sets, max_iterations=K, first_call_iterations=first_call, delta=sy.DELTA, **grp["params"])
        assert ref["executed"] == E
        out = _run(gpu_ctx, [pb], 20, K, grp["params"], [sets], first_call=first_call)
        assert (out["counts"][0, :E] >= 0).all() and (out["counts"][0, E:] == -1).all()
        assert m.decision_is_stable(ref, sy.DELTA)
        _compare(out, 0, pb, ref, sy.measured_variant_distance(False), ("first_call", first_call, K), sets)


def test_invalid_sets_count_zero(gpu_ctx):
    """a set with an index outside [0, n) and a set of six copies of one point are no hypotheses: count 0, no fault; the rest is unchanged"""
    grp, cands, ress = sy.gpu_batch_model(False)[0]
    (pb, sets), r = cands[1], ress[1]                                          # n = 63
    s = sets.copy()
    s[0] = [0, 1, 2, 3, 4, 63]; s[1] = [-1, 1, 2, 3, 4, 5]; s[2] = [7] * 6; s[3] = [1 << 30, 1, 2, 3, 4, 5]; s[4] = [0, 1, 2, 3, 4, 4]
    out = _run(gpu_ctx, [pb], 63, sy.ITERATIONS, grp["params"], [s])
    gpu_ctx.check_status()
    assert out["counts"][0, :5].tolist() == [0] * 5
    ref = m.solve(pb, s, max_iterations=sy.ITERATIONS, delta=sy.DELTA, **grp["params"])
    assert ref["counts"][:5].tolist() == [0] * 5 and m.decision_is_stable(ref, sy.DELTA)
    _compare(out, 0, pb, ref, sy.measured_variant_distance(False), "invalid sets", s)


def test_bad_counts_and_capacity(gpu_ctx):
    """a candidate with n outside [0, max_n] sets the status word and writes only outcome 0; max_n = 8193 and K = 1025 are refused, a
    bad parameter is named"""
    import orbhip
    grp, cands, ress = sy.gpu_batch_model(False)[2]
    pbs, sets = [c[0] for c in cands], [c[1] for c in cands]
    out = _run(gpu_ctx, pbs, 24, sy.ITERATIONS, grp["params"], sets, n_override=[25, 20])
    with pytest.raises(orbhip.OrbHipError) as e:
        gpu_ctx.check_status()
    assert e.value.code == orbhip.E_CAPACITY
    gpu_ctx.check_status()                                                     # reported once, then clear
    assert out["outcome"][0] == 0 and out["n_inliers"][0] == 0 and out["stats"][0].tolist() == [0, -1, 0, 0]
    assert (out["inlier"][0] == SENT_U8).all() and (out["Tcw"][0] == SENT_F).all() and (out["counts"][0] == SENT_I).all()
    assert out["outcome"][1] == ress[1]["outcome"] and out["n_inliers"][1] == ress[1]["n_inliers"]      # its neighbour is served
    out = _run(gpu_ctx, pbs, 24, sy.ITERATIONS, grp["params"], sets, n_override=[-1, 0])
    with pytest.raises(orbhip.OrbHipError):
        gpu_ctx.check_status()
    assert out["outcome"].tolist() == [0, 0] and (out["inlier"] == SENT_U8).all()
    cam = orbhip.sim3_camera(s3.K_VGA)
    for max_n, K in ((8193, 300), (64, 1025)):
        with pytest.raises(orbhip.OrbHipError) as e:
            orbhip.mlpnp_solver_device(gpu_ctx, 8, 8, 8, 8, 1, max_n, cam, orbhip.mlpnp_params(max_iterations=K), 8, 8, 8, 8, 8)
        assert e.value.code == orbhip.E_CAPACITY
    for kw, field in ((dict(min_set=5), "min_set"), (dict(min_inliers=0), "min_inliers"), (dict(max_iterations=0), "max_iterations"),
                      (dict(probability=1.0), "probability"), (dict(epsilon=0.0), "epsilon"), (dict(th2=0.0), "th2"),
                      (dict(first_call_iterations=-1), "first_call_iterations"), (dict(resume_at=-1), "resume_at")):
        with pytest.raises(orbhip.OrbHipError) as e:
            orbhip.mlpnp_solver_device(gpu_ctx, 8, 8, 8, 8, 1, 64, cam, orbhip.mlpnp_params(**kw), 8, 8, 8, 8, 8)
        assert e.value.code == orbhip.E_BADARG and field in str(e.value), field
    # the host form applies the same rules before it stages anything, for an empty candidate too
    empty = (np.zeros((0, 3), F32), np.zeros((0, 2), F32), np.zeros(0, F32))
    for kw, field in ((dict(min_set=5), "min_set"), (dict(max_iterations=1025), "1024"), (dict(th2=-1.0), "th2")):
        with pytest.raises(orbhip.OrbHipError) as e:
            orbhip.mlpnp_solver_host(gpu_ctx, *empty, cam, orbhip.mlpnp_params(draw_sets=False, **kw), np.zeros((max(kw.get("max_iterations", 300), 1), 6), np.int32))
        assert field in str(e.value), (field, str(e.value))
    gpu_ctx.check_status()
