"""HIP-vs-model parity of the batched Sim3Solver (Horn RANSAC for loop candidates), through the C ABI, the host form, the class and the
SearchByBoW -> Sim3Solver -> OptimizeSim3 chain.  The yardstick is the float32 numpy model (tests/sim3_solver_model.py) on the committed
batch (tests/synth_sim3_solver.py): budget, converged flag, winning iteration, n_inliers and inlier flags identical on EVERY pair, count[k]
identical on every iteration whose margin is >= delta = 1e-3, (R12, t12, s12) within a bound that is measured here, not fixed: 4 x the
largest distance between the model run with numpy.linalg.eigh and with its Jacobi solver after rounding to float, and at least one float
ulp of the pair's largest entry.  The preconditions of that comparison are checked on the model in tests/test_sim3_solver_model.py."""
import ctypes
import os
import subprocess
import numpy as np
import pytest

import ransac_sets_model as rs
import sim3_solver_model as m
import synth_sim3_solver as sy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_sim3solver_smoke")
SENT_U8, SENT_F, SENT_I = 7, 123.0, -9                           # what the kernels must not touch keeps these values
F32 = np.float32


def _cams(pb):
    import orbhip
    return orbhip.sim3_camera(pb["cam1"]["K"], pb["cam1"]["kb8"]), orbhip.sim3_camera(pb["cam2"]["K"], pb["cam2"]["kb8"])


def _run(ctx, pbs, max_n, iterations, min_inliers, sets=None, seed=0, n_override=None, stats=True, counts=True, probability=sy.PROBABILITY):
    """device form -> dict of numpy arrays; sets = list of [iterations][3] (draw_sets = 0) or None (drawn on the device)"""
    import torch
    import orbhip
    P = len(pbs)
    X1 = np.zeros((P, max_n, 3), F32); X2 = np.zeros((P, max_n, 3), F32); m1 = np.zeros((P, max_n), F32); m2 = np.zeros((P, max_n), F32)
    n = np.array([len(pb["X1c"]) for pb in pbs], np.int32)
    for f, pb in enumerate(pbs):
        k = min(n[f], max_n)
        X1[f, :k] = pb["X1c"][:k]; X2[f, :k] = pb["X2c"][:k]; m1[f, :k] = pb["max1"][:k]; m2[f, :k] = pb["max2"][:k]
    if n_override is not None:
        n = np.asarray(n_override, np.int32)
    S = np.full((P, iterations, 3), SENT_I, np.int32)
    if sets is not None:
        for f, s in enumerate(sets):
            S[f] = s[:iterations]
    t = [torch.from_numpy(a).cuda() for a in (X1, X2, m1, m2, n, S)]
    conv = torch.full((P,), SENT_U8, dtype=torch.uint8, device="cuda")
    R = torch.full((P, 9), SENT_F, dtype=torch.float32, device="cuda"); tt = torch.full((P, 3), SENT_F, dtype=torch.float32, device="cuda")
    sc = torch.full((P,), SENT_F, dtype=torch.float32, device="cuda")
    nin = torch.full((P,), SENT_I, dtype=torch.int32, device="cuda")
    inl = torch.full((P, max_n), SENT_U8, dtype=torch.uint8, device="cuda")
    st = torch.full((P, 3), SENT_I, dtype=torch.int32, device="cuda")
    cnt = torch.full((P, iterations), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c1, c2 = _cams(pbs[0])
    p = orbhip.sim3_solver_params(probability, min_inliers, iterations, pbs[0]["fix_scale"], sets is None, seed)
    orbhip.sim3_solver_device(ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), P, max_n, c1, c2, p,
                              t[5].data_ptr(), conv.data_ptr(), R.data_ptr(), tt.data_ptr(), sc.data_ptr(), nin.data_ptr(), inl.data_ptr(),
                              st.data_ptr() if stats else None, cnt.data_ptr() if counts else None)
    ctx.synchronize()
    return dict(converged=conv.cpu().numpy(), R12=R.cpu().numpy(), t12=tt.cpu().numpy(), s12=sc.cpu().numpy(), n_inliers=nin.cpu().numpy(),
                inlier=inl.cpu().numpy(), stats=st.cpu().numpy(), counts=cnt.cpu().numpy(), sets=t[5].cpu().numpy())


def _rts(h):
    return np.r_[np.asarray(h["R12"], F32).reshape(9), np.asarray(h["t12"], F32).reshape(3), F32(h["s12"])].astype(np.float64)


def _measured_solver_distance(batch, res, per_pair=20):
    """the largest |eigh - Jacobi| over (R12, t12, s12) after rounding to float, on the first iterations and the winner of every pair"""
    worst = 0.0
    for (pb, sets), r in zip(batch, res):
        for k in sorted(set(range(min(per_pair, r["budget"]))) | ({r["winner"]} if r["winner"] >= 0 else set())):
            s = sets[k]
            a = _rts(r["hyps"][k]); b = _rts(m.horn(pb["X1c"][s], pb["X2c"][s], pb["fix_scale"], "eigh"))
            if np.isfinite(a).all() and np.isfinite(b).all():
                worst = max(worst, float(np.abs(a - b).max()))
    return worst


def _check_estimate(got, ref, measured, tag):
    """got / ref = (R12 [9], t12 [3], s12) flat; NaN entries must coincide; -> distance"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    fin = ~np.isnan(ref)
    if not fin.any():
        return 0.0
    d = float(np.abs(got[fin] - ref[fin]).max())
    bound = max(4 * measured, float(np.spacing(F32(np.abs(ref[fin]).max()))))
    assert d <= bound, (tag, d, bound)
    return d


@pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])
@pytest.mark.parametrize("fix_scale", [False, True], ids=["free_scale", "fix_scale"])
def test_batch_matches_the_model(gpu_ctx, kb8, fix_scale):
    """n = 0, 2 (below min_inliers = 3), 3 (budget 1, cannot converge), 4, 20, 63, 64, 65, 129, 300, 3073 (one above the LDS-resident
    limit), every point behind camera 2, ten coincident points (NaN hypotheses, count 0), outliers only (last arg-max, not converged).
    Sets from the host.  No pair is left out of any comparison."""
    batch, ref = sy.gpu_batch_model(kb8, fix_scale)
    pbs, sets = [b[0] for b in batch], [b[1] for b in batch]
    assert [len(pb["X1c"]) for pb in pbs] == [0, 2, 3, 4, 20, 63, 64, 65, 129, 300, sy.LDS_MAX + 1, 40, 10, 20]
    out = _run(gpu_ctx, pbs, sy.MAX_N, sy.ITERATIONS, sy.MIN_INLIERS, sets)
    gpu_ctx.check_status()
    measured = _measured_solver_distance(batch, ref)
    worst, compared, skipped = 0.0, 0, 0
    for f, (pb, r) in enumerate(zip(pbs, ref)):
        n, B = len(pb["X1c"]), r["budget"]
        assert out["stats"][f][0] == B, (f, out["stats"][f], B)
        assert (out["inlier"][f, n:] == SENT_U8).all(), f                  # rows at n and above are untouched
        assert (out["counts"][f, B:] == -1).all(), f                       # iterations the budget leaves out
        assert np.array_equal(out["sets"][f], sets[f]), f                  # draw_sets = 0: the caller's sets are read only
        if B == 0:                                                         # n < min_inliers
            assert (out["converged"][f], out["n_inliers"][f]) == (0, 0) and not out["inlier"][f, :n].any(), f
            assert (out["R12"][f] == SENT_F).all() and (out["t12"][f] == SENT_F).all() and out["s12"][f] == SENT_F, f
            assert out["stats"][f].tolist() == [0, -1, 0], f
            continue
        far = r["margins"] >= sy.DELTA
        np.testing.assert_array_equal(out["counts"][f, :B][far], r["counts"][far], err_msg="pair %d" % f)
        compared += int(far.sum()); skipped += int((~far).sum())
        assert (out["converged"][f], out["stats"][f][1], out["n_inliers"][f]) == (int(r["converged"]), r["winner"], r["n_inliers"]), \
            (f, out["converged"][f], out["stats"][f], out["n_inliers"][f], r["converged"], r["winner"], r["n_inliers"])
        np.testing.assert_array_equal(out["inlier"][f, :n], r["inlier"].astype(np.uint8), err_msg="pair %d" % f)
        assert out["stats"][f][2] == out["counts"][f, r["winner"]], f
        if r["converged"]:
            assert out["n_inliers"][f] == out["counts"][f, r["winner"]] == int(out["inlier"][f, :n].sum()), f      # the same device function
        got = np.r_[out["R12"][f], out["t12"][f], out["s12"][f]].astype(np.float64)
        d = _check_estimate(got, _rts(r), measured, "pair %d" % f)
        worst = max(worst, d)
        print("pair %2d (n = %4d): budget %3d, %s at iteration %3d, %4d inliers, distance to the model %.3e" %
              (f, n, B, "converged" if r["converged"] else "not converged", r["winner"], r["n_inliers"], d))
    print("eigh vs Jacobi in the model (measured): %.3e; largest distance to the model in (R12, t12, s12): %.3e; counts compared on %d "
          "iterations, %d within delta left to the flags" % (measured, worst, compared, skipped))


@pytest.mark.parametrize("iterations", [1, 20, 63, 64, 65, 300])
def test_iteration_counts(gpu_ctx, iterations):
    """one 129-point pair, min_inliers 30: the formula's budget is 364, so every cap up to 300 is the budget"""
    batch, _ = sy.gpu_batch_model(False, False)
    pb, sets = batch[8]
    r = m.solve(pb, sets, sy.PROBABILITY, 30, iterations, delta=sy.DELTA)
    assert r["budget"] == iterations and len(pb["X1c"]) == 129 and m.decision_is_stable(r, 30, sy.DELTA)
    out = _run(gpu_ctx, [pb], 129, iterations, 30, [sets])
    far = r["margins"] >= sy.DELTA
    np.testing.assert_array_equal(out["counts"][0][far], r["counts"][far])
    assert (out["converged"][0], out["stats"][0].tolist()[:2], out["n_inliers"][0]) == (int(r["converged"]), [iterations, r["winner"]], r["n_inliers"])
    np.testing.assert_array_equal(out["inlier"][0], r["inlier"].astype(np.uint8))
    _check_estimate(np.r_[out["R12"][0], out["t12"][0], out["s12"][0]].astype(np.float64), _rts(r), 0.0, "iterations %d" % iterations)
    # without the optional arrays: the same answers
    o2 = _run(gpu_ctx, [pb], 129, iterations, 30, [sets], stats=False, counts=False)
    assert all(out[k].tobytes() == o2[k].tobytes() for k in ("converged", "R12", "t12", "s12", "n_inliers", "inlier"))
    assert (o2["stats"] == SENT_I).all() and (o2["counts"] == SENT_I).all()


def test_device_drawn_sets(gpu_ctx):
    batch, _ = sy.gpu_batch_model(False, False)
    pbs = [batch[8][0], batch[4][0], batch[1][0], batch[9][0]]                # n = 129, 20, 2, 300
    a = _run(gpu_ctx, pbs, 300, 65, 1, None, seed=5)
    for f, pb in enumerate(pbs):
        n = len(pb["X1c"])
        s = np.sort(a["sets"][f], axis=1)
        assert np.array_equal(a["sets"][f], rs.device_sets(5, f, n, 65, 3)), f
        if n < 3:
            assert (s == -1).all(), f
        else:
            assert s.min() >= 0 and s.max() < n and (s[:, 1:] != s[:, :-1]).all(), f
            assert len(np.unique(a["sets"][f], axis=0)) > 55, f              # 65 draws, not one repeated
    b = _run(gpu_ctx, pbs, 300, 65, 1, None, seed=5)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert not np.array_equal(_run(gpu_ctx, pbs, 300, 65, 1, None, seed=6)["sets"][0], a["sets"][0])
    # the same seed gives the same sets alone and inside a larger batch (the key is (seed, pair, iteration, draw): the first pair)
    alone = _run(gpu_ctx, pbs[:1], 300, 65, 1, None, seed=5)
    assert all(alone[k][0].tobytes() == a[k][0].tobytes() for k in a)
    # fed back as the caller's sets: identical outputs byte for byte
    c = _run(gpu_ctx, pbs, 300, 65, 1, [a["sets"][f] for f in range(len(pbs))])
    assert all(a[k].tobytes() == c[k].tobytes() for k in a)
    # the sets exactly (tests/ransac_sets_model.py): n = 2 (no set), 3 and 4 (every draw meets a moved slot or the last one) and 20; 300
    # iterations take the prepare kernel's 256 threads on a second trip; seed 5 and a seed above 2^63
    ns = (2, 3, 4, 20)
    small = [dict(pbs[1], X1c=pbs[1]["X1c"][:n], X2c=pbs[1]["X2c"][:n], max1=pbs[1]["max1"][:n], max2=pbs[1]["max2"][:n]) for n in ns]
    for seed in (5, 2 ** 63 + 7):
        d = _run(gpu_ctx, small, 20, 300, 1, None, seed=seed)
        for f, n in enumerate(ns):
            assert np.array_equal(d["sets"][f], rs.device_sets(seed, f, n, 300, 3)), (seed, n)


def test_capacity_and_bad_arguments(gpu_ctx):
    import orbhip
    batch, _ = sy.gpu_batch_model(False, False)
    pb, sets = batch[5]

    def fails(code, text, **kw):
        args = dict(max_n=64, iterations=20, min_inliers=3, probability=0.99)
        args.update(kw)
        with pytest.raises(orbhip.OrbHipError) as e:
            _run(gpu_ctx, [pb], args["max_n"], args["iterations"], args["min_inliers"], [np.resize(sets, (max(args["iterations"], 1), 3))],
                 probability=args["probability"])
        assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
    fails(-4, "8192", max_n=8193)                                          # ORBHIP_E_CAPACITY, nothing launched
    fails(-4, "1024", iterations=1025)
    fails(-1, "min_inliers", min_inliers=0)                                # ORBHIP_E_BADARG with the field named
    fails(-1, "probability", probability=1.0)
    fails(-1, "probability", probability=0.0)
    p = orbhip.sim3_solver_params(0.99, 3, 0)
    c1, c2 = _cams(pb)
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.sim3_solver_device(gpu_ctx, *([8] * 5), 1, 64, c1, c2, p, *([8] * 7))
    assert e.value.code == -1 and "max_iterations" in str(e.value)
    gpu_ctx.check_status()
    # a count above max_n (or a negative one): the status word, rows untouched, the neighbours as without it
    sub, ss = [batch[5][0], batch[6][0], batch[7][0]], [batch[5][1], batch[6][1], batch[7][1]]
    good = _run(gpu_ctx, sub, 65, 40, 3, ss)
    gpu_ctx.check_status()
    for bad_n in (66, -1):
        out = _run(gpu_ctx, sub, 65, 40, 3, ss, n_override=[63, bad_n, 65])
        with pytest.raises(orbhip.OrbHipError) as e:
            gpu_ctx.check_status()
        assert e.value.code == -4
        gpu_ctx.check_status()                                             # reported once, then clear
        assert (out["inlier"][1] == SENT_U8).all() and (out["R12"][1] == SENT_F).all() and (out["t12"][1] == SENT_F).all() and out["s12"][1] == SENT_F
        assert (out["counts"][1] == SENT_I).all() and (out["converged"][1], out["n_inliers"][1], out["stats"][1].tolist()) == (0, 0, [0, -1, 0])
        for k in (0, 2):
            assert all(out[key][k].tobytes() == good[key][k].tobytes() for key in good), (bad_n, k)


@pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])
def test_host_form_equals_device_form(gpu_ctx, kb8):
    import orbhip
    batch, _ = sy.gpu_batch_model(kb8, False)
    pbs, sets = [b[0] for b in batch], [b[1] for b in batch]
    dev = _run(gpu_ctx, pbs, sy.MAX_N, sy.ITERATIONS, sy.MIN_INLIERS, sets)
    for f in (0, 1, 2, 4, 6, 8, 10, 12, 13):
        pb = pbs[f]
        n = len(pb["X1c"])
        c1, c2 = _cams(pb)
        p = orbhip.sim3_solver_params(sy.PROBABILITY, sy.MIN_INLIERS, sy.ITERATIONS, pb["fix_scale"], False)
        h = orbhip.sim3_solver_host(gpu_ctx, pb["X1c"], pb["X2c"], pb["max1"], pb["max2"], c1, c2, p, sets[f], R12=np.full(9, SENT_F), t12=np.full(3, SENT_F), s12=SENT_F)
        assert h["converged"] == bool(dev["converged"][f]) and h["n_inliers"] == dev["n_inliers"][f], f
        assert h["R12"].tobytes() == dev["R12"][f].tobytes() and h["t12"].tobytes() == dev["t12"][f].tobytes(), f
        assert np.array([h["s12"]], F32).tobytes() == dev["s12"][f:f + 1].tobytes(), f
        assert h["inlier"].tobytes() == dev["inlier"][f, :n].tobytes() and np.array_equal(h["stats"], dev["stats"][f]), f
        if dev["stats"][f][0]:
            assert np.array_equal(h["counts"], dev["counts"][f]), f
    # device-drawn sets come back through the host form too
    p = orbhip.sim3_solver_params(sy.PROBABILITY, 6, 40, False, True, 11)
    c1, c2 = _cams(pbs[8])
    h = orbhip.sim3_solver_host(gpu_ctx, pbs[8]["X1c"], pbs[8]["X2c"], pbs[8]["max1"], pbs[8]["max2"], c1, c2, p)
    d = _run(gpu_ctx, [pbs[8]], 129, 40, 6, None, seed=11)
    assert np.array_equal(h["sets"], d["sets"][0]) and h["n_inliers"] == d["n_inliers"][0] and h["R12"].tobytes() == d["R12"][0].tobytes()


# ------------------------------------------------------------------ the class
def _libc_randint():
    """DUtils::Random::RandomInt(0, d - 1) on libc's rand() in the state a process starts in (the reference seeds it nowhere for this class)"""
    libc = ctypes.CDLL(None)
    libc.srand(1)
    return lambda d: int((libc.rand() / (2147483647 + 1.0)) * d)


@pytest.mark.parametrize("scene", sorted(sy.CLASS_SCENES))
def test_class_drop_in(tmp_path, scene):
    """lib/host_sim3solver_smoke: ~150 matches with bad and missing map points and map points without keypoint in KF2; LoopClosing's
    iterate(20, ...) loop and, on two of the scenes, find() in a process of its own -- each on rand()'s unseeded stream -- against the
    model's chunked run."""
    spec = sy.CLASS_SCENES[scene]
    sc = sy.make_scene(**spec)
    pb, index, n1 = sy.class_problem(sc)                                   # the constructor's gathering, restated
    N = len(index)
    assert 90 <= N <= 150 and (sc["kf1_mp"] < 0).any() and (sc["matches"] < 0).any() and sc["mp_bad"].any()
    assert bool(len(sc["matched_kf"])) == spec["matched_kf"] and (not spec["matched_kf"] or (sc["matched_kf"] == 3).any())
    mi, it = int(sc["min_inliers"][0]), int(sc["max_iterations"][0])
    budget = m.iteration_budget(N, 0.99, mi, it)
    sets = m.draw_sets_reference(N, budget, _libc_randint())               # 3 * mRansacMaxIts draws at once
    res = m.solve(pb, sets, 0.99, mi, it, delta=sy.DELTA)                  # the preconditions of the comparison, on this scene
    assert (res["margins"] < sy.DELTA).mean() <= 0.05 and m.decision_is_stable(res, mi, sy.DELTA)
    assert res["converged"] == (not spec.get("outliers_only", False))
    measured = _measured_solver_distance([(pb, sets)], [res])
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    sy.s3.write_flat(fin, sc)
    for mode, pre in (("loop", ""), ("find", "find_")):
        if mode == "find" and scene not in ("own_keyframe", "not_converging"):
            continue
        cs = m.ChunkedSolver(pb, sets, n1, index, 0.99, mi, it)
        calls, ret_empty = 0, []
        while True:
            want = cs.iterate(20) if mode == "loop" else cs.find()
            calls += 1; ret_empty.append(int(want["T12"] is None))
            if mode == "find" or want["converged"] or want["no_more"]:
                break
        r = subprocess.run([EXE, fin, fout, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        out = sy.s3.read_flat(fout)
        assert np.array_equal(out[pre + "sets"].reshape(-1, 3), sets), (scene, mode)
        if mode == "loop":
            assert (out["converged"][0], out["no_more"][0], out["calls"][0]) == (int(want["converged"]), int(want["no_more"]), calls)
            assert out["ret_empty"].tolist() == ret_empty
        assert out[pre + "n_inliers"][0] == want["n_inliers"]
        np.testing.assert_array_equal(out[pre + "inliers"].astype(bool), want["inliers"])
        R, t, s = cs.estimated()
        d = _check_estimate(np.r_[out[pre + "R"], out[pre + "t"], out[pre + "s"]].astype(np.float64), _rts(dict(R12=R, t12=t, s12=s)), measured, scene + mode)
        T = out[pre + "T"]
        T_want = want["T12"] if (mode == "loop" or want["converged"]) else None  # find() is the overload that returns nothing short of convergence
        assert (T.size == 0) == (T_want is None), (scene, mode)
        if T_want is not None and np.isfinite(T_want).all():
            ulp = float(np.spacing(F32(np.abs(T_want).max())))
            # one more float product (s * R) on each side: an ulp of R, one of s, half of the product
            assert np.abs(T.astype(np.float64) - T_want.reshape(-1)).max() <= max(8 * measured, 3 * ulp)
        print("%s %s: %d correspondences, %s after %d iterations in %d calls, %d inliers, distance to the model %.3e (measured eigh vs Jacobi %.3e)" %
              (scene, mode, N, "converged" if want["converged"] else "not converged", cs.iterations, calls, want["n_inliers"], d, measured))


# ------------------------------------------------------------------ match -> solve -> refine on one stream
def _quat_from_R(R, sqrt):
    """Eigen::Quaterniond(R), the trace branch (rotations well below 90 degrees): (x, y, z, w)"""
    t = sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0)
    w = 0.5 * t
    t = 0.5 / t
    return [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t, w]


def test_chain_bow_solver_refine():
    """search_by_bow_kf_device, a torch gather of the matched points, sim3_solver_device and optimize_sim3_device on ONE context whose
    stream is torch's: nothing waits on the host between them.  The model chain: the matcher's oracle, the float32 solver model, the
    analytic OptimizeSim3 model; the refined Sim3 within that test's bound (1e-9)."""
    import torch
    import orbhip
    import oracle_match_bind as om
    import sim3_opt_model as opt
    rng = np.random.default_rng(91)
    c = om.make_bow_case(rng, 400, 420, 60)
    c["valid2"] = np.ones(len(c["kp_f"]), np.uint8)
    n_ref, m_ref = om.search_by_bow_kf(c, 0.75, True)
    nk, nf = len(c["kp_k"]), len(c["kp_f"])
    matched = np.nonzero(m_ref[:nk] >= 0)[0]
    assert n_ref == len(matched) >= 60
    # geometry consistent with the matches: KF1's keypoint i sees X1c[i]; its match sees the same point through the true Sim3
    pb = sy.make_pair(92, nk, outlier_share=0.25)
    X1 = pb["X1c"]; X2 = np.zeros((nf, 3), F32); X2[:, 2] = 5
    X2[m_ref[matched]] = pb["X2c"][matched]
    cam = sy.camera()
    r = np.random.RandomState(93)
    obs1 = (opt.project_smooth(cam, X1.astype(np.float64)) + 0.5 * r.normal(size=(nk, 2))).astype(F32).astype(np.float64)
    obs2 = (opt.project_smooth(cam, X2.astype(np.float64)) + 0.5 * r.normal(size=(nf, 2))).astype(F32).astype(np.float64)
    MIN_INL, ITS, MN, MNODE = 20, 300, 512, 2048
    # ---- the model chain
    g1, g2 = X1[matched], X2[m_ref[matched]]
    spb = dict(X1c=g1, X2c=g2, max1=np.full(len(matched), 9.0, F32), max2=np.full(len(matched), 9.0, F32), cam1=cam, cam2=cam, fix_scale=False)
    sets = sy.host_sets(94, len(matched), ITS)
    sref = m.solve(spb, sets, 0.99, MIN_INL, ITS, delta=sy.DELTA)
    assert sref["converged"] and m.decision_is_stable(sref, MIN_INL, sy.DELTA)
    R64 = sref["R12"].astype(np.float64)
    S0 = np.array(_quat_from_R(R64, np.sqrt) + list(sref["t12"].astype(np.float64)) + [float(sref["s12"])])
    oref = opt.solve(dict(P1c=g1.astype(np.float64), P2c=g2.astype(np.float64), obs1=obs1[matched], obs2=obs2[m_ref[matched]], w1=np.ones(len(matched)),
                          w2=np.ones(len(matched)), cam1=cam, cam2=cam, th2=10.0, fix_scale=False, sim3=S0))
    assert oref["iters2"] > 0 and oref["margin"] > 1e-6
    # ---- the device chain
    s = torch.cuda.Stream()
    ctx = orbhip.Context(0, s.cuda_stream)
    try:
        ki, ks, kf = om.feature_vector_csr(c["nid_k"]); fi, fs, ff = om.feature_vector_csr(c["nid_f"])
        pad = lambda a, k, dt: np.r_[np.asarray(a, dt), np.zeros(k - len(a), dt)]
        host = dict(ki=pad(ki, MNODE, np.int32), ks=pad(ks, MNODE + 1, np.int32), kf=pad(kf, MN, np.int32), kn=np.array([len(ki)], np.int32),
                    fi=pad(fi, MNODE, np.int32), fs=pad(fs, MNODE + 1, np.int32), ff=pad(ff, MN, np.int32), fn=np.array([len(fi)], np.int32),
                    va=pad(c["valid"], MN, np.uint8), vb=pad(c["valid2"], MN, np.uint8), n1=np.array([nk], np.int32), n2=np.array([nf], np.int32))
        kpk = np.zeros(MN, orbhip.KP_DTYPE); kpk[:nk] = c["kp_k"]; kpf = np.zeros(MN, orbhip.KP_DTYPE); kpf[:nf] = c["kp_f"]
        dk = np.zeros((MN, 32), np.uint8); dk[:nk] = c["d_k"]; df = np.zeros((MN, 32), np.uint8); df[:nf] = c["d_f"]
        host.update(kpk=kpk.view(np.uint8), kpf=kpf.view(np.uint8), dk=dk, df=df)
        pad3 = lambda a, w, dt: np.r_[np.asarray(a, dt), np.zeros((MN - len(a), w), dt)]
        host.update(X1=pad3(X1, 3, F32), X2=pad3(X2, 3, F32), o1=pad3(obs1, 2, np.float64), o2=pad3(obs2, 2, np.float64), sets=sets[None])
        with torch.cuda.stream(s):
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
            m12 = torch.full((1, MN), -1, dtype=torch.int32, device="cuda"); nm = torch.zeros(1, dtype=torch.int32, device="cuda")
            orbhip.search_by_bow_kf_device(ctx, [t[k].data_ptr() for k in ("ki", "ks", "kf", "kn", "va", "kpk", "dk", "n1")],
                                           [t[k].data_ptr() for k in ("fi", "fs", "ff", "fn", "vb", "kpf", "df", "n2")], 1, MNODE, MN, MN, 0.75, True,
                                           m12.data_ptr(), nm.data_ptr())
            # the gather: matched rows first, in keypoint order (a stable sort, no host-side count)
            mm = m12[0]
            ok = (mm >= 0) & (torch.arange(MN, device="cuda") < nk)
            order = torch.argsort((~ok).to(torch.int8), stable=True)
            j = mm.clamp(min=0).long()[order]
            n = ok.sum().to(torch.int32).reshape(1)
            gX1 = t["X1"][order].contiguous().reshape(1, MN, 3); gX2 = t["X2"][j].contiguous().reshape(1, MN, 3)
            thr = torch.full((1, MN), 9.0, dtype=torch.float32, device="cuda")
            conv = torch.zeros(1, dtype=torch.uint8, device="cuda"); R = torch.zeros(1, 9, device="cuda"); tt = torch.zeros(1, 3, device="cuda")
            sc = torch.zeros(1, device="cuda"); nin = torch.zeros(1, dtype=torch.int32, device="cuda"); inl = torch.zeros(1, MN, dtype=torch.uint8, device="cuda")
            c1 = orbhip.sim3_camera(cam["K"], None)
            orbhip.sim3_solver_device(ctx, gX1.data_ptr(), gX2.data_ptr(), thr.data_ptr(), thr.data_ptr(), n.data_ptr(), 1, MN, c1, c1,
                                      orbhip.sim3_solver_params(0.99, MIN_INL, ITS, False, False), t["sets"].data_ptr(), conv.data_ptr(), R.data_ptr(),
                                      tt.data_ptr(), sc.data_ptr(), nin.data_ptr(), inl.data_ptr())
            # (R12, t12, s12) -> g2o::Sim3, in double on the device
            Rd = R.double().reshape(3, 3)
            sim3 = torch.stack(_quat_from_R(Rd, torch.sqrt) + [tt[0, 0].double(), tt[0, 1].double(), tt[0, 2].double(), sc[0].double()]).reshape(1, 8).contiguous()
            P1 = gX1.double().contiguous(); P2 = gX2.double().contiguous()
            o1 = t["o1"][order].contiguous(); o2 = t["o2"][j].contiguous()
            w = torch.ones(1, MN, dtype=torch.float64, device="cuda")
            flag = torch.zeros(1, MN, dtype=torch.uint8, device="cuda"); nopt = torch.zeros(1, dtype=torch.int32, device="cuda")
            orbhip.optimize_sim3_device(ctx, P1.data_ptr(), P2.data_ptr(), o1.data_ptr(), o2.data_ptr(), w.data_ptr(), w.data_ptr(), n.data_ptr(), 1, MN,
                                        c1, c1, 10.0, False, sim3.data_ptr(), flag.data_ptr(), nopt.data_ptr(), None)
        ctx.synchronize()                                                  # the first and only wait on the host
        ctx.check_status()
        assert int(n.item()) == len(matched) and int(conv.item()) == 1 and int(nin.item()) == sref["n_inliers"]
        got0 = np.r_[R.cpu().numpy().reshape(9), tt.cpu().numpy().reshape(3), sc.cpu().numpy()].astype(np.float64)
        d0 = np.abs(got0 - _rts(sref)).max()
        S = sim3.cpu().numpy()[0]
        dq = min(np.abs(S[:4] - oref["sim3"][:4]).max(), np.abs(S[:4] + oref["sim3"][:4]).max())
        d = max(dq, np.abs(S[4:] - oref["sim3"][4:]).max())
        print("chain: %d matches, solver: %d inliers, distance to the model %.3e; refined: nIn %d (model %d), distance %.3e" %
              (len(matched), int(nin.item()), d0, int(nopt.item()), oref["n_in"], d))
        assert int(nopt.item()) == oref["n_in"] and np.array_equal(flag.cpu().numpy()[0, :len(matched)], oref["flag"])
        assert d <= 1e-9
    finally:
        ctx.close()
