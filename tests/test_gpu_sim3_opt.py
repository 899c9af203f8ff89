"""HIP-vs-model parity of the batched Sim3 refinement (Optimizer::OptimizeSim3), through the C ABI, the host form and the class method.
The yardstick is the ANALYTIC numpy model (tests/sim3_opt_model.py): flags, return values, nCorrespondences and nBad identical, (q up
to sign, t, s) within 1e-9 -- the bar tests/test_gpu_pose.py sets for this LM (only the order of the sums differs).  The preconditions
of that comparison (no decisive chi2 near th2, insensitivity to the summation order) are checked on the model in
tests/test_sim3_opt_model.py."""
import os
import subprocess
import numpy as np
import pytest

import synth_sim3 as s

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_sim3_smoke")
SENT = 9                                                       # flag rows the kernel must not touch keep this value
_model_cache = {}


def _model(kb8, fix_scale):
    """the analytic model on the committed batch: computed once, shared, never modified"""
    import sim3_opt_model as m
    key = (kb8, fix_scale)
    if key not in _model_cache:
        probs = s.gpu_batch(kb8, fix_scale)
        _model_cache[key] = (probs, [m.solve(p) for p in probs])
    return _model_cache[key]


def _cams(p):
    import orbhip
    return orbhip.sim3_camera(p["cam1"]["K"], p["cam1"]["kb8"]), orbhip.sim3_camera(p["cam2"]["K"], p["cam2"]["kb8"])


def _run(gpu_ctx, probs, max_edges, n_override=None, stats=True):
    """-> sim3 [P][8], flag [P][max_edges], n_in [P], stats [P][4] (device form)"""
    import torch
    import orbhip
    P = len(probs)
    A = dict(P1c=np.zeros((P, max_edges, 3)), P2c=np.zeros((P, max_edges, 3)), obs1=np.zeros((P, max_edges, 2)), obs2=np.zeros((P, max_edges, 2)),
             w1=np.zeros((P, max_edges)), w2=np.zeros((P, max_edges)))
    n = np.array([len(p["P1c"]) for p in probs], np.int32)
    for f, p in enumerate(probs):
        k = min(n[f], max_edges)
        for key in A:
            A[key][f, :k] = np.asarray(p[key])[:k]
    if n_override is not None:
        n = np.asarray(n_override, np.int32)
    sim3 = np.stack([p["sim3"] for p in probs]).astype(np.float64)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in A.items()}
    dn = torch.from_numpy(n).cuda(); ds = torch.from_numpy(sim3).cuda()
    flag = torch.full((P, max_edges), SENT, dtype=torch.uint8, device="cuda")
    nin = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    st = torch.full((P, 4), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c1, c2 = _cams(probs[0])
    orbhip.optimize_sim3_device(gpu_ctx, t["P1c"].data_ptr(), t["P2c"].data_ptr(), t["obs1"].data_ptr(), t["obs2"].data_ptr(), t["w1"].data_ptr(),
                                t["w2"].data_ptr(), dn.data_ptr(), P, max_edges, c1, c2, probs[0]["th2"], probs[0]["fix_scale"], ds.data_ptr(),
                                flag.data_ptr(), nin.data_ptr(), st.data_ptr() if stats else None)
    gpu_ctx.synchronize()
    return ds.cpu().numpy(), flag.cpu().numpy(), nin.cpu().numpy(), st.cpu().numpy()


def _dist(a, b):
    dq = min(np.abs(a[:4] - b[:4]).max(), np.abs(a[:4] + b[:4]).max())
    return max(dq, np.abs(a[4:] - b[4:]).max())


@pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])
@pytest.mark.parametrize("fix_scale", [False, True], ids=["free_scale", "fix_scale"])
def test_batch_matches_the_analytic_model(gpu_ctx, kb8, fix_scale):
    """n = 0, 9, 10, 12 with 3 gross outliers (pass 1 leaves 9: answers 0, Sim3 untouched, flags 1 set), 63, 64, 65, 129, 300, a pair
    whose every row has z < 0, n = max_edges = 512.  No case is left out of the comparison."""
    probs, ref = _model(kb8, fix_scale)
    assert [len(p["P1c"]) for p in probs] == [0, 9, 10, 12, 63, 64, 65, 129, 300, 40, 512]
    assert (ref[3]["n_corr"], ref[3]["n_bad"], ref[3]["n_in"]) == (12, 3, 0) and (ref[9]["n_corr"], ref[9]["flag"].tolist()) == (0, [3] * 40)
    sim3, flag, nin, st = _run(gpu_ctx, probs, s.MAX_EDGES)
    worst = 0.0
    for f, (p, r) in enumerate(zip(probs, ref)):
        n = len(p["P1c"])
        np.testing.assert_array_equal(flag[f, :n], r["flag"], err_msg="pair %d" % f)
        assert (flag[f, n:] == SENT).all(), f                              # rows at index n and above are untouched
        assert (nin[f], st[f][0], st[f][1]) == (r["n_in"], r["n_corr"], r["n_bad"]), (f, nin[f], st[f], r["n_in"], r["n_corr"], r["n_bad"])
        if r["iters2"] == 0:
            assert sim3[f].tobytes() == np.asarray(p["sim3"], np.float64).tobytes(), f      # the early 0: g2oS12 is not written
        else:
            d = _dist(sim3[f], r["sim3"])
            worst = max(worst, d)
            print("pair %d (n = %d): distance to the model %.3e, LM iterations %d / trials %d (model %d / %d)" %
                  (f, n, d, st[f][2], st[f][3], r["lm_iters"], r["lm_trials"]))
            assert d <= 1e-9, (f, d)
        # LM iteration and trial counts are bounded, not compared (tests/test_gpu_pose.py:58-63: the sign of rho of a zero-progress
        # trial depends on the summation order): at most 5 + 10 iterations, each with 1..100 trials
        if r["n_corr"] == 0:
            assert (st[f][2], st[f][3]) == (0, 0)
        else:
            assert 1 <= st[f][2] <= (15 if r["iters2"] else 5) and st[f][2] <= st[f][3] <= 100 * st[f][2], (f, st[f])
    print("largest distance to the model in (q, t, s): %.3e" % worst)


def test_alone_and_in_the_batch_and_twice_bit_identical(gpu_ctx):
    probs, _ = _model(False, False)
    a = _run(gpu_ctx, probs, s.MAX_EDGES)
    b = _run(gpu_ctx, probs, s.MAX_EDGES)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for f in (4, 8):
        one = _run(gpu_ctx, [probs[f]], s.MAX_EDGES)
        for x, y in zip(one, a):
            assert x[0].tobytes() == y[f].tobytes(), f
    # without the optional stats array: the same answers
    c = _run(gpu_ctx, probs, s.MAX_EDGES, stats=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], c[:3])) and (c[3] == -9).all()


def test_oversized_pair_sets_the_status_word_and_writes_nothing_outside_its_row(gpu_ctx):
    import orbhip
    probs, _ = _model(False, False)
    sub = [probs[4], probs[5], probs[6]]
    good = _run(gpu_ctx, sub, 128)
    gpu_ctx.check_status()
    sim3, flag, nin, st = _run(gpu_ctx, sub, 128, n_override=[63, 129, 65])
    with pytest.raises(orbhip.OrbHipError) as e:
        gpu_ctx.check_status()
    assert e.value.code == -4                                              # ORBHIP_E_CAPACITY
    gpu_ctx.check_status()                                                 # reported once, then clear
    assert (flag[1] == SENT).all() and sim3[1].tobytes() == np.asarray(sub[1]["sim3"], np.float64).tobytes()
    assert nin[1] == 0 and (st[1] == 0).all()
    for k in (0, 2):
        assert sim3[k].tobytes() == good[0][k].tobytes() and flag[k].tobytes() == good[1][k].tobytes() and nin[k] == good[2][k]


def test_negative_count_sets_the_status_word_and_writes_nothing(gpu_ctx):
    import orbhip
    probs, _ = _model(False, False)
    sub = [probs[4], probs[5]]
    good = _run(gpu_ctx, sub, 128)
    gpu_ctx.check_status()
    sim3, flag, nin, st = _run(gpu_ctx, sub, 128, n_override=[-1, 64])
    with pytest.raises(orbhip.OrbHipError) as e:
        gpu_ctx.check_status()
    assert e.value.code == -4
    assert (flag[0] == SENT).all() and sim3[0].tobytes() == np.asarray(sub[0]["sim3"], np.float64).tobytes() and nin[0] == 0 and (st[0] == 0).all()
    assert sim3[1].tobytes() == good[0][1].tobytes() and flag[1].tobytes() == good[1][1].tobytes() and nin[1] == good[2][1]


def test_more_than_8192_edges_is_a_capacity_error(gpu_ctx):
    import orbhip
    probs, _ = _model(False, False)
    with pytest.raises(orbhip.OrbHipError) as e:
        import torch
        z = torch.zeros(64, dtype=torch.float64, device="cuda")
        c1, c2 = _cams(probs[1])
        orbhip.optimize_sim3_device(gpu_ctx, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 8193,
                                    c1, c2, 10.0, False, z.data_ptr(), z.data_ptr(), z.data_ptr(), None)
    assert e.value.code == -4                                              # ORBHIP_E_CAPACITY, nothing launched


@pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])
def test_host_form_equals_device_form_bit_for_bit(gpu_ctx, kb8):
    import orbhip
    probs, _ = _model(kb8, False)
    dev = _run(gpu_ctx, probs, s.MAX_EDGES)
    for f, p in enumerate(probs):
        c1, c2 = _cams(p)
        sim3, flag, nin, st = orbhip.optimize_sim3_host(gpu_ctx, p["P1c"], p["P2c"], p["obs1"], p["obs2"], p["w1"], p["w2"], c1, c2, p["th2"],
                                                        p["fix_scale"], p["sim3"])
        n = len(p["P1c"])
        assert sim3.tobytes() == dev[0][f].tobytes() and flag.tobytes() == dev[1][f, :n].tobytes() and nin == dev[2][f], f
        assert np.array_equal(st, dev[3][f]), (f, st, dev[3][f])


def test_golden(gpu_ctx):
    """Committed fixture (four small pairs with the analytic model's outputs), compared without importing the model."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sim3_opt_golden.npz"))
    for k in range(int(g["count"])):
        rows, meta = g["rows%d" % k].astype(np.float64), g["meta%d" % k]          # layouts: tools/gen_sim3_golden.py
        cam = dict(K=tuple(meta[:4]), kb8=None if np.isnan(meta[4]) else tuple(meta[4:8]))
        p = dict(P1c=rows[:, 0:3], P2c=rows[:, 3:6], obs1=rows[:, 6:8], obs2=rows[:, 8:10], w1=rows[:, 10], w2=rows[:, 11],
                 cam1=cam, cam2=cam, th2=float(meta[8]), fix_scale=bool(meta[9]), sim3=meta[10:18])
        sim3, flag, nin, st = _run(gpu_ctx, [p], 128)
        n = len(rows)
        np.testing.assert_array_equal(flag[0, :n], g["flag%d" % k])
        assert [nin[0], st[0][0], st[0][1]] == [int(v) for v in meta[26:29]]
        assert _dist(sim3[0], meta[18:26]) <= 1e-9, (k, _dist(sim3[0], meta[18:26]))


# ------------------------------------------------------------------ the class method
@pytest.mark.parametrize("scene", sorted(s.CLASS_SCENES))
def test_class_method_on_two_stand_in_keyframes(tmp_path, scene):
    """lib/host_sim3_smoke: ~150 map points, some i2 < 0, bad and missing map points: vpMatches1's NULL pattern, the return value and
    g2oS12 against the model on the restated edge loop; mAcumHessian all zero."""
    import sim3_opt_model as m
    spec = s.CLASS_SCENES[scene]
    sc = s.make_keyframes(**spec)
    pb, index, n_no_kp2 = s.class_problem(sc)                             # the independent restatement of src/Optimizer.cc:4007-4233
    assert 90 <= len(index) <= 150 and (n_no_kp2 >= 10 if spec["all_points"] else n_no_kp2 == 0), (len(index), n_no_kp2)
    assert (sc["kf1_mp"] < 0).any() and (sc["matches"] < 0).any() and sc["mp_bad"].any()
    ref = m.solve(pb)
    assert ref["margin"] > 1e-6 and ref["iters2"] > 0 and ref["n_bad"] > 0
    fin, fout = str(tmp_path / "a.in"), str(tmp_path / "a.out")
    s.write_flat(fin, sc)
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = s.read_flat(fout)
    expect_null = (sc["matches"] < 0)
    expect_null[index[(ref["flag"] == 1) | (ref["flag"] == 2)]] = True
    np.testing.assert_array_equal(out["matches_null"].astype(bool), expect_null)
    assert out["ret"][0] == ref["n_in"]
    d = _dist(out["sim3"].view(np.float64), ref["sim3"])
    print("class method: %d rows, nIn %d, distance to the model %.3e" % (len(index), ref["n_in"], d))
    assert d <= 1e-9
    assert not out["hessian"].view(np.float64).any()
