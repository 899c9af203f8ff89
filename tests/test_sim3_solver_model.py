"""CPU tests of the Sim3Solver model (tests/sim3_solver_model.py) and the PRECONDITIONS of the GPU comparison
(tests/test_gpu_sim3_solver.py), evaluated on the committed batch (tests/synth_sim3_solver.py).  The preconditions are checks, not knobs: a
batch seed that violates one is replaced, never delta.

delta = 1e-3: one float ulp in a transform entry moves a point of ~10 m by ~1e-6 m, ~2e-4 px at f ~ 458 and z >= 2; on the 3 px residual
of the smallest threshold (9) that is ~1.5e-4 relative in the error; delta is ~7 times that."""
import numpy as np
import pytest

import sim3_solver_model as m
import synth_sim3_solver as sy

KEYS = [(False, False), (False, True), (True, False), (True, True)]
IDS = ["pinhole-free_scale", "pinhole-fix_scale", "kb8-free_scale", "kb8-fix_scale"]


def _angle(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.astype(np.float64).T @ Rb) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])
def test_recovers_the_true_sim3_on_noise_free_data(kb8):
    pb = sy.make_pair(11, 60, kb8=kb8, noise=0.0, outlier_share=0.3)
    inl = np.nonzero(~pb["outlier_true"])[0]
    sets = sy.host_sets(12, 60, 40, inl, 1.0)
    r = m.solve(pb, sets, min_inliers=6, max_iterations=40)
    assert r["converged"] and r["winner"] == 0 and r["n_inliers"] == len(inl)
    assert np.array_equal(r["inlier"], ~pb["outlier_true"])
    assert _angle(r["R12"], pb["R_true"]) < 1e-2 and np.abs(r["t12"] - pb["t_true"]).max() < 1e-3 and abs(r["s12"] - pb["s_true"]) < 1e-4


def test_fix_scale_gives_a_scale_of_exactly_one():
    pb = sy.make_pair(21, 40, fix_scale=True)
    r = m.solve(pb, sy.host_sets(22, 40, 30), max_iterations=30)
    assert all(h["s12"] == np.float32(1.0) for h in r["hyps"])
    pb = sy.make_pair(21, 40, fix_scale=False)
    r = m.solve(pb, sy.host_sets(22, 40, 30), max_iterations=30)
    assert all(h["s12"] != np.float32(1.0) for h in r["hyps"])


def test_thresholds_are_truncated_as_a_vector_of_size_t_truncates_them():
    assert m.truncated_threshold(1.44) == 13.0 and 9.210 * 1.44 > 13.2
    assert [m.truncated_threshold(v) for v in sy.SIGMA2] == [9.0, 13.0, 19.0, 27.0, 39.0, 57.0, 82.0, 118.0]
    # err < max compares the float error with that integer: 13.1 is no inlier at sigma^2 = 1.44
    pb = dict(X1c=np.array([[0, 0, 5]], np.float32), X2c=np.array([[0, 0, 5]], np.float32), max1=np.array([13.0], np.float32),
              max2=np.array([13.0], np.float32), cam1=sy.camera(), cam2=sy.camera(), fix_scale=True)
    p1, p2 = m.prepare(pb)
    shift = np.float32(np.sqrt(13.1) * 5 / sy.s3.K_VGA[0])
    hyp = dict(sR12=np.eye(3, dtype=np.float32), t12=np.array([shift, 0, 0], np.float32), sR21=np.eye(3, dtype=np.float32), t21=np.array([-shift, 0, 0], np.float32))
    inl, _, (e1, e2) = m.check_inliers(pb, hyp, p1, p2)
    assert 13.0 < e1[0] < 13.26 and not inl[0]


def test_scan_rule_ties_go_to_the_later_iteration_and_the_first_count_above_min_inliers_converges():
    assert m.scan([2, 5, 5, 3], 6) == (False, 2)
    assert m.scan([0, 0, 0], 6) == (False, 2)                               # 0 >= 0: even an empty hypothesis becomes the best
    assert m.scan([6, 6, 7, 9], 6) == (True, 2)                             # 6 is not above 6; 7 is, and 9 is never looked at
    assert m.scan([7], 6) == (True, 0)
    assert m.scan([5, 6, 4, 6, 1], 6) == (False, 3)


@pytest.mark.parametrize("case", ["converging", "not_converging"])
def test_running_in_chunks_of_20_equals_one_find(case):
    pb = sy.make_pair(31, 80, outlier_share=0.5, mode="outliers_only" if case == "not_converging" else None)
    sets = sy.host_sets(32, 80, 300)
    idx = np.arange(80) * 2
    a = m.ChunkedSolver(pb, sets, 160, idx, min_inliers=30)
    b = m.ChunkedSolver(pb, sets, 160, idx, min_inliers=30)
    ra, calls = m.loop_closing_run(a, 20)
    rb = b.find()
    assert ra["converged"] == rb["converged"] == (case == "converging") and ra["n_inliers"] == rb["n_inliers"]
    assert np.array_equal(ra["inliers"], rb["inliers"]) and a.best == b.best and a.iterations == b.iterations
    assert calls == (a.iterations + 19) // 20 and (a.iterations == a.max_its) == ra["no_more"]
    assert all(np.array_equal(x, y) for x, y in zip(a.estimated(), b.estimated()))
    if case == "converging":
        assert np.array_equal(ra["T12"], rb["T12"]) and ra["inliers"][1::2].sum() == 0 and ra["inliers"].sum() == ra["n_inliers"] > 30
    else:
        assert a.max_its == 86 and calls == 5 and ra["no_more"]      # ceil(4.60517 / 0.0541756) = ceil(85.005)
        assert ra["T12"] is None or ra["T12"].shape == (4, 4)
        assert not ra["inliers"].any() and a.best == m.scan(a.res["counts"], 30)[1]


def test_iteration_budget_formula_and_its_saturation():
    assert m.iteration_budget(5, 0.99, 6, 300) == 0                         # N < minInliers: bNoMore
    assert m.iteration_budget(6, 0.99, 6, 300) == 1                         # minInliers == N
    assert m.iteration_budget(4, 0.99, 3, 300) == 9                         # ceil(log(0.01) / log(1 - 0.75^3)) = ceil(8.41)
    assert m.iteration_budget(12, 0.99, 6, 300) == 35                       # epsilon = 0.5: ceil(34.5)
    assert m.iteration_budget(100, 0.99, 15, 300) == 300                    # 1363 capped
    assert m.iteration_budget(100, 0.99, 15, 5000) == 1363
    assert m.iteration_budget(8192, 0.99, 1, 1024) == 1024                  # the quotient (2.5e12) is beyond int: saturates to the cap
    assert m.iteration_budget(8192, 0.5, 1, 7) == 7
    assert m.iteration_budget(3, 0.99, 2, 300) == 14                        # epsilon = 2/3: ceil(4.60517 / 0.35140) = ceil(13.1)


def test_the_jacobi_solver_and_eigh_give_the_same_rotations():
    worst = 0.0
    for seed in range(6):
        pb = sy.make_pair(40 + seed, 50, fix_scale=bool(seed & 1))
        for s in sy.host_sets(60 + seed, 50, 40):
            a = m.horn(pb["X1c"][s], pb["X2c"][s], pb["fix_scale"], "jacobi")
            b = m.horn(pb["X1c"][s], pb["X2c"][s], pb["fix_scale"], "eigh")
            d = max(np.abs(a[k].astype(np.float64) - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in ("R12", "t12", "s12", "sR12", "sR21", "t21"))
            worst = max(worst, d)
    print("jacobi vs eigh after rounding to float: %.3g relative" % worst)
    assert worst <= 8 * np.finfo(np.float32).eps


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_preconditions_of_the_gpu_comparison(key):
    batch, res = sy.gpu_batch_model(*key)
    assert [len(pb["X1c"]) for pb, _ in batch] == [0, 2, 3, 4, 20, 63, 64, 65, 129, 300, sy.LDS_MAX + 1, 40, 10, 20]
    # the cases the batch is there for
    assert [r["budget"] for r in res[:4]] == [0, 0, 1, 9] and not res[2]["converged"]
    assert (batch[11][0]["X2c"][:, 2] < 0).all() and res[11]["converged"]                       # behind camera 2: no z test anywhere
    assert not res[12]["converged"] and not res[12]["counts"].any() and np.isnan(res[12]["s12" if not key[1] else "t12"]).all()
    assert res[12]["winner"] == res[12]["budget"] - 1
    assert not res[13]["converged"] and res[13]["counts"].max() <= sy.MIN_INLIERS and res[13]["winner"] >= 0
    for k, r in enumerate(res):
        if not r["budget"]:
            continue
        near = int((r["margins"] < sy.DELTA).sum())
        print("pair %d: %d of %d iterations within %g of a threshold" % (k, near, r["budget"], sy.DELTA))
        assert near <= 0.05 * r["budget"], k                                 # (a): a cap
        assert m.decision_is_stable(r, sy.MIN_INLIERS, sy.DELTA), k          # (b)


def test_float32_and_float64_scoring_count_the_same_away_from_the_thresholds():
    batch, res = sy.gpu_batch_model(True, False)
    for k in (5, 8, 9, 11):
        pb, sets = batch[k]
        r64 = m.solve(pb, sets, sy.PROBABILITY, sy.MIN_INLIERS, sy.ITERATIONS, f64=True)
        far = res[k]["margins"] >= sy.DELTA
        assert np.array_equal(r64["counts"][far], res[k]["counts"][far]), k
        assert (r64["converged"], r64["winner"]) == (res[k]["converged"], res[k]["winner"])
