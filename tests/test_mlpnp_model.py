"""CPU tests of the numpy model of MLPnPsolver (tests/mlpnp_model.py) on the committed batch (tests/synth_mlpnp.py): it recovers the true
poses, its Jacobian is the derivative, its planar rule and budget are the reference's, and the preconditions of the GPU comparison
(tests/test_gpu_mlpnp.py) hold: on every iteration that bears on a decision no error lies within delta = 1e-3 (relative) of its threshold,
and every decomposition variant of the model takes the same decisions with the same counts.  A seed that breaks a precondition is
replaced in tests/synth_mlpnp.py; delta stays."""
import numpy as np
import pytest

import mlpnp_model as m
import synth_mlpnp as sy

KB8 = pytest.mark.parametrize("kb8", [False, True], ids=["pinhole", "kb8"])


def _all(kb8):
    for grp, cands, ress in sy.gpu_batch_model(kb8):
        for (pb, sets), r in zip(cands, ress):
            yield grp, pb, sets, r


def test_ransac_parameters():
    """SetRansacParameters (:218-253) on the sizes of the batch"""
    assert m.ransac_parameters(6, min_inliers=6) == (6, 1)                      # nMin == N: one iteration
    assert m.ransac_parameters(9, min_inliers=10, epsilon=0.5) == (10, 0)       # N < nMin: bNoMore at once
    assert m.ransac_parameters(20, min_inliers=10, epsilon=0.5) == (10, 35)     # ceil(log(0.01) / log(1 - 0.5^3))
    assert m.ransac_parameters(200) == (80, 70) and m.ransac_parameters(15) == (8, 28)
    assert m.ransac_parameters(200, max_iterations=50) == (80, 50)


def test_planar_rule():
    """rank 2 exactly for points in a plane through the origin (one coordinate exactly zero); a thin slab is not planar"""
    r = np.random.RandomState(5)
    X = r.uniform(-3, 3, (30, 3))
    assert m.fullpiv_rank(X.T @ X) == 3
    X[:, 2] = 0.0
    assert m.fullpiv_rank(X.T @ X) == 2
    X[:, 2] = 1e-6 * r.normal(size=30)
    assert m.fullpiv_rank(X.T @ X) == 3
    X[:, 1:] = 0.0
    assert m.fullpiv_rank(X.T @ X) == 1 and m.fullpiv_rank(np.zeros((3, 3))) == 0


def test_jacobian_is_the_derivative_and_nan_at_zero():
    r = np.random.RandomState(11)
    worst = 0.0
    for _ in range(20):
        x = np.zeros(6)
        x[:3] = r.normal(size=3); x[:3] *= r.uniform(0.1, 2.5) / np.linalg.norm(x[:3]); x[3:] = np.r_[r.uniform(-1, 1, 2), 10.0]
        X = r.uniform(-3, 3, (8, 3))
        NS = np.stack([m.nullspace(np.r_[r.uniform(-0.5, 0.5, 2), 1.0], "random", r) for _ in range(8)])
        _, J = m.residuals_and_jacs(x, X, NS)
        Jn = np.zeros_like(J)
        for k in range(6):
            d = np.zeros(6); d[k] = 1e-6
            Jn[:, k] = (m.residuals_and_jacs(x + d, X, NS)[0] - m.residuals_and_jacs(x - d, X, NS)[0]) / 2e-6
        worst = max(worst, float(np.abs(J - Jn).max() / np.abs(J).max()))
    print("largest relative distance to central differences: %.2e" % worst)
    assert worst < 1e-7                                                         # central differences with h = 1e-6: O(h^2) + eps / h
    _, J0 = m.residuals_and_jacs(np.r_[0.0, 0.0, 0.0, 0.1, 0.2, 10.0], X, NS)
    assert np.isnan(J0[:, :3]).all() and np.isfinite(J0[:, 3:]).all()


@KB8
def test_model_recovers_the_true_pose(kb8):
    """returned poses (6-point hypotheses that hold more than nMin): rotation within 0.02, translation within 0.25 at depth 10 -- a set of
    six keypoints with 0.5 px noise at f = 458 spread over a VGA image; the inliers are the true ones"""
    seen = {0: 0, 1: 0, 2: 0}
    for grp, pb, sets, r in _all(kb8):
        seen[r["outcome"]] += 1
        if r["outcome"] != 1:
            continue
        R, t = r["T"][:9].reshape(3, 3), r["T"][9:]
        assert np.abs(R - pb["R_true"]).max() < 0.02 and np.abs(t - pb["t_true"]).max() < 0.25, (grp["name"], len(pb["Xw"]))
        assert (r["inlier"] & ~pb["outlier_true"]).sum() >= 0.9 * (~pb["outlier_true"]).sum()       # a gross outlier may fall inside by chance
    assert seen[0] >= 1 and seen[1] >= 8 and seen[2] >= 2, seen                 # every outcome occurs


@KB8
def test_batch_cases(kb8):
    B = sy.gpu_batch_model(kb8)
    by = {grp["name"]: (cands, ress) for grp, cands, ress in B}
    assert [len(pb["Xw"]) for pb, _ in by["default"][0]] == [15, 63, 64, 65, 200, 40, 64, 60, sy.LDS_MAX + 1]
    for k in (5, 6):                                                            # planar: world z exactly 0, and the model takes the planar branch
        pb = by["default"][0][k][0]
        assert (pb["Xw"][:, 2] == 0).all() and m.fullpiv_rank(pb["Xw"].astype(np.float64).T @ pb["Xw"].astype(np.float64)) == 2
    r = by["default"][1][7]                                                     # the scripted scan: outlier sets, an all-inlier set, a better one
    assert (r["counts"][:5] < r["nmin"]).all() and r["nmin"] < r["counts"][5] < r["counts"][6] and (r["outcome"], r["ret"], r["nref"]) == (1, 5, 1)
    (pb, _), r = by["budget_1"][0][0], by["budget_1"][1][0]
    assert (len(pb["Xw"]), r["nmin"], r["budget"], r["outcome"], r["n_inliers"], r["nref"]) == (6, 6, 1, 2, 6, 1)      # 6 of 6 is not MORE than nMin
    r9, r20 = by["refine_needs_more"][1]
    assert (r9["nmin"], r9["budget"], r9["outcome"]) == (10, 0, 0)
    assert (r20["nmin"], r20["budget"], r20["outcome"], r20["n_inliers"]) == (10, 35, 2, 10)
    assert r20["counts"][:35].max() == 10 and r20["nref"] == int((r20["counts"][:35] == 10).sum()) >= 2      # Refine() is called on each, none holds MORE


@KB8
def test_preconditions_of_the_gpu_comparison(kb8):
    worst = np.inf
    for grp, pb, sets, r in _all(kb8):
        assert m.decision_is_stable(r, sy.DELTA), (grp["name"], len(pb["Xw"]))
        last = r["ret"] if r["outcome"] == 1 else r["executed"] - 1
        for k in range(last + 1):
            if r["hi"][k] >= r["nmin"] - 1:
                worst = min(worst, r["margins"][k])
    print("smallest margin on a deciding iteration: %.3e (delta = %.0e)" % (worst, sy.DELTA))


@KB8
def test_decomposition_variants_take_the_same_decisions(kb8):
    """numpy.linalg or the model's own Jacobi / LDL^T, closed-form or randomly turned null spaces and eigenframe signs: the same counts on
    the deciding iterations (no two best counts tie differently), the same outcome, flags and Refine() calls; the poses' distance is printed"""
    worst = 0.0
    for grp, pb, sets, r in _all(kb8):
        if len(pb["Xw"]) >= 200:
            continue                                                            # the two large candidates decide by iteration 2 with 30 / 1000 inliers to spare
        for v, (lin, null) in enumerate(m.VARIANTS[1:]):
            q = m.solve(pb, sets, max_iterations=sy.ITERATIONS, lin=lin, null=null, seed=31 + v, delta=sy.DELTA,
                        upto=r["ret"] + 2 if r["outcome"] == 1 else None, **grp["params"])          # a returned candidate: up to two iterations past it
            tag = (grp["name"], len(pb["Xw"]), lin, null)
            assert (q["outcome"], q["ret"], q["ret_count"], q["n_inliers"], q["nref"], q["bests"]) == \
                (r["outcome"], r["ret"], r["ret_count"], r["n_inliers"], r["nref"], r["bests"]), tag
            assert np.array_equal(q["inlier"], r["inlier"]), tag
            far = r["margins"][:q["executed"]] >= sy.DELTA
            assert np.array_equal(q["counts"][:q["executed"]][far], r["counts"][:q["executed"]][far]), tag
            if r["T"] is not None:
                worst = max(worst, float(np.abs(q["T"] - r["T"]).max()))
    print("largest distance between the variants' returned poses (double): %.3e; after rounding to float: %.3e" %
          (worst, sy.measured_variant_distance(kb8)))
