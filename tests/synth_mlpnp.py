"""Synthetic relocalisation candidates for the MLPnPsolver tests: a VGA camera (Pinhole or KannalaBrandt8, tests/synth_sim3.py), a true
pose Tcw with a rotation of 0.1-2.5 rad (clear of w = 0, where the reference's Jacobian is NaN, and of pi) and the world 10 in front of
the camera, world points in a box of half-width 3 (or in the plane z = 0 EXACTLY for a planar candidate), pixel noise 0.5, 30-50 % gross
outliers, sigma2 from the keypoint's octave; the committed GPU batch with its host-made sets, in groups that share one set of RANSAC
parameters (one library call each)."""
import numpy as np
import mlpnp_model as m
import sim3_solver_model as s3m
import synth_sim3 as s3

F32 = np.float32
SIGMA2 = ((F32(1.2) ** np.arange(8, dtype=F32)) ** 2).astype(F32)          # mvLevelSigma2
LDS_MAX = 4096                                                              # PNP_LDS_MAX of csrc/mlpnp_kernels.hip
DELTA = 1e-3
ITERATIONS = 300


def camera(kb8=False):
    return s3.camera(kb8)


def rot(axis, angle):
    return m.rodrigues2rot(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle)


def make_candidate(seed, n, kb8=False, noise=0.5, outlier_share=0.4, planar=False, n_inliers=None):
    """-> dict(Xw, p2d, sigma2 float32, cam, R_true, t_true, outlier_true [n])"""
    r = np.random.RandomState(seed)
    cam = camera(kb8)
    R = rot(r.normal(size=3), r.uniform(0.1, 2.5))
    t = np.r_[r.uniform(-1, 1, 2), 10.0 + r.uniform(-1, 1)]
    Xw = r.uniform(-3, 3, (n, 3))
    if planar:
        Xw[:, 2] = 0.0
    Xw = Xw.astype(F32)
    Xc = Xw.astype(np.float64) @ R.T + t
    uv = s3m.project(cam, Xc, f64=True) + noise * r.normal(size=(n, 2))
    out = np.zeros(n, bool)
    k = int(round(outlier_share * n)) if n_inliers is None else n - n_inliers
    if k:
        out[r.choice(n, k, replace=False)] = True
        uv[out] = np.c_[r.uniform(20, 620, k), r.uniform(20, 460, k)]
    return dict(Xw=Xw, p2d=uv.astype(F32), sigma2=SIGMA2[r.randint(0, 8, n)], cam=cam, R_true=R, t_true=t, outlier_true=out)


def host_sets(seed, n, iterations, inliers=None, inlier_share=0.0):
    """sets as a caller supplies them (draw_sets = 0): 6 distinct indices per iteration; with inlier_share, that share of the iterations
    draws among `inliers` only"""
    r = np.random.RandomState(seed)
    sets = np.full((iterations, 6), -1, np.int32)
    if n < 6:
        return sets
    for k in range(iterations):
        pool = inliers if (inliers is not None and len(inliers) >= 6 and r.uniform() < inlier_share) else np.arange(n)
        sets[k] = r.choice(pool, 6, replace=False)
    return sets


def scripted_sets(pb, seed, iterations, params):
    """sets that script the scan: five sets that hold outliers, then an all-inlier set, then an all-inlier set that counts more"""
    r = np.random.RandomState(seed)
    n = len(pb["Xw"])
    good, bad = np.nonzero(~pb["outlier_true"])[0], np.nonzero(pb["outlier_true"])[0]
    sets = host_sets(seed + 1, n, iterations)
    for k in range(5):
        sets[k] = np.r_[r.choice(bad, 3, replace=False), r.choice(good, 3, replace=False)]
    nmin, _ = m.ransac_parameters(n, params["probability"], params["min_inliers"], iterations, 6, params["epsilon"])
    q = dict(pb); q["max_err"] = (pb["sigma2"] * F32(params["th2"])).astype(F32); q["f"] = m.bearings(pb["cam"], pb["p2d"])
    tried = []
    for k in range(40):                                                        # spread sets, and clustered ones (a weaker pose: fewer inliers)
        if k % 2:
            s = good[np.argsort(np.linalg.norm(pb["p2d"][good] - pb["p2d"][r.choice(good)], axis=1))[:6]]
        else:
            s = r.choice(good, 6, replace=False)
        c = int(m.check_inliers(q, m.hypothesis(q, s))[0].sum())
        tried.append((c, s))
    tried = sorted([t for t in tried if t[0] >= nmin], key=lambda t: t[0])
    assert len(tried) >= 2 and tried[-1][0] > tried[0][0]
    sets[5], sets[6] = tried[0][1], tried[-1][1]
    return sets


# ------------------------------------------------------------------ the committed GPU batch (tests/test_gpu_mlpnp.py; its preconditions
# in tests/test_mlpnp_model.py).  A group is one library call: its candidates share the RANSAC parameters.
DEFAULTS = dict(probability=0.99, min_inliers=8, epsilon=0.4, th2=5.991)
GROUPS = [
    dict(name="default", params=DEFAULTS,
         specs=[dict(n=15, outlier_share=0.3), dict(n=63, outlier_share=0.3), dict(n=64, outlier_share=0.4), dict(n=65, outlier_share=0.5),
                dict(n=200, outlier_share=0.45), dict(n=40, outlier_share=0.3, planar=True), dict(n=64, outlier_share=0.4, planar=True),
                dict(n=60, outlier_share=0.4, scripted=True), dict(n=LDS_MAX + 1, outlier_share=0.3)]),
    dict(name="budget_1", params=dict(DEFAULTS, min_inliers=6), specs=[dict(n=6, outlier_share=0.0)]),
    dict(name="refine_needs_more", params=dict(DEFAULTS, min_inliers=10, epsilon=0.5),
         specs=[dict(n=9, outlier_share=0.0), dict(n=20, n_inliers=10, inlier_share=0.6)]),
]
# (kb8) -> first seed of the batch, chosen so that the preconditions of tests/test_mlpnp_model.py hold (a seed that violates one is
# replaced, never a bound)
BATCH_SEEDS = {False: 9100, True: 9500}


def gpu_batch(kb8):
    """-> [(group, [(problem, sets [ITERATIONS][6])])]"""
    base = BATCH_SEEDS[bool(kb8)]
    out = []
    for g, grp in enumerate(GROUPS):
        cands = []
        for k, spec in enumerate(grp["specs"]):
            spec = dict(spec)
            share = spec.pop("inlier_share", 0.5)
            scripted = spec.pop("scripted", False)
            seed = base + 20 * g + k
            pb = make_candidate(seed, kb8=kb8, **spec)
            n = len(pb["Xw"])
            sets = scripted_sets(pb, seed + 500, ITERATIONS, grp["params"]) if scripted else \
                host_sets(seed + 500, n, ITERATIONS, np.nonzero(~pb["outlier_true"])[0], share)
            cands.append((pb, sets))
        out.append((grp, cands))
    return out


_batch_cache = {}


def gpu_batch_model(kb8):
    """the model (numpy.linalg, closed-form null spaces) on the committed batch: computed once per process, shared, never modified
    -> [(group, [(problem, sets)], [result])]"""
    key = bool(kb8)
    if key not in _batch_cache:
        _batch_cache[key] = [(grp, cands, [m.solve(pb, sets, max_iterations=ITERATIONS, delta=DELTA, **grp["params"]) for pb, sets in cands])
                             for grp, cands in gpu_batch(key)]
    return _batch_cache[key]


def variant_poses(pb, sets, res):
    """the returned pose of a candidate under every decomposition variant of the model, on the same sets"""
    if res["outcome"] == 0:
        return []
    q = dict(pb); q["f"] = res["f"]; q["max_err"] = res["max_err"]
    out = []
    for v, (lin, null) in enumerate(m.VARIANTS):
        rng = np.random.RandomState(77 + v)
        out.append(m.hypothesis(q, sets[res["ret"]], lin, null, rng))          # both outcomes return a 6-point hypothesis
    return out


def measured_variant_distance(kb8):
    """the largest distance, after rounding to float, between the model's decomposition variants over the returned poses of the batch"""
    worst = 0.0
    for grp, cands, ress in gpu_batch_model(kb8):
        for (pb, sets), res in zip(cands, ress):
            P = [p.astype(F32).astype(np.float64) for p in variant_poses(pb, sets, res)]
            for a in P:
                for b in P:
                    if np.isfinite(a).all() and np.isfinite(b).all():
                        worst = max(worst, float(np.abs(a - b).max()))
    return worst
