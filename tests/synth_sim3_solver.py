"""Synthetic loop candidates for the Sim3Solver tests: a VGA camera (Pinhole or KannalaBrandt8, tests/synth_sim3.py), a true Sim3 S12
(rotation up to ~17 degrees, translation up to 0.5, scale 0.5-2 or 1 under fix_scale), points at depth 2-20 spread over image 1, 3-D noise
worth `noise` pixels at the point's depth, a share of gross outliers, thresholds from the pyramid's sigma^2 truncated as the reference
truncates them; the committed GPU batch with its host-drawn sets; the flat-file scenes of lib/host_sim3solver_smoke and the constructor's
gathering (src/Sim3Solver.cc:35-124) restated independently of host/*.cc."""
import numpy as np
import sim3_opt_model as om
import sim3_solver_model as m
import synth_sim3 as s3

F32 = np.float32
SIGMA2 = ((F32(1.2) ** np.arange(8, dtype=F32)) ** 2).astype(F32)          # mvLevelSigma2
LDS_MAX = 3072                                                              # S3S_LDS_MAX of csrc/sim3solver_kernels.hip


def camera(kb8=False):
    return s3.camera(kb8)


def make_pair(seed, n, kb8=False, fix_scale=False, noise=0.7, outlier_share=0.3, mode=None):
    """-> problem dict of sim3_solver_model (X1c, X2c float32, max1, max2, cam1, cam2, fix_scale) plus R_true / t_true / s_true and
    outlier_true [n].  mode: None, "neg_z2" (every point behind camera 2), "coincident" (one point n times), "outliers_only"."""
    r = np.random.RandomState(seed)
    cam = camera(kb8)
    fx, fy, cx, cy = s3.K_VGA
    ax = r.normal(size=3); ax /= np.linalg.norm(ax)
    s_true = 1.0 if fix_scale else float(np.exp(r.uniform(np.log(0.5), np.log(2.0))))
    S = om.sim3_exp(np.r_[ax * r.uniform(0.05, 0.3), np.zeros(4)])
    R = om.quat_to_R(S[:4])
    if mode == "neg_z2":
        R = R @ np.diag([1.0, -1.0, -1.0])                                 # half a turn about x: what camera 1 sees lies behind camera 2
    t = r.uniform(-0.5, 0.5, 3)
    z = r.uniform(2, 20, n)
    uv = np.c_[r.uniform(20, 620, n), r.uniform(20, 460, n)]
    X1 = np.c_[(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z]
    X2 = ((X1 - t) @ R) / s_true if n else np.zeros((0, 3))               # X1 = s R X2 + t
    out = np.zeros(n, bool)
    if mode == "outliers_only":
        out[:] = True
    elif n:
        out[r.choice(n, int(round(outlier_share * n)), replace=False)] = True
    z2 = np.abs(X2[:, 2]) if n else z
    X1 = X1 + (noise * z / fx)[:, None] * r.normal(size=(n, 3))
    X2 = X2 + (noise * z2 / fx)[:, None] * r.normal(size=(n, 3))
    if out.any():                                                           # gross: somewhere else in front of (or behind) camera 2
        k = int(out.sum())
        zz = r.uniform(2, 20, k) * np.sign(X2[out, 2])
        X2[out] = np.c_[(r.uniform(20, 620, k) - cx) / fx * zz, (r.uniform(20, 460, k) - cy) / fy * zz, zz]
    if mode == "coincident" and n:
        X1[:] = X1[0]; X2[:] = X2[0]
    l1, l2 = r.randint(0, 8, n), r.randint(0, 8, n)
    thr = np.array([m.truncated_threshold(v) for v in SIGMA2], F32)
    return dict(X1c=X1.astype(F32), X2c=X2.astype(F32), max1=thr[l1], max2=thr[l2], cam1=cam, cam2=cam, fix_scale=bool(fix_scale),
                R_true=R, t_true=t, s_true=s_true, outlier_true=out)


def host_sets(seed, n, iterations, inliers=None, inlier_share=0.0):
    """sets as a caller supplies them (draw_sets = 0): 3 distinct indices per iteration; with inlier_share, that share of the iterations
    draws among `inliers` only"""
    r = np.random.RandomState(seed)
    sets = np.full((iterations, 3), -1, np.int32)
    if n < 3:
        return sets
    for k in range(iterations):
        pool = inliers if (inliers is not None and len(inliers) >= 3 and r.uniform() < inlier_share) else np.arange(n)
        sets[k] = r.choice(pool, 3, replace=False)
    return sets


# ------------------------------------------------------------------ the committed GPU batch (tests/test_gpu_sim3_solver.py; its
# preconditions in tests/test_sim3_solver_model.py).  One min_inliers for the batch: 3, so that n = 3 runs with a budget of 1 and
# cannot converge, and n = 0 / n = 2 are below it.
MIN_INLIERS = 3
ITERATIONS = 300
PROBABILITY = 0.99
DELTA = 1e-3
BATCH_SPEC = [dict(n=0), dict(n=2), dict(n=3, outlier_share=0.0), dict(n=4, outlier_share=0.0), dict(n=20), dict(n=63, outlier_share=0.2),
              dict(n=64, outlier_share=0.4), dict(n=65, outlier_share=0.59), dict(n=129), dict(n=300, outlier_share=0.5),
              dict(n=LDS_MAX + 1, outlier_share=0.4, noise=0.0, inlier_share=0.9), dict(n=40, mode="neg_z2"), dict(n=10, mode="coincident"),
              dict(n=20, mode="outliers_only")]
MAX_N = LDS_MAX + 1
# (kb8, fix_scale) -> first seed of the batch, chosen so that the preconditions of tests/test_sim3_solver_model.py hold (a seed that
# violates one is replaced, never a bound)
BATCH_SEEDS = {(False, False): 7100, (False, True): 7200, (True, False): 7300, (True, True): 7401}


def gpu_batch(kb8, fix_scale):
    """-> [(problem, sets [ITERATIONS][3])]"""
    base = BATCH_SEEDS[(bool(kb8), bool(fix_scale))]
    out = []
    for k, spec in enumerate(BATCH_SPEC):
        spec = dict(spec)
        share = spec.pop("inlier_share", 0.0)
        pb = make_pair(base + k, kb8=kb8, fix_scale=fix_scale, **spec)
        out.append((pb, host_sets(base + 50 + k, len(pb["X1c"]), ITERATIONS, np.nonzero(~pb["outlier_true"])[0], share)))
    return out


_batch_cache = {}


def gpu_batch_model(kb8, fix_scale):
    """the float32 model on the committed batch: computed once per process, shared, never modified"""
    key = (bool(kb8), bool(fix_scale))
    if key not in _batch_cache:
        batch = gpu_batch(*key)
        _batch_cache[key] = (batch, [m.solve(pb, sets, PROBABILITY, MIN_INLIERS, ITERATIONS, delta=DELTA) for pb, sets in batch])
    return _batch_cache[key]


# ------------------------------------------------------------------ stand-in keyframes for lib/host_sim3solver_smoke (the class)
def make_scene(seed, n=150, kb8=False, fix_scale=False, matched_kf=False, outliers_only=False, min_inliers=15, max_iterations=300):
    """~n keypoints in KF1 with a map point each and a matched map point of the other map each, seen by KF2 at a shuffled keypoint index;
    ~5 % of each side's map points bad, ~5 % of KF1's keypoints without map point, ~5 % unmatched, ~5 % of the matched points without
    keypoint in KF2 (negative index).  matched_kf: a non-empty vpKeyFrameMatchedMP naming KF2 or a third keyframe per match."""
    r = np.random.RandomState(seed)
    pb = make_pair(seed + 1, n, kb8=kb8, fix_scale=fix_scale, outlier_share=0.35, mode="outliers_only" if outliers_only else None)
    T1, T2 = s3._pose(r), s3._pose(r)

    def to_world(T, Pc):
        T = T.astype(np.float64)
        return ((Pc.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F32)
    X1, X2 = to_world(T1, pb["X1c"]), to_world(T2, pb["X2c"])
    perm = r.permutation(n)                                                 # keypoint index in KF2 of matched point i
    unseen = r.uniform(size=n) < 0.05
    kf2_mp = np.full(n, -1, np.int32)
    kf2_mp[perm[~unseen]] = n + np.nonzero(~unseen)[0]
    kf3_mp = np.full(n, -1, np.int32)
    kf3_mp[r.permutation(n)[: n // 2]] = n + r.permutation(n)[: n // 2]     # the third keyframe sees half of them, elsewhere
    kf1_mp = np.arange(n, dtype=np.int32); kf1_mp[r.uniform(size=n) < 0.05] = -1
    matches = n + np.arange(n, dtype=np.int32); matches[r.uniform(size=n) < 0.05] = -1
    cam = np.array(list(s3.K_VGA) + (list(s3.KB8) if kb8 else []), F32)
    kp = lambda: r.uniform(0, 600, (n, 2)).astype(F32)
    return dict(Tcw1=T1, Tcw2=T2, cam_type=np.array([int(kb8)]), cam=cam, sigma2=SIGMA2, kp1=kp(), oct1=r.randint(0, 8, n), kp2=kp(),
                oct2=r.randint(0, 8, n), kp3=kp(), oct3=r.randint(0, 8, n), mp_pos=np.r_[X1, X2], mp_bad=(r.uniform(size=2 * n) < 0.05).astype(np.int32),
                kf1_mp=kf1_mp, kf2_mp=kf2_mp, kf3_mp=kf3_mp, matches=matches,
                matched_kf=(r.randint(2, 4, n) if matched_kf else np.zeros(0, int)).astype(np.int32), fix_scale=np.array([int(fix_scale)]),
                min_inliers=np.array([min_inliers]), max_iterations=np.array([max_iterations]), probability=np.array([0.99], F32))


def class_problem(sc):
    """the constructor's gathering (:35-124) on a flat-file scene -> (problem of the model, mvnIndices1, mN1).  As written there, pKFm is
    pKF2 whatever vpKeyFrameMatchedMP holds: the flag that would re-read it is set only when the vector was EMPTY and has just been filled
    with pKF2."""
    T1, T2 = sc["Tcw1"].reshape(4, 4), sc["Tcw2"].reshape(4, 4)
    X = sc["mp_pos"].reshape(-1, 3)
    idx_in_kf1 = {int(mp): i for i, mp in enumerate(sc["kf1_mp"]) if mp >= 0}              # GetIndexInKeyFrame
    idx_in_kf2 = {int(mp): i for i, mp in enumerate(sc["kf2_mp"]) if mp >= 0}
    rows = dict(X1c=[], X2c=[], max1=[], max2=[])
    index = []
    for i1, m2 in enumerate(sc["matches"]):
        if m2 < 0:
            continue
        m1 = sc["kf1_mp"][i1]
        if m1 < 0:
            continue
        if sc["mp_bad"][m1] or sc["mp_bad"][m2]:
            continue
        k1, k2 = idx_in_kf1.get(int(m1), -1), idx_in_kf2.get(int(m2), -1)
        if k1 < 0 or k2 < 0:
            continue
        rows["max1"].append(m.truncated_threshold(sc["sigma2"][sc["oct1"][k1]]))
        rows["max2"].append(m.truncated_threshold(sc["sigma2"][sc["oct2"][k2]]))
        rows["X1c"].append(s3.gemm_add(T1[:3, :3], X[m1], T1[:3, 3])); rows["X2c"].append(s3.gemm_add(T2[:3, :3], X[m2], T2[:3, 3]))
        index.append(i1)
    c = np.asarray(sc["cam"], F32).astype(np.float64)
    cam = dict(K=tuple(c[:4]), kb8=tuple(c[4:8]) if sc["cam_type"][0] else None)
    pb = dict(X1c=np.array(rows["X1c"], F32).reshape(-1, 3), X2c=np.array(rows["X2c"], F32).reshape(-1, 3), max1=np.array(rows["max1"], F32),
              max2=np.array(rows["max2"], F32), cam1=cam, cam2=cam, fix_scale=bool(sc["fix_scale"][0]))
    return pb, np.array(index, int), len(sc["matches"])


# the scenes of tests/test_gpu_sim3_solver.py::test_class_drop_in (seeds chosen as BATCH_SEEDS were)
CLASS_SCENES = {"own_keyframe": dict(seed=8110, kb8=False, fix_scale=False, matched_kf=False),
                "matched_keyframes-fix_scale": dict(seed=8120, kb8=False, fix_scale=True, matched_kf=True),
                "own_keyframe-kb8": dict(seed=8130, kb8=True, fix_scale=False, matched_kf=False),
                "not_converging": dict(seed=8140, kb8=False, fix_scale=False, matched_kf=True, outliers_only=True)}
