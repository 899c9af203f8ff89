"""Synthetic keyframe pairs for the OptimizeSim3 tests: a VGA camera (Pinhole or KannalaBrandt8), a true Sim3 S12 (rotation up to ~17
degrees, translation up to 0.5, scale 0.5-2 or 1 under fix_scale), points at depth 2-20 spread over image 1, pixel noise, gross
outliers (>= 20 px), a share of rows without keypoint in KF2 (normalised "observation" at octave 0 -- src/Optimizer.cc:4161-4181,
:4178 passes mnTrackScaleLevel as the keypoint's size --) and a share of rows with P2c.z < 0, and an initial Sim3 off by a few degrees, a few cm and a few percent."""
import numpy as np
import sim3_opt_model as m

K_VGA = (458.654, 457.296, 322.215, 238.375)
KB8 = (-0.0034, 0.0007, -0.0021, 0.0002)
TH2 = 10.0                                                  # LoopClosing's th2 (src/LoopClosing.cc:532, :742)


def camera(kb8=False):
    return dict(K=K_VGA, kb8=KB8 if kb8 else None)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def make_pair(seed, n, kb8=False, fix_scale=False, noise=0.7, outliers=0, no_kp2=0.0, neg_z=0.0, exact=False):
    """-> problem dict of sim3_opt_model plus sim3_true, outlier_true [n] bool.  outliers: a count (int) of gross ones; no_kp2 / neg_z:
    shares of rows; exact: no float rounding of the inputs (noise-free convergence tests)."""
    r = np.random.RandomState(seed)
    cam = camera(kb8)
    fx, fy, cx, cy = cam["K"]
    ax = r.normal(size=3); ax /= np.linalg.norm(ax)
    s_true = 1.0 if fix_scale else float(np.exp(r.uniform(np.log(0.5), np.log(2.0))))
    S_true = m.sim3_exp(np.r_[ax * r.uniform(0.05, 0.3), np.zeros(4)])
    S_true[4:7] = r.uniform(-0.5, 0.5, 3); S_true[7] = s_true
    z = r.uniform(2, 20, n)
    uv = np.c_[r.uniform(20, 620, n), r.uniform(20, 460, n)]
    P1 = np.c_[(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z]
    P2 = m.sim3_map(m.sim3_inverse(S_true), P1) if n else np.zeros((0, 3))
    # the cameras see the points where the model's own projection puts them
    obs1 = m.project_smooth(cam, P1) + noise * r.normal(size=(n, 2)) if n else np.zeros((0, 2))
    obs2 = m.project_smooth(cam, P2) + noise * r.normal(size=(n, 2)) if n else np.zeros((0, 2))
    lev1 = r.randint(0, 8, n); lev2 = r.randint(0, 8, n)
    out = np.zeros(n, bool)
    if outliers:
        idx = r.choice(n, int(outliers), replace=False)
        ang = r.uniform(0, 2 * np.pi, len(idx)); mag = r.uniform(20, 60, len(idx))
        obs1[idx] += np.c_[mag * np.cos(ang), mag * np.sin(ang)]
        out[idx] = True
    nokp = r.uniform(size=n) < no_kp2
    negz = (r.uniform(size=n) < neg_z) & ~nokp
    P2[negz] *= -1.0
    if not exact:
        P1 = _f32(P1); P2 = _f32(P2); obs1 = _f32(obs1); obs2 = _f32(obs2)
    if nokp.any():                                          # float arithmetic of :4163-4165
        p = P2[nokp].astype(np.float32)
        invz = np.float32(1) / p[:, 2]
        obs2[nokp] = np.c_[p[:, 0] * invz, p[:, 1] * invz].astype(np.float64)
    sig2 = (1.0 / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32).astype(np.float64)
    lev2[nokp] = 0                                          # cv::KeyPoint(pt, mnTrackScaleLevel): a size, the octave stays 0 (:4178, :4220)
    pert = np.r_[r.normal(size=3) * 0.02, r.normal(size=3) * 0.03, 0.0 if fix_scale else r.normal() * 0.03]
    S0 = m.sim3_mul(m.sim3_exp(pert), S_true)
    return dict(P1c=P1, P2c=P2, obs1=obs1, obs2=obs2, w1=sig2[lev1], w2=sig2[lev2], cam1=cam, cam2=cam, th2=TH2, fix_scale=bool(fix_scale),
                sim3=S0, sim3_true=S_true, outlier_true=out | nokp, no_edge=negz, no_kp2_rows=nokp)


# ------------------------------------------------------------------ the committed GPU batch (tests/test_gpu_sim3_opt.py, preconditions in
# tests/test_sim3_opt_model.py): n = 0, 9, 10, 12 with 3 gross outliers, 63, 64, 65, 129, 300, every row with z < 0, n = max_edges = 512
MAX_EDGES = 512
BATCH_SPEC = [dict(n=0), dict(n=9, noise=0.3), dict(n=10, noise=0.3), dict(n=12, noise=0.3, outliers=3), dict(n=63, outliers=6, no_kp2=0.1),
              dict(n=64, outliers=5), dict(n=65, outliers=8, neg_z=0.1), dict(n=129, outliers=20, no_kp2=0.2, neg_z=0.05),
              dict(n=300, outliers=40, no_kp2=0.1), dict(n=40, neg_z=1.0), dict(n=512, outliers=60, no_kp2=0.05, neg_z=0.02)]
# (kb8, fix_scale) -> first seed of the batch, chosen so that the preconditions of tests/test_sim3_opt_model.py hold (a seed that
# violates one is replaced, never a bound)
BATCH_SEEDS = {(False, False): 4440, (False, True): 4520, (True, False): 5300, (True, True): 5400}


def gpu_batch(kb8, fix_scale):
    base = BATCH_SEEDS[(bool(kb8), bool(fix_scale))]
    return [make_pair(base + k, kb8=kb8, fix_scale=fix_scale, **spec) for k, spec in enumerate(BATCH_SPEC)]


def summation_orders(n, count=6):
    """row orders for the summation-order precondition: the reversal and count - 1 fixed random permutations"""
    r = np.random.RandomState(n + 17)
    return [np.arange(n)[::-1]] + [r.permutation(n) for _ in range(count - 1)]


# the seed set of the numeric-vs-analytic comparison (Pinhole only: tests/test_sim3_opt_model.py says why)
NUMERIC_SET = [dict(seed=5000 + k, n=n, fix_scale=fs, outliers=o, no_kp2=nk) for k, (n, fs, o, nk) in enumerate(
    [(40, False, 4, 0.0), (40, True, 4, 0.0), (120, False, 15, 0.1), (120, True, 15, 0.1), (300, False, 30, 0.2), (300, True, 30, 0.0),
     (20, False, 2, 0.0), (64, True, 0, 0.0)])]


# ------------------------------------------------------------------ two stand-in keyframes for lib/host_sim3_smoke (the class method)
def write_flat(path, arrays):
    """named flat arrays (host/flatfile.h): float -> float32, integer -> int32, float64 kept bit for bit as bytes when named in RAW64"""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint8:
                kind, raw = 2, a.reshape(-1)
            elif a.dtype.kind == "f":
                kind, raw = 1, a.astype(np.float32).reshape(-1)
            else:
                kind, raw = 0, a.astype(np.int32).reshape(-1)
            f.write(name.encode().ljust(24, b"\0")[:24]); f.write(struct.pack("<ii", kind, raw.size)); f.write(raw.tobytes())


def read_flat(path):
    import struct
    out = {}
    with open(path, "rb") as f:
        (n,) = struct.unpack("<i", f.read(4))
        for _ in range(n):
            name = f.read(24).split(b"\0")[0].decode()
            kind, cnt = struct.unpack("<ii", f.read(8))
            dt = (np.int32, np.float32, np.uint8)[kind]
            out[name] = np.frombuffer(f.read(cnt * np.dtype(dt).itemsize), dt).copy()
    return out


def _pose(r):
    ax = r.normal(size=3); ax /= np.linalg.norm(ax)
    T = np.eye(4)
    T[:3, :3] = m.quat_to_R(m.sim3_exp(np.r_[ax * r.uniform(0.1, 0.6), np.zeros(4)])[:4])
    T[:3, 3] = r.uniform(-1, 1, 3)
    return T.astype(np.float32)


def make_keyframes(seed, n=150, kb8=False, fix_scale=False, all_points=True):
    """~n keypoints in KF1 with a map point each, a matched map point of the other map each (seen by KF2 at a shuffled keypoint index, or
    by no keypoint of KF2 for ~15 %), ~5 % of each side's map points bad, ~5 % of KF1's keypoints without map point, ~5 % unmatched,
    30 gross outliers.  -> the flat-file arrays of host/host_sim3_smoke.cc"""
    r = np.random.RandomState(seed)
    pb = make_pair(seed + 1, n, kb8=kb8, fix_scale=fix_scale, outliers=30, no_kp2=0.15, neg_z=0.03)
    T1, T2 = _pose(r), _pose(r)

    def to_world(T, Pc):
        T = T.astype(np.float64)
        return ((Pc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)           # R^T (P - t)
    X1, X2 = to_world(T1, pb["P1c"]), to_world(T2, pb["P2c"])
    nokp = pb["no_kp2_rows"]                                              # the rows make_pair gave a normalised "observation"
    perm = r.permutation(n)                                               # keypoint index in KF2 of row i
    kf2_mp = np.full(n, -1, np.int32)
    kf2_mp[perm[~nokp]] = n + np.nonzero(~nokp)[0]
    kp2 = np.zeros((n, 2), np.float32)
    kp2[perm] = pb["obs2"].astype(np.float32)
    kp2[perm[nokp]] = r.uniform(0, 600, (int(nokp.sum()), 2)).astype(np.float32)    # some other keypoint lives there
    sig2 = (1.0 / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
    lev = lambda w: np.array([int(np.argmin(np.abs(sig2.astype(np.float64) - v))) for v in w], np.int32)
    oct2 = np.zeros(n, np.int32); oct2[perm] = lev(pb["w2"])
    mp_level = r.randint(-1, 12, 2 * n).astype(np.int32)                  # mnTrackScaleLevel: -1 (Frame.cc:564) or anything; never an index
    kf1_mp = np.arange(n, dtype=np.int32); kf1_mp[r.uniform(size=n) < 0.05] = -1
    matches = n + np.arange(n, dtype=np.int32); matches[r.uniform(size=n) < 0.05] = -1
    cam = np.array(list(K_VGA) + (list(KB8) if kb8 else []), np.float32)
    return dict(Tcw1=T1, Tcw2=T2, cam_type=np.array([int(kb8)]), cam=cam, inv_sigma2=sig2, kp1=pb["obs1"].astype(np.float32), oct1=lev(pb["w1"]),
                kp2=kp2, oct2=oct2, mp_pos=np.r_[X1, X2], mp_bad=(r.uniform(size=2 * n) < 0.05).astype(np.int32), mp_level=mp_level,
                kf1_mp=kf1_mp, kf2_mp=kf2_mp, matches=matches, sim3=np.ascontiguousarray(pb["sim3"], np.float64).view(np.uint8),
                th2=np.array([TH2], np.float32), fix_scale=np.array([int(fix_scale)]), all_points=np.array([int(all_points)]))


# ------------------------------------------------------------------ the class method's edge loop, restated independently of host/*.cc
F32 = np.float32


def gemm_add(R, x, t):
    """host/cvmath.h mul_add = OpenCV's small-matrix gemm on CV_32F: the row's products summed in float, then (float)(sum * 1.0 + t)"""
    out = np.zeros(3, F32)
    for i in range(3):
        acc = F32(F32(F32(R[i][0]) * F32(x[0]) + F32(R[i][1]) * F32(x[1])) + F32(R[i][2]) * F32(x[2]))
        out[i] = F32(np.float64(acc) + np.float64(t[i]))
    return out


def edge_loop(sc, all_points):
    """src/Optimizer.cc:4007-4233 on the flat-file scene -> (problem rows for the model, index i of every row, rows with i2 < 0)"""
    T1, T2 = sc["Tcw1"].reshape(4, 4), sc["Tcw2"].reshape(4, 4)
    kp1, kp2 = sc["kp1"].reshape(-1, 2), sc["kp2"].reshape(-1, 2)
    X = sc["mp_pos"].reshape(-1, 3)
    idx_in_kf2 = {int(mp): i2 for i2, mp in enumerate(sc["kf2_mp"]) if mp >= 0}            # GetIndexInKeyFrame(pKF2)
    rows = dict(P1c=[], P2c=[], obs1=[], obs2=[], w1=[], w2=[])
    index = []
    n_no_kp2 = 0
    for i, m2 in enumerate(sc["matches"]):
        if m2 < 0:
            continue
        m1 = sc["kf1_mp"][i]
        i2 = idx_in_kf2.get(int(m2), -1)
        if m1 < 0:
            continue
        if sc["mp_bad"][m1] or sc["mp_bad"][m2]:
            continue
        P1 = gemm_add(T1[:3, :3], X[m1], T1[:3, 3]); P2 = gemm_add(T2[:3, :3], X[m2], T2[:3, 3])
        if i2 < 0 and not all_points:
            continue
        rows["P1c"].append(P1.astype(np.float64)); rows["P2c"].append(P2.astype(np.float64))
        rows["obs1"].append(kp1[i].astype(np.float64)); rows["w1"].append(float(sc["inv_sigma2"][sc["oct1"][i]]))
        if i2 >= 0:
            rows["obs2"].append(kp2[i2].astype(np.float64)); rows["w2"].append(float(sc["inv_sigma2"][sc["oct2"][i2]]))
        else:
            n_no_kp2 += 1
            invz = F32(1) / P2[2]
            rows["obs2"].append(np.array([P2[0] * invz, P2[1] * invz], np.float64)); rows["w2"].append(float(sc["inv_sigma2"][0]))      # :4178: octave 0
        index.append(i)
    shapes = dict(P1c=(0, 3), P2c=(0, 3), obs1=(0, 2), obs2=(0, 2), w1=(0,), w2=(0,))
    return {k: np.array(v, np.float64).reshape((len(v),) + shapes[k][1:]) for k, v in rows.items()}, np.array(index, int), n_no_kp2


def class_problem(sc):
    """the model's problem for a flat-file scene -> (problem, index i of every row, rows with i2 < 0)"""
    rows, index, n_no_kp2 = edge_loop(sc, bool(sc["all_points"][0]))
    c = np.asarray(sc["cam"], np.float32).astype(np.float64)                # mvParameters are float
    cam = dict(K=tuple(c[:4]), kb8=tuple(c[4:8]) if sc["cam_type"][0] else None)
    return dict(rows, cam1=cam, cam2=cam, th2=TH2, fix_scale=bool(sc["fix_scale"][0]), sim3=sc["sim3"].view(np.float64)), index, n_no_kp2


# the scenes of tests/test_gpu_sim3_opt.py::test_class_method_on_two_stand_in_keyframes (seeds chosen as BATCH_SEED was)
CLASS_SCENES = {"all_points": dict(seed=9210, all_points=True, kb8=False, fix_scale=False),
                "kf2_points_only-fix_scale": dict(seed=9220, all_points=False, kb8=False, fix_scale=True),
                "all_points-kb8": dict(seed=9230, all_points=True, kb8=True, fix_scale=False)}
