"""Synthetic frames for the inertial pose-only optimisations (PoseInertialOptimizationLastKeyFrame / LastFrame): one frame's visual
edges in frame-index order, the previous state (last keyframe or previous frame), a preintegration record consistent with the true
motion, its covariance's information blocks and (LastFrame) a prior.  No oracle, no GPU code in here."""
import numpy as np
from synth_iba import _rot, KF, PREINT  # noqa: F401

G = np.array([0, 0, -float(np.float32(9.81))])
EUROC = dict(cam=(458.654, 457.296, 367.215, 248.375, 47.9), camera_model=0)
# the TUM-VI 512 x 512 rig (tests/test_stereo_fisheye_oracle.py): two KannalaBrandt8 cameras, Tlr inverted to Trl
_Tlr = np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224, 0.101063427414194],
                 [-0.000823363992158, 0.998899461915674, 0.046895490788700, 0.001946204678584],
                 [-0.000656143613644, -0.046896036240590, 0.998899560146304, 0.001015350132563]])
TUMVI = dict(cam=(190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0), camera_model=1,
             kb=(0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182),
             Trl=np.concatenate([_Tlr[:, :3].T, -(_Tlr[:, :3].T @ _Tlr[:, 3])[:, None]], 1),
             cam2=(190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983), camera2_model=1,
             kb2=(0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039))
RCB = _rot(np.array([0.02, -0.01, 1.55]))
TCB = np.array([0.065, -0.02, 0.01])


def camera(kind):
    """kind: 'mono' / 'stereo' (EuRoC-like pinhole) or 'rig' (TUM-VI KB8 pair) -> pose_inertial_model.Camera"""
    import pose_inertial_model as pm
    c = dict(TUMVI if kind == "rig" else EUROC)
    return pm.Camera(Rcb=RCB, tcb=TCB, **c)


def rig(kind):
    """orbhip.PimRig of camera(kind) (for the device calls)."""
    import orbhip
    c = camera(kind)
    kw = dict(cam=c.cam, Rcb=c.Rcb, tcb=c.tcb, camera_model=c.model, kb=c.kb)
    if c.Trl is not None:
        kw.update(Trl=c.Trl, cam2=c.cam2, camera2_model=c.model2, kb2=c.kb2)
    return orbhip.pim_rig(**kw)


def _kb(Xc, f, k):
    th = np.arctan2(np.hypot(Xc[0], Xc[1]), Xc[2]); psi = np.arctan2(Xc[1], Xc[0])
    r = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
    return np.array([f[0] * r * np.cos(psi) + f[2], f[1] * r * np.sin(psi) + f[3]])


def _state(R, p, v, bg, ba):
    s = np.zeros(KF)
    s[0:9] = R.reshape(-1); s[9:12] = p; s[12:15] = v; s[15:18] = bg; s[18:21] = ba
    return s


def _spd(rng, scales):
    n = len(scales)
    Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
    M = np.eye(n) + 0.1 * (Q - np.eye(n))
    S = np.diag(np.sqrt(scales))
    A = S @ M @ np.diag(rng.uniform(0.5, 2.0, n)) @ M.T @ S
    return 0.5 * (A + A.T)


def _clean(I):
    I = 0.5 * (I + I.T)
    w, V = np.linalg.eigh(I)
    return (V * np.where(w < 1e-12, 0.0, w)) @ V.T


def make_frame(seed, cam_kind="mono", mode=0, n_points=300, noise_free=False, outlier_frac=0.05, n_close=6, behind=True,
               state_noise=1.0, dt=0.05, prev_true=None):
    """cam_kind 'mono' (Pinhole, monocular edges), 'stereo' (Pinhole, a mix of stereo and monocular edges) or 'rig' (TUM-VI KB8
    pair: left edges [0, Nleft), right-camera edges after).  Returns (frame dict in the layout of pose_inertial_model.solve, true
    current state).  noise_free: exact observations and preintegration, no outliers: the true state is a zero-residual point.
    prev_true: the previous frame's true state (a trajectory), else drawn at random.  behind: one monocular Pinhole edge's map point is
    mirrored through the camera centre (same pixel, negative depth: only isDepthPositive rejects it); on the rig a point behind the
    camera keeps another point's observation."""
    rng = np.random.default_rng(seed)
    rig = cam_kind == "rig"
    c = TUMVI if rig else EUROC
    fx, fy, cx, cy, bf = c["cam"]
    W_, H_ = (512, 512) if rig else (752, 480)
    # true motion: previous state, then a constant-acceleration / constant-rate step of dt
    Rwc0 = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    R1 = Rwc0 @ _rot(rng.normal(0, 0.1, 3)) @ RCB.T
    p1 = rng.normal(0, 1.0, 3); v1 = rng.normal(0, 0.6, 3)
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    if prev_true is not None:
        R1, p1, v1 = prev_true[0:9].reshape(3, 3), prev_true[9:12].copy(), prev_true[12:15].copy()
        bg, ba = prev_true[15:18].copy(), prev_true[18:21].copy()
    prev = _state(R1, p1, v1, bg, ba)
    b_lin_g = bg if noise_free else bg + rng.normal(0, 2e-3, 3)
    b_lin_a = ba if noise_free else ba + rng.normal(0, 1e-2, 3)
    JRg = -dt * (np.eye(3) + rng.normal(0, 0.03, (3, 3)))
    JVa = -dt * (np.eye(3) + rng.normal(0, 0.05, (3, 3)))
    JPa = -0.5 * dt * dt * (np.eye(3) + rng.normal(0, 0.05, (3, 3)))
    JVg = rng.normal(0, 0.3 * dt * dt, (3, 3))
    JPg = rng.normal(0, 0.1 * dt ** 3, (3, 3))
    dR0 = _rot(rng.normal(0, 0.05, 3))
    dV0 = rng.normal(0, 0.2, 3)
    dP0 = rng.normal(0, 0.01, 3)
    rec = np.concatenate([[dt], dR0.reshape(-1), dV0, dP0, JRg.reshape(-1), JVg.reshape(-1), JVa.reshape(-1), JPg.reshape(-1),
                          JPa.reshape(-1), b_lin_g, b_lin_a])
    if not noise_free:
        rec = rec.astype(np.float32).astype(np.float64)                  # IMU::Preintegrated holds float cv::Mat
    rec_dR = rec[1:10].reshape(3, 3)
    # bias-corrected deltas at the previous bias (ImuTypes.cc:357-378) and the current state they imply
    dbg, dba = bg - rec[61:64], ba - rec[64:67]
    dR = rec_dR @ _rot(rec[16:25].reshape(3, 3) @ dbg)
    U, _, Vt = np.linalg.svd(dR); dR = U @ Vt
    dV = rec[10:13] + rec[25:34].reshape(3, 3) @ dbg + rec[34:43].reshape(3, 3) @ dba
    dP = rec[13:16] + rec[43:52].reshape(3, 3) @ dbg + rec[52:61].reshape(3, 3) @ dba
    R2 = R1 @ dR
    v2 = v1 + G * dt + R1 @ dV
    p2 = p1 + v1 * dt + 0.5 * G * dt * dt + R1 @ dP
    if not noise_free:
        R2 = R2 @ _rot(rng.normal(0, 3e-4, 3)); v2 = v2 + rng.normal(0, 2e-3, 3); p2 = p2 + rng.normal(0, 1e-3, 3)
    bg2 = bg if noise_free else bg + rng.normal(0, 1e-5, 3)
    ba2 = ba if noise_free else ba + rng.normal(0, 1e-4, 3)
    true_cur = _state(R2, p2, v2, bg2, ba2)
    # information: C [15][15] SPD (float), EdgeInertial's inv(C[0:9,0:9]) cleaned as G2oTypes.cc:700-714, RW blocks inverted
    C = np.linalg.inv(_spd(rng, np.concatenate([rng.uniform(2e5, 4e6, 3), rng.uniform(2e4, 4e5, 3), rng.uniform(1e5, 3e6, 3),
                                                rng.uniform(2e7, 2e8, 3), rng.uniform(2e4, 2e5, 3)])))
    C = (0.5 * (C + C.T)).astype(np.float32).astype(np.float64)
    info = _clean(np.linalg.pinv(C[0:9, 0:9]).astype(np.float32).astype(np.float64))
    info_g = np.linalg.pinv(C[9:12, 9:12]).astype(np.float32).astype(np.float64)
    info_a = np.linalg.pinv(C[12:15, 12:15]).astype(np.float32).astype(np.float64)
    # visual edges at the true current pose
    Rcw = RCB @ R2.T; tcw = RCB @ (-(R2.T @ p2)) + TCB
    Rrl, trl = (c["Trl"][:, :3], c["Trl"][:, 3]) if rig else (None, None)
    inv_levels = (1.0 / (1.2 ** (2 * np.arange(8)))).astype(np.float32)
    left, right = [], []
    for i in range(n_points):
        depth = rng.uniform(1.5, 9.5) if i < n_close else rng.uniform(10.5, 30.0)
        u0, v0 = rng.uniform(20, W_ - 20), rng.uniform(20, H_ - 20)
        if rig:
            ray = np.array([(u0 - cx) / fx, (v0 - cy) / fy, 1.0])
            ray = ray / np.linalg.norm(ray) * min(1.0, 1.2 / max(np.linalg.norm(ray[:2]), 1e-9))
            ray[2] = max(ray[2], 0.35); ray = ray / np.linalg.norm(ray)
            Xc = ray * depth / ray[2]
        else:
            Xc = np.array([(u0 - cx) / fx * depth, (v0 - cy) / fy * depth, depth])
        Xw = R2 @ (RCB.T @ (Xc - TCB)) + p2
        octv = int(rng.integers(0, 8))
        s = 0.0 if noise_free else 0.7 * 1.2 ** octv
        close = 1 if i < n_close else 0
        if rig:
            uv = _kb(Xc, c["cam"], c["kb"])
            if 0 < uv[0] < W_ and 0 < uv[1] < H_ and rng.random() < 0.8:
                left.append((Xw, np.array([*(uv + rng.normal(0, s, 2)), -1.0]), inv_levels[octv], 0, close, Xc))
            Xr = Rrl @ Xc + trl
            if Xr[2] > 0.3 and rng.random() < 0.5:
                ur = _kb(Xr, c["cam2"], c["kb2"])
                if 0 < ur[0] < W_ and 0 < ur[1] < H_:
                    right.append((Xw, np.array([*(ur + rng.normal(0, s, 2)), -1.0]), inv_levels[octv], 2, close, Xc))
        else:
            u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            st = cam_kind == "stereo" and rng.random() < 0.6
            ob = np.array([u + rng.normal(0, s), v + rng.normal(0, s), (u - bf / Xc[2] + rng.normal(0, s)) if st else -1.0])
            left.append((Xw, ob, inv_levels[octv], 1 if st else 0, close, Xc))
    edges = left + right
    fr_behind = -1
    Xw = np.array([e[0] for e in edges]).reshape(-1, 3)
    obs = np.array([e[1] for e in edges]).reshape(-1, 3)
    if not noise_free and len(edges):
        bad = rng.random(len(edges)) < outlier_frac
        obs[bad, :2] += rng.uniform(-30, 30, (int(bad.sum()), 2))
        if behind:                                                        # a map point behind the current camera
            if rig:
                j = int(rng.integers(0, len(edges)))
                Xc_b = np.array([0.3, -0.2, -4.0])
                Xw[j] = R2 @ (RCB.T @ (Xc_b - TCB)) + p2 if edges[j][3] != 2 else R2 @ (RCB.T @ (Rrl.T @ (Xc_b - trl) - TCB)) + p2
            else:
                mono = [i for i, e in enumerate(edges) if e[3] == 0 and not e[4]]
                if mono:
                    j = mono[int(rng.integers(0, len(mono)))]
                    bad[j] = False
                    obs[j, :2] = edges[j][1][:2]
                    Xw[j] = R2 @ (RCB.T @ (-edges[j][5] - TCB)) + p2        # Xc -> -Xc: the same pixel
                    fr_behind = j
        obs = obs.astype(np.float32).astype(np.float64)                  # cv::KeyPoint / mvuRight are float
        Xw = Xw.astype(np.float32).astype(np.float64)                    # MapPoint::GetWorldPos is float
    fr = dict(Xw=np.ascontiguousarray(Xw), obs=np.ascontiguousarray(obs),
              inv_sigma2=np.array([float(e[2]) for e in edges], np.float64), kind=np.array([e[3] for e in edges], np.uint8),
              close=np.array([e[4] for e in edges], np.uint8), prev=prev, preint=rec, info=info.reshape(-1),
              info_g=info_g.reshape(-1), info_a=info_a.reshape(-1), behind=fr_behind)
    # initial estimate: Tracking's prediction, truth + noise
    k = 0.0 if noise_free and state_noise == 0 else state_noise
    R0 = R2 @ _rot(rng.normal(0, 0.01 * k, 3))
    fr["state"] = _state(R0, p2 + rng.normal(0, 0.03 * k, 3), v2 + rng.normal(0, 0.05 * k, 3), bg2 + rng.normal(0, 1e-3 * k, 3),
                         ba2 + rng.normal(0, 1e-2 * k, 3))
    if mode == 1:
        # the previous frame's estimate (free here) and its prior (ConstraintPoseImu of the previous solve), centred near it
        pn = 0.0 if noise_free else 1.0
        fr["prior"] = prev.copy()
        fr["prior"][0:9] = (R1 @ _rot(rng.normal(0, 1e-3 * pn, 3))).reshape(-1)
        fr["prior"][9:21] += rng.normal(0, 1, 12) * np.repeat([3e-3, 5e-3, 1e-4, 1e-3], 3) * pn
        fr["prior_H"] = _clean(_spd(rng, np.concatenate([rng.uniform(1e5, 1e6, 3), rng.uniform(1e4, 1e5, 3), rng.uniform(1e3, 1e4, 3),
                                                          rng.uniform(1e7, 1e8, 3), rng.uniform(1e4, 1e5, 3)]))).reshape(-1)
        fr["prev"] = prev.copy()
        if not noise_free:
            fr["prev"][0:9] = (R1 @ _rot(rng.normal(0, 2e-3, 3))).reshape(-1)
            fr["prev"][9:21] += rng.normal(0, 1, 12) * np.repeat([5e-3, 1e-2, 1e-4, 1e-3], 3)
    return fr, true_cur
