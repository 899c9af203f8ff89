"""Seeded synthetic maps for the FullInertialBA tests and the probe (no oracle, no GPU code): the arrays of orbhip_iba_window for a
whole map, made from synth_iba's temporal window.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import synth_iba as si


def make_map(seed, K, pts_per_kf=20, stereo_frac=0.5, fisheye_rig=False, no_imu=(), gap=(), fixed=(), fixed_only_point=False,
             state_noise=1.0, outlier_frac=0.02, bias0_sigma=None):
    """K temporal keyframes (array order newest first, as synth_iba), all free and all with IMU states, chained by K - 1 inertial
    edges; monocular and stereo observations (left and right monocular ones with fisheye_rig).  Options:
      no_imu:   keyframes without IMU states (pose vertex only; the inertial edges that touch them are not made, :517)
      gap:      keyframes without mPrevKF (the edge INTO them is not made, :507-511)
      fixed:    keyframes fixed as bFixLocal does (two adjacent ones keep their inertial edge in the map)
      fixed_only_point: the first point that a fixed keyframe sees loses its edges to free keyframes (bAllFixed, :751-755)
      bias0_sigma: the biases are moved so that the true ones are about zero (the preintegrations' linearisation biases move with
                them: EdgeInertial only sees the difference) and every estimate starts at N(0, bias0_sigma).  The prior edges pull
                towards zero with information up to 1e10: a start far from zero makes their term all of chi2.
    -> (synth_iba.Window, shared bias [6] = the biases of keyframe 0, the last one admitted)."""
    w = si.make_window(seed, n_opt=K - 1, n_fixed_vis=0, n_points=max(pts_per_kf * K, 0), stereo_frac=stereo_frac, outlier_frac=outlier_frac,
                       state_noise=state_noise, fisheye_rig=fisheye_rig)
    d = dict(w.d)
    for k in ("edge_kf", "edge_point", "edge_stereo", "edge_inv_sigma2", "edge_close", "in_kf1", "in_kf2", "in_robust"):
        d[k] = np.asarray(d[k]).copy()
    d["edge_obs"] = np.asarray(d["edge_obs"], np.float64).reshape(-1, 3).copy()
    for k, width in (("in_preint", si.PREINT), ("in_info", 81), ("in_info_g", 9), ("in_info_a", 9)):
        d[k] = np.asarray(d[k], np.float64).reshape(-1, width).copy()
    kf_fixed = np.zeros(K, np.uint8)
    kf_imu = np.ones(K, np.uint8)
    last = np.flatnonzero(d["in_robust"] != 0)
    d["in_info"][last] *= 100.0                              # (the window's 1e-2 on the edge into its fixed keyframe: not in a full BA)
    d["in_robust"] = np.ones(len(d["in_kf1"]), np.uint8)
    rng = np.random.default_rng(7000 + seed)
    d["kf_state"] = np.asarray(d["kf_state"], np.float64).copy()
    # the oldest keyframe was the window's fixed one: give it an estimate off the truth like the others
    d["kf_state"][K - 1, 9:12] += rng.normal(0, 0.02 * state_noise, 3)
    d["kf_state"][K - 1, 12:15] += rng.normal(0, 0.03 * state_noise, 3)
    if bias0_sigma is not None:
        shift = np.asarray(d["kf_true"])[K - 1, 15:21]
        d["in_preint"][:, 61:67] -= shift
        b0 = rng.normal(0, bias0_sigma, 6)
        d["kf_state"][:, 15:21] = b0 + rng.normal(0, 0.1 * bias0_sigma, (K, 6))
        d["kf_state"][0, 15:21] = b0
    kf_imu[list(no_imu)] = 0
    kf_fixed[list(fixed)] = 1
    keep = np.ones(len(d["in_kf1"]), bool)
    for m in range(len(keep)):
        k1, k2 = int(d["in_kf1"][m]), int(d["in_kf2"][m])
        if not kf_imu[k1] or not kf_imu[k2] or k2 in gap:
            keep[m] = False
    for k in ("in_kf1", "in_kf2", "in_robust", "in_preint", "in_info", "in_info_g", "in_info_a"):
        d[k] = d[k][keep]
    if fixed_only_point:
        ek, el = d["edge_kf"], d["edge_point"]
        cand = [l for l in np.unique(el) if kf_fixed[ek[el == l]].any() and (~kf_fixed[ek[el == l]].astype(bool)).any()]
        assert cand, "no point is seen by a fixed and a free keyframe"
        l = cand[0]
        drop = (el == l) & (kf_fixed[ek] == 0)
        for k in ("edge_kf", "edge_point", "edge_stereo", "edge_inv_sigma2", "edge_close", "edge_obs"):
            d[k] = d[k][~drop]
        d["fixed_only_point"] = int(l)
    d["kf_fixed"], d["kf_imu"] = kf_fixed, kf_imu
    win = si.Window(d)
    return win, win.kf0[0, 15:21].copy()


def empty_map():
    """A map without keyframes (the batch entry point skips it)."""
    w, _ = make_map(1, 2, pts_per_kf=0)
    d = dict(w.d)
    for k in ("kf_fixed", "kf_imu"):
        d[k] = np.zeros(0, np.uint8)
    d["kf_state"] = np.zeros((0, si.KF))
    for k in ("in_kf1", "in_kf2", "in_robust"):
        d[k] = np.zeros(0, np.int32)
    for k, width in (("in_preint", si.PREINT), ("in_info", 81), ("in_info_g", 9), ("in_info_a", 9)):
        d[k] = np.zeros((0, width))
    return si.Window(d), np.zeros(6)


# ---------------------------------------------------------------------------------------------- the class method's flat-file scene
INV_SIGMA2 = (1.0 / (1.2 ** (2 * np.arange(8)))).astype(np.float32)


def class_scene(win, its, b_init, priors, loop_id=0, fix_local=False, stop=-1, extra_kf=True, bad_kf=None):
    """The flat-file scene of host_full_iba_smoke for a single-camera map: the keyframes in array order with ids 10, 12, ... growing with
    time, an extra keyframe beyond max_kf_id that also sees every point (extra_kf), keyframe bad_kf flagged bad (its inertial link and
    its observations are left out, :515, :659), fixed keyframes marked as bFixLocal finds them (mnBALocalForKF = maxKFid).
    stop: -1 no flag, 0 / 1 its value.  -> arrays (host/flatfile.h kinds by dtype)."""
    a, d = win.arrays, win.d
    assert "Trl" not in d, "the driver builds single-camera keyframes"
    K = win.n_kf
    n = K + (1 if extra_kf else 0)
    ids = np.array([10 + 2 * (K - 1 - k) for k in range(K)] + ([10 + 2 * K] if extra_kf else []), np.int32)
    max_id = int(ids[:K].max())
    Rcb, tcb = win.Rcb.reshape(3, 3), win.tcb
    Tcb = np.eye(4); Tcb[:3, :3] = Rcb; Tcb[:3, 3] = tcb
    kf0 = np.concatenate([win.kf0, win.kf0[:1]]) if extra_kf else win.kf0
    Tcw = np.zeros((n, 4, 4))
    for k in range(n):
        Rwb, twb = kf0[k, :9].reshape(3, 3), kf0[k, 9:12]
        Tcw[k] = np.eye(4); Tcw[k, :3, :3] = Rcb @ Rwb.T; Tcw[k, :3, 3] = -Rcb @ Rwb.T @ twb + tcb
    prev = -np.ones(n, np.int32); hasp = np.zeros(n, np.int32)
    pre = np.zeros((n, 67)); C = np.tile(np.eye(15), (n, 1, 1))
    for m in range(win.n_inertial):
        k1, k2 = int(a["in_kf1"][m]), int(a["in_kf2"][m])
        prev[k2] = k1; hasp[k2] = 1; pre[k2] = a["in_preint"][m]
        C[k2, :9, :9] = np.linalg.inv(a["in_info"][m].reshape(9, 9))
        C[k2, 9:12, 9:12] = np.linalg.inv(a["in_info_g"][m].reshape(3, 3)); C[k2, 12:15, 12:15] = np.linalg.inv(a["in_info_a"][m].reshape(3, 3))
    if extra_kf:
        prev[K] = 0
    imu = np.concatenate([a["kf_imu"], [1]])[:n].astype(np.int32)
    bad = np.zeros(n, np.int32)
    if bad_kf is not None:
        bad[bad_kf] = 1
    local = np.where(np.concatenate([a["kf_fixed"], [0]])[:n] != 0, max_id, 0).astype(np.int32)
    key_off = [0]; kx, ky, kur, koct = [], [], [], []
    ob_mp, ob_kf, ob_idx = [], [], []
    order = np.lexsort((a["edge_point"], a["edge_kf"]))
    per_kf = {k: [] for k in range(n)}
    for e in order:
        per_kf[int(a["edge_kf"][e])].append(int(e))
    if extra_kf:
        per_kf[K] = list(per_kf[0])
    for k in range(n):
        for i, e in enumerate(per_kf[k]):
            o = int(np.argmin(np.abs(INV_SIGMA2 - np.float32(a["edge_inv_sigma2"][e]))))
            kx.append(a["edge_obs"][e, 0]); ky.append(a["edge_obs"][e, 1]); kur.append(a["edge_obs"][e, 2] if a["edge_stereo"][e] == 1 else -1.0); koct.append(o)
            ob_mp.append(int(a["edge_point"][e])); ob_kf.append(k); ob_idx.append(i)
        key_off.append(len(kx))
    f32 = lambda x: np.asarray(x, np.float32)
    return dict(its=np.array([its], np.int32), fix_local=np.array([int(fix_local)], np.int32), loop_id=np.array([loop_id], np.int32),
                b_init=np.array([int(b_init)], np.int32), stop=np.array([stop], np.int32), prior=f32(priors), max_kf_id=np.array([max_id], np.int32),
                cam=f32(win.cam), inv_sigma2=INV_SIGMA2, Tcb=f32(Tcb), kf_id=ids, kf_prev=prev, kf_bad=bad, kf_imu=imu, kf_local=local,
                kf_fixedfor=np.zeros(n, np.int32), Tcw=f32(Tcw), vel=f32(kf0[:, 12:15]), bias=f32(kf0[:, 15:21]), has_preint=hasp,
                pre_dT=f32(pre[:, 0]), pre_dR=f32(pre[:, 1:10]), pre_dV=f32(pre[:, 10:13]), pre_dP=f32(pre[:, 13:16]), pre_JRg=f32(pre[:, 16:25]),
                pre_JVg=f32(pre[:, 25:34]), pre_JVa=f32(pre[:, 34:43]), pre_JPg=f32(pre[:, 43:52]), pre_JPa=f32(pre[:, 52:61]), pre_b=f32(pre[:, 61:67]),
                pre_C=f32(C), key_off=np.array(key_off, np.int32), key_x=f32(kx), key_y=f32(ky), key_ur=f32(kur), key_oct=np.array(koct, np.int32),
                mp_pos=f32(win.pts0), ob_mp=np.array(ob_mp, np.int32), ob_kf=np.array(ob_kf, np.int32), ob_idx=np.array(ob_idx, np.int32))


def abi_map_of_scene(win, sc, out, b_init, bad_kf=None):
    """The orbhip_iba_window the class method packs from a scene: the map's own keyframes (the extra one is beyond max_kf_id), the float
    values the stand-in classes hold, body poses and edge information as the driver reports them, a bad keyframe's link and
    observations left out.  -> (synth_iba.Window, shared bias [6])."""
    a = win.arrays
    K = win.n_kf
    d = dict(win.d)
    kf = np.zeros((K, 21))
    kf[:, :9] = out["Rwb"].reshape(-1, 9)[:K]; kf[:, 9:12] = out["twb"].reshape(-1, 3)[:K]
    kf[:, 12:15] = sc["vel"][:K]; kf[:, 15:21] = sc["bias"][:K]
    kf[a["kf_imu"] == 0, 12:] = 0
    d["kf_state"] = kf
    d["points"] = sc["mp_pos"].astype(np.float64).reshape(-1, 3)
    Tcb = sc["Tcb"].astype(np.float64)
    d["Rcb"], d["tcb"] = Tcb[:3, :3], Tcb[:3, 3]
    d["cam"] = tuple(float(x) for x in sc["cam"])
    info = out["info"].view(np.float64).reshape(-1, 81)
    keep_i = np.array([bad_kf is None or int(k2) != bad_kf for k2 in a["in_kf2"]], bool)
    d["in_preint"] = np.asarray(a["in_preint"], np.float32).astype(np.float64)[keep_i]
    d["in_info"] = info[a["in_kf2"]][keep_i]
    for key, o in (("in_info_g", 9), ("in_info_a", 12)):
        blk = sc["pre_C"].reshape(-1, 15, 15)[a["in_kf2"]][:, o:o + 3, o:o + 3].astype(np.float64)
        d[key] = np.linalg.inv(blk).astype(np.float32).astype(np.float64).reshape(-1, 9)[keep_i]
    for key in ("in_kf1", "in_kf2", "in_robust"):
        d[key] = np.asarray(a[key])[keep_i]
    keep_e = np.array([bad_kf is None or int(k) != bad_kf for k in a["edge_kf"]], bool)
    for key in ("edge_kf", "edge_point", "edge_stereo", "edge_close", "edge_obs"):
        d[key] = np.asarray(a[key])[keep_e]
    d["edge_inv_sigma2"] = np.asarray(a["edge_inv_sigma2"], np.float32).astype(np.float64)[keep_e]
    # pIncKF: the last keyframe of the map with mnId <= maxKFid, here the last row of the map
    return si.Window(d), kf[K - 1, 15:21].copy()
