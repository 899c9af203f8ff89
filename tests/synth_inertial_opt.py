"""Synthetic maps for Optimizer::InertialOptimization: keyframes on a smooth 6-DoF trajectory with real excitation (rotation about all
three axes, non-constant acceleration), a true gravity direction, a true scale (monocular maps store positions divided by it) and true
biases; one preintegration record per link, consistent with the true motion; initial values made as LocalMapping::InitializeIMU makes
them (src/LocalMapping.cc:1265-1301): velocities from position differences, Rwg from the summed -Rwb dV, scale 1, biases 0.
No oracle, no GPU code in here."""
import numpy as np
from synth_iba import _rot, KF, PREINT  # noqa: F401
from synth_pose_inertial import _spd, _clean

GRAVITY = float(np.float32(9.81))
IO_GLOBAL = 16


def _traj(rng):
    """p(t), v(t), R(t) of the body in the true (gravity-aligned) world: sums of sinusoids."""
    A = rng.uniform(0.3, 1.2, (3, 2)); W = rng.uniform(0.7, 2.6, (3, 2)); PH = rng.uniform(0, 2 * np.pi, (3, 2))
    B = rng.uniform(0.15, 0.6, 3); WB = rng.uniform(0.5, 1.9, 3); PB = rng.uniform(0, 2 * np.pi, 3)

    def p(t):
        return (A * np.sin(W * t + PH)).sum(1)

    def v(t):
        return (A * W * np.cos(W * t + PH)).sum(1)

    def R(t):
        a = B * np.sin(WB * t + PB)
        return _rot(np.array([0, 0, a[2]])) @ _rot(np.array([0, a[1], 0])) @ _rot(np.array([a[0], 0, 0]))
    return p, v, R


def make_map(seed, n_kf, mono=True, scale_true=None, noise=0.0, gaps=(), dt_range=(0.2, 0.45), bias_true=None, aligned=False):
    """-> dict(kf [n][21], link [n] uint8, preint [n][67], info [n][81], glob [16]: the call's inputs with InitializeIMU's seed values;
    truth: dict(Rwg, scale, bg, ba, vel [n][3] in map units)).  gaps: keyframe indices whose link is cut (a second chain starts there).
    noise: standard deviation factor of the preintegration noise (0: the truth is a zero-residual point).  aligned: the map frame is
    gravity-aligned already (Rwg = I: what overloads (b) and (c) assume, together with scale 1)."""
    rng = np.random.default_rng(seed)
    p_of, v_of, R_of = _traj(rng)
    Rwg_true = _rot(rng.normal(0, 0.35, 3))                    # map frame <- gravity-aligned frame
    if aligned:
        Rwg_true = np.eye(3)
    s_true = float(rng.uniform(1.6, 3.2)) if scale_true is None else float(scale_true)
    if not mono:
        s_true = 1.0
    bg = rng.normal(0, 0.01, 3) if bias_true is None else np.asarray(bias_true[0], np.float64)
    ba = rng.normal(0, 0.05, 3) if bias_true is None else np.asarray(bias_true[1], np.float64)
    g_w = np.array([0, 0, -GRAVITY])
    ts = np.concatenate([[0.0], np.cumsum(rng.uniform(dt_range[0], dt_range[1], max(n_kf - 1, 0)))])
    # metric states in the map frame (the map frame is the true world rotated by Rwg_true)
    Rm = [Rwg_true @ R_of(t) for t in ts]
    pm = [Rwg_true @ p_of(t) for t in ts]
    vm = [Rwg_true @ v_of(t) for t in ts]
    g_m = Rwg_true @ g_w
    kf = np.zeros((n_kf, KF)); link = np.zeros(n_kf, np.uint8)
    preint = np.zeros((n_kf, PREINT)); info = np.zeros((n_kf, 81))
    for k in range(n_kf):
        kf[k, 0:9] = Rm[k].reshape(-1)
        kf[k, 9:12] = pm[k] / s_true
        if k == 0 or k in gaps:
            continue
        link[k] = 1
        dt = ts[k] - ts[k - 1]
        R1 = Rm[k - 1]
        dR = R1.T @ Rm[k]
        dV = R1.T @ (vm[k] - vm[k - 1] - g_m * dt)
        dP = R1.T @ (pm[k] - pm[k - 1] - vm[k - 1] * dt - 0.5 * g_m * dt * dt)
        if noise:
            dR = dR @ _rot(rng.normal(0, 2e-4 * noise, 3)); dV = dV + rng.normal(0, 2e-3 * noise, 3); dP = dP + rng.normal(0, 5e-4 * noise, 3)
        JRg = -dt * (np.eye(3) + rng.normal(0, 0.03, (3, 3)))
        JVa = -dt * (np.eye(3) + rng.normal(0, 0.05, (3, 3)))
        JPa = -0.5 * dt * dt * (np.eye(3) + rng.normal(0, 0.05, (3, 3)))
        JVg = rng.normal(0, 0.3 * dt * dt, (3, 3))
        JPg = rng.normal(0, 0.1 * dt ** 3, (3, 3))
        # the record is linearised at bias 0; corrected to the true bias it gives the true deltas
        dR0 = dR @ _rot(JRg @ bg).T
        dV0 = dV - JVg @ bg - JVa @ ba
        dP0 = dP - JPg @ bg - JPa @ ba
        preint[k] = np.concatenate([[dt], dR0.reshape(-1), dV0, dP0, JRg.reshape(-1), JVg.reshape(-1), JVa.reshape(-1), JPg.reshape(-1),
                                    JPa.reshape(-1), np.zeros(3), np.zeros(3)])
        C = np.linalg.inv(_spd(rng, np.concatenate([rng.uniform(2e5, 4e6, 3), rng.uniform(2e4, 4e5, 3), rng.uniform(1e5, 3e6, 3)])))
        C = (0.5 * (C + C.T)).astype(np.float32).astype(np.float64)
        info[k] = _clean(np.linalg.pinv(C).astype(np.float32).astype(np.float64)).reshape(-1)
    truth = dict(Rwg=Rwg_true, scale=s_true, bg=bg, ba=ba, vel=np.array(vm).reshape(n_kf, 3) / s_true, g=g_m)
    # InitializeIMU's seed: velocities from position differences (each link sets both of its keyframes), Rwg from the summed -Rwb dV
    dirG = np.zeros(3)
    for k in range(n_kf):
        if not link[k]:
            continue
        dirG -= kf[k - 1, 0:9].reshape(3, 3) @ preint[k, 10:13]
        vel = (kf[k, 9:12] - kf[k - 1, 9:12]) / preint[k, 0]
        kf[k, 12:15] = vel; kf[k - 1, 12:15] = vel
    glob = np.zeros(IO_GLOBAL)
    Rwg0 = np.eye(3)
    if np.linalg.norm(dirG) > 0 and not aligned:
        dirG = dirG / np.linalg.norm(dirG)
        gI = np.array([0, 0, -1.0])
        v = np.cross(gI, dirG); nv = np.linalg.norm(v)
        if nv > 1e-12:
            Rwg0 = _rot(v * np.arccos(np.clip(gI @ dirG, -1, 1)) / nv)
    glob[0:9] = Rwg0.reshape(-1); glob[9] = 1.0
    return dict(kf=kf, link=link, preint=preint, info=info, glob=glob, truth=truth, mono=mono)


def refine_start(mp, angle_deg=15.0, scale_factor=1.4, seed=0):
    """The map with the truth's velocities and biases and a start for overload (d): Rwg `angle_deg` off the truth, scale off by
    `scale_factor`."""
    rng = np.random.default_rng(seed)
    t = mp["truth"]
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in mp.items()}
    out["kf"][:, 12:15] = t["vel"]
    out["kf"][:, 15:18] = t["bg"]; out["kf"][:, 18:21] = t["ba"]
    ax = rng.normal(0, 1, 2); ax = ax / np.linalg.norm(ax)
    out["glob"] = mp["glob"].copy()
    # the true Rwg takes (0, 0, -G) to the map's gravity: any rotation about z in front of it does too; perturb about an x-y axis
    out["glob"][0:9] = (t["Rwg"] @ _rot(np.deg2rad(angle_deg) * np.array([ax[0], ax[1], 0.0]))).reshape(-1)
    out["glob"][9] = t["scale"] * scale_factor
    out["glob"][10:13] = t["bg"]; out["glob"][13:16] = t["ba"]
    return out


def pack(maps):
    """A batch in the device call's layout: (kf_off [m+1] int32, kf [K][21], link [K], preint [K][67], info [K][81], glob [m][16])."""
    off = np.zeros(len(maps) + 1, np.int32)
    off[1:] = np.cumsum([len(m["kf"]) for m in maps])
    cat = lambda k, w, t: (np.concatenate([np.asarray(m[k], t).reshape(-1, w) for m in maps]) if off[-1] else np.zeros((0, w), t))  # noqa: E731
    return off, cat("kf", KF, np.float64), cat("link", 1, np.uint8).reshape(-1), cat("preint", PREINT, np.float64), cat("info", 81, np.float64), \
        np.array([m["glob"] for m in maps], np.float64).reshape(-1, IO_GLOBAL)


# ---------------------------------------------------------------------------------------------- scenes for the class (host smoke driver)
def write_flat(path, arrays):
    """host/flatfile.h: float arrays as float32, integer arrays as int32, uint8 arrays raw (doubles travel as their bytes)."""
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


def raw(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint8).reshape(-1)


def class_scene(mp, overload, mono=False, fixed_vel=False, priorG=1e2, priorA=1e6, seed=0, extra_kf=True, bad_kf=None, far_bias=()):
    """The flat-file scene of host_inertial_opt_smoke for a map: the keyframes in a shuffled order (Map::GetAllKeyFrames() promises none),
    ids 10, 12, 14, ... along the chain, an extra keyframe beyond max_kf_id (extra_kf), keyframe bad_kf marked bad (its edge is left
    out: a gap), keyframes far_bias with a gyro bias 0.02 off the front keyframe's.  -> (arrays, chain: scene row of chain position i)."""
    rng = np.random.default_rng(seed)
    n = len(mp["kf"])
    Rcb = _rot(np.array([0.02, -0.01, 1.55])); tcb = np.array([0.065, -0.02, 0.01])
    m = n + (1 if extra_kf else 0)
    perm = rng.permutation(m)                       # scene row r holds chain keyframe perm[r] (the extra one is chain index n)
    row_of = np.argsort(perm)
    ids = np.array([10 + 2 * k for k in range(m)])
    bias0 = np.concatenate([rng.normal(0, 0.002, 3), rng.normal(0, 0.003, 3)])
    A = {k: [] for k in ("kf_id", "kf_prev", "kf_bad", "Tcw", "vel", "bias", "has_preint", "pre_dT", "pre_dR", "pre_dV", "pre_dP", "pre_JRg", "pre_JVg",
                         "pre_JVa", "pre_JPg", "pre_JPa", "pre_b", "pre_C")}
    for r in range(m):
        k = int(perm[r])
        src = min(k, n - 1)
        Rwb, twb = mp["kf"][src, 0:9].reshape(3, 3), mp["kf"][src, 9:12] + (5.0 if k >= n else 0.0)
        Rcw = Rcb @ Rwb.T
        T = np.eye(4); T[:3, :3] = Rcw; T[:3, 3] = tcb - Rcw @ twb
        linked = k >= 1 and (k >= n or mp["link"][k])
        A["kf_id"].append(ids[k]); A["kf_prev"].append(int(row_of[k - 1]) if linked else -1)
        A["kf_bad"].append(1 if bad_kf is not None and k == bad_kf else 0)
        A["Tcw"].append(T.reshape(-1)); A["vel"].append(mp["kf"][src, 12:15])
        b = bias0.copy()
        if k in far_bias:
            b[0] += 0.02
        A["bias"].append(b)
        A["has_preint"].append(1 if linked else 0)
        pi = mp["preint"][src if linked and k < n else 0]
        if linked and k >= n:
            pi = mp["preint"][n - 1]
        A["pre_dT"].append(pi[0]); A["pre_dR"].append(pi[1:10]); A["pre_dV"].append(pi[10:13]); A["pre_dP"].append(pi[13:16])
        A["pre_JRg"].append(pi[16:25]); A["pre_JVg"].append(pi[25:34]); A["pre_JVa"].append(pi[34:43]); A["pre_JPg"].append(pi[43:52])
        A["pre_JPa"].append(pi[52:61]); A["pre_b"].append(pi[61:67])
        C = np.linalg.inv(_spd(rng, np.concatenate([rng.uniform(2e5, 4e6, 3), rng.uniform(2e4, 4e5, 3), rng.uniform(1e5, 3e6, 3),
                                                    rng.uniform(2e7, 2e8, 3), rng.uniform(2e4, 2e5, 3)])))
        A["pre_C"].append((0.5 * (C + C.T)).reshape(-1))
    arrays = {k: np.array(v, np.float64 if k not in ("kf_id", "kf_prev", "kf_bad", "has_preint") else np.int32) for k, v in A.items()}
    Tcb = np.eye(4); Tcb[:3, :3] = Rcb; Tcb[:3, 3] = tcb
    arrays.update(overload=np.array([overload], np.int32), mono=np.array([int(mono)], np.int32), fixed_vel=np.array([int(fixed_vel)], np.int32),
                  prior=np.array([priorG, priorA], np.float64), max_kf_id=np.array([ids[n - 1]], np.int32), Tcb=Tcb.reshape(-1),
                  list=np.array([int(row_of[k]) for k in range(n)][::-1], np.int32),
                  Rwg=raw(mp["glob"][0:9]), scale=raw(mp["glob"][9:10]), bg=raw(np.array([7.0, 8.0, 9.0])), ba=raw(np.array([-7.0, -8.0, -9.0])))
    return arrays, row_of[:n]
