"""numpy model of Optimizer::FullInertialBA's optimisation (reference src/Optimizer.cc:420-851; vertices and edges include/G2oTypes.h,
src/G2oTypes.cc; Levenberg-Marquardt Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp), written over a dtype parameter
(float64 and longdouble).  TEST INFRASTRUCTURE ONLY: no device code, no oracle code.

A map is a synth_iba.Window (the arrays of orbhip_iba_window).  Two modes:
  shared (bInit):   one gyro-bias and one accelerometer-bias vertex for the map, never fixed, read by every EdgeInertial; EdgePriorGyro /
                    EdgePriorAcc on them (error 0 - b, information prior I, Jacobian written as +I (G2oTypes.cc:971-983), no robust
                    kernel); no EdgeGyroRW / EdgeAccRW.  Unknowns: 6 per free keyframe, 9 with IMU states, the shared 6 last.
  per keyframe:     15 / 6 unknowns per free keyframe, EdgeGyroRW / EdgeAccRW (J = [-I, I]) beside every EdgeInertial.
g2o's activity rule: an edge is active iff one of its vertices is not fixed.  With shared biases an inertial edge between two fixed
keyframes is therefore active (chi2 and the shared block); without them it is not.  A point that only fixed keyframes see is no
vertex (bAllFixed, :751-755): its edges are left out, it is not moved.
The schedule is one optimize(its): lambda_0 given, rho = (chi2 - chi2_trial) / (dx . (lambda dx + b) + 1e-3), the fork's stop after
three iterations that gain less than 1e-3 of chi2.  optimize() records a trace per iteration; decisive_prefix() gives the
iterations whose decisions do not hang on rounding.  Nothing is fixed in the reference's initialisation calls, so the system has
four gauge directions (translation, yaw about gravity) that only lambda holds: see remove_gauge()."""
import numpy as np

LD = np.longdouble
END_ITERATIONS, END_TRIALS, END_NBAD = 0, 1, 2
GRAVITY = float(np.float32(9.81))
GROUPS = ("R", "t", "v", "bias", "X", "chi", "lam")


def default_params(its, b_init, prior_g=1e2, prior_a=1e6, lambda_init=1e-5, max_trials=100):
    """The parameters of a FullInertialBA call (priors are floats in the reference's signature)."""
    return dict(iterations=int(its), lambda_init=float(lambda_init), max_trials=int(max_trials), shared=bool(b_init),
                prior_g=float(np.float32(prior_g)) if b_init else 0.0, prior_a=float(np.float32(prior_a)) if b_init else 0.0,
                robust="all", all_fixed="drop")


def local_params(large=False):
    """LocalInertialBA's optimize() through the same model: the window's own robust flags, lambda_0 = 1 (1e-2 when bLarge), and no
    bAllFixed rule (its points are those of the free keyframes; a point that only fixed keyframes see stays a vertex)."""
    return dict(iterations=4 if large else 10, lambda_init=1e-2 if large else 1.0, max_trials=100, shared=False, prior_g=0.0, prior_a=0.0,
                robust="window", all_fixed="keep")


# ---------------------------------------------------------------------------------------------- SO(3), batched, dtype kept
def skew(w):
    S = np.zeros(w.shape[:-1] + (3, 3), w.dtype)
    S[..., 0, 1] = -w[..., 2]; S[..., 0, 2] = w[..., 1]; S[..., 1, 0] = w[..., 2]
    S[..., 1, 2] = -w[..., 0]; S[..., 2, 0] = -w[..., 1]; S[..., 2, 1] = w[..., 0]
    return S


def inv3(A):
    c0 = A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1]
    c1 = A[..., 1, 2] * A[..., 2, 0] - A[..., 1, 0] * A[..., 2, 2]
    c2 = A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]
    det = A[..., 0, 0] * c0 + A[..., 0, 1] * c1 + A[..., 0, 2] * c2
    I = np.zeros_like(A)
    I[..., 0, 0] = c0; I[..., 0, 1] = A[..., 0, 2] * A[..., 2, 1] - A[..., 0, 1] * A[..., 2, 2]; I[..., 0, 2] = A[..., 0, 1] * A[..., 1, 2] - A[..., 0, 2] * A[..., 1, 1]
    I[..., 1, 0] = c1; I[..., 1, 1] = A[..., 0, 0] * A[..., 2, 2] - A[..., 0, 2] * A[..., 2, 0]; I[..., 1, 2] = A[..., 0, 2] * A[..., 1, 0] - A[..., 0, 0] * A[..., 1, 2]
    I[..., 2, 0] = c2; I[..., 2, 1] = A[..., 0, 1] * A[..., 2, 0] - A[..., 0, 0] * A[..., 2, 1]; I[..., 2, 2] = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    return I / det[..., None, None]


def nearest_rot(R):
    """IMU::NormalizeRotation / ExpSO3's clean-up (U V^T of an SVD): Newton's polar iteration to convergence."""
    for _ in range(6):
        R = (R + np.swapaxes(inv3(R), -1, -2)) / 2
    return R


def _rodrigues(w, a, b):
    W = skew(w)
    return np.eye(3, dtype=w.dtype) + a[..., None, None] * W + b[..., None, None] * (W @ W)


def exp_so3(w, eps, normalize):
    """ImuTypes.cc:48-60 (eps 1e-4, as computed) / G2oTypes.cc:991-1008 (eps 1e-5, made a rotation)."""
    t = w.dtype.type
    d2 = np.sum(w * w, -1); d = np.sqrt(d2)
    small = d < eps
    ds, d2s = np.where(small, t(1), d), np.where(small, t(1), d2)
    R = _rodrigues(w, np.where(small, t(1), np.sin(ds) / ds), np.where(small, t(0.5), (1 - np.cos(ds)) / d2s))
    return nearest_rot(R) if normalize else R


def log_so3(R):
    """G2oTypes.cc:1010-1025."""
    t = R.dtype.type
    w = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2
    c = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) * t(0.5)
    out = (c > 1) | (c < -1)
    th = np.arccos(np.where(out, t(0), c)); s = np.sin(th)
    keep = out | (np.abs(s) < 1e-5)
    f = np.where(keep, t(1), th / np.where(keep, t(1), s))
    return w * f[..., None]


def inv_right_jac(v):
    """G2oTypes.cc:1032-1044."""
    t = v.dtype.type
    d2 = np.sum(v * v, -1); d = np.sqrt(d2)
    small = d < 1e-5
    ds, d2s = np.where(small, t(1), d), np.where(small, t(1), d2)
    return _rodrigues(v, np.where(small, t(0), t(0.5) + 0 * d), np.where(small, t(0), 1 / d2s - (1 + np.cos(ds)) / (2 * ds * np.sin(ds))))


def right_jac(v):
    """G2oTypes.cc:1046-1061."""
    t = v.dtype.type
    d2 = np.sum(v * v, -1); d = np.sqrt(d2)
    small = d < 1e-5
    ds, d2s = np.where(small, t(1), d), np.where(small, t(1), d2)
    return _rodrigues(v, np.where(small, t(0), -(1 - np.cos(ds)) / d2s), np.where(small, t(0), (ds - np.sin(ds)) / (d2s * ds)))


# ---------------------------------------------------------------------------------------------- the problem
class Problem:
    """The constant part of a map in `dtype`: topology, observations, preintegrations, the unknowns' layout."""

    def __init__(self, win, prm, dtype, smooth=False):
        self.dtype = dt = np.dtype(dtype)
        self.smooth = smooth                                 # KannalaBrandt8's float atan2f left out (difference quotients)
        a, d = win.arrays, win.d
        self.shared = bool(prm["shared"])
        self.nk, self.L = win.n_kf, win.n_points
        self.fixed = a["kf_fixed"] != 0
        self.imu = a["kf_imu"] != 0
        c = lambda x: np.asarray(x, np.float64).astype(dt)
        Rcb, tcb = c(win.Rcb).reshape(3, 3), c(win.tcb)
        self.cam = [dict(Rcb=Rcb, tcb=tcb, f=c(win.cam[:4]), model=int(d.get("camera_model", 0)), kb=c(d.get("kb", (0, 0, 0, 0))))]
        self.bf = c(win.cam[4])
        if "Trl" in d:                                       # Rcb[1] = Rrl Rcb[0], tcb[1] = Rrl tcb[0] + trl (G2oTypes.cc:57-67)
            Trl = c(d["Trl"]).reshape(3, 4)
            self.cam.append(dict(Rcb=Trl[:, :3] @ Rcb, tcb=Trl[:, :3] @ tcb + Trl[:, 3], f=c(d["cam2"]), model=int(d.get("camera2_model", 0)),
                                 kb=c(d.get("kb2", (0, 0, 0, 0)))))
        # visual edges; those of a point no free keyframe sees are left out (bAllFixed)
        ek, el = a["edge_kf"].astype(np.int64), a["edge_point"].astype(np.int64)
        free_seen = np.zeros(self.L, bool)
        free_seen[el[~self.fixed[ek]]] = True
        keep = free_seen[el] if prm.get("all_fixed", "drop") == "drop" else np.ones(len(el), bool)
        self.ek, self.el = ek[keep], el[keep]
        self.etype = a["edge_stereo"].astype(np.int64)[keep]
        self.obs = c(a["edge_obs"]).reshape(-1, 3)[keep]
        self.is2 = c(a["edge_inv_sigma2"])[keep]
        self.E = len(self.ek)
        self.active_pt = np.bincount(self.el, minlength=self.L) > 0
        # inertial edges
        k1, k2 = a["in_kf1"].astype(np.int64), a["in_kf2"].astype(np.int64)
        keep_i = np.ones(len(k1), bool) if self.shared else ~(self.fixed[k1] & self.fixed[k2])
        self.k1, self.k2 = k1[keep_i], k2[keep_i]
        self.M = len(self.k1)
        self.pre = c(a["in_preint"]).reshape(-1, 67)[keep_i]
        self.info = c(a["in_info"]).reshape(-1, 9, 9)[keep_i]
        self.info_g = c(a["in_info_g"]).reshape(-1, 3, 3)[keep_i] if not self.shared else None
        self.info_a = c(a["in_info_a"]).reshape(-1, 3, 3)[keep_i] if not self.shared else None
        self.robust = np.ones(self.M, bool) if prm["robust"] == "all" else (a["in_robust"] != 0)[keep_i]
        self.prior_g, self.prior_a = dt.type(prm["prior_g"]), dt.type(prm["prior_a"])
        # unknowns: keyframe blocks in keyframe order, the shared biases last
        self.freek = np.flatnonzero(~self.fixed)
        wide = 9 if self.shared else 15
        dims = np.where(self.imu[self.freek], wide, 6)
        self.dims = dims
        off = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
        self.xoff = -np.ones(self.nk, np.int64); self.xoff[self.freek] = off[:-1]
        self.blk = -np.ones(self.nk, np.int64); self.blk[self.freek] = np.arange(len(self.freek))
        self.n = int(off[-1]) + (6 if self.shared else 0)
        self.os = int(off[-1])
        # thHuberMono = sqrt(5.991) etc. are floats handed to setDelta(double) (:629-630); delta^2 is their double product
        dm, ds = float(np.sqrt(np.float32(5.991))), float(np.sqrt(np.float32(7.815)))
        st = self.etype == 1
        self.delta = np.where(st, dt.type(ds), dt.type(dm)); self.dsqr = np.where(st, dt.type(ds * ds), dt.type(dm * dm))
        di = float(np.sqrt(16.92))
        self.delta_i, self.dsqr_i = dt.type(di), dt.type(di * di)
        # Schur complement: every ordered pair of free-keyframe edges of one point
        fe = np.flatnonzero(self.blk[self.ek] >= 0)
        self.fe = fe
        self.bf_, self.pf = self.blk[self.ek[fe]], self.el[fe]
        self.cols6 = self.xoff[self.ek[fe]][:, None] + np.arange(6)
        if len(fe):
            order = np.argsort(self.pf, kind="stable")
            lf = self.pf[order]
            starts = np.flatnonzero(np.r_[True, lf[1:] != lf[:-1]])
            cnt = np.diff(np.r_[starts, len(lf)])
            c2 = cnt * cnt
            grp = np.repeat(np.arange(len(cnt)), c2)
            k = np.arange(int(c2.sum())) - np.repeat(np.cumsum(c2) - c2, c2)
            self.i1 = order[starts[grp] + k // cnt[grp]]; self.i2 = order[starts[grp] + k % cnt[grp]]
        else:
            self.i1 = self.i2 = np.zeros(0, np.int64)

    def initial_state(self, win, shared_bias=None):
        dt = self.dtype
        kf = np.asarray(win.kf0, np.float64).astype(dt).reshape(-1, 21)
        S = dict(R=kf[:, :9].reshape(-1, 3, 3).copy(), t=kf[:, 9:12].copy(), v=kf[:, 12:15].copy(), bg=kf[:, 15:18].copy(), ba=kf[:, 18:21].copy(),
                 X=np.asarray(win.pts0, np.float64).astype(dt).reshape(-1, 3).copy(), sb=np.zeros(6, dt))
        if self.shared:
            S["sb"] = np.asarray(shared_bias, np.float64).astype(dt).reshape(6).copy()
        return S

    def edge_bias(self, S):
        """(gyro, accelerometer) bias vertices of every inertial edge's FIRST keyframe (or the shared pair)."""
        if self.shared:
            return np.broadcast_to(S["sb"][:3], (self.M, 3)), np.broadcast_to(S["sb"][3:], (self.M, 3))
        return S["bg"][self.k1], S["ba"][self.k1]


def project(P, cam, X, smooth=False):
    """GeometricCamera::project / projectJac (Pinhole.cpp:41-47, :81-91; KannalaBrandt8.cpp:52-69, :166-195) -> uv [m,2], J [m,2,3]."""
    dt = X.dtype; t = dt.type
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    fx, fy, cx, cy = cam["f"]
    J = np.zeros((len(X), 2, 3), dt)
    if cam["model"] == 0:
        uv = np.stack([fx * x / z + cx, fy * y / z + cy], -1)
        J[:, 0, 0] = fx / z; J[:, 0, 2] = -fx * x / (z * z); J[:, 1, 1] = fy / z; J[:, 1, 2] = -fy * y / (z * z)
        return uv, J
    k = cam["kb"]
    r2 = x * x + y * y; r = np.sqrt(r2)
    if smooth:
        th_p, psi = np.arctan2(r, z), np.arctan2(y, x)
    else:                                                    # atan2f / sqrtf: the projection's angles are floats
        f32 = lambda v: np.asarray(v).astype(np.float32)
        th_p = np.arctan2(np.sqrt(f32(r2)).astype(np.float64), f32(z).astype(np.float64)).astype(np.float32).astype(dt)
        psi = np.arctan2(f32(y).astype(np.float64), f32(x).astype(np.float64)).astype(np.float32).astype(dt)
    t2 = th_p * th_p
    rr = th_p * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    uv = np.stack([fx * rr * np.cos(psi) + cx, fy * rr * np.sin(psi) + cy], -1)
    th = np.arctan2(r, z)                                    # projectJac works in double
    t2 = th * th
    f = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    fd = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
    z2 = z * z; r3 = r2 * r; q = r2 * (r2 + z2)
    J[:, 0, 0] = fx * (fd * z * x * x / q + f * y * y / r3)
    J[:, 1, 0] = fy * (fd * z * y * x / q - f * y * x / r3)
    J[:, 0, 1] = fx * (fd * z * y * x / q - f * y * x / r3)
    J[:, 1, 1] = fy * (fd * z * y * y / q + f * x * x / r3)
    J[:, 0, 2] = -fx * fd * x / (r2 + z2); J[:, 1, 2] = -fy * fd * y / (r2 + z2)
    return uv, J


def visual(P, S, jac=False):
    """EdgeMono / EdgeStereo (G2oTypes.h:349-482, G2oTypes.cc:349-423): err [E,3] (row 2 zero unless stereo) and, with jac, the
    Jacobians w.r.t. the point [E,3,3] and the pose's (rotation, translation) [E,3,6]."""
    dt = P.dtype
    err = np.zeros((P.E, 3), dt)
    Jx = np.zeros((P.E, 3, 3), dt) if jac else None
    Jp = np.zeros((P.E, 3, 6), dt) if jac else None
    Rbw = np.swapaxes(S["R"], 1, 2)
    for ci, cam in enumerate(P.cam):
        sel = np.flatnonzero((P.etype == 2) == (ci == 1))
        if not len(sel):
            continue
        k, l = P.ek[sel], P.el[sel]
        Xb = np.einsum("eab,eb->ea", Rbw[k], S["X"][l] - S["t"][k])
        Xc = Xb @ cam["Rcb"].T + cam["tcb"]
        uv, pj2 = project(P, cam, Xc, P.smooth)
        st = P.etype[sel] == 1
        err[sel, :2] = P.obs[sel, :2] - uv
        err[sel, 2] = np.where(st, P.obs[sel, 2] - (uv[:, 0] - P.bf / Xc[:, 2]), 0)
        if jac:
            pj = np.zeros((len(sel), 3, 3), dt)
            pj[:, :2] = pj2
            pj[st, 2] = pj2[st, 0]
            pj[st, 2, 2] += P.bf / (Xc[st, 2] * Xc[st, 2])
            PR = pj @ cam["Rcb"]
            Jx[sel] = -PR @ Rbw[k]
            Jp[sel, :, :3] = -PR @ skew(Xb)                 # Xb' = Xb + [Xb]x ur - ut under Rwb Exp(ur), twb + Rwb ut
            Jp[sel, :, 3:] = PR
    return err, Jx, Jp


def inertial(P, S, jac=False):
    """EdgeInertial (G2oTypes.cc:720-800) -> err [M,9] and, with jac, J [M,9,24] over (pose1 6, v1 3, bg 3, ba 3, pose2 6, v2 3)."""
    dt = P.dtype; t = dt.type
    M = P.M
    if M == 0:
        return np.zeros((0, 9), dt), np.zeros((0, 9, 24), dt)
    p = P.pre
    dT = p[:, 0]
    m33 = lambda o: p[:, o:o + 9].reshape(-1, 3, 3)
    dR0, dV0, dP0 = m33(1), p[:, 10:13], p[:, 13:16]
    JRg, JVg, JVa, JPg, JPa = m33(16), m33(25), m33(34), m33(43), m33(52)
    bg, ba = P.edge_bias(S)
    dbg, dba = bg - p[:, 61:64], ba - p[:, 64:67]
    mv = lambda A, x: np.einsum("mab,mb->ma", A, x)
    w = mv(JRg, dbg)
    dR = nearest_rot(dR0 @ exp_so3(w, 1e-4, False))          # GetDeltaRotation (ImuTypes.cc:351-358)
    dV = dV0 + mv(JVg, dbg) + mv(JVa, dba)
    dP = dP0 + mv(JPg, dbg) + mv(JPa, dba)
    R1, R2 = S["R"][P.k1], S["R"][P.k2]
    R1t = np.swapaxes(R1, 1, 2)
    g = np.array([0, 0, -GRAVITY], np.float64).astype(dt)
    eR = np.swapaxes(dR, 1, 2) @ R1t @ R2
    er = log_so3(eR)
    va = mv(R1t, S["v"][P.k2] - S["v"][P.k1] - g * dT[:, None])
    vb = mv(R1t, S["t"][P.k2] - S["t"][P.k1] - S["v"][P.k1] * dT[:, None] - g * (dT * dT / 2)[:, None])
    err = np.concatenate([er, va - dV, vb - dP], 1)
    if not jac:
        return err, None
    J = np.zeros((M, 9, 24), dt)
    iJr = inv_right_jac(er)
    I3 = np.eye(3, dtype=dt)
    J[:, 0:3, 0:3] = -iJr @ np.swapaxes(R2, 1, 2) @ R1
    J[:, 3:6, 0:3] = skew(va)
    J[:, 6:9, 0:3] = skew(vb)
    J[:, 6:9, 3:6] = -I3
    J[:, 3:6, 6:9] = -R1t
    J[:, 6:9, 6:9] = -R1t * dT[:, None, None]
    J[:, 0:3, 9:12] = -iJr @ np.swapaxes(eR, 1, 2) @ right_jac(w) @ JRg
    J[:, 3:6, 9:12] = -JVg
    J[:, 6:9, 9:12] = -JPg
    J[:, 3:6, 12:15] = -JVa
    J[:, 6:9, 12:15] = -JPa
    J[:, 0:3, 15:18] = iJr
    J[:, 6:9, 18:21] = R1t @ R2
    J[:, 3:6, 21:24] = R1t
    return err, J


def inertial_columns(P, m):
    """Unknown of every column of edge m's 9 x 24 Jacobian, -1 = fixed."""
    o1, o2 = P.xoff[P.k1[m]], P.xoff[P.k2[m]]
    c = -np.ones(24, np.int64)
    if o1 >= 0:
        c[0:9] = o1 + np.arange(9)
    if P.shared:
        c[9:15] = P.os + np.arange(6)
    elif o1 >= 0:
        c[9:15] = o1 + 9 + np.arange(6)
    if o2 >= 0:
        c[15:24] = o2 + np.arange(9)
    return c


def _rho(chi, delta, dsqr):
    with np.errstate(invalid="ignore"):
        return np.where(chi <= dsqr, chi, 2 * np.sqrt(chi) * delta - dsqr)


def _rho1(chi, delta, dsqr):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(chi <= dsqr, chi.dtype.type(1), delta / np.sqrt(chi))


def evaluate(P, S):
    """computeActiveErrors + activeRobustChi2 -> dict(chi, the per-edge pieces)."""
    ev, _, _ = visual(P, S)
    chi_v = P.is2 * np.sum(ev * ev, 1)
    ei, _ = inertial(P, S)
    chi_i = np.einsum("ma,mab,mb->m", ei, P.info, ei) if P.M else np.zeros(0, P.dtype)
    chi = np.sum(_rho(chi_v, P.delta, P.dsqr)) + np.sum(np.where(P.robust, _rho(chi_i, P.delta_i, P.dsqr_i), chi_i))
    out = dict(ev=ev, chi_v=chi_v, ei=ei, chi_i=chi_i)
    if P.shared:
        sb = S["sb"]
        chi = chi + P.prior_g * (sb[:3] @ sb[:3]) + P.prior_a * (sb[3:] @ sb[3:])
    elif P.M:
        eg, ea = S["bg"][P.k2] - S["bg"][P.k1], S["ba"][P.k2] - S["ba"][P.k1]
        chi = chi + np.sum(np.einsum("ma,mab,mb->m", eg, P.info_g, eg)) + np.sum(np.einsum("ma,mab,mb->m", ea, P.info_a, ea))
        out.update(eg=eg, ea=ea)
    out["chi"] = chi
    return out


def build(P, S, ev):
    """buildSystem: the keyframe-side H [n,n] and b [n], the points' Hll [L,3,3], bl [L,3] and the blocks W [free edges,6,3]."""
    dt = P.dtype
    n = P.n
    _, Jx, Jp = visual(P, S, True)
    w = _rho1(ev["chi_v"], P.delta, P.dsqr) * P.is2
    r = ev["ev"]
    Hll = np.zeros((P.L, 3, 3), dt); bl = np.zeros((P.L, 3), dt)
    np.add.at(Hll, P.el, np.einsum("eda,e,edb->eab", Jx, w, Jx))
    np.add.at(bl, P.el, -np.einsum("eda,e,ed->ea", Jx, w, r))
    H = np.zeros((n, n), dt); b = np.zeros(n, dt)
    fe = P.fe
    c6 = P.cols6
    if len(fe):
        np.add.at(H, (c6[:, :, None], c6[:, None, :]), np.einsum("eda,e,edb->eab", Jp[fe], w[fe], Jp[fe]))
        np.add.at(b, c6, -np.einsum("eda,e,ed->ea", Jp[fe], w[fe], r[fe]))
    W = np.einsum("eda,e,edb->eab", Jp[fe], w[fe], Jx[fe])
    _, J = inertial(P, S, True)
    wi = np.where(P.robust, _rho1(ev["chi_i"], P.delta_i, P.dsqr_i), dt.type(1)) if P.M else None
    Jrw = np.concatenate([-np.eye(3, dtype=dt), np.eye(3, dtype=dt)], 1)
    for m in range(P.M):
        cols = inertial_columns(P, m)
        keep = cols >= 0
        if keep.any():
            Jk, ck = J[m][:, keep], cols[keep]
            Om = wi[m] * P.info[m]
            H[np.ix_(ck, ck)] += Jk.T @ (Om @ Jk)
            b[ck] += -(Jk.T @ (Om @ ev["ei"][m]))
        if not P.shared:                                     # EdgeGyroRW / EdgeAccRW (G2oTypes.h:642-651, :684-687)
            o1, o2 = P.xoff[P.k1[m]], P.xoff[P.k2[m]]
            for s, Om, e in ((9, P.info_g[m], ev["eg"][m]), (12, P.info_a[m], ev["ea"][m])):
                cols = np.concatenate([o1 + s + np.arange(3) if o1 >= 0 else -np.ones(3, np.int64), o2 + s + np.arange(3) if o2 >= 0 else -np.ones(3, np.int64)])
                keep = cols >= 0
                Jk, ck = Jrw[:, keep], cols[keep]
                H[np.ix_(ck, ck)] += Jk.T @ (Om @ Jk)
                b[ck] += -(Jk.T @ (Om @ e))
    if P.shared:                                             # the two prior edges: e = 0 - b, J = +I: H += prior I, b += -J^T Omega e = prior b
        o = P.os
        pr = np.concatenate([np.full(3, P.prior_g), np.full(3, P.prior_a)]).astype(dt)
        H[o + np.arange(6), o + np.arange(6)] += pr
        b[o:o + 6] += pr * S["sb"]
    return dict(H=H, b=b, Hll=Hll, bl=bl, W=W)


def ldlt_solve(A, b):
    """LDL^T without pivoting -> x or None (a pivot that is not positive and finite)."""
    n = len(b)
    dt = A.dtype
    Lm = np.zeros((n, n), dt); d = np.zeros(n, dt)
    for j in range(n):
        v = Lm[j, :j] * d[:j]
        d[j] = A[j, j] - np.dot(Lm[j, :j], v)
        if not (d[j] > 0 and np.isfinite(d[j])):
            return None
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ v) / d[j]
    y = np.zeros(n, dt)
    for i in range(n):
        y[i] = b[i] - np.dot(Lm[i, :i], y[:i])
    y /= d
    x = np.zeros(n, dt)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - np.dot(Lm[i + 1:, i], x[i + 1:])
    return x


def solve(P, sysm, lam):
    """One trial's linear solve through the landmark Schur complement -> (x [n], xl [L,3]) or None."""
    dt = P.dtype
    H, b, Hll, bl, W = sysm["H"], sysm["b"], sysm["Hll"], sysm["bl"], sysm["W"]
    act = P.active_pt
    Di = np.zeros((P.L, 3, 3), dt)
    if act.any():
        Di[act] = inv3(Hll[act] + lam * np.eye(3, dtype=dt))
    S = H + lam * np.eye(P.n, dtype=dt)
    bs = b.copy()
    if len(P.fe):
        Y = W @ Di[P.pf]
        np.add.at(bs, P.cols6, -np.einsum("eac,ec->ea", Y, bl[P.pf]))
        nb = len(P.freek)
        S6 = np.zeros((nb, nb, 6, 6), dt)
        for c in range(0, len(P.i1), 200000):
            a_, b_ = P.i1[c:c + 200000], P.i2[c:c + 200000]
            np.add.at(S6, (P.bf_[a_], P.bf_[b_]), -np.einsum("eac,ebc->eab", Y[a_], W[b_]))
        rows = P.xoff[P.freek][:, None] + np.arange(6)
        S[rows[:, None, :, None], rows[None, :, None, :]] += S6
    x = ldlt_solve(S, bs) if P.n else np.zeros(0, dt)
    if x is None:
        return None
    cl = bl.copy()
    if len(P.fe):
        np.add.at(cl, P.pf, -np.einsum("eab,ea->eb", W, x[P.cols6]))
    xl = np.einsum("lab,lb->la", Di, cl)
    return x, xl


def apply_step(P, S, x, xl):
    """oplus: ImuCamPose::Update (G2oTypes.cc:192-220: twb += Rwb ut, Rwb <- Rwb Exp(ur)); velocities, biases and points add."""
    N = {k: v.copy() for k, v in S.items()}
    fk = P.freek
    o = P.xoff[fk]
    ur = x[o[:, None] + np.arange(3)]; ut = x[o[:, None] + 3 + np.arange(3)]
    N["t"][fk] = S["t"][fk] + np.einsum("kab,kb->ka", S["R"][fk], ut)
    N["R"][fk] = S["R"][fk] @ exp_so3(ur, 1e-5, True)
    fi = fk[P.imu[fk]]
    oi = P.xoff[fi]
    N["v"][fi] = S["v"][fi] + x[oi[:, None] + 6 + np.arange(3)]
    if P.shared:
        N["sb"] = S["sb"] + x[P.os:P.os + 6]
    else:
        N["bg"][fi] = S["bg"][fi] + x[oi[:, None] + 9 + np.arange(3)]
        N["ba"][fi] = S["ba"][fi] + x[oi[:, None] + 12 + np.arange(3)]
    N["X"] = S["X"] + np.where(P.active_pt[:, None], xl, 0)
    return N


def state_out(P, S):
    """(kf [nk,21], X [L,3], shared bias [6]) as the call returns them: with shared biases every keyframe with IMU states holds them."""
    bg, ba = S["bg"].copy(), S["ba"].copy()
    if P.shared:
        bg[P.imu] = S["sb"][:3]; ba[P.imu] = S["sb"][3:]
    kf = np.concatenate([S["R"].reshape(-1, 9), S["t"], S["v"], bg, ba], 1)
    return kf, S["X"].copy(), S["sb"].copy()


def optimize(win, prm, dtype=np.float64, shared_bias=None):
    """-> dict(kf, X, sb (in `dtype`), iterations, trials, reason, chi_first, chi_last (of the returned estimate), chi_eval (of the last
    trial, accepted or not: what activeRobustChi2 gives after optimize()), lam, n, trace).  trace: one dict per iteration
    with chi and lam after it, trials, accepted (per trial), dchi = |chi before - chi after| and step: per group the largest change
    proposed by a trial of the iteration that moved chi2 by less than 1e-9 of it (one that rounding may accept or reject)."""
    P = Problem(win, prm, dtype)
    t = P.dtype.type
    S = P.initial_state(win, shared_bias)
    ev = evaluate(P, S)
    chi_cur = ev["chi"]
    chi_first = chi_eval = chi_cur
    lam, ni, nbad = t(prm["lambda_init"]), t(2), 0
    iters = trials = 0
    reason = END_ITERATIONS
    trace = []
    for it in range(prm["iterations"]):
        iters += 1
        ini = chi_cur
        sysm = build(P, S, ev)
        rho, q, acc = t(0), 0, []
        step = {g: 0.0 for g in ("R", "t", "v", "bias", "X")}
        while True:
            r = solve(P, sysm, lam)
            good = False
            if r is not None:
                x, xl = r
                St = apply_step(P, S, x, xl)
                evt = evaluate(P, St)
                chi_t = chi_eval = evt["chi"]
                if abs(chi_cur - chi_t) < 1e-9 * abs(chi_cur):
                    bias = np.abs(x[P.os:]).max() if P.shared else max([np.abs(St["bg"] - S["bg"]).max(), np.abs(St["ba"] - S["ba"]).max()])
                    for g_, v_ in (("R", np.abs(St["R"] - S["R"]).max()), ("t", np.abs(St["t"] - S["t"]).max()), ("v", np.abs(St["v"] - S["v"]).max()),
                                   ("bias", bias), ("X", np.abs(St["X"] - S["X"]).max() if P.L else 0.0)):
                        step[g_] = max(step[g_], float(v_))
                scale = np.sum(x * (lam * x + sysm["b"])) + np.sum((xl * (lam * xl + sysm["bl"]))[P.active_pt]) + t(1e-3)
                rho = (chi_cur - chi_t) / scale
                good = bool(rho > 0 and np.isfinite(chi_t))
            else:
                rho = t(-1)
            if good:
                alpha = min(1 - (2 * rho - 1) ** 3, t(2) / 3)
                lam = lam * max(t(1) / 3, alpha)
                ni = t(2)
                chi_cur, S, ev = chi_t, St, evt
            else:
                lam = lam * ni
                ni = ni * 2
            acc.append(good)
            q += 1; trials += 1
            if not (rho < 0 and q < prm["max_trials"]):
                break
        trace.append(dict(chi=chi_cur, lam=lam, trials=q, accepted=acc, dchi=abs(ini - chi_cur), step=step))
        if q == prm["max_trials"] or rho == 0:
            reason = END_TRIALS
            break
        nbad = nbad + 1 if (ini - chi_cur) * 1000 < ini else 0
        if nbad >= 3:
            reason = END_NBAD
            break
    kf, X, sb = state_out(P, S)
    return dict(kf=kf, X=X, sb=sb, iterations=iters, trials=trials, reason=reason, chi_first=chi_first, chi_last=chi_cur, chi_eval=chi_eval, lam=lam, n=P.n,
                trace=trace, active_pt=P.active_pt, free=~P.fixed, imu=P.imu, shared=P.shared)


def decisive_prefix(trace_ld):
    """The iterations before the first one whose extended-precision |dchi2| falls below 1e-9 chi2: past it rho is rounding noise."""
    for i, r in enumerate(trace_ld):
        if not r["dchi"] >= 1e-9 * abs(r["chi"]):
            return i
    return len(trace_ld)


def prefix_totals(run, pre):
    """(iterations, trials, flattened trial decisions, lambda) after the first `pre` iterations of a run."""
    tr = run["trace"][:pre]
    return len(tr), sum(r["trials"] for r in tr), [a for r in tr for a in r["accepted"]], (tr[-1]["lam"] if tr else None)


# ---------------------------------------------------------------------------------------------- gauge
def remove_gauge(kf, X, ref_kf):
    """Nothing is fixed in the initialisation calls: a solution is defined up to a translation and a yaw about gravity (z).  Fits that
    4-DoF transform on the keyframe positions (kf -> ref_kf, least squares) and applies it to rotations, positions, velocities and
    points.  -> (kf, X) in the dtype of the inputs."""
    kf = np.asarray(kf).copy(); X = np.asarray(X).copy()
    dt = kf.dtype
    p, q = kf[:, 9:12], np.asarray(ref_kf)[:, 9:12].astype(dt)
    pc, qc = p.mean(0), q.mean(0)
    a, b = p - pc, q - qc
    th = np.arctan2(np.sum(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), np.sum(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]))
    c, s = np.cos(th), np.sin(th)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dt)
    tr = qc - Rz @ pc
    kf[:, :9] = (Rz @ kf[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    kf[:, 9:12] = p @ Rz.T + tr
    kf[:, 12:15] = kf[:, 12:15] @ Rz.T
    if len(X):
        X = X @ Rz.T + tr
    return kf, X
