"""CPU model of Optimizer::InertialOptimization (reference src/Optimizer.cc:5303-5908, the four overloads).  TEST INFRASTRUCTURE ONLY.

numpy restates, from the reference text and over a dtype parameter (float64 or np.longdouble):
  * EdgeInertialGS::computeError / linearizeOplus (src/G2oTypes.cc:826-927) for all eight vertices, vectorised over the edges, with
    the bias-corrected deltas of IMU::Preintegrated (src/ImuTypes.cc:357-378) and the SO(3) functions of src/G2oTypes.cc:991-1063;
  * EdgePriorGyro / EdgePriorAcc (include/G2oTypes.h:784-830; error = 0 - b, Jacobian +I as src/G2oTypes.cc:971-983 sets it);
  * the vertex updates: velocities and biases add, GDirection::Update, VertexScale::oplusImpl (include/G2oTypes.h:254-314);
  * g2o's Levenberg-Marquardt as the fork has it (core/optimization_algorithm_levenberg.cpp:61-169: tau 1e-50, rho = dchi2 /
    (scale + 1e-3), lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)) or *= ni, ni *= 2, up to 100 trials, Terminate on rho == 0, on 100
    trials, or after three iterations in a row that gained less than 1e-3 of their chi2) and Gauss-Newton
    (core/optimization_algorithm_gauss_newton.cpp:50-93).

What the model pins where the reference leaves room:
  * unknowns: the velocities in keyframe order, then gyro bias, accelerometer bias, gravity direction (2), scale; a fixed unknown is
    absent; a keyframe without an edge has no unknown (its vertex is never active);
  * the system is bordered block-tridiagonal.  solve_system eliminates it block by block (numpy has no extended-precision LAPACK, and
    a map of 4096 keyframes has no dense form that fits); dense_system gives the same matrix densely, and the tests hold the two
    against each other.  A factorisation fails when a pivot of the LDL^T without pivoting is <= 0 or not finite; LM then counts a
    failed trial, GN applies the last successful step once more (g2o updates with the solver's x regardless) and stops;
  * NormalizeRotation (U V^T of an SVD) is the polar factor, computed by Newton's iteration in the working precision;
  * the information is read as its upper triangle (the reference's is symmetric to rounding);
  * chi2 or lambda not finite at the start of an iteration ends the map (in g2o every further trial would be rejected);
  * with fixed biases (bFixedVel) the two prior edges have only fixed vertices and are not active (core/sparse_optimizer.cpp:234,
    allVerticesFixed): they add nothing to chi2, which matters to the stop test (iniChi - currentChi) * 1e3 < iniChi.
"""
import numpy as np

KF, PREINT, IO_GLOBAL = 21, 67, 16
GRAVITY = float(np.float32(9.81))
END_ITERATIONS, END_TERMINATE, END_SOLVER, END_NONFINITE = 0, 1, 2, 3


def default_params(overload, mono=False, fixed_vel=False, priorG=1e2, priorA=1e6):
    """The reference's settings per overload 0..3 = (a)..(d)."""
    priorG, priorA = float(np.float32(priorG)), float(np.float32(priorA))
    if overload == 3:
        return dict(free_vel_bias=0, free_gdir=1, free_scale=1, gauss_newton=1, iterations=10, max_trials=100, lambda_init=0.0,
                    prior_g=0.0, prior_a=0.0)
    if overload == 0:
        return dict(free_vel_bias=0 if fixed_vel else 1, free_gdir=1, free_scale=1 if mono else 0, gauss_newton=0, iterations=200,
                    max_trials=100, lambda_init=1e3 if priorG != 0 else 0.0, prior_g=priorG, prior_a=priorA)
    return dict(free_vel_bias=1, free_gdir=0, free_scale=0, gauss_newton=0, iterations=200, max_trials=100, lambda_init=1e3,
                prior_g=priorG, prior_a=priorA)


# ---------------------------------------------------------------------------------------------- SO(3), batched over the leading axis
def _skew(w):
    W = np.zeros(w.shape[:-1] + (3, 3), w.dtype)
    W[..., 0, 1] = -w[..., 2]; W[..., 0, 2] = w[..., 1]
    W[..., 1, 0] = w[..., 2]; W[..., 1, 2] = -w[..., 0]
    W[..., 2, 0] = -w[..., 1]; W[..., 2, 1] = w[..., 0]
    return W


def _inv3(A):
    c = np.empty_like(A)
    c[..., 0, 0] = A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1]
    c[..., 0, 1] = A[..., 0, 2] * A[..., 2, 1] - A[..., 0, 1] * A[..., 2, 2]
    c[..., 0, 2] = A[..., 0, 1] * A[..., 1, 2] - A[..., 0, 2] * A[..., 1, 1]
    c[..., 1, 0] = A[..., 1, 2] * A[..., 2, 0] - A[..., 1, 0] * A[..., 2, 2]
    c[..., 1, 1] = A[..., 0, 0] * A[..., 2, 2] - A[..., 0, 2] * A[..., 2, 0]
    c[..., 1, 2] = A[..., 0, 2] * A[..., 1, 0] - A[..., 0, 0] * A[..., 1, 2]
    c[..., 2, 0] = A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]
    c[..., 2, 1] = A[..., 0, 1] * A[..., 2, 0] - A[..., 0, 0] * A[..., 2, 1]
    c[..., 2, 2] = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    det = A[..., 0, 0] * c[..., 0, 0] + A[..., 0, 1] * c[..., 1, 0] + A[..., 0, 2] * c[..., 2, 0]
    return c / det[..., None, None]


def normalize_rotation(R):
    for _ in range(3):
        R = (R + np.swapaxes(_inv3(R), -1, -2)) / 2
    return R


def exp_so3(w, eps, normalize):
    """ExpSO3 of src/G2oTypes.cc:991-1008 (eps 1e-5, normalised) / src/ImuTypes.cc:48-60 (eps 1e-4, as it is)."""
    dt = w.dtype
    d2 = (w * w).sum(-1); d = np.sqrt(d2)
    small = d < eps
    ds, d2s = np.where(small, dt.type(1), d), np.where(small, dt.type(1), d2)
    a = np.where(small, dt.type(1), np.sin(ds) / ds)
    b = np.where(small, dt.type(1) / 2, (1 - np.cos(ds)) / d2s)
    W = _skew(w)
    R = np.eye(3, dtype=dt) + a[..., None, None] * W + b[..., None, None] * (W @ W)
    return normalize_rotation(R) if normalize else R


def log_so3(R):
    dt = R.dtype
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    w = np.stack([(R[..., 2, 1] - R[..., 1, 2]) / 2, (R[..., 0, 2] - R[..., 2, 0]) / 2, (R[..., 1, 0] - R[..., 0, 1]) / 2], -1)
    c = (tr - 1) / 2
    inside = (c <= 1) & (c >= -1)
    th = np.arccos(np.clip(c, -1, 1))
    s = np.sin(th)
    use = inside & (np.abs(s) >= 1e-5)
    f = np.where(use, th / np.where(use, s, dt.type(1)), dt.type(1))
    return w * f[..., None]


def _jac_coeffs(v, fa, fb):
    dt = v.dtype
    d2 = (v * v).sum(-1); d = np.sqrt(d2)
    small = d < 1e-5
    ds = np.where(small, dt.type(1), d)
    W = _skew(v)
    J = np.eye(3, dtype=dt) + fa(ds)[..., None, None] * W + fb(ds)[..., None, None] * (W @ W)
    return np.where(small[..., None, None], np.eye(3, dtype=dt), J)


def inv_right_jac(v):
    return _jac_coeffs(v, lambda d: 0 * d + 0.5, lambda d: 1 / (d * d) - (1 + np.cos(d)) / (2 * d * np.sin(d)))


def right_jac(v):
    return _jac_coeffs(v, lambda d: -(1 - np.cos(d)) / (d * d), lambda d: (d - np.sin(d)) / (d * d * d))


# ---------------------------------------------------------------------------------------------- the edges
class Problem:
    """One map in the working precision.  kf [n][21] (Rwb, twb, velocity, biases), link [n], preint [n][67], info [n][81]."""

    def __init__(self, mp, dtype):
        self.dtype = np.dtype(dtype)
        t = self.dtype.type
        self.n = len(mp["kf"])
        kf = np.asarray(mp["kf"], np.float64).astype(dtype).reshape(self.n, KF)
        self.R = kf[:, 0:9].reshape(-1, 3, 3).copy(); self.p = kf[:, 9:12].copy(); self.vel0 = kf[:, 12:15].copy()
        self.link = np.asarray(mp["link"]).astype(bool).copy()
        if self.n:
            self.link[0] = False
        self.e2 = np.nonzero(self.link)[0]; self.e1 = self.e2 - 1
        pi = np.asarray(mp["preint"], np.float64).astype(dtype).reshape(self.n, PREINT)[self.e2]
        self.dT = pi[:, 0]
        self.dR, self.dV, self.dP = pi[:, 1:10].reshape(-1, 3, 3), pi[:, 10:13], pi[:, 13:16]
        self.JRg, self.JVg, self.JVa = pi[:, 16:25].reshape(-1, 3, 3), pi[:, 25:34].reshape(-1, 3, 3), pi[:, 34:43].reshape(-1, 3, 3)
        self.JPg, self.JPa = pi[:, 43:52].reshape(-1, 3, 3), pi[:, 52:61].reshape(-1, 3, 3)
        self.b_lin = pi[:, 61:67]
        om = np.asarray(mp["info"], np.float64).astype(dtype).reshape(self.n, 9, 9)[self.e2]
        up = np.triu(om)
        self.Om = up + np.swapaxes(np.triu(om, 1), -1, -2)
        self.active = np.zeros(self.n, bool)
        self.active[self.e1] = True; self.active[self.e2] = True
        self.g_I = np.array([0, 0, -GRAVITY]).astype(dtype)
        self.glob0 = np.asarray(mp["glob"], np.float64).astype(dtype)
        _ = t


def edge_error(P, vel, glob, R=None, p=None, jac=False):
    """EdgeInertialGS::computeError for every edge: e [E][9]; with jac, also the eight Jacobian blocks of linearizeOplus:
    dict(p1 [E][9][6], v1 [E][9][3], bg, ba [E][9][3], p2 [E][9][6], v2 [E][9][3], gd [E][9][2], s [E][9][1])."""
    dt = P.dtype
    R = P.R if R is None else R
    p = P.p if p is None else p
    Rwg, s, bg, ba = glob[0:9].reshape(3, 3), glob[9], glob[10:13], glob[13:16]
    e1, e2 = P.e1, P.e2
    dbg, dba = bg - P.b_lin[:, 0:3], ba - P.b_lin[:, 3:6]
    w = np.einsum("eij,ej->ei", P.JRg, dbg)
    dR = normalize_rotation(P.dR @ exp_so3(w, 1e-4, False))
    dV = P.dV + np.einsum("eij,ej->ei", P.JVg, dbg) + np.einsum("eij,ej->ei", P.JVa, dba)
    dP = P.dP + np.einsum("eij,ej->ei", P.JPg, dbg) + np.einsum("eij,ej->ei", P.JPa, dba)
    g = Rwg @ P.g_I
    Rbw1 = np.swapaxes(R[e1], -1, -2)
    Rwb2 = R[e2]
    T = P.dT[:, None]
    eR = np.swapaxes(dR, -1, -2) @ Rbw1 @ Rwb2
    er = log_so3(eR)
    dvel = vel[e2] - vel[e1]
    dpos = p[e2] - p[e1] - vel[e1] * T
    va = np.einsum("eij,ej->ei", Rbw1, s * dvel - g * T)
    vb = np.einsum("eij,ej->ei", Rbw1, s * dpos - g * T * T / 2)
    e = np.concatenate([er, va - dV, vb - dP], 1)
    if not jac:
        return e
    E = len(e2)
    invJr = inv_right_jac(er)
    J = {k: np.zeros((E, 9, c), dt) for k, c in (("p1", 6), ("v1", 3), ("bg", 3), ("ba", 3), ("p2", 6), ("v2", 3), ("gd", 2), ("s", 1))}
    J["p1"][:, 0:3, 0:3] = -invJr @ np.swapaxes(Rwb2, -1, -2) @ R[e1]
    J["p1"][:, 3:6, 0:3] = _skew(va)
    J["p1"][:, 6:9, 0:3] = _skew(vb)
    J["p1"][:, 6:9, 3:6] = -s * np.eye(3, dtype=dt)
    J["v1"][:, 3:6] = -s * Rbw1
    J["v1"][:, 6:9] = -s * Rbw1 * T[:, :, None]
    J["bg"][:, 0:3] = -invJr @ np.swapaxes(eR, -1, -2) @ right_jac(w) @ P.JRg
    J["bg"][:, 3:6] = -P.JVg
    J["bg"][:, 6:9] = -P.JPg
    J["ba"][:, 3:6] = -P.JVa
    J["ba"][:, 6:9] = -P.JPa
    J["p2"][:, 0:3, 0:3] = invJr
    J["p2"][:, 6:9, 3:6] = s * (Rbw1 @ Rwb2)
    J["v2"][:, 3:6] = s * Rbw1
    Gm = np.zeros((3, 2), dt); Gm[0, 1] = -GRAVITY; Gm[1, 0] = GRAVITY
    dG = Rwg @ Gm
    RdG = Rbw1 @ dG
    J["gd"][:, 3:6] = -RdG * T[:, :, None]
    J["gd"][:, 6:9] = -RdG * (T * T)[:, :, None] / 2
    J["s"][:, 3:6, 0] = np.einsum("eij,ej->ei", Rbw1, dvel)
    J["s"][:, 6:9, 0] = np.einsum("eij,ej->ei", Rbw1, dpos)
    return e, J


def update_glob(glob, xb, free):
    """The vertex updates of the border: xb over (bg 3, ba 3, gdir 2, scale 1), fixed ones ignored."""
    out = glob.copy()
    if free["free_vel_bias"]:
        out[10:16] = glob[10:16] + xb[0:6]
    if free["free_gdir"]:
        w = np.array([xb[6], xb[7], 0]).astype(glob.dtype)
        out[0:9] = (glob[0:9].reshape(3, 3) @ exp_so3(w, 1e-5, True)).reshape(-1)
    if free["free_scale"]:
        out[9] = glob[9] * np.exp(xb[8])
    return out


def update_pose(R, p, k, d):
    """ImuCamPose::Update of keyframe k (src/G2oTypes.cc:195-219): twb += Rwb ut, Rwb <- Rwb ExpSO3(ur); d = (ur, ut).  For the
    finite-difference tests (the poses are fixed in every overload)."""
    R, p = R.copy(), p.copy()
    p[k] = p[k] + R[k] @ d[3:6]
    R[k] = R[k] @ exp_so3(d[0:3], 1e-5, True)
    return R, p


def chi2_of(P, vel, glob, prm):
    e = edge_error(P, vel, glob)
    oe = np.einsum("eij,ej->ei", P.Om, e)
    t = P.dtype.type
    chi = (e * oe).sum(1).sum() if len(e) else t(0)
    if not prm["free_vel_bias"]:                            # the prior edges' vertices are fixed: g2o leaves such edges out of the active set
        return chi
    bg, ba = glob[10:13], glob[13:16]
    return chi + t(prm["prior_g"]) * (bg @ bg) + t(prm["prior_a"]) * (ba @ ba)


# ---------------------------------------------------------------------------------------------- the normal equations and their solution
def border_columns(prm):
    c = []
    if prm["free_vel_bias"]:
        c += [0, 1, 2, 3, 4, 5]
    if prm["free_gdir"]:
        c += [6, 7]
    if prm["free_scale"]:
        c += [8]
    return c


def build(P, vel, glob, prm):
    """-> chi2, D [n][3][3], O [n][3][3] (block (k-1, k), zero without a link), B [n][3][9], C [9][9], rv [n][3], rb [9]: H and
    b = -J^T Omega e over the full border width (the fixed columns are dropped by the solver)."""
    dt = P.dtype
    t = dt.type
    n = P.n
    e, J = edge_error(P, vel, glob, jac=True)
    Jb = np.concatenate([J["bg"], J["ba"], J["gd"], J["s"]], 2)                  # [E][9][9]
    if not prm["free_gdir"]:
        Jb[:, :, 6:8] = 0
    if not prm["free_scale"]:
        Jb[:, :, 8] = 0
    if not prm["free_vel_bias"]:
        Jb[:, :, 0:6] = 0
    Om = P.Om
    oe = np.einsum("eij,ej->ei", Om, e)
    chi = (e * oe).sum(1).sum() if len(e) else t(0)
    D, O, B, rv = np.zeros((n, 3, 3), dt), np.zeros((n, 3, 3), dt), np.zeros((n, 3, 9), dt), np.zeros((n, 3), dt)
    Tt = lambda A: np.swapaxes(A, -1, -2)      # noqa: E731
    OJ1, OJ2, OJb = Om @ J["v1"], Om @ J["v2"], Om @ Jb
    if prm["free_vel_bias"]:
        D[P.e1] += Tt(J["v1"]) @ OJ1
        D[P.e2] += Tt(J["v2"]) @ OJ2
        O[P.e2] = Tt(J["v1"]) @ OJ2
        B[P.e1] += Tt(J["v1"]) @ OJb
        B[P.e2] += Tt(J["v2"]) @ OJb
        rv[P.e1] -= np.einsum("eij,ei->ej", J["v1"], oe)
        rv[P.e2] -= np.einsum("eij,ei->ej", J["v2"], oe)
    C = (Tt(Jb) @ OJb).sum(0) if len(e) else np.zeros((9, 9), dt)
    rb = -np.einsum("eij,ei->j", Jb, oe) if len(e) else np.zeros(9, dt)
    bg, ba = glob[10:13], glob[13:16]
    pg, pa = t(prm["prior_g"]), t(prm["prior_a"])
    if prm["free_vel_bias"]:                                # prior edges: e = -b, J = +I: H += prior I, b = -J^T Omega e = +prior b
        chi = chi + pg * (bg @ bg) + pa * (ba @ ba)         # (with fixed biases the edges are not active: sparse_optimizer.cpp:234)
        C[0:3, 0:3] += pg * np.eye(3, dtype=dt); C[3:6, 3:6] += pa * np.eye(3, dtype=dt)
        rb[0:3] += pg * bg; rb[3:6] += pa * ba
    return chi, D, O, B, C, rv, rb


def _ldl3(A):
    """Pivots and inverse of a symmetric 3x3 by LDL^T without pivoting; None when a pivot is <= 0 or not finite."""
    d0 = A[0, 0]
    if not (d0 > 0 and np.isfinite(d0)):
        return None
    l10, l20 = A[1, 0] / d0, A[2, 0] / d0
    d1 = A[1, 1] - l10 * A[1, 0]
    if not (d1 > 0 and np.isfinite(d1)):
        return None
    l21 = (A[2, 1] - l20 * A[1, 0]) / d1
    d2 = A[2, 2] - l20 * A[2, 0] - l21 * l21 * d1
    if not (d2 > 0 and np.isfinite(d2)):
        return None
    Li = np.eye(3, dtype=A.dtype)
    Li[1, 0] = -l10; Li[2, 1] = -l21; Li[2, 0] = l10 * l21 - l20
    return Li.T @ np.diag(np.array([1 / d0, 1 / d1, 1 / d2])) @ Li


def _ldl_solve(A, b):
    n = len(b)
    Lm = np.eye(n, dtype=A.dtype); d = np.zeros(n, A.dtype)
    for j in range(n):
        dj = A[j, j] - (Lm[j, :j] * Lm[j, :j] * d[:j]).sum()
        if not (dj > 0 and np.isfinite(dj)):
            return None
        d[j] = dj
        for i in range(j + 1, n):
            Lm[i, j] = (A[i, j] - (Lm[i, :j] * Lm[j, :j] * d[:j]).sum()) / dj
    y = b.copy()
    for i in range(n):
        y[i] = y[i] - (Lm[i, :i] * y[:i]).sum()
    y = y / d
    for i in range(n - 1, -1, -1):
        y[i] = y[i] - (Lm[i + 1:, i] * y[i + 1:]).sum()
    return y


def solve_system(P, prm, lam, D, O, B, C, rv, rb):
    """(H + lambda I) x = b of the free, active unknowns -> (xv [n][3], xb [9]) with zeros for the absent ones, or None."""
    dt = P.dtype
    n = P.n
    cols = border_columns(prm)
    nb = len(cols)
    lam = dt.type(lam)
    S = C[np.ix_(cols, cols)] + lam * np.eye(nb, dtype=dt)
    sb = rb[cols].copy()
    xv = np.zeros((n, 3), dt)
    if prm["free_vel_bias"]:
        I3 = np.eye(3, dtype=dt)
        Dinv, Bt, rt, G = [None] * n, [None] * n, [None] * n, [None] * n
        for k in range(n):
            if not P.active[k]:
                continue
            Dk, Bk, rk = D[k] + lam * I3, B[k][:, cols].copy(), rv[k].copy()
            if P.link[k]:                                    # coupled to k - 1 (active by construction)
                G[k] = Dinv[k - 1] @ O[k]
                Dk = Dk - G[k].T @ O[k]
                Bk = Bk - G[k].T @ Bt[k - 1]
                rk = rk - G[k].T @ rt[k - 1]
            Di = _ldl3(Dk)
            if Di is None:
                return None
            Dinv[k], Bt[k], rt[k] = Di, Bk, rk
            S = S - Bk.T @ Di @ Bk
            sb = sb - Bk.T @ (Di @ rk)
    xbf = _ldl_solve(S, sb) if nb else np.zeros(0, dt)
    if xbf is None:
        return None
    xb = np.zeros(9, dt)
    xb[cols] = xbf
    if prm["free_vel_bias"]:
        for k in range(n - 1, -1, -1):
            if not P.active[k]:
                continue
            y = Dinv[k] @ (rt[k] - Bt[k] @ xbf)
            if k + 1 < n and P.link[k + 1]:
                y = y - G[k + 1] @ xv[k + 1]
            xv[k] = y
    return xv, xb


def dense_system(P, prm, lam, D, O, B, C, rv, rb):
    """The same system densely: (H + lambda I [m][m], b [m], index lists of the velocity unknowns' keyframes and the border columns)."""
    dt = P.dtype
    act = np.nonzero(P.active)[0] if prm["free_vel_bias"] else np.zeros(0, int)
    pos = {int(k): i for i, k in enumerate(act)}
    cols = border_columns(prm)
    m = 3 * len(act) + len(cols)
    H, b = np.zeros((m, m), dt), np.zeros(m, dt)
    o = 3 * len(act)
    for k in act:
        i = 3 * pos[int(k)]
        H[i:i + 3, i:i + 3] = D[k]
        b[i:i + 3] = rv[k]
        H[i:i + 3, o:] = B[k][:, cols]; H[o:, i:i + 3] = B[k][:, cols].T
        if P.link[k]:
            j = 3 * pos[int(k) - 1]
            H[j:j + 3, i:i + 3] = O[k]; H[i:i + 3, j:j + 3] = O[k].T
    H[o:, o:] = C[np.ix_(cols, cols)]
    b[o:] = rb[cols]
    return H + dt.type(lam) * np.eye(m, dtype=dt), b, act, cols


# ---------------------------------------------------------------------------------------------- the optimisation
def optimize(mp, prm, dtype=np.float64):
    """-> dict(kf [n][21], glob [16] (both in `dtype`; kf as the call would return it), iterations, trials, reason, chi_first, chi_last,
    lam, trace: one dict per iteration run with chi, lam (after it), trials, accepted (per trial), dchi = |chi before - chi after|,
    step = the largest change proposed by a trial of the iteration whose |dchi2| is below 1e-9 chi2 -- one that rounding may accept
    or reject -- per group Rwg / scale / bg / ba / vel)."""
    P = Problem(mp, dtype)
    t = P.dtype.type
    vel, glob = P.vel0.copy(), P.glob0.copy()
    trace = []
    iters = trials = 0
    reason = END_ITERATIONS
    free = prm
    if prm["gauss_newton"]:
        xv_last, xb_last = np.zeros((P.n, 3), P.dtype), np.zeros(9, P.dtype)
        chi_first = None
        lam = t(0)
        for it in range(prm["iterations"]):
            chi, D, O, B, C, rv, rb = build(P, vel, glob, prm)
            if chi_first is None:
                chi_first = chi
            if not np.isfinite(chi):
                reason = END_NONFINITE
                break
            iters += 1
            r = solve_system(P, prm, 0, D, O, B, C, rv, rb)
            if r is not None:
                xv_last, xb_last = r
            vel = vel + xv_last
            glob = update_glob(glob, xb_last, free)
            trace.append(dict(chi=chi, lam=t(0), trials=0, accepted=[], dchi=t(0), ok=r is not None))
            if r is None:
                reason = END_SOLVER
                break
        if chi_first is None:
            chi_first = chi2_of(P, vel, glob, prm)
        chi_cur = chi2_of(P, vel, glob, prm)
    else:
        chi_cur = chi2_of(P, vel, glob, prm)
        chi_first = chi_cur
        lam, ni, nbad = t(prm["lambda_init"]), t(2), 0
        cols = border_columns(prm)
        for it in range(prm["iterations"]):
            if not np.isfinite(chi_cur) or not np.isfinite(lam):
                reason = END_NONFINITE
                break
            iters += 1
            ini = chi_cur
            chi, D, O, B, C, rv, rb = build(P, vel, glob, prm)
            if it == 0 and not prm["lambda_init"] > 0:
                mx = t(0)
                if prm["free_vel_bias"] and P.active.any():
                    mx = max(mx, np.abs(D[P.active][:, [0, 1, 2], [0, 1, 2]]).max())
                for c in cols:
                    mx = max(mx, abs(C[c, c]))
                lam = t(1e-50) * mx
            rho, q, acc = t(0), 0, []
            step = dict(Rwg=0.0, scale=0.0, bg=0.0, ba=0.0, vel=0.0)
            while q < prm["max_trials"]:
                r = solve_system(P, prm, lam, D, O, B, C, rv, rb)
                trials += 1
                good = False
                if r is not None:
                    xv, xb = r
                    vel_t, glob_t = vel + xv, update_glob(glob, xb, free)
                    chi_t = chi2_of(P, vel_t, glob_t, prm)
                    dg = np.abs(glob_t - glob)
                    if abs(chi_cur - chi_t) < 1e-9 * abs(chi_cur):      # a trial whose acceptance is rounding noise
                        for g_, v_ in (("Rwg", dg[0:9].max()), ("scale", dg[9]), ("bg", dg[10:13].max()), ("ba", dg[13:16].max()),
                                       ("vel", np.abs(xv).max() if xv.size else 0.0)):
                            step[g_] = max(step[g_], float(v_))
                    scale = (xv * (lam * xv + rv)).sum() + (xb[cols] * (lam * xb[cols] + rb[cols])).sum() + t(1e-3)
                    rho = (chi_cur - chi_t) / scale
                    good = bool(rho > 0 and np.isfinite(chi_t))
                    if good:
                        alpha = min(1 - (2 * rho - 1) ** 3, t(2) / 3)
                        lam = lam * max(t(1) / 3, alpha)
                        ni = t(2)
                        chi_cur, vel, glob = chi_t, vel_t, glob_t
                else:
                    rho = t(-1)
                if not good:
                    lam = lam * ni
                    ni = ni * 2
                acc.append(good)
                q += 1
                if not rho < 0:
                    break
            trace.append(dict(chi=chi_cur, lam=lam, trials=q, accepted=acc, dchi=abs(ini - chi_cur), ok=True, step=step))
            if q == prm["max_trials"] or rho == 0:
                reason = END_TERMINATE
                break
            nbad = nbad + 1 if (ini - chi_cur) * 1000 < ini else 0
            if nbad >= 3:
                reason = END_TERMINATE
                break
    kf = np.asarray(mp["kf"], np.float64).astype(dtype).reshape(P.n, KF).copy()
    if prm["free_vel_bias"]:
        kf[:, 12:15] = vel
        kf[:, 15:21] = glob[10:16]
    return dict(kf=kf, glob=glob, iterations=iters, trials=trials, reason=reason, chi_first=chi_first, chi_last=chi_cur, lam=lam,
                trace=trace)


def decisive_prefix(trace_ld):
    """The iterations before the first one whose extended-precision |dchi2| falls below 1e-9 chi2: past it rho is rounding noise."""
    for i, r in enumerate(trace_ld):
        if not r["dchi"] >= 1e-9 * abs(r["chi"]):
            return i
    return len(trace_ld)
