"""Numpy float64 model of Optimizer::OptimizeSim3 (the 8-argument overload, reference src/Optimizer.cc:3932-4328), written from the
reference text: g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h), VertexSim3Expmap / EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ
(include/OptimizableTypes.h:146-215), g2o's Levenberg-Marquardt (g2o/core/optimization_algorithm_levenberg.cpp:61-194, with this
tree's _tau = 1e-50 and 100 trials after a failure, :47,:51), RobustKernelHuber (robust_kernel_impl.cpp:65-91), the numerical
Jacobian of BaseBinaryEdge (base_binary_edge.hpp:136-200) and the two-pass schedule of :4237-4327.  It is the yardstick of the device
kernel and shares no code with it.

A problem is a dict: P1c, P2c [n][3], obs1, obs2 [n][2], w1, w2 [n] (inv sigma^2), cam1, cam2 = dict(K=(fx, fy, cx, cy), kb8=None or
(k1..k4)), th2 (the reference's float), fix_scale, sim3 [8] = (qx qy qz qw tx ty tz s).  Rows are the correspondences that passed the
map-point tests of :4025-4080; the P3D2c.z < 0 test of :4082 is part of the model (flag 3).  The weights arrive ready: for a row
without keypoint in KF2 w2 is mvInvLevelSigma2[0] -- :4178 passes mnTrackScaleLevel to cv::KeyPoint as the SIZE, so the octave read at
:4220 is the default 0 (tests/synth_sim3.py builds the rows that way)."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------ g2o::Sim3
def quat_rot(q, v):
    """Eigen's quaternion * vector: v + w * (2 qv x v) + qv x (2 qv x v); q = (x, y, z, w), v [..., 3]"""
    qv = q[:3]
    uv = 2.0 * np.cross(np.broadcast_to(qv, v.shape), v)
    return v + q[3] * uv + np.cross(np.broadcast_to(qv, v.shape), uv)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d)"""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t; q[1] = (R[0, 2] - R[2, 0]) * t; q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t; q[j] = (R[j, i] + R[i, j]) * t; q[k] = (R[k, i] + R[i, k]) * t
    return q


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def sim3_exp(u):
    """g2o::Sim3(Vector7d), sim3.h:70-142: all four branches; the small-angle ones use R = I + Omega + Omega^2"""
    omega, upsilon, sigma = u[:3], u[3:6], u[6]
    theta = np.sqrt(omega @ omega)
    Om = skew(omega); Om2 = Om @ Om; I = np.eye(3)
    s = np.exp(sigma)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A = 1. / 2.; B = 1. / 6.
            R = I + Om + Om @ Om
        else:
            theta2 = theta * theta
            A = (1 - np.cos(theta)) / theta2
            B = (theta - np.sin(theta)) / (theta2 * theta)
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = I + Om + Om2
        else:
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
            a = s * np.sin(theta); b = s * np.cos(theta)
            theta2 = theta * theta; sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    W = A * Om + B * Om2 + C * I
    return np.r_[quat_from_R(R), W @ upsilon, s]


def sim3_mul(a, b):
    return np.r_[quat_mul(a[:4], b[:4]), a[7] * quat_rot(a[:4], b[4:7]) + a[4:7], a[7] * b[7]]


def sim3_inverse(a):
    qc = np.r_[-a[:3], a[3]]
    return np.r_[qc, quat_rot(qc, (-1. / a[7]) * a[4:7]), 1. / a[7]]


def sim3_map(S, X):
    return S[7] * quat_rot(S[:4], X) + S[4:7]


def sim3_distance(a, b):
    """max over (q up to sign, t, s) of the absolute difference"""
    dq = min(np.abs(a[:4] - b[:4]).max(), np.abs(a[:4] + b[:4]).max())
    return max(dq, np.abs(a[4:] - b[4:]).max())


# ------------------------------------------------------------------ GeometricCamera::project / projectJac
def project(cam, P):
    fx, fy, cx, cy = cam["K"]
    if cam.get("kb8") is None:                                   # Pinhole.cpp:41-47
        return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1)
    k = cam["kb8"]                                               # KannalaBrandt8.cpp:52-69: theta and psi pass through float
    x2y2 = P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]
    rf = np.sqrt(x2y2.astype(np.float32)).astype(np.float64)
    theta = np.arctan2(rf, P[:, 2].astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    psi = np.arctan2(P[:, 1].astype(np.float32).astype(np.float64), P[:, 0].astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    t2 = theta * theta; t3 = theta * t2; t5 = t3 * t2; t7 = t5 * t2; t9 = t7 * t2
    r = theta + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], 1)


def project_smooth(cam, P):
    """the same projection without the float roundings of theta / psi (what projectJac differentiates)"""
    if cam.get("kb8") is None:
        return project(cam, P)
    fx, fy, cx, cy = cam["K"]; k = cam["kb8"]
    theta = np.arctan2(np.sqrt(P[:, 0] ** 2 + P[:, 1] ** 2), P[:, 2]); psi = np.arctan2(P[:, 1], P[:, 0])
    r = theta + k[0] * theta ** 3 + k[1] * theta ** 5 + k[2] * theta ** 7 + k[3] * theta ** 9
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], 1)


def project_jac(cam, P):
    """[n][2][3]: Pinhole.cpp:81-91, KannalaBrandt8.cpp:166-195"""
    fx, fy = cam["K"][:2]
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    J = np.zeros((len(P), 2, 3))
    if cam.get("kb8") is None:
        J[:, 0, 0] = fx / z; J[:, 0, 2] = -fx * x / (z * z)
        J[:, 1, 1] = fy / z; J[:, 1, 2] = -fy * y / (z * z)
        return J
    k = cam["kb8"]
    x2 = x * x; y2 = y * y; z2 = z * z; r2 = x2 + y2; r = np.sqrt(r2); r3 = r2 * r
    theta = np.arctan2(r, z)
    t2 = theta * theta; t3 = t2 * theta; t4 = t2 * t2; t5 = t4 * theta; t6 = t2 * t4; t7 = t6 * theta; t8 = t4 * t4; t9 = t8 * theta
    f = theta + t3 * k[0] + t5 * k[1] + t7 * k[2] + t9 * k[3]
    fd = 1 + 3 * k[0] * t2 + 5 * k[1] * t4 + 7 * k[2] * t6 + 9 * k[3] * t8
    J[:, 0, 0] = fx * (fd * z * x2 / (r2 * (r2 + z2)) + f * y2 / r3)
    J[:, 1, 0] = fy * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3)
    J[:, 0, 1] = fx * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3)
    J[:, 1, 1] = fy * (fd * z * y2 / (r2 * (r2 + z2)) + f * x2 / r3)
    J[:, 0, 2] = -fx * fd * x / (r2 + z2)
    J[:, 1, 2] = -fy * fd * y / (r2 + z2)
    return J


# ------------------------------------------------------------------ edges
def errors(pb, S):
    """computeError of both edges of every row -> e12 [n][2], e21 [n][2]"""
    e12 = pb["obs1"] - project(pb["cam1"], sim3_map(S, pb["P2c"]))
    e21 = pb["obs2"] - project(pb["cam2"], sim3_map(sim3_inverse(S), pb["P1c"]))
    return e12, e21


def chi2(e, w):
    """e^T (w I) e as g2o evaluates it: e . (information * e)"""
    return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])


def _dmap(y):
    """[n][3][7] = [ -[y]x | I | y ]"""
    n = len(y)
    D = np.zeros((n, 3, 7))
    D[:, 0, 1] = y[:, 2]; D[:, 0, 2] = -y[:, 1]
    D[:, 1, 0] = -y[:, 2]; D[:, 1, 2] = y[:, 0]
    D[:, 2, 0] = y[:, 1]; D[:, 2, 1] = -y[:, 0]
    D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
    D[:, :, 6] = y
    return D


def jacobians_analytic(pb, S):
    """d e / d delta for S <- Sim3(delta) * S at delta = 0 -> J12, J21 [n][2][7]"""
    y = sim3_map(S, pb["P2c"])
    J12 = -np.einsum("nij,njk->nik", project_jac(pb["cam1"], y), _dmap(y))
    Si = sim3_inverse(S)
    y2 = sim3_map(Si, pb["P1c"])
    D2 = -Si[7] * np.einsum("ij,njk->nik", quat_to_R(Si[:4]), _dmap(pb["P1c"]))
    J21 = -np.einsum("nij,njk->nik", project_jac(pb["cam2"], y2), D2)
    if pb["fix_scale"]:
        J12[:, :, 6] = 0; J21[:, :, 6] = 0
    return J12, J21


def jacobians_numeric(pb, S, delta=1e-9):
    """BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:147-173): central differences through push / oplus / pop of the vertex"""
    n = len(pb["P1c"])
    J12 = np.zeros((n, 2, 7)); J21 = np.zeros((n, 2, 7))
    scalar = 1.0 / (2 * delta)
    for d in range(7):
        add = np.zeros(7)
        add[d] = delta
        a12, a21 = errors(pb, oplus(pb, S, add))
        add[d] = -delta
        b12, b21 = errors(pb, oplus(pb, S, add))
        J12[:, :, d] = scalar * (a12 - b12)
        J21[:, :, d] = scalar * (a21 - b21)
    return J12, J21


def oplus(pb, S, update):
    """VertexSim3Expmap::oplusImpl (it writes the zero into the caller's vector)"""
    if pb["fix_scale"]:
        update[6] = 0
    return sim3_mul(sim3_exp(update), S)


# ------------------------------------------------------------------ g2o
def _huber(e, delta, dsqr):
    sq = np.sqrt(np.where(e > dsqr, e, 1.0))
    inl = e <= dsqr
    return np.where(inl, e, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def _solve_dense(H, b):
    """LinearSolverDense: LDL^T, `false` unless positive definite"""
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return False, None
    x = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return bool(np.all(np.isfinite(x))), x


class _Lm:
    def __init__(self, pb, jacobian):
        self.pb = pb
        self.jac = jacobians_analytic if jacobian == "analytic" else jacobians_numeric
        th2 = np.float32(pb["th2"])
        self.delta = float(np.float32(np.sqrt(th2)))                      # Optimizer.cc:3992
        self.dsqr = float(np.float32(self.delta * self.delta))           # `float dsqr` (robust_kernel_impl.h:84)
        self.x = np.zeros(7)
        self.iters = 0
        self.trials = 0

    def robust_chi2(self, S, act, robust):
        e12, e21 = errors(self.pb, S)
        c = np.r_[chi2(e12[act], self.pb["w1"][act]), chi2(e21[act], self.pb["w2"][act])]
        return float(np.sum(_huber(c, self.delta, self.dsqr)[0] if robust else c))

    def optimize(self, S, act, iterations, robust):
        """SparseOptimizer::optimize(iterations) -> (estimate, state of the last computeActiveErrors)"""
        pb = self.pb
        lam = 0.0; ni = 2.0; nbad = 0
        S_ev = S
        for it in range(iterations):
            e12, e21 = errors(pb, S)
            J12, J21 = self.jac(pb, S)
            e = np.r_[e12[act], e21[act]]; J = np.r_[J12[act], J21[act]]; w = np.r_[pb["w1"][act], pb["w2"][act]]
            c = chi2(e, w)
            if robust:
                rho0, rho1 = _huber(c, self.delta, self.dsqr)
            else:
                rho0, rho1 = c, np.ones_like(c)
            ww = rho1 * w
            H = np.einsum("nia,n,nib->ab", J, ww, J)
            b = np.einsum("nia,ni->a", J, -(ww[:, None] * e))
            current = float(np.sum(rho0)); ini = current
            S_ev = S
            if it == 0:
                lam = 1e-50 * np.max(np.abs(np.diag(H))); ni = 2.0; nbad = 0
            rho = 0.0; qmax = 0
            while True:
                S_bk = S
                ok2, xn = _solve_dense(H + lam * np.eye(7), b)
                if ok2:
                    self.x = xn
                S = oplus(pb, S, self.x)
                temp = self.robust_chi2(S, act, robust)
                S_ev = S
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                scale = float(np.sum(self.x * (lam * self.x + b))) + 1e-3
                rho /= scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha); ni = 2.0; current = temp
                else:
                    lam *= ni; ni *= 2
                    S = S_bk
                qmax += 1; self.trials += 1
                if not (rho < 0 and qmax < 100):
                    break
            self.iters += 1
            if qmax == 100 or rho == 0:
                break
            if (ini - current) * 1e3 < ini:
                nbad += 1
            else:
                nbad = 0
            if nbad >= 3:
                break
        return S, S_ev


def solve(problem, jacobian="analytic", reverse=False, order=None):
    """-> dict(sim3 [8], flag [n] uint8 (0 inlier, 1 dropped after pass 1, 2 dropped after pass 2, 3 no edge), n_in (the return value),
    n_corr, n_bad, iters2 (the iteration budget of pass 2, 0 = not run), lm_iters, lm_trials, margin (the smallest relative distance of a
    decisive chi2 to th2)).  reverse / order: the same problem with its rows reversed / permuted (a summation-order perturbation); the
    flags come back in the problem's own order."""
    pb = dict(problem)
    n = len(problem["P1c"])
    if order is None:
        order = np.arange(n)[::-1] if reverse else np.arange(n)
    order = np.asarray(order, int)
    for k in ("P1c", "P2c", "obs1", "obs2", "w1", "w2"):
        pb[k] = np.ascontiguousarray(np.asarray(problem[k], np.float64)[order])
    th2 = float(np.float32(pb["th2"]))
    S = np.asarray(pb["sim3"], np.float64).copy()
    flag = np.where(pb["P2c"][:, 2] < 0, 3, 0).astype(np.uint8) if n else np.zeros(0, np.uint8)
    n_corr = int(np.sum(flag == 0))
    out = dict(sim3=S.copy(), n_in=0, n_corr=n_corr, n_bad=0, iters2=0, lm_iters=0, lm_trials=0, margin=np.inf)
    if n_corr > 0:
        lm = _Lm(pb, jacobian)
        act = flag == 0
        S, S_ev = lm.optimize(S, act, 5, True)
        # :4244-4271 -- no computeError(): the stored errors are those of the last LM trial, accepted or not
        e12, e21 = errors(pb, S_ev)
        c = np.maximum(chi2(e12, pb["w1"]), chi2(e21, pb["w2"]))
        both = np.r_[chi2(e12, pb["w1"])[act], chi2(e21, pb["w2"])[act]]
        out["margin"] = float(np.min(np.abs(both - th2) / th2))
        flag[act & (c > th2)] = 1
        n_bad = int(np.sum(flag == 1))
        out["n_bad"] = n_bad
        if n_corr - n_bad >= 10:
            act = flag == 0
            out["iters2"] = 10 if n_bad > 0 else 5
            S, _ = lm.optimize(S, act, out["iters2"], False)
            e12, e21 = errors(pb, S)
            c = np.maximum(chi2(e12, pb["w1"]), chi2(e21, pb["w2"]))
            both = np.r_[chi2(e12, pb["w1"])[act], chi2(e21, pb["w2"])[act]]
            out["margin"] = min(out["margin"], float(np.min(np.abs(both - th2) / th2)))
            flag[act & (c > th2)] = 2
            out["n_in"] = int(np.sum(flag == 0))
            out["sim3"] = S
        out["lm_iters"] = lm.iters; out["lm_trials"] = lm.trials
    out["flag"] = np.zeros(n, np.uint8)
    out["flag"][order] = flag
    return out
