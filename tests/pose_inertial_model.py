"""CPU model of Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:7479-7872, :7874-8299).
TEST INFRASTRUCTURE ONLY.

The edge pieces come from the oracle (oracle_iba_bind: EdgeInertial, ImuCamPose::Update, LogSO3); numpy restates the rest in
double: EdgeMonoOnlyPose / EdgeStereoOnlyPose (src/G2oTypes.cc:349-395, :460-508, vectorised over the frame's edges and checked
against the oracle's EdgeMono / EdgeStereo in the tests), EdgeGyroRW / EdgeAccRW (include/G2oTypes.h:632-700), EdgePriorPoseImu
(src/G2oTypes.cc:929-969), g2o's Gauss-Newton (core/optimization_algorithm_gauss_newton.cpp:50-93, core/sparse_optimizer.cpp:
376-390, solvers/linear_solver_dense.h:65-113), the four rounds with their outlier classification, the recovery, the Hessian of the
new prior, Optimizer::Marginalize (:5187-5267) and the ConstraintPoseImu constructor (include/G2oTypes.h:708-719).

What the model pins where the reference leaves room:
  * unknowns in g2o's vertex order: current frame pose 0:6, velocity 6:9, gyro bias 9:12, accelerometer bias 12:15, then (LastFrame)
    the previous frame's 15 at 15:30;
  * a factorisation is "not positive" when a pivot of the LDL^T without pivoting is <= 0 or not finite (Eigen::LDLT pivots and
    treats a zero pivot as semi-definite; a Gauss-Newton Hessian with IMU information is positive definite, so the two agree
    whenever it matters).  Then BlockSolver::solve leaves x as the last successful step (zero before the first, the vector is
    allocated once per optimizer and kept across rounds), GN applies that x once more and optimize() stops the round;
  * the visual edges' chi2 at classification is the one of the last computeActiveErrors (start of the last iteration run);
    edges that sat out the round (level 1) get computeError at the current estimate.
"""
import numpy as np
import oracle_iba_bind as oib

KF = 21
LKF, LF = 0, 1
MONO_GATES = {LKF: np.float32([12, 7.5, 5.991, 5.991]), LF: np.float32([5.991, 5.991, 5.991, 5.991])}
STEREO_GATES = np.float32([15.6, 9.8, 7.815, 7.815])
DELTA_MONO, DELTA_STEREO, DELTA_PRIOR = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))), 5.0


class Camera:
    """The rig of one call: Tcb, camera 0 (Pinhole or KannalaBrandt8), optional camera 1 + Trl.  struct() gives the oracle's
    problem view (for oib.edge_visual)."""

    def __init__(self, cam, Rcb, tcb, camera_model=0, kb=(0, 0, 0, 0), Trl=None, cam2=None, camera2_model=0, kb2=(0, 0, 0, 0)):
        self.cam = tuple(float(c) for c in cam)
        self.Rcb, self.tcb = np.asarray(Rcb, np.float64).reshape(3, 3), np.asarray(tcb, np.float64).reshape(3)
        self.model, self.kb = int(camera_model), np.asarray(kb, np.float64)
        self.Trl = None if Trl is None else np.asarray(Trl, np.float64).reshape(3, 4)
        self.cam2, self.model2, self.kb2 = cam2, int(camera2_model), np.asarray(kb2, np.float64)
        self.views = [(self.Rcb, self.tcb, self.cam[:4], self.model, self.kb)]
        if self.Trl is not None:
            R2 = self.Trl[:, :3] @ self.Rcb
            t2 = self.Trl[:, :3] @ self.tcb + self.Trl[:, 3]
            self.views.append((R2, t2, tuple(float(c) for c in cam2), self.model2, self.kb2))

    def struct(self, cls):
        p = cls()
        for i in range(9):
            p.Rcb[i] = float(self.Rcb.reshape(-1)[i])
        for i in range(3):
            p.tcb[i] = float(self.tcb[i])
        p.fx, p.fy, p.cx, p.cy, p.bf = self.cam
        p.camera_model = self.model
        for i in range(4):
            p.kb[i] = float(self.kb[i]); p.kb2[i] = float(self.kb2[i])
        if self.Trl is not None:
            p.has_cam2 = 1
            for i in range(12):
                p.Trl[i] = float(self.Trl.reshape(-1)[i])
            p.fx2, p.fy2, p.cx2, p.cy2 = [float(c) for c in self.cam2]
            p.camera2_model = self.model2
        return p


# ---------------------------------------------------------------------------------------------- visual edges (vectorised)
def _project(view, Xc):
    Rcb, tcb, (fx, fy, cx, cy), model, k = view
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    if model == 1:           # KannalaBrandt8::project (float theta / psi, KannalaBrandt8.cpp:52-69)
        f32 = np.float32
        theta = np.arctan2(np.sqrt((x * x + y * y).astype(f32)).astype(np.float64), z.astype(f32).astype(np.float64)).astype(f32).astype(np.float64)
        psi = np.arctan2(y.astype(f32).astype(np.float64), x.astype(f32).astype(np.float64)).astype(f32).astype(np.float64)
        t2 = theta * theta; t3 = theta * t2; t5 = t3 * t2; t7 = t5 * t2; t9 = t7 * t2
        r = theta + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9
        return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], 1)
    return np.stack([fx * x / z + cx, fy * y / z + cy], 1)


def _project_jac(view, Xc):
    Rcb, tcb, (fx, fy, cx, cy), model, k = view
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    J = np.zeros((len(Xc), 2, 3))
    if model == 1:           # KannalaBrandt8::projectJac (:166-195)
        x2, y2, z2 = x * x, y * y, z * z
        r2 = x2 + y2; r = np.sqrt(r2); r3 = r2 * r
        th = np.arctan2(r, z)
        t2 = th * th; t4 = t2 * t2; t6 = t2 * t4; t8 = t4 * t4
        f = th + t2 * th * k[0] + t4 * th * k[1] + t6 * th * k[2] + t8 * th * k[3]
        fd = 1 + 3 * k[0] * t2 + 5 * k[1] * t4 + 7 * k[2] * t6 + 9 * k[3] * t8
        J[:, 0, 0] = fx * (fd * z * x2 / (r2 * (r2 + z2)) + f * y2 / r3)
        J[:, 1, 0] = fy * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3)
        J[:, 0, 1] = fx * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3)
        J[:, 1, 1] = fy * (fd * z * y2 / (r2 * (r2 + z2)) + f * x2 / r3)
        J[:, 0, 2] = -fx * fd * x / (r2 + z2)
        J[:, 1, 2] = -fy * fd * y / (r2 + z2)
    else:
        J[:, 0, 0] = fx / z; J[:, 0, 2] = -fx * x / (z * z)
        J[:, 1, 1] = fy / z; J[:, 1, 2] = -fy * y / (z * z)
    return J


def cam_pose(view, s):
    """Rcw, tcw of a camera of the rig at body state s (ImuCamPose::Update, G2oTypes.cc:212-219)."""
    Rwb, twb = s[0:9].reshape(3, 3), s[9:12]
    Rcb, tcb = view[0], view[1]
    return Rcb @ Rwb.T, Rcb @ (-(Rwb.T @ twb)) + tcb


def visual(camera, s, Xw, obs, kind, jac=True):
    """Errors [n][3] (row 2 = 0 for mono), camera-frame points [n][3] and pose Jacobians [n][3][6] of EdgeMonoOnlyPose (kind 0: left,
    2: right camera) / EdgeStereoOnlyPose (kind 1)."""
    n = len(Xw)
    err, Xc, Jp = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3, 6))
    bf = camera.cam[4]
    for cam_idx in range(len(camera.views)):
        sel = (kind == 2) if cam_idx == 1 else (kind != 2)
        if not sel.any():
            continue
        view = camera.views[cam_idx]
        Rcw, tcw = cam_pose(view, s)
        Xc_ = Xw[sel] @ Rcw.T + tcw
        uv = _project(view, Xc_)
        e = np.zeros((len(Xc_), 3))
        e[:, :2] = obs[sel, :2] - uv
        st = kind[sel] == 1
        e[st, 2] = obs[sel][st, 2] - (uv[st, 0] - bf * (1 / Xc_[st, 2]))
        err[sel], Xc[sel] = e, Xc_
        if not jac:
            continue
        pj = np.zeros((len(Xc_), 3, 3))
        pj[:, :2] = _project_jac(view, Xc_)
        pj[st, 2] = pj[st, 0]
        pj[st, 2, 2] += bf * (1.0 / (Xc_[st, 2] * Xc_[st, 2]))
        Rcb, tcb = view[0], view[1]
        Xb = (Xc_ - tcb) @ Rcb                                # Rbc Xc + tbc
        PR = pj @ Rcb
        J = np.zeros((len(Xc_), 3, 6))
        J[:, :, 0] = PR[:, :, 1] * -Xb[:, None, 2] + PR[:, :, 2] * Xb[:, None, 1]
        J[:, :, 1] = PR[:, :, 0] * Xb[:, None, 2] + PR[:, :, 2] * -Xb[:, None, 0]
        J[:, :, 2] = PR[:, :, 0] * -Xb[:, None, 1] + PR[:, :, 1] * Xb[:, None, 0]
        J[:, :, 3:6] = PR
        J[~st, 2] = 0
        Jp[sel] = J
    return err, Xc, Jp


def huber_w(chi2, delta):
    """rho'(chi2) of g2o::RobustKernelHuber (the weight of the information in the quadratic form)."""
    return np.where(chi2 <= delta * delta, 1.0, delta / np.sqrt(np.maximum(chi2, 1e-300)))


# ---------------------------------------------------------------------------------------------- IMU and prior edges
def inv_right_jac(v):
    d2 = float(v @ v); d = np.sqrt(d2)
    if d < 1e-5:
        return np.eye(3)
    W = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + 0.5 * W + (1.0 / d2 - (1.0 + np.cos(d)) / (2.0 * d * np.sin(d))) * (W @ W)


def prior_edge(s, prior, jac=True):
    """EdgePriorPoseImu::computeError / linearizeOplus (G2oTypes.cc:940-969): error [15], J [15][15] over (pose 6, v, bg, ba)."""
    Rp, Rwb = prior[0:9].reshape(3, 3), s[0:9].reshape(3, 3)
    er = oib.log_so3(Rp.T @ Rwb)
    e = np.concatenate([er, Rp.T @ (s[9:12] - prior[9:12]), s[12:15] - prior[12:15], s[15:18] - prior[15:18], s[18:21] - prior[18:21]])
    if not jac:
        return e, None
    J = np.zeros((15, 15))
    J[0:3, 0:3] = inv_right_jac(er)
    J[3:6, 3:6] = Rp.T @ Rwb
    J[6:15, 6:15] = np.eye(9)
    return e, J


def imu_stack(fr, s, p, mode):
    """The IMU-side edges as one stack in the unknowns' order: (J [rows][n], e [rows], blocks [(row0, Omega, robust delta or None)])."""
    n = 15 if mode == LKF else 30
    prev = fr["prev"] if mode == LKF else p
    ei, Ji = oib.edge_inertial(prev, s, fr["preint"])
    rows = 15 if mode == LKF else 30
    J, e = np.zeros((rows, n)), np.zeros(rows)
    e[0:9] = ei
    J[0:9, 0:9] = Ji[:, 15:24]                       # pose2, v2 = the current frame
    if mode == LF:
        J[0:9, 15:30] = Ji[:, 0:15]                  # pose1, v1, bg1, ba1 = the previous frame
    e[9:12] = s[15:18] - prev[15:18]; J[9:12, 9:12] = np.eye(3)            # EdgeGyroRW: VG2 - VG1
    e[12:15] = s[18:21] - prev[18:21]; J[12:15, 12:15] = np.eye(3)         # EdgeAccRW
    blocks = [(0, fr["info"].reshape(9, 9), None), (9, fr["info_g"].reshape(3, 3), None), (12, fr["info_a"].reshape(3, 3), None)]
    if mode == LF:
        J[9:12, 24:27] = -np.eye(3); J[12:15, 27:30] = -np.eye(3)
        ep, Jp = prior_edge(p, fr["prior"])
        e[15:30] = ep; J[15:30, 15:30] = Jp
        blocks.append((15, fr["prior_H"].reshape(15, 15), DELTA_PRIOR))
    return J, e, blocks


def imu_normal(J, e, blocks, robust=True):
    H = np.zeros((J.shape[1], J.shape[1])); b = np.zeros(J.shape[1])
    for r0, Om, delta in blocks:
        k = len(Om)
        Jr, er = J[r0:r0 + k], e[r0:r0 + k]
        w = 1.0
        if robust and delta is not None:
            w = float(huber_w(np.array(er @ Om @ er), delta))
        H += w * Jr.T @ Om @ Jr
        b -= w * Jr.T @ (Om @ er)
    return H, b


# ---------------------------------------------------------------------------------------------- dense helpers
def ldlt_solve(H, b):
    """The step of a positive definite H (Cholesky = LDL^T without pivoting); None when a pivot is <= 0 or not finite."""
    if not np.all(np.isfinite(H)):
        return None
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def marginalize(H, start, end):
    """Optimizer::Marginalize (Optimizer.cc:5187-5267): the Schur complement of block [start, end] with the JacobiSVD pseudo-inverse
    (singular values <= 1e-6 dropped); the block is symmetric, so V S+ U^T = sum v v^T / lambda over |lambda| > 1e-6."""
    n = len(H)
    keep = [i for i in range(n) if i < start or i > end]
    mb = list(range(start, end + 1))
    Hb = H[np.ix_(mb, mb)]
    w, V = np.linalg.eigh(Hb)
    winv = np.where(np.abs(w) > 1e-6, 1.0 / np.where(w == 0, 1.0, w), 0.0)
    invHb = (V * winv) @ V.T
    res = np.zeros_like(H)
    res[np.ix_(keep, keep)] = H[np.ix_(keep, keep)] - H[np.ix_(keep, mb)] @ invHb @ H[np.ix_(mb, keep)]
    return res


def constraint_pose_imu(H):
    """ConstraintPoseImu's constructor (include/G2oTypes.h:708-719): H = (H + H) / 2 as written, self-adjoint eigen-decomposition
    (the lower triangle), eigenvalues < 1e-12 set to 0, reassembled."""
    H = (H + H) / 2
    w, V = np.linalg.eigh(H)
    w = np.where(w < 1e-12, 0.0, w)
    return (V * w) @ V.T


# ---------------------------------------------------------------------------------------------- the optimisation
def residual(fr, camera, mode, s, p):
    """The whole weighted residual (sqrt-information whitened, no robust kernel): for the finite-difference tests."""
    n = len(fr["Xw"])
    out = []
    if n:
        err, _, _ = visual(camera, s, fr["Xw"], fr["obs"], fr["kind"], jac=False)
        for i in range(n):
            k = 3 if fr["kind"][i] == 1 else 2
            out.append(np.sqrt(fr["inv_sigma2"][i]) * err[i, :k])
    J, e, blocks = imu_stack(fr, s, p, mode)
    for r0, Om, _ in blocks:
        Lc = np.linalg.cholesky(Om)
        out.append(Lc.T @ e[r0:r0 + len(Om)])
    return np.concatenate(out)


def normal_equations(fr, camera, mode, s, p, level0, robust_vis, robust_prior=True):
    n = 15 if mode == LKF else 30
    H, b = np.zeros((n, n)), np.zeros(n)
    act = np.nonzero(level0)[0]
    chi2 = np.zeros(len(fr["Xw"]))
    if len(act):
        kind = fr["kind"][act]
        err, _, Jp = visual(camera, s, fr["Xw"][act], fr["obs"][act], kind)
        is2 = fr["inv_sigma2"][act]
        c2 = is2 * np.einsum("ij,ij->i", err, err)
        chi2[act] = c2
        w = np.ones(len(act))
        if robust_vis:
            w = huber_w(c2, np.where(kind == 1, DELTA_STEREO, DELTA_MONO))
        ww = w * is2
        H[0:6, 0:6] += np.einsum("e,eri,erj->ij", ww, Jp, Jp)
        b[0:6] -= np.einsum("e,eri,er->i", ww, Jp, err)
    J, e, blocks = imu_stack(fr, s, p, mode)
    Hi, bi = imu_normal(J, e, blocks, robust_prior)
    return H + Hi, b + bi, chi2


def solve(fr, camera, mode, rec_init=False):
    """-> dict(state [21], prev [21] (LastFrame's free previous state), outlier [n] bool, ret, H [15][15] (ConstraintPoseImu::H),
    rounds, iterations, fails, n_bad, recovered (the recovery ran), chi2 / depth_ok [n] (the last classification's inputs))."""
    n_e = len(fr["Xw"])
    kind = np.asarray(fr["kind"])
    s = np.array(fr["state"], np.float64)
    p = np.array(fr["prev"], np.float64) if mode == LF else None
    nx = 15 if mode == LKF else 30
    x_last = np.zeros(nx)
    outlier = np.zeros(n_e, bool)
    robust_vis = True
    n_edges_total = n_e + (3 if mode == LKF else 4)
    rounds = iters = fails = 0
    n_bad = n_inl = 0
    mono = kind != 1
    for it in range(4):
        rounds += 1
        level0 = ~outlier
        s_lin, p_lin = s, p
        for _ in range(10):
            s_lin, p_lin = s, p
            H, b, _ = normal_equations(fr, camera, mode, s, p, level0, robust_vis)
            x = ldlt_solve(H, b)
            iters += 1
            ok = x is not None
            if ok:
                x_last = x
            else:
                fails += 1
            s = oib.kf_update(s, x_last[0:15])
            if mode == LF:
                p = oib.kf_update(p, x_last[15:30])
            if not ok:
                break
        # classification (:7720-7790 / :8129-8198)
        gate_m = MONO_GATES[mode][it]
        gate_close = np.float32(1.5 * float(gate_m))
        gate_s = STEREO_GATES[it]
        chi2 = np.zeros(n_e)
        depth_ok = np.ones(n_e, bool)
        if n_e:
            err_l, _, _ = visual(camera, s_lin, fr["Xw"], fr["obs"], kind, jac=False)
            err_c, Xc, _ = visual(camera, s, fr["Xw"], fr["obs"], kind, jac=False)
            err = np.where(outlier[:, None], err_c, err_l)
            chi2 = fr["inv_sigma2"] * np.einsum("ij,ij->i", err, err)
            depth_ok = Xc[:, 2] > 0.0
        c32 = chi2.astype(np.float32)
        close = np.asarray(fr["close"], bool)
        bad_m = ((c32 > gate_m) & ~close) | (close & (c32 > gate_close)) | ~depth_ok
        bad_s = c32 > gate_s
        outlier = np.where(mono, bad_m, bad_s)
        n_bad = int(outlier.sum()); n_inl = n_e - n_bad
        if it == 2:
            robust_vis = False
        if n_edges_total < 10:
            break
    recovered = n_inl < 30 and not rec_init
    if recovered:                                    # recovery (:7795-7822 / :8202-8230)
        n_bad = 0
        if n_e:
            err_c, _, _ = visual(camera, s, fr["Xw"], fr["obs"], kind, jac=False)
            chi2_r = fr["inv_sigma2"] * np.einsum("ij,ij->i", err_c, err_c)
            good = np.where(mono, chi2_r < 18.0, chi2_r < 24.0)
            outlier = outlier & ~good
            n_bad = int((~good).sum())
    # the new prior (:7831-7869 / :8242-8296): raw information, inlier visual edges, the final estimate
    Hf, _, _ = normal_equations(fr, camera, mode, s, p, ~outlier, robust_vis=False, robust_prior=False)
    if mode == LF:
        Hf = marginalize(Hf, 15, 29)[0:15, 0:15]
    Hc = constraint_pose_imu(Hf)
    return dict(state=s, prev=p, outlier=outlier, ret=n_e - n_bad, H=Hc, rounds=rounds, iterations=iters, fails=fails, n_bad=n_bad,
                recovered=recovered, chi2=chi2, depth_ok=depth_ok)
