"""Numpy model of Optimizer::OptimizeEssentialGraph4DoF's optimisation (reference src/Optimizer.cc:8305-8610) written from the reference
text over a dtype parameter (float64 / longdouble).  TEST INFRASTRUCTURE ONLY: it imports nothing from the kernels' side.

  vertex state, both loads              ImuCamPose(KeyFrame*) / ImuCamPose(Rwc, twc, KeyFrame*), src/G2oTypes.cc:24-71, :121-146
  oplus                                 VertexPose4DoF::oplusImpl -> ImuCamPose::UpdateW, include/G2oTypes.h:175-185, G2oTypes.cc:222-256
  ExpSO3 (eps 1e-5, normalised), LogSO3 G2oTypes.cc:991-1023
  residual                              Edge4DoF::computeError, G2oTypes.h:847-852
  numeric Jacobians, delta = 1e-9       g2o/core/base_binary_edge.hpp:136-200
  quadratic form, diagonal information  base_binary_edge.hpp:55-90; src/Optimizer.cc:8378-8381
  lambda start tau * max |H(j, j)|      g2o/core/optimization_algorithm_levenberg.cpp:171-185 (tau = 1e-50, :47)
  LM control                            optimization_algorithm_levenberg.cpp:61-169

A vertex is a row of 36 numbers, Rwb 9 | twb 3 | Rcw 9 | tcw 3 | Rcb 9 | tcb 3 (the ABI's layout), plus the model's DR, Rwb0 and its.
Rcw / tcw are loaded and derived from Rwb / twb only at a vertex's first oplus (derive_at_load=True derives them at the load instead: a
switch for the test that shows the cases tell the two apart).  IMU::NormalizeRotation (U V^T of an SVD) is the nearest rotation, taken
here by Newton steps of the polar decomposition to convergence; float_roundtrip=True restates the reference's cv::Mat round trip inside
ExpSO3: the un-normalised matrix cast to float32, the nearest rotation in float32, cast back.
The linear system is dense and solved by essential_graph_model.ldlt_solve (no pivoting; fails on a zero or non-finite pivot)."""
import numpy as np
from essential_graph_model import ldlt_solve, decisive_prefix, prefix_totals, END_ITERATIONS, END_TERMINATE, END_NBAD, END_SOLVE_FAILED  # noqa: F401

LD = np.longdouble
EPS_BRANCH = 0.00001
DELTA = 1e-9
INFO_REFERENCE = (1e3, 1e3, 1.0, 1.0, 1.0, 1.0)              # (0,0) set twice, (2,2) never: yaw keeps weight 1
O_RWB, O_TWB, O_RCW, O_TCW, O_RCB, O_TCB = 0, 9, 12, 21, 24, 33


class Margins:
    """Smallest distance of the evaluated branch arguments to their thresholds: |sin(theta)| of LogSO3 and d of ExpSO3 against 1e-5.
    (LogSO3's other early return, cos(theta) outside [-1, 1], gives what the |sin| < 1e-5 branch gives: no threshold of its own.)"""

    def __init__(self):
        self.log_s = self.exp_d = np.inf

    def note(self, name, dist):
        if dist.size:
            setattr(self, name, min(getattr(self, name), float(np.min(dist))))

    def smallest(self):
        return min(self.log_s, self.exp_d)


def skew(w):
    O = np.zeros(w.shape[:-1] + (3, 3), w.dtype)
    O[..., 0, 1] = -w[..., 2]; O[..., 0, 2] = w[..., 1]; O[..., 1, 0] = w[..., 2]
    O[..., 1, 2] = -w[..., 0]; O[..., 2, 0] = -w[..., 1]; O[..., 2, 1] = w[..., 0]
    return O


def _inv3(A):
    c0 = A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1]
    c1 = A[..., 1, 2] * A[..., 2, 0] - A[..., 1, 0] * A[..., 2, 2]
    c2 = A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]
    det = A[..., 0, 0] * c0 + A[..., 0, 1] * c1 + A[..., 0, 2] * c2
    I = np.zeros_like(A)
    I[..., 0, 0] = c0; I[..., 0, 1] = A[..., 0, 2] * A[..., 2, 1] - A[..., 0, 1] * A[..., 2, 2]; I[..., 0, 2] = A[..., 0, 1] * A[..., 1, 2] - A[..., 0, 2] * A[..., 1, 1]
    I[..., 1, 0] = c1; I[..., 1, 1] = A[..., 0, 0] * A[..., 2, 2] - A[..., 0, 2] * A[..., 2, 0]; I[..., 1, 2] = A[..., 0, 2] * A[..., 1, 0] - A[..., 0, 0] * A[..., 1, 2]
    I[..., 2, 0] = c2; I[..., 2, 1] = A[..., 0, 1] * A[..., 2, 0] - A[..., 0, 0] * A[..., 2, 1]; I[..., 2, 2] = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    return I / det[..., None, None]


def nearest_rotation(R, steps=4):
    """U V^T of R's SVD for an R a rounding error away from a rotation: R <- (R + R^-T) / 2 converges quadratically."""
    half = R.dtype.type(0.5)
    for _ in range(steps):
        R = half * (R + np.swapaxes(_inv3(R), -1, -2))
    return R


def exp_so3(w, margins=None, float_roundtrip=False):
    dt = w.dtype
    d2 = np.sum(w * w, -1)
    d = np.sqrt(d2)
    if margins is not None:
        margins.note("exp_d", np.abs(d - dt.type(EPS_BRANCH)))
    W = skew(w)
    W2 = W @ W
    small = d < dt.type(EPS_BRANCH)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(small, dt.type(1), np.sin(d) / d)
        b = np.where(small, dt.type(0.5), (1 - np.cos(d)) / d2)
    R = np.eye(3, dtype=dt) + a[..., None, None] * W + b[..., None, None] * W2
    if float_roundtrip:
        return nearest_rotation(R.astype(np.float32)).astype(dt)
    return nearest_rotation(R)


def log_so3(R, margins=None):
    dt = R.dtype
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    w = np.stack([(R[..., 2, 1] - R[..., 1, 2]) / 2, (R[..., 0, 2] - R[..., 2, 0]) / 2, (R[..., 1, 0] - R[..., 0, 1]) / 2], -1)
    c = (tr - 1) * dt.type(0.5)
    outside = (c > 1) | (c < -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(np.clip(c, -1, 1))
        s = np.sin(theta)
        if margins is not None:
            margins.note("log_s", np.abs(np.abs(s) - dt.type(EPS_BRANCH)))
        f = np.where(outside | (np.abs(s) < dt.type(EPS_BRANCH)), dt.type(1), theta / s)
    return f[..., None] * w


def inv_right_jacobian(v):
    dt = v.dtype
    d2 = np.sum(v * v, -1)
    d = np.sqrt(d2)
    W = skew(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(d < 1e-5, dt.type(1) / 12, 1 / d2 - (1 + np.cos(d)) / (2 * d * np.sin(d)))
    return np.eye(3, dtype=dt) + dt.type(0.5) * W + k[..., None, None] * (W @ W)


def load(state36, dt, derive_at_load=False):
    """-> the vertices as a dict of arrays [V, ...]."""
    a = np.asarray(state36, np.float64).reshape(-1, 36).astype(dt)
    V = len(a)
    S = dict(Rwb=a[:, 0:9].reshape(V, 3, 3).copy(), twb=a[:, 9:12].copy(), Rcw=a[:, 12:21].reshape(V, 3, 3).copy(), tcw=a[:, 21:24].copy(),
             Rcb=a[:, 24:33].reshape(V, 3, 3).copy(), tcb=a[:, 33:36].copy(), its=np.zeros(V, np.int64))
    S["Rwb0"] = S["Rwb"].copy()
    S["DR"] = np.broadcast_to(np.eye(3, dtype=dt), (V, 3, 3)).copy()
    if derive_at_load:
        S["Rcw"], S["tcw"] = derive(S["Rwb"], S["twb"], S["Rcb"], S["tcb"])
    return S


def derive(Rwb, twb, Rcb, tcb):
    Rbw = np.swapaxes(Rwb, -1, -2)
    tbw = -np.einsum("...ij,...j->...i", Rbw, twb)
    return Rcb @ Rbw, np.einsum("...ij,...j->...i", Rcb, tbw) + tcb


def oplus_arrays(Rwb0, DR, twb, Rcb, tcb, u, margins=None, float_roundtrip=False):
    """UpdateW on batches -> (DR, Rwb, twb, Rcw, tcw)."""
    w = np.zeros(u.shape[:-1] + (3,), u.dtype)
    w[..., 2] = u[..., 0]
    DR = exp_so3(w, margins, float_roundtrip) @ DR
    Rwb = DR @ Rwb0
    twb = twb + u[..., 1:4]
    Rcw, tcw = derive(Rwb, twb, Rcb, tcb)
    return DR, Rwb, twb, Rcw, tcw


def oplus(S, idx, u, margins=None, its_step=True, float_roundtrip=False):
    """oplus of the vertices idx with u [len(idx), 4] -> a new state; its_step carries UpdateW's `its >= 5` lines."""
    N = {k: v.copy() for k, v in S.items()}
    DR, Rwb, twb, Rcw, tcw = oplus_arrays(S["Rwb0"][idx], S["DR"][idx], S["twb"][idx], S["Rcb"][idx], S["tcb"][idx], u, margins, float_roundtrip)
    its = S["its"][idx] + 1
    if its_step:
        hit = its >= 5
        DR[hit, 0, 2] = 0.0; DR[hit, 1, 2] = 0.0; DR[hit, 2, 0] = 0.0; DR[hit, 2, 1] = 0.0       # NormalizeRotation(DR)'s result is discarded
        its = np.where(hit, 0, its)
    N["DR"][idx], N["Rwb"][idx], N["twb"][idx], N["Rcw"][idx], N["tcw"][idx], N["its"][idx] = DR, Rwb, twb, Rcw, tcw, its
    return N


def residual(Ri, ti, Rj, tj, meas, margins=None):
    dR, dt_ = meas[..., :9].reshape(meas.shape[:-1] + (3, 3)), meas[..., 9:12]
    RjT = np.swapaxes(Rj, -1, -2)
    er = log_so3((Ri @ RjT) @ np.swapaxes(dR, -1, -2), margins)
    et = np.einsum("...ij,...j->...i", Ri, -np.einsum("...ij,...j->...i", RjT, tj)) + ti - dt_
    return np.concatenate([er, et], -1)


def edge_errors(S, v0, v1, meas, margins=None):
    return residual(S["Rcw"][v0], S["tcw"][v0], S["Rcw"][v1], S["tcw"][v1], meas, margins)


def numeric_jacobians(S, v0, v1, meas, free, delta=DELTA, margins=None, float_roundtrip=False):
    """-> (Ji, Jj) [E, 6, 4]: central differences through oplus on a copy of the vertex; a fixed vertex gets zeros."""
    dt = meas.dtype
    dl = dt.type(delta)
    scalar = dt.type(1) / (2 * dl)
    E = len(v0)
    J = np.zeros((2, E, 6, 4), dt)
    for side, vs in ((0, v0), (1, v1)):
        fr = free[vs]
        other = v1 if side == 0 else v0
        for c in range(4):
            pm = []
            for sg in (dl, -dl):
                u = np.zeros((E, 4), dt); u[:, c] = sg
                _, _, _, Rp, tp = oplus_arrays(S["Rwb0"][vs], S["DR"][vs], S["twb"][vs], S["Rcb"][vs], S["tcb"][vs], u, margins, float_roundtrip)
                Ro, to = S["Rcw"][other], S["tcw"][other]
                pm.append(residual(Rp, tp, Ro, to, meas, margins) if side == 0 else residual(Ro, to, Rp, tp, meas, margins))
            J[side, :, :, c] = np.where(fr[:, None], scalar * (pm[0] - pm[1]), 0)
    return J[0], J[1]


def analytic_jacobians(S, v0, v1, meas):
    """Derived separately (at the DERIVED camera poses): with z the world's vertical, E = Rcw_i Rcw_j^T dRij^T, c_j the camera centre,
    d e_rot / d yaw_i = -Jr^-1(e_rot) E^T Rcw_i z,   d e_t / d yaw_i = -Rcw_i (z x (c_j - twb_i)),   d e_t / d t_i = -Rcw_i,
    d e_rot / d yaw_j = +Jr^-1(e_rot) E^T Rcw_i z,   d e_t / d yaw_j = +Rcw_i (z x (c_j - twb_j)),   d e_t / d t_j = +Rcw_i."""
    dt = meas.dtype
    Rcw, tcw = derive(S["Rwb"], S["twb"], S["Rcb"], S["tcb"])
    Ri, Rj, tj = Rcw[v0], Rcw[v1], tcw[v1]
    dR = meas[:, :9].reshape(-1, 3, 3)
    Em = (Ri @ np.swapaxes(Rj, -1, -2)) @ np.swapaxes(dR, -1, -2)
    er = log_so3(Em)
    z = np.array([0, 0, 1], dt)
    Riz = Ri @ z
    a = np.einsum("eij,ej->ei", inv_right_jacobian(er) @ np.swapaxes(Em, -1, -2), Riz)
    cj = -np.einsum("eji,ej->ei", Rj, tj)
    Ji, Jj = np.zeros((len(v0), 6, 4), dt), np.zeros((len(v0), 6, 4), dt)
    Ji[:, :3, 0], Jj[:, :3, 0] = -a, a
    zx = lambda v: np.stack([-v[:, 1], v[:, 0], np.zeros(len(v), dt)], -1)      # z x v
    Ji[:, 3:, 0] = -np.einsum("eij,ej->ei", Ri, zx(cj - S["twb"][v0]))
    Jj[:, 3:, 0] = np.einsum("eij,ej->ei", Ri, zx(cj - S["twb"][v1]))
    Ji[:, 3:, 1:], Jj[:, 3:, 1:] = -Ri, Ri
    return Ji, Jj


def quadratic_form(e, Ji, Jj, info):
    """-> per edge Hii, Hij, Hjj [E, 4, 4], bi, bj [E, 4], chi2 [E]."""
    W = info[None, :, None]
    Hii, Hij, Hjj = np.einsum("era,erb->eab", Ji, W * Ji), np.einsum("era,erb->eab", Ji, W * Jj), np.einsum("era,erb->eab", Jj, W * Jj)
    we = info[None, :] * e
    return Hii, Hij, Hjj, -np.einsum("era,er->ea", Ji, we), -np.einsum("era,er->ea", Jj, we), np.sum(e * we, -1)


def build_system(S, g, info, margins=None, float_roundtrip=False, jacobians=None):
    """-> (H dense [n, n], b [n], errors [E, 6]): 4x4 blocks and 4-vectors summed over the active edges in edge order."""
    dt = info.dtype
    v0, v1, meas, fidx = g["a_v0"], g["a_v1"], g["a_meas"].astype(dt), g["free_idx"]
    n = 4 * g["n_free"]
    e = edge_errors(S, v0, v1, meas, margins)
    Ji, Jj = jacobians if jacobians is not None else numeric_jacobians(S, v0, v1, meas, g["free"], margins=margins, float_roundtrip=float_roundtrip)
    Hii, Hij, Hjj, bi, bj, _ = quadratic_form(e, Ji, Jj, info)
    H, b = np.zeros((n, n), dt), np.zeros(n, dt)
    for k in range(len(v0)):
        fi, fj = fidx[v0[k]], fidx[v1[k]]
        if fi >= 0:
            H[4 * fi:4 * fi + 4, 4 * fi:4 * fi + 4] += Hii[k]; b[4 * fi:4 * fi + 4] += bi[k]
        if fj >= 0:
            H[4 * fj:4 * fj + 4, 4 * fj:4 * fj + 4] += Hjj[k]; b[4 * fj:4 * fj + 4] += bj[k]
        if fi >= 0 and fj >= 0:
            H[4 * fi:4 * fi + 4, 4 * fj:4 * fj + 4] += Hij[k]; H[4 * fj:4 * fj + 4, 4 * fi:4 * fi + 4] += Hij[k].T
    return H, b, e


def dense_system(S, g, info):
    """The same system from one stacked Jacobian: J^T W J and -J^T W e of the whole graph (checks the block assembly)."""
    dt = info.dtype
    v0, v1, meas, fidx = g["a_v0"], g["a_v1"], g["a_meas"].astype(dt), g["free_idx"]
    e = edge_errors(S, v0, v1, meas)
    Ji, Jj = numeric_jacobians(S, v0, v1, meas, g["free"])
    E, n = len(v0), 4 * g["n_free"]
    J = np.zeros((6 * E, n), dt)
    for k in range(E):
        for f, Jk in ((fidx[v0[k]], Ji[k]), (fidx[v1[k]], Jj[k])):
            if f >= 0:
                J[6 * k:6 * k + 6, 4 * f:4 * f + 4] = Jk
    W = np.tile(info, E)
    return J.T @ (W[:, None] * J), -J.T @ (W * e.reshape(-1))


def prepare(graph):
    """The optimiser's view of an ABI graph: free numbering in vertex order, the active edges (at least one free endpoint) in edge order."""
    fixed = np.asarray(graph["fixed"]).astype(bool)
    free = ~fixed
    fidx = np.where(free, np.cumsum(free) - 1, -1)
    v0, v1 = np.asarray(graph["edge_v0"], np.int64), np.asarray(graph["edge_v1"], np.int64)
    act = free[v0] | free[v1] if len(v0) else np.zeros(0, bool)
    return dict(free=free, free_idx=fidx, n_free=int(free.sum()), a_v0=v0[act], a_v1=v1[act],
                a_meas=np.asarray(graph["edge_meas"], np.float64).reshape(-1, 12)[act], active=act)


def default_params(iterations=20, info_diag=INFO_REFERENCE, lambda_init=0.0):
    return dict(iterations=iterations, lambda_init=lambda_init, tau=1e-50, info_diag=tuple(info_diag), max_trials=100)


def to_state36(S, state_in, free):
    out = np.asarray(state_in, np.float64).reshape(-1, 36).astype(S["twb"].dtype)
    V = len(out)
    new = np.concatenate([S["Rwb"].reshape(V, 9), S["twb"], S["Rcw"].reshape(V, 9), S["tcw"]], 1)
    out[free, :24] = new[free]
    return out


def optimize(graph, state36, params, dt=np.float64, its_step=True, derive_at_load=False, float_roundtrip=False):
    """SparseOptimizer::optimize(iterations) under OptimizationAlgorithmLevenberg.  -> dict(est [V, 36], chi_first, chi_last, lam,
    iterations, trials, reason, trace (per iteration: chi, dchi, trials (chi2, rho, lambda, accepted), accepted, est, lam, b0 = the
    iteration's b), margins, n, n_free, free, lam0 = the start lambda, accepted_iterations)."""
    g = prepare(graph)
    S = load(state36, dt, derive_at_load)
    info = np.asarray(params["info_diag"], np.float64).astype(dt)
    mg = Margins()
    out = dict(est=to_state36(S, state36, g["free"]), chi_first=dt(0), chi_last=dt(0), lam=dt(0), iterations=0, trials=0, reason=END_ITERATIONS, trace=[],
               margins=mg, n=4 * g["n_free"], n_free=g["n_free"], free=g["free"], lam0=dt(0), accepted_iterations=0)
    if g["n_free"] == 0 or len(g["a_v0"]) == 0:
        return out
    n = 4 * g["n_free"]
    fl = np.flatnonzero(g["free"])
    meas = g["a_meas"].astype(dt)
    chi_of = lambda St: np.sum(np.sum(info * edge_errors(St, g["a_v0"], g["a_v1"], meas, mg) ** 2, -1))
    lam, ni, nbad = dt(0), dt(2), 0
    x = np.zeros(n, dt)
    any_solved = False
    cur = dt(0)
    for it in range(params["iterations"]):
        cur = chi_of(S)
        if it == 0:
            out["chi_first"] = cur
        ini = cur
        H, b, _ = build_system(S, g, info, mg, float_roundtrip)
        if it == 0:
            lam = dt(params["lambda_init"]) if params["lambda_init"] > 0 else dt(params["tau"]) * np.max(np.abs(np.diag(H)))
            out["lam0"] = lam
        rho, qmax, trials = dt(0), 0, []
        while True:
            bk = S
            sol = ldlt_solve(H + lam * np.eye(n, dtype=dt), b)
            ok2 = sol is not None
            if ok2:
                x = sol
            any_solved = any_solved or ok2
            S = oplus(S, fl, x.reshape(-1, 4), mg, its_step, float_roundtrip)
            tmp = chi_of(S) if ok2 else dt(np.finfo(np.float64).max)
            scale = np.sum(x * (lam * x + b)) + dt(1e-3)
            rho = (cur - tmp) / scale
            used = lam
            good = bool(rho > 0 and np.isfinite(tmp))
            if good:
                alpha = min(1 - (2 * rho - 1) ** 3, dt(2) / 3)
                lam = lam * max(dt(1) / 3, alpha); ni = dt(2); cur = tmp
            else:
                lam = lam * ni; ni = ni * 2; S = bk
            trials.append((tmp, rho, used, good))
            qmax += 1
            if not (rho < 0 and qmax < params["max_trials"]):
                break
        out["iterations"] += 1; out["trials"] += qmax
        out["accepted_iterations"] += 1 if trials[-1][3] else 0
        out["trace"].append(dict(chi=ini, dchi=ini - cur, trials=trials, accepted=[t[3] for t in trials], est=to_state36(S, state36, g["free"]), lam=lam, b0=b,
                                 DR=S["DR"].copy()))
        if qmax == params["max_trials"] or rho == 0:
            out["reason"] = END_SOLVE_FAILED if (it == 0 and not any_solved) else END_TERMINATE
            break
        nbad = nbad + 1 if (ini - cur) * 1000 < ini else 0
        if nbad >= 3:
            out["reason"] = END_NBAD
            break
    if out["reason"] != END_SOLVE_FAILED:
        out["est"] = to_state36(S, state36, g["free"])
    out["chi_last"], out["lam"] = cur, lam
    return out
