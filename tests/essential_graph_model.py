"""Numpy model of Optimizer::OptimizeEssentialGraph's optimisation (reference src/Optimizer.cc:2347-2663) written from the reference
text over a dtype parameter (float64 / longdouble).  TEST INFRASTRUCTURE ONLY: it imports nothing from the kernels' side.

  Sim3 exp / log / * / inverse / map    Thirdparty/g2o/g2o/types/sim3.h:70-142, 148-230, 266-272, 233-236, 144-146
  residual log(Sji S_i S_j^-1)          types_seven_dof_expmap.h:106-114
  numeric Jacobians, delta = 1e-9       g2o/core/base_binary_edge.hpp:136-200 through VertexSim3Expmap::oplusImpl (:60-69)
  quadratic form, identity information  base_binary_edge.hpp:55-90
  LM control                            g2o/core/optimization_algorithm_levenberg.cpp:61-194 (lambda_init by the user, :171-174)
  point correction                      src/Optimizer.cc:2636-2660

A Sim3 is (qx qy qz qw tx ty tz s); all functions work on arrays [..., 8] / [..., 7].  The linear system is dense; it is solved by the
model's own L D L^T without pivoting (numpy.linalg has nothing for longdouble), which fails on a zero or non-finite pivot and then leaves
x as it was, as the reference's solver does.  Every run reports its per-trial trace and the smallest distance of any evaluated branch
argument to its threshold: |sigma| and d of Sim3::log against 1e-5 and 1 - 1e-5, theta and |sigma| of the exponential against 1e-5."""
import numpy as np

LD = np.longdouble
EPS_BRANCH = 0.00001
DELTA = 1e-9
END_ITERATIONS, END_TERMINATE, END_NBAD, END_SOLVE_FAILED = 0, 1, 2, 3


class Margins:
    """Smallest distance of the evaluated branch arguments to their thresholds."""

    def __init__(self):
        self.log_sigma = self.log_d = self.exp_theta = self.exp_sigma = np.inf

    def note(self, name, dist):
        if dist.size:
            setattr(self, name, min(getattr(self, name), float(np.min(dist))))

    def smallest(self):
        return min(self.log_sigma, self.log_d, self.exp_theta, self.exp_sigma)

    def as_dict(self):
        return dict(log_sigma=self.log_sigma, log_d=self.log_d, exp_theta=self.exp_theta, exp_sigma=self.exp_sigma)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def quat_rot(q, v):
    """Eigen's quaternion * vector (no normalisation)."""
    uv = _cross(q[..., :3], v)
    uv = uv + uv
    return v + q[..., 3:4] * uv + _cross(q[..., :3], uv)


def quat_mul(a, b):
    aw, bw = a[..., 3], b[..., 3]
    w = aw * bw - np.sum(a[..., :3] * b[..., :3], -1)
    v = aw[..., None] * b[..., :3] + bw[..., None] * a[..., :3] + _cross(a[..., :3], b[..., :3])
    return np.concatenate([v, w[..., None]], -1)


def quat_to_R(q):
    """Eigen's toRotationMatrix."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def R_to_quat(R):
    """Eigen::Quaterniond(Matrix3d): the trace branch, else the largest diagonal element picks (i, j, k)."""
    dt = R.dtype
    half = dt.type(0.5)
    R00, R11, R22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    tr = R00 + R11 + R22
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + 1)
        q0 = np.stack([(R[..., 2, 1] - R[..., 1, 2]) * (half / t), (R[..., 0, 2] - R[..., 2, 0]) * (half / t), (R[..., 1, 0] - R[..., 0, 1]) * (half / t), half * t], -1)
        out = [q0]
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            t = np.sqrt(R[..., i, i] - R[..., j, j] - R[..., k, k] + 1)
            q = np.zeros(R.shape[:-2] + (4,), dt)
            q[..., i] = half * t
            t = half / t
            q[..., 3] = (R[..., k, j] - R[..., j, k]) * t
            q[..., j] = (R[..., j, i] + R[..., i, j]) * t
            q[..., k] = (R[..., k, i] + R[..., i, k]) * t
            out.append(q)
    i = np.where(R11 > R00, 1, 0)
    i = np.where(R22 > np.where(i == 0, R00, R11), 2, i)
    sel = np.where(tr > 0, 0, i + 1)
    res = out[0]
    for c in (1, 2, 3):
        res = np.where((sel == c)[..., None], out[c], res)
    return res


def skew(w):
    O = np.zeros(w.shape[:-1] + (3, 3), w.dtype)
    O[..., 0, 1] = -w[..., 2]; O[..., 0, 2] = w[..., 1]; O[..., 1, 0] = w[..., 2]
    O[..., 1, 2] = -w[..., 0]; O[..., 2, 0] = -w[..., 1]; O[..., 2, 1] = w[..., 0]
    return O


def _abc(sigma, theta, s, small_sigma, small_theta):
    """A, B, C of sim3.h:93-128 / :168-213 for all four branches at once."""
    dt = sigma.dtype
    one = dt.type(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        th2, sg2 = theta * theta, sigma * sigma
        A_st = (1 - np.cos(theta)) / th2
        B_st = (theta - np.sin(theta)) / (th2 * theta)
        C_l = (s - 1) / sigma
        A_lt = ((sigma - 1) * s + 1) / sg2
        B_lt = ((dt.type(0.5) * sg2 - sigma + 1) * s) / (sg2 * sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), th2 + sg2
        A_ll = (a * sigma + (1 - b) * theta) / (theta * c)
        B_ll = (C_l - ((b - 1) * sigma + a * theta) / c) * one / th2
    A = np.where(small_sigma, np.where(small_theta, one / 2, A_st), np.where(small_theta, A_lt, A_ll))
    B = np.where(small_sigma, np.where(small_theta, one / 6, B_st), np.where(small_theta, B_lt, B_ll))
    C = np.where(small_sigma, one, C_l)
    return A, B, C


def s3_exp(u, margins=None):
    """g2o::Sim3(Vector7d): the small-angle branches use R = I + Omega + Omega^2 (not 1/2 Omega^2), kept."""
    dt = u.dtype
    eps = dt.type(EPS_BRANCH)
    om, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt(np.sum(om * om, -1))
    if margins is not None:
        margins.note("exp_theta", np.abs(theta - eps)); margins.note("exp_sigma", np.abs(np.abs(sigma) - eps))
    s = np.exp(sigma)
    small_sigma, small_theta = np.abs(sigma) < eps, theta < eps
    A, B, C = _abc(sigma, theta, s, small_sigma, small_theta)
    O = skew(om)
    O2 = O @ O
    with np.errstate(invalid="ignore", divide="ignore"):
        ra = np.where(small_theta, dt.type(1), np.sin(theta) / theta)
        rb = np.where(small_theta, dt.type(1), (1 - np.cos(theta)) / (theta * theta))
    I = np.eye(3, dtype=dt)
    R = I + ra[..., None, None] * O + rb[..., None, None] * O2
    W = A[..., None, None] * O + B[..., None, None] * O2 + C[..., None, None] * I
    t = np.einsum("...ij,...j->...i", W, ups)
    return np.concatenate([R_to_quat(R), t, s[..., None]], -1)


def _lu_solve3(W, t):
    """Eigen's PartialPivLU of a 3x3: row pivoting on the column's largest magnitude (first one on ties)."""
    M = np.concatenate([W, t[..., None]], -1).reshape(-1, 3, 4).copy()
    ar = np.arange(len(M))
    for k in range(2):
        p = k + np.argmax(np.abs(M[:, k:, k]), 1)
        rk, rp = M[ar, k].copy(), M[ar, p].copy()
        M[ar, k], M[ar, p] = rp, rk
        for r in range(k + 1, 3):
            l = M[:, r, k] / M[:, k, k]
            M[:, r, k + 1:] = M[:, r, k + 1:] - l[:, None] * M[:, k, k + 1:]
    x2 = M[:, 2, 3] / M[:, 2, 2]
    x1 = (M[:, 1, 3] - M[:, 1, 2] * x2) / M[:, 1, 1]
    x0 = (M[:, 0, 3] - M[:, 0, 1] * x1 - M[:, 0, 2] * x2) / M[:, 0, 0]
    return np.stack([x0, x1, x2], -1).reshape(t.shape)


def s3_log(S, margins=None):
    dt = S.dtype
    eps = dt.type(EPS_BRANCH)
    s = S[..., 7]
    sigma = np.log(s)
    R = quat_to_R(S[..., :4])
    d = dt.type(0.5) * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    if margins is not None:
        margins.note("log_sigma", np.abs(np.abs(sigma) - eps)); margins.note("log_d", np.abs(d - (1 - eps)))
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small_sigma, small_theta = np.abs(sigma) < eps, d > 1 - eps
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(d)
        f = np.where(small_theta, dt.type(0.5), theta / (2 * np.sqrt(1 - d * d)))
    om = f[..., None] * dR
    A, B, C = _abc(sigma, theta, s, small_sigma, small_theta)
    O = skew(om)
    W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3, dtype=dt)
    ups = _lu_solve3(W, S[..., 4:7])
    return np.concatenate([om, ups, sigma[..., None]], -1)


def s3_mul(a, b):
    t = a[..., 7:8] * quat_rot(a[..., :4], b[..., 4:7]) + a[..., 4:7]
    return np.concatenate([quat_mul(a[..., :4], b[..., :4]), t, (a[..., 7] * b[..., 7])[..., None]], -1)


def s3_inverse(a):
    q = a[..., :4] * np.array([-1, -1, -1, 1], a.dtype)
    t = quat_rot(q, (-1 / a[..., 7:8]) * a[..., 4:7])
    return np.concatenate([q, t, 1 / a[..., 7:8]], -1)


def s3_map(S, X):
    return S[..., 7:8] * quat_rot(S[..., :4], X) + S[..., 4:7]


def edge_errors(est, v0, v1, meas, margins=None):
    """computeError of every edge: log(Sji * S_i * S_j^-1)."""
    return s3_log(s3_mul(s3_mul(meas, est[v0]), s3_inverse(est[v1])), margins)


def oplus(S, u, fix_scale, margins=None):
    """VertexSim3Expmap::oplusImpl: Sim3(update) * estimate, update[6] = 0 under _fix_scale."""
    if fix_scale:
        u = u.copy(); u[..., 6] = 0
    return s3_mul(s3_exp(u, margins), S)


def numeric_jacobians(est, v0, v1, meas, free, fix_scale, delta=DELTA, margins=None):
    """-> (Ji, Jj) [E, 7, 7]: central differences through oplus; a fixed vertex gets zeros."""
    dt = est.dtype
    dl = dt.type(delta)
    scalar = dt.type(1) / (2 * dl)
    E = len(v0)
    J = np.zeros((2, E, 7, 7), dt)
    for side, vs in ((0, v0), (1, v1)):
        fr = free[vs]
        for c in range(7):
            pm = []
            for sg in (dl, -dl):
                u = np.zeros((E, 7), dt); u[:, c] = sg
                Sp = oplus(est[vs], u, fix_scale, margins)
                a, b = (Sp, est[v1]) if side == 0 else (est[v0], Sp)
                pm.append(s3_log(s3_mul(s3_mul(meas, a), s3_inverse(b)), margins))
            J[side, :, :, c] = np.where(fr[:, None], scalar * (pm[0] - pm[1]), 0)
    return J[0], J[1]


def ldlt_solve(A, b, nb=32):
    """Dense L D L^T without pivoting (lower triangle of A), blocked right-looking; None on a zero / non-finite pivot."""
    n = len(b)
    L = np.tril(A).copy()
    d = np.zeros(n, A.dtype)
    for p0 in range(0, n, nb):
        p1 = min(p0 + nb, n)
        for j in range(p0, p1):
            dj = L[j, j]
            if dj == 0 or not np.isfinite(dj):
                return None
            d[j] = dj
            col = L[j + 1:, j].copy()
            l = col / dj
            L[j + 1:, j] = l
            if j + 1 < p1:                                   # inside the panel: all rows below, the panel's remaining columns
                L[j + 1:, j + 1:p1] -= np.outer(l, col[:p1 - j - 1])
        if p1 < n:
            P = L[p1:, p0:p1]
            L[p1:, p1:] -= np.tril((P * d[p0:p1]) @ P.T)
    y = np.array(b, A.dtype)
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y = y / d
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    return y


def build_system(est, g, dt, margins=None):
    """-> (H dense [n, n], b [n], errors [E, 7]) over the active edges in edge order."""
    v0, v1, meas, free, fidx = g["a_v0"], g["a_v1"], g["a_meas"].astype(dt), g["free"], g["free_idx"]
    n = 7 * g["n_free"]
    e = edge_errors(est, v0, v1, meas, margins)
    Ji, Jj = numeric_jacobians(est, v0, v1, meas, free, g["fix_scale"], margins=margins)
    H, b = np.zeros((n, n), dt), np.zeros(n, dt)
    Hii, Hij, Hjj = np.einsum("era,erb->eab", Ji, Ji), np.einsum("era,erb->eab", Ji, Jj), np.einsum("era,erb->eab", Jj, Jj)
    bi, bj = -np.einsum("era,er->ea", Ji, e), -np.einsum("era,er->ea", Jj, e)
    for k in range(len(v0)):
        fi, fj = fidx[v0[k]], fidx[v1[k]]
        if fi >= 0:
            H[7 * fi:7 * fi + 7, 7 * fi:7 * fi + 7] += Hii[k]; b[7 * fi:7 * fi + 7] += bi[k]
        if fj >= 0:
            H[7 * fj:7 * fj + 7, 7 * fj:7 * fj + 7] += Hjj[k]; b[7 * fj:7 * fj + 7] += bj[k]
        if fi >= 0 and fj >= 0:
            H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += Hij[k]; H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += Hij[k].T
    return H, b, e


def prepare(graph, fix_scale):
    """The optimiser's view of an ABI graph (dict of fixed, edge_v0, edge_v1, edge_meas): free numbering in vertex order, the active
    edges (at least one free endpoint, sparse_optimizer.cpp:234) in edge order."""
    fixed = np.asarray(graph["fixed"]).astype(bool)
    free = ~fixed
    fidx = np.where(free, np.cumsum(free) - 1, -1)
    v0, v1 = np.asarray(graph["edge_v0"], np.int64), np.asarray(graph["edge_v1"], np.int64)
    act = free[v0] | free[v1] if len(v0) else np.zeros(0, bool)
    return dict(free=free, free_idx=fidx, n_free=int(free.sum()), a_v0=v0[act], a_v1=v1[act],
                a_meas=np.asarray(graph["edge_meas"], np.float64).reshape(-1, 8)[act], fix_scale=bool(fix_scale), active=act)


def default_params(iterations=20, fix_scale=False):
    return dict(iterations=iterations, lambda_init=1e-16, fix_scale=fix_scale, max_trials=100)


def optimize(graph, sim3, params, dt=np.float64):
    """SparseOptimizer::optimize(iterations) under OptimizationAlgorithmLevenberg.  -> dict(est, chi_first, chi_last, lam, iterations,
    trials, reason, trace (one dict per iteration: chi = chi2 at its start, dchi = chi2 gained, trials: list of (chi2, rho, lambda,
    accepted), est = estimates at its end), margins, n)."""
    g = prepare(graph, params["fix_scale"])
    est = np.asarray(sim3, np.float64).reshape(-1, 8).astype(dt)
    est0 = est.copy()
    mg = Margins()
    out = dict(est=est, chi_first=dt(0), chi_last=dt(0), lam=dt(0), iterations=0, trials=0, reason=END_ITERATIONS, trace=[], margins=mg,
               n=7 * g["n_free"], n_free=g["n_free"], free=g["free"])
    if g["n_free"] == 0 or len(g["a_v0"]) == 0:
        return out
    n = 7 * g["n_free"]
    fl = np.flatnonzero(g["free"])
    meas = g["a_meas"].astype(dt)
    chi_of = lambda E: np.sum(np.sum(edge_errors(E, g["a_v0"], g["a_v1"], meas, mg) ** 2, -1))
    lam, ni, nbad = dt(params["lambda_init"]), dt(2), 0
    x = np.zeros(n, dt)
    any_solved = False
    for it in range(params["iterations"]):
        cur = chi_of(est)
        if it == 0:
            out["chi_first"] = cur
        ini = cur
        H, b, _ = build_system(est, g, dt, mg)
        rho, qmax, trials = dt(0), 0, []
        while True:
            bk = est.copy()
            sol = ldlt_solve(H + lam * np.eye(n, dtype=dt), b)
            ok2 = sol is not None
            if ok2:
                x = sol
            any_solved = any_solved or ok2
            xs = x.reshape(-1, 7)
            if params["fix_scale"]:
                xs[:, 6] = 0                                 # written through to the solver's x
            est = est.copy()
            est[fl] = oplus(est[fl], xs, params["fix_scale"], mg)
            tmp = chi_of(est) if ok2 else dt(np.finfo(np.float64).max)
            scale = np.sum(x * (lam * x + b)) + dt(1e-3)
            rho = (cur - tmp) / scale
            used = lam
            good = bool(rho > 0 and np.isfinite(tmp))
            if good:
                alpha = min(1 - (2 * rho - 1) ** 3, dt(2) / 3)
                lam = lam * max(dt(1) / 3, alpha); ni = dt(2); cur = tmp
            else:
                lam = lam * ni; ni = ni * 2; est = bk
            trials.append((tmp, rho, used, good))
            qmax += 1
            if not (rho < 0 and qmax < params["max_trials"]):
                break
        out["iterations"] += 1; out["trials"] += qmax
        out["trace"].append(dict(chi=ini, dchi=ini - cur, trials=trials, accepted=[t[3] for t in trials], est=est.copy(), lam=lam))
        if qmax == params["max_trials"] or rho == 0:
            out["reason"] = END_SOLVE_FAILED if (it == 0 and not any_solved) else END_TERMINATE
            break
        nbad = nbad + 1 if (ini - cur) * 1000 < ini else 0
        if nbad >= 3:
            out["reason"] = END_NBAD
            break
    out["est"] = est0 if out["reason"] == END_SOLVE_FAILED else est
    out["chi_last"], out["lam"] = cur, lam
    return out


def decisive_prefix(trace_ld):
    """inertial_opt_model.decisive_prefix's rule: the iterations before the first one whose extended-precision |dchi2| falls below
    1e-9 chi2 -- past it rho is rounding noise."""
    for i, r in enumerate(trace_ld):
        if not abs(r["dchi"]) >= 1e-9 * abs(r["chi"]):
            return i
    return len(trace_ld)


def prefix_totals(run, pre):
    """(iterations, trials, accept flags, lambda) of the first `pre` iterations of a run."""
    tr = run["trace"][:pre]
    flags = [a for r in tr for a in r["accepted"]]
    return len(tr), len(flags), flags, (tr[-1]["lam"] if tr else None)


def correct_points(Xw, ref, Scw, Swc):
    """src/Optimizer.cc:2636-2660: corrected_Swc[ref].map(Scw[ref].map(Xw)) in double on the float position, rounded once to float
    (computed here in longdouble: the reference's double result is within a double ulp of it); ref < 0: copied through."""
    Xw, ref = np.asarray(Xw, np.float32).reshape(-1, 3), np.asarray(ref)
    ok = (ref >= 0) & (ref < len(Scw))
    r = np.where(ok, ref, 0)
    y = s3_map(np.asarray(Swc, np.float64).astype(LD)[r], s3_map(np.asarray(Scw, np.float64).astype(LD)[r], Xw.astype(LD)))
    return np.where(ok[:, None], y.astype(np.float64).astype(np.float32), Xw)
