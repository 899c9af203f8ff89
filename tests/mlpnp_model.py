"""numpy model of MLPnPsolver, written from the reference's text (src/MLPnPsolver.cpp; line numbers below are that file's): the yardstick
of tests/test_gpu_mlpnp.py and of the stand-alone CPU program of tests/test_mlpnp_abi.py.  computePose (:345-651) runs in double,
CheckInliers (:255-286) in float32 with the reference's rounding points.  Where the reference calls Eigen the model can use numpy.linalg
(lin="numpy": svd for the last right singular vector and the nearest rotation, eigh for the eigenframe, solve for the normal equations)
or arithmetic of its own (lin="jacobi": cyclic Jacobi, the polar factor from the eigenvectors of T^T T, L D L^T), and the null-space
bases can be the closed form (null="closed") or that basis turned by a random orthogonal 2x2 (null="random", with the eigenframe's signs
flipped at random too): the pose does not depend on these choices beyond what Gauss-Newton's stop rule leaves, and the largest distance
between the variants is the scale of the GPU comparison's bound.
The Jacobian is the derivative of N^T normalize(R(w) X + T) from d(R X)/dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2 (Gallego and
Yezzi 2015); tests/test_mlpnp_model.py checks it against central differences.  It divides by |w|^2 as the reference's generated code
does: NaN at w = 0."""
import math
import numpy as np
import ransac_sets_model
import sim3_solver_model as s3m

F32 = np.float32
EPS = float(np.finfo(np.float64).eps)
VARIANTS = (("numpy", "closed"), ("jacobi", "closed"), ("numpy", "random"), ("jacobi", "random"))


# ------------------------------------------------------------------ SetRansacParameters (:218-253)
def ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=6, epsilon=0.4):
    """-> (nMin, budget); budget 0 for n < nMin (iterate() says bNoMore at once)"""
    eps = F32(epsilon)
    nmin = max(int(F32(n) * eps), min_inliers, min_set)
    if n < nmin:
        return nmin, 0
    if nmin == n:
        b = 1
    else:
        eps = max(eps, F32(nmin) / F32(n))
        q = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
        b = q if q < max_iterations else max_iterations
    return nmin, max(1, min(b, max_iterations))


def draw_sets_reference(n, iterations, randint):
    """:118-138 with randint(d) = DUtils::Random::RandomInt(0, d - 1)"""
    return ransac_sets_model.draw_sets_reference(n, iterations, randint, 6)


def bearings(cam, p2d):
    """:77-78: unproject(pt) / z in float"""
    import oracle_match_bind as om
    params = np.array(list(cam["K"]) + list(cam["kb8"] if cam["kb8"] is not None else (0, 0, 0, 0)), F32)
    out = np.zeros((len(p2d), 3), F32)
    for i, (u, v) in enumerate(np.asarray(p2d, F32)):
        ray = om.camera_unproject_f(0 if cam["kb8"] is None else 1, params, u, v)
        out[i] = ray / ray[2]
    return out


# ------------------------------------------------------------------ pieces of computePose
def jacobi_eig(A, sweeps=30):
    """cyclic Jacobi on a symmetric matrix, a pair left alone once |apq| <= eps sqrt(|app aqq|) -> (eigenvalues, eigenvectors as
    columns), unsorted"""
    A = np.array(A, np.float64); n = len(A); V = np.eye(n)
    for _ in range(sweeps):
        rot = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if not apq * apq > (EPS * EPS) * abs(A[p, p] * A[q, q]):        # the relative rule; false for NaN
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
                G = np.array([[c, s], [-s, c]])
                A[:, [p, q]] = A[:, [p, q]] @ G
                A[[p, q], :] = G.T @ A[[p, q], :]
                V[:, [p, q]] = V[:, [p, q]] @ G
                rot = True
        if not rot:
            break
    return np.diag(A).copy(), V


def fullpiv_rank(M):
    """FullPivHouseholderQR<Matrix3d>::rank(): full pivoting, the factorisation stops at a corner below eps * 3 of the first one, and
    the rank counts the pivots above |largest pivot| * eps * 3"""
    Q = np.array(M, np.float64); n = 3
    prec = EPS * n
    pivots = []; biggest = None
    for k in range(n):
        corner = np.abs(Q[k:, k:])
        r, c = np.unravel_index(np.argmax(corner), corner.shape)
        b = corner[r, c]
        if k == 0:
            biggest = b
            if not b > 0:
                return 0
        if b <= biggest * prec:
            break
        Q[[k, k + r], :] = Q[[k + r, k], :]; Q[:, [k, k + c]] = Q[:, [k + c, k]]
        x = Q[k:, k].copy()
        beta = -np.linalg.norm(x) if x[0] >= 0 else np.linalg.norm(x)
        v = x.copy(); v[0] -= beta
        vv = float(v @ v)
        if vv > 0:
            Q[k:, k:] -= np.outer(v, (2.0 / vv) * (v @ Q[k:, k:]))
        pivots.append(abs(beta))
    if not pivots:
        return 0
    return int(sum(p > max(pivots) * prec for p in pivots))


def nullspace(f, mode="closed", rng=None):
    """an orthonormal basis of the plane orthogonal to f -> [3][2]"""
    a = np.abs(f); e = np.zeros(3)
    e[0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if a[1] <= a[2] else 2)] = 1.0
    r = np.cross(f, e); r /= np.linalg.norm(r)
    s = np.cross(f, r); s /= np.linalg.norm(s)
    B = np.stack([r, s], 1)
    if mode == "random":
        ang = rng.uniform(0, 2 * math.pi); sg = rng.choice([-1.0, 1.0])
        B = B @ np.array([[math.cos(ang), -sg * math.sin(ang)], [math.sin(ang), sg * math.cos(ang)]])
    return B


def nearest_rotation(T, lin):
    if lin == "numpy":
        U, _, Vt = np.linalg.svd(T)
        return U @ Vt
    lam, V = jacobi_eig(T.T @ T)
    with np.errstate(all="ignore"):
        return T @ (V @ np.diag(1.0 / np.sqrt(lam)) @ V.T)


def rodrigues2rot(w):
    n = np.linalg.norm(w)
    R = np.eye(3)
    if n > EPS:
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = R + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):
    with np.errstate(all="ignore"):
        wnorm = np.arccos((np.trace(R) - 1.0) / 2.0)
    if wnorm > EPS:                                                             # false for NaN too
        return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wnorm / (2.0 * math.sin(wnorm)))
    return np.zeros(3)


def residuals_and_jacs(x, X, NS):
    """:754-1010 -> (r [2n], J [2n][6]) for x = (w, T), points X [n][3], null spaces NS [n][3][2]"""
    w, T = x[:3], x[3:]
    R = rodrigues2rot(w)
    with np.errstate(all="ignore"):
        v = X @ R.T + T
        nv = np.linalg.norm(v, axis=1)
        vh = v / nv[:, None]
        r = np.einsum("nik,ni->nk", NS, vh)                                     # [n][2]
        P = (np.eye(3)[None] - vh[:, :, None] * vh[:, None, :]) / nv[:, None, None]
        G = np.einsum("nik,nij->nkj", NS, P)                                    # N^T (I - v v^T) / |v| : [n][2][3]
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        M = (np.outer(w, w) + (R.T - np.eye(3)) @ Wx) / (w @ w)
        J = np.zeros((len(X), 2, 6))
        for i in range(len(X)):
            Xx = np.array([[0, -X[i, 2], X[i, 1]], [X[i, 2], 0, -X[i, 0]], [-X[i, 1], X[i, 0], 0]])
            J[i, :, :3] = G[i] @ (-R @ Xx @ M)
            J[i, :, 3:] = G[i]
    return r.reshape(-1), J.reshape(-1, 6)


def ldlt_solve(H, g):
    n = len(g); L = np.eye(n); D = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            D[j] = H[j, j] - (L[j, :j] ** 2) @ D[:j]
            for i in range(j + 1, n):
                L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]) @ D[:j]) / D[j]
        y = np.zeros(n)
        for i in range(n):
            y[i] = g[i] - L[i, :i] @ y[:i]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = y[i] / D[i] - L[i + 1:, i] @ x[i + 1:]
    return x


def gauss_newton(x, X, NS, lin):
    """mlpnp_gn (:687-752)"""
    x = x.copy()
    for _ in range(5):
        r, J = residuals_and_jacs(x, X, NS)
        H = J.T @ J; g = J.T @ r
        with np.errstate(all="ignore"):
            if lin == "numpy" and np.isfinite(H).all():
                try:
                    dx = np.linalg.solve(H, g)
                except np.linalg.LinAlgError:
                    dx = ldlt_solve(H, g)
            else:
                dx = ldlt_solve(H, g)
            a = np.abs(dx)
            mx, mn = a[0], a[0]                                                 # Eigen's visitors start from the first coefficient
            for v in a[1:]:
                if v > mx: mx = v
                if v < mn: mn = v
            if mx > 5.0 or mn > 1.0:
                break
            dl = np.abs(J @ dx)
            m = dl[0]
            for v in dl[1:]:
                if v > m: m = v
            x = x - dx
            if m < 1e-5:
                break
    return x


def linear_pose(f, X, lin="numpy", null="closed", rng=None):
    """:345-642 up to the start of Gauss-Newton -> (x0 [6], NS, planar)"""
    n = len(X)
    NS = np.stack([nullspace(f[i], null, rng) for i in range(n)])
    M = X.T @ X
    E = np.eye(3)
    planar = fullpiv_rank(M) == 2
    if planar:
        if lin == "numpy":
            lam, V = np.linalg.eigh(M)
        else:
            lam, V = jacobi_eig(M)
            o = np.argsort(lam, kind="stable"); V = V[:, o]
        E = V.T.copy()
        if null == "random":
            E = E * rng.choice([-1.0, 1.0], 3)[:, None]
    Xe = X @ E.T
    if planar:
        A = np.zeros((2 * n, 9))
        for c in range(2):
            rows = slice(c, 2 * n, 2)
            for i in range(3):
                A[rows, 2 * i] = NS[:, i, c] * Xe[:, 1]; A[rows, 2 * i + 1] = NS[:, i, c] * Xe[:, 2]; A[rows, 6 + i] = NS[:, i, c]
    else:
        A = np.zeros((2 * n, 12))
        for c in range(2):
            rows = slice(c, 2 * n, 2)
            for i in range(3):
                for j in range(3):
                    A[rows, 3 * i + j] = NS[:, i, c] * Xe[:, j]
                A[rows, 9 + i] = NS[:, i, c]
    AtA = A.T @ A
    if lin == "numpy":
        res = np.linalg.svd(AtA)[2][-1]
    else:
        lam, V = jacobi_eig(AtA)
        res = V[:, int(np.argmin(lam))]
    with np.errstate(all="ignore"):
        if planar:                                                              # :524-586
            c1 = np.array([res[0], res[2], res[4]]); c2 = np.array([res[1], res[3], res[5]])
            tmp = np.stack([np.cross(c1, c2), c1, c2], 1).T                     # columns (c0 c1 c2), then transposeInPlace
            scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            R1 = nearest_rotation(tmp, lin)
            if np.linalg.det(R1) < 0:
                R1 = -R1
            R1 = E.T @ R1
            t = scale * res[6:9]
            R1 = -R1.T
            if np.linalg.det(R1) < 0:
                R1[:, 2] *= -1
            R2 = R1 * np.array([-1.0, -1.0, 1.0])[None, :]
            cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
            vals = []
            for Rc, tc in cands:
                v = X[:6] @ Rc.T + tc
                v = v / np.linalg.norm(v, axis=1)[:, None]
                s = 0.0
                for p in range(6):
                    s += 1.0 - v[p] @ f[p]
                vals.append(s)
            k = 0
            for i in range(1, 4):
                if vals[i] < vals[k]:
                    k = i
            Rout, tout = cands[k]
        else:                                                                   # :589-629
            tmp = res[:9].reshape(3, 3).T
            scale = 1.0 / math.pow(abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])), 1.0 / 3.0)
            Rr = nearest_rotation(tmp, lin)
            if np.linalg.det(Rr) < 0:
                Rr = -Rr
            t1 = Rr @ (scale * res[9:12])
            err = []; tinv = []
            for sgn in (1.0, -1.0):
                ti = -Rr.T @ (sgn * t1)
                v = X[:6] @ Rr + ti                                             # rows of Rr^T X
                v = v / np.linalg.norm(v, axis=1)[:, None]
                s = 0.0
                for p in range(6):
                    s += 1.0 - v[p] @ f[p]
                err.append(s); tinv.append(ti)
            tout = tinv[0] if err[0] < err[1] else tinv[1]
            Rout = Rr.T
        x0 = np.r_[rot2rodrigues(Rout), tout]
    return x0, NS, planar


def compute_pose(f, X, lin="numpy", null="closed", rng=None):
    """computePose on bearings f [n][3] and points X [n][3] (float inputs, double arithmetic) -> T [12] = R row-major, t"""
    f = np.asarray(f, np.float64); X = np.asarray(X, np.float64)
    x0, NS, _ = linear_pose(f, X, lin, null, rng)
    x = gauss_newton(x0, X, NS, lin)
    return np.r_[rodrigues2rot(x[:3]).reshape(9), x[3:]]


# ------------------------------------------------------------------ CheckInliers (:255-286)
def check_inliers(pb, T):
    """-> (inlier [n] bool, error2 [n] float32); a hypothesis with a NaN entry has no inliers"""
    X = np.asarray(pb["Xw"], F32).astype(np.float64); n = len(X)
    if n == 0 or np.isnan(T).any():
        return np.zeros(n, bool), np.full(n, np.nan, F32)
    with np.errstate(all="ignore"):
        P = np.stack([(((T[3 * i] * X[:, 0] + T[3 * i + 1] * X[:, 1]) + T[3 * i + 2] * X[:, 2]) + T[9 + i]).astype(F32) for i in range(3)], -1)
        uv = s3m.project(pb["cam"], P)
        p = np.asarray(pb["p2d"], F32)
        dx = p[:, 0] - uv[:, 0]; dy = p[:, 1] - uv[:, 1]
        e2 = (dx * dx + dy * dy).astype(F32)
        return e2 < pb["max_err"], e2


def margin_and_bounds(pb, e2, delta):
    """(smallest relative distance of an error to its threshold, fewest and most inliers when every comparison within delta may go either way)"""
    m = np.asarray(pb["max_err"], np.float64)
    with np.errstate(all="ignore"):
        e = e2.astype(np.float64)
        rel = np.abs(e - m) / m
        lo = int((e < m * (1 - delta)).sum()); hi = int((e < m * (1 + delta)).sum())
    rel = rel[np.isfinite(rel)]
    return (float(rel.min()) if rel.size else np.inf), lo, hi


def valid_set(s, n):
    s = [int(v) for v in s]
    return all(0 <= v < n for v in s) and len(set(s)) == 6


def hypothesis(pb, s, lin="numpy", null="closed", rng=None):
    n = len(pb["Xw"])
    if not valid_set(s, n):
        return np.full(12, np.nan)
    s = np.asarray(s, np.int64)
    return compute_pose(pb["f"][s], pb["Xw"][s], lin, null, rng)


def discarded_refinement(pb, flags, lin="numpy", null="closed", rng=None):
    """what Refine() (:288-321) computes and throws away: computePose on the best's inliers fills a local `result` that is never copied
    into mRi / mti.  Not part of solve(); tests/test_mlpnp_abi.py uses N-point solves of this kind to exercise csrc/mlpnp_core.h."""
    idx = np.nonzero(flags)[0]
    return compute_pose(pb["f"][idx], pb["Xw"][idx], lin, null, rng)


def solve(pb, sets, probability=0.99, min_inliers=8, max_iterations=300, min_set=6, epsilon=0.4, th2=5.991, first_call_iterations=0,
          resume_at=0, lin="numpy", null="closed", seed=0, delta=1e-3, upto=None):
    """one candidate: pb = dict(Xw [n][3] f32, p2d [n][2] f32, sigma2 [n] f32, cam); sets [max_iterations][6].  -> dict(nmin, budget,
    executed, counts, margins, lo, hi, hyps, outcome, ret (returning iteration; outcome 2: the best's; -1), ret_count, n_inliers, inlier,
    T (float64 [12] of the returned pose) / Tcw (its float32), nref (Refine() calls: iterations up to the return whose count reached
    nMin), bests (the iterations that set a new best)).  upto: evaluate iterations 0 .. upto only (a variant run that is compared up to
    a known return).
    Refine() AS WRITTEN (:288-342): its computePose fills a local `result`; mRi / mti are assigned only in iterate() (:150-162), so the
    CheckInliers() at :324 scores the CURRENT iteration's hypothesis again, mnRefinedInliers is count[k], mvbRefinedInliers its flags and
    mRefinedTcw that hypothesis rounded to float.  Refine() "succeeds" exactly when count[k] > nMin, and iterate() returns hypothesis k."""
    rng = np.random.RandomState(seed)
    pb = dict(pb)
    n = len(pb["Xw"])
    pb["max_err"] = (np.asarray(pb["sigma2"], F32) * F32(th2)).astype(F32)
    pb["f"] = bearings(pb["cam"], pb["p2d"]) if "f" not in pb else pb["f"]
    nmin, budget = ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon)
    E = min(max_iterations, max(budget, first_call_iterations)) if budget else 0
    if upto is not None:
        E = min(E, upto + 1)
    out = dict(nmin=nmin, budget=budget, executed=E, counts=np.full(max_iterations, -1, np.int32), margins=np.full(E, np.inf), lo=np.zeros(E, int),
               hi=np.zeros(E, int), hyps=[], outcome=0, ret=-1, ret_count=0, n_inliers=0, inlier=np.zeros(n, bool), T=None, Tcw=None, nref=0,
               bests=[], f=pb["f"], max_err=pb["max_err"])
    flags = []
    for k in range(E):
        T = hypothesis(pb, sets[k], lin, null, rng)
        inl, e2 = check_inliers(pb, T)
        out["hyps"].append(T); flags.append(inl)
        out["counts"][k] = int(inl.sum())
        out["margins"][k], out["lo"][k], out["hi"][k] = margin_and_bounds(pb, e2, delta)
    best, bestk = 0, -1
    for k in range(E):                                                          # :113-197
        c = int(out["counts"][k])
        if c < nmin:                                                            # :167
            continue
        if c > best:                                                            # :170-182
            best, bestk = c, k
            out["bests"].append(k)
        out["nref"] += 1                                                        # :184 Refine(): CheckInliers() on mRi / mti of iteration k
        if c > nmin and k >= resume_at:                                         # :329 -> :186-193
            out.update(outcome=1, ret=k, ret_count=c, n_inliers=c, inlier=flags[k], T=out["hyps"][k])
            break
    if out["outcome"] == 0 and bestk >= 0:                                      # :199-212
        out.update(outcome=2, ret=bestk, ret_count=best, n_inliers=best, inlier=flags[bestk], T=out["hyps"][bestk])
    if out["T"] is not None:
        out["Tcw"] = out["T"].astype(F32)
    return out


def decision_is_stable(res, delta):
    """the precondition of a count-for-count comparison: up to the return, no iteration that could reach nMin whichever way its close
    comparisons go (which includes every new best, every count within 1 of nMin and the returning iteration) has an error within delta
    (relative) of its threshold"""
    nmin = res["nmin"]
    last = res["ret"] if res["outcome"] == 1 else res["executed"] - 1
    for k in range(last + 1):
        if res["margins"][k] < delta and res["hi"][k] >= nmin - 1:
            return False
    return True
