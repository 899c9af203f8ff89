"""numpy model of Sim3Solver, written from the reference text (src/Sim3Solver.cc, include/Sim3Solver.h): the yardstick of the HIP solver.

  * inputs are float32 (mvX3Dc1 / mvX3Dc2 are CV_32F); ComputeSim3 (:316-427) runs in double on them and T12 / T21 / R12 / t12 / s12
    are rounded once to float32 -- the library's documented choice; the eigenvector comes from this file's cyclic Jacobi iteration (the
    kernel's order of operations) or, as a cross-check, from numpy.linalg.eigh;
  * CheckInliers (:430-454) in float32 in the reference's operation order: Rcw * X + tcw as OpenCV's small-matrix gemm (the row's products
    summed in float, then (float)(sum * 1.0 + t * 1.0)), GeometricCamera::project (Pinhole.cpp:34-37, KannalaBrandt8.cpp:28-45, no z
    test), Mat::dot as a double sum rounded once, err < max against the TRUNCATED threshold (std::vector<size_t>, Sim3Solver.h:78-79);
    f64=True evaluates the same expressions in double (the precondition tests compare the two);
  * SetRansacParameters (:126-150) with the library's saturation, the scan rule of iterate() (:170-213) and the class-level chunked run.
Per iteration the model also reports the margin min_i |err - max| / max over both errors: how close the count is to flipping."""
import math
import numpy as np
import ransac_sets_model

F32 = np.float32


# ------------------------------------------------------------------ thresholds and budget
def truncated_threshold(sigma2):
    """mvnMaxError.push_back(9.210 * sigmaSquare) into a std::vector<size_t>: 1.44 -> 13, not 13.26"""
    return float(int(9.210 * float(F32(sigma2))))


def iteration_budget(n, probability, min_inliers, max_iterations):
    """mRansacMaxIts of SetRansacParameters; 0 for N < mRansacMinInliers (iterate answers bNoMore at once).  Where the reference converts
    a quotient beyond INT_MAX to int unchecked, the library saturates to max_iterations."""
    if n < min_inliers:
        return 0
    if min_inliers == n:
        its = 1
    else:
        eps = float(F32(min_inliers) / F32(n))
        with np.errstate(divide="ignore"):
            q = np.ceil(np.log(1 - probability) / np.log(np.float64(1) - np.float64(eps) ** 3))
        its = int(q) if q < max_iterations else max_iterations
    return max(1, min(its, max_iterations))


# ------------------------------------------------------------------ Horn
def jacobi_eig4_max(N):
    """eigenvector of the largest eigenvalue of the symmetric 4x4 N by cyclic Jacobi, operation for operation as csrc/horn_sim3.h; among
    equal eigenvalues the lowest index wins"""
    A = [[float(N[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    fro = 0.0
    for i in range(4):
        for j in range(4):
            fro += A[i][j] * A[i][j]
    thr = 1e-17 * math.sqrt(fro) if fro == fro else fro                   # NaN stays NaN: no comparison holds, no rotation
    for _ in range(30):
        rot = False
        for p in range(3):
            for r in range(p + 1, 4):
                apq = A[p][r]
                if not abs(apq) > thr:
                    continue
                app, aqq = A[p][p], A[r][r]
                theta = (aqq - app) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][r]
                    V[k][p] = c * vkp - s * vkq
                    V[k][r] = s * vkp + c * vkq
                    if k == p or k == r:
                        continue
                    akp, akq = A[k][p], A[k][r]
                    A[k][p] = A[p][k] = c * akp - s * akq
                    A[k][r] = A[r][k] = s * akp + c * akq
                A[p][p] = app - t * apq
                A[r][r] = aqq + t * apq
                A[p][r] = A[r][p] = 0.0
                rot = True
        if not rot:
            break
    m = 0
    for k in (1, 2, 3):
        if A[k][k] > A[m][m]:
            m = k
    return np.array([V[i][m] for i in range(4)])


def horn(P1, P2, fix_scale, solver="jacobi"):
    """ComputeSim3 on one set: P1 / P2 [3 points][3] float32 -> dict of float32 sR12 [3][3], t12, sR21, t21, R12, s12"""
    P1 = np.asarray(P1, F32).astype(np.float64)
    P2 = np.asarray(P2, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        O1 = ((P1[0] + P1[1]) + P1[2]) / 3.0
        O2 = ((P2[0] + P2[1]) + P2[2]) / 3.0
        Pr1, Pr2 = P1 - O1, P2 - O2                                         # [point][coordinate]
        M = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                M[i, j] = (Pr2[0, i] * Pr1[0, j] + Pr2[1, i] * Pr1[1, j]) + Pr2[2, i] * Pr1[2, j]
        N11 = M[0, 0] + M[1, 1] + M[2, 2]; N12 = M[1, 2] - M[2, 1]; N13 = M[2, 0] - M[0, 2]; N14 = M[0, 1] - M[1, 0]
        N22 = M[0, 0] - M[1, 1] - M[2, 2]; N23 = M[0, 1] + M[1, 0]; N24 = M[2, 0] + M[0, 2]
        N33 = -M[0, 0] + M[1, 1] - M[2, 2]; N34 = M[1, 2] + M[2, 1]; N44 = -M[0, 0] - M[1, 1] + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]])
        if solver == "eigh":
            q = np.linalg.eigh(N)[1][:, 3] if np.isfinite(N).all() else np.full(4, np.nan)
        else:
            q = jacobi_eig4_max(N)
        nv = math.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
        ang = math.atan2(nv, q[0])
        r = np.array([2.0 * ang * q[1], 2.0 * ang * q[2], 2.0 * ang * q[3]]) / np.float64(nv)
        theta = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        if theta < np.finfo(np.float64).eps:
            R = np.eye(3)
        else:
            c, s = np.cos(theta), np.sin(theta)
            c1, it = 1.0 - c, 1.0 / theta
            kx, ky, kz = r[0] * it, r[1] * it, r[2] * it
            R = np.array([[c + c1 * kx * kx, c1 * kx * ky - s * kz, c1 * kx * kz + s * ky],
                          [c1 * kx * ky + s * kz, c + c1 * ky * ky, c1 * ky * kz - s * kx],
                          [c1 * kx * kz - s * ky, c1 * ky * kz + s * kx, c + c1 * kz * kz]])
        s12 = np.float64(1.0)
        if not fix_scale:
            nom = den = np.float64(0.0)
            for k in range(3):
                for i in range(3):
                    p3 = (R[i, 0] * Pr2[k, 0] + R[i, 1] * Pr2[k, 1]) + R[i, 2] * Pr2[k, 2]
                    nom = nom + Pr1[k, i] * p3
                    den = den + p3 * p3
            s12 = nom / den
        t = np.array([O1[i] - s12 * ((R[i, 0] * O2[0] + R[i, 1] * O2[1]) + R[i, 2] * O2[2]) for i in range(3)])
        sRi = (np.float64(1.0) / s12) * R.T
        t21 = np.array([-((sRi[i, 0] * t[0] + sRi[i, 1] * t[1]) + sRi[i, 2] * t[2]) for i in range(3)])
        return dict(sR12=(s12 * R).astype(F32), t12=t.astype(F32), sR21=sRi.astype(F32), t21=t21.astype(F32), R12=R.astype(F32), s12=F32(s12))


# ------------------------------------------------------------------ projection and scoring
def project(cam, P, f64=False):
    """GeometricCamera::project on rows of P [n][3]; cam = dict(K=(fx, fy, cx, cy), kb8=None | (k1..k4)), parameters narrowed to float"""
    T = np.float64 if f64 else F32
    fx, fy, cx, cy = [T(F32(v)) for v in cam["K"]]
    x, y, z = [np.asarray(P[:, k], T) for k in range(3)]
    with np.errstate(all="ignore"):
        if cam["kb8"] is None:
            return np.stack([fx * x / z + cx, fy * y / z + cy], -1)
        k = [T(F32(v)) for v in cam["kb8"]]
        x2_plus_y2 = x * x + y * y
        theta = np.arctan2(np.sqrt(x2_plus_y2).astype(np.float64), z.astype(np.float64)).astype(T)
        psi = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(T)
        theta2 = theta * theta; theta3 = theta * theta2; theta5 = theta3 * theta2; theta7 = theta5 * theta2; theta9 = theta7 * theta2
        r = theta + k[0] * theta3 + k[1] * theta5 + k[2] * theta7 + k[3] * theta9
        c, s = np.cos(psi.astype(np.float64)).astype(T), np.sin(psi.astype(np.float64)).astype(T)
        return np.stack([fx * r * c + cx, fy * r * s + cy], -1)


def gemm_add(R, X, t, f64=False):
    """rows of X through Rcw * X + tcw as cv::gemm's small-matrix path computes it on CV_32F"""
    T = np.float64 if f64 else F32
    R = np.asarray(R, T); X = np.asarray(X, T); t = np.asarray(t, T)
    with np.errstate(all="ignore"):
        cols = []
        for i in range(3):
            s = R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2]
            cols.append((s.astype(np.float64) * 1.0 + np.float64(t[i]) * 1.0).astype(T))
        return np.stack(cols, -1)


def prepare(pb, f64=False):
    """FromCameraToImage (:492-506): mvP1im1 / mvP2im2"""
    return project(pb["cam1"], np.asarray(pb["X1c"], F32), f64), project(pb["cam2"], np.asarray(pb["X2c"], F32), f64)


def check_inliers(pb, hyp, p1, p2, f64=False):
    """-> (inlier [n] bool, margin): margin = min_i |err - max| / max over both errors (inf when nothing is comparable)"""
    T = np.float64 if f64 else F32
    X1, X2 = np.asarray(pb["X1c"], F32), np.asarray(pb["X2c"], F32)
    m1, m2 = np.asarray(pb["max1"], T), np.asarray(pb["max2"], T)
    if len(X1) == 0:
        return np.zeros(0, bool), np.inf, (np.zeros(0, T), np.zeros(0, T))
    with np.errstate(all="ignore"):
        d1 = np.asarray(p1, T) - project(pb["cam1"], gemm_add(hyp["sR12"], X2, hyp["t12"], f64), f64)
        d2 = project(pb["cam2"], gemm_add(hyp["sR21"], X1, hyp["t21"], f64), f64) - np.asarray(p2, T)
        e1 = (d1[:, 0].astype(np.float64) ** 2 + d1[:, 1].astype(np.float64) ** 2).astype(T)
        e2 = (d2[:, 0].astype(np.float64) ** 2 + d2[:, 1].astype(np.float64) ** 2).astype(T)
        inl = (e1 < m1) & (e2 < m2)
        rel = np.r_[np.abs(e1.astype(np.float64) - m1) / m1, np.abs(e2.astype(np.float64) - m2) / m2]
    rel = rel[np.isfinite(rel)]
    return inl, (float(rel.min()) if rel.size else np.inf), (e1, e2)


def count_bounds(pb, e1, e2, delta):
    """(fewest, most) inliers when every comparison within delta of its threshold may go either way"""
    m1, m2 = np.asarray(pb["max1"], np.float64), np.asarray(pb["max2"], np.float64)
    with np.errstate(all="ignore"):
        e1 = e1.astype(np.float64); e2 = e2.astype(np.float64)
        lo = (e1 < m1 * (1 - delta)) & (e2 < m2 * (1 - delta))
        hi = (e1 < m1 * (1 + delta)) & (e2 < m2 * (1 + delta))
    return int(lo.sum()), int(hi.sum())


# ------------------------------------------------------------------ the scan rule and one candidate
def scan(counts, min_inliers):
    """iterate()'s rule over the counts of iterations 0 .. budget-1 -> (converged, winner): the first count > min_inliers converges;
    without one the best is the LAST arg-max (>= updates the best, which starts at 0)"""
    best, winner = 0, -1
    for k, c in enumerate(counts):
        if c >= best:
            best, winner = c, k
            if c > min_inliers:
                return True, k
    return False, winner


def draw_sets_reference(n, iterations, randint):
    """:175-189: per iteration 3 draws, randint(d) = RandomInt(0, d - 1), the drawn slot refilled with the last one; -1 for n < 3"""
    if n < 3:
        return np.full((iterations, 3), -1, np.int32)
    return ransac_sets_model.draw_sets_reference(n, iterations, randint, 3)


def solve(pb, sets, probability=0.99, min_inliers=6, max_iterations=300, solver="jacobi", f64=False, delta=None):
    """one candidate: pb = dict(X1c, X2c [n][3] float32, max1, max2 [n] truncated thresholds, cam1, cam2, fix_scale), sets [>= budget][3]
    -> dict(budget, counts [budget], margins [budget], converged, winner, n_inliers, inlier [n] bool, R12, t12, s12, hyps, bounds)"""
    n = len(pb["X1c"])
    budget = iteration_budget(n, probability, min_inliers, max_iterations)
    out = dict(budget=budget, counts=np.zeros(budget, int), margins=np.full(budget, np.inf), converged=False, winner=-1, n_inliers=0,
               inlier=np.zeros(n, bool), R12=None, t12=None, s12=None, hyps=[], bounds=[])
    if budget == 0:
        return out
    p1, p2 = prepare(pb, f64)
    X1, X2 = np.asarray(pb["X1c"], F32), np.asarray(pb["X2c"], F32)
    flags = []
    for k in range(budget):
        s = np.asarray(sets[k])
        if (s < 0).any() or (s >= n).any():                                 # no hypothesis: NaN, count 0
            h = dict(sR12=np.full((3, 3), np.nan, F32), t12=np.full(3, np.nan, F32), sR21=np.full((3, 3), np.nan, F32), t21=np.full(3, np.nan, F32),
                     R12=np.full((3, 3), np.nan, F32), s12=F32(np.nan))
        else:
            h = horn(X1[s], X2[s], pb["fix_scale"], solver)
        inl, mg, (e1, e2) = check_inliers(pb, h, p1, p2, f64)
        out["hyps"].append(h); flags.append(inl)
        out["counts"][k] = int(inl.sum()); out["margins"][k] = mg
        if delta is not None:
            out["bounds"].append(count_bounds(pb, e1, e2, delta))
    conv, w = scan(out["counts"], min_inliers)
    out.update(converged=conv, winner=w, R12=out["hyps"][w]["R12"], t12=out["hyps"][w]["t12"], s12=out["hyps"][w]["s12"])
    if conv:
        out.update(n_inliers=int(out["counts"][w]), inlier=flags[w])
    return out


def decision_is_stable(res, min_inliers, delta):
    """precondition (b): converged flag, winning iteration and the winner's flags are the same however the comparisons within delta go"""
    if res["budget"] == 0:
        return True
    lo = np.array([b[0] for b in res["bounds"]]); hi = np.array([b[1] for b in res["bounds"]])
    w = res["winner"]
    if res["converged"]:
        return bool((hi[:w] <= min_inliers).all() and lo[w] > min_inliers and res["margins"][w] >= delta)
    return bool((hi <= min_inliers).all() and (hi[:w] <= lo[w]).all() and (hi[w + 1:] < lo[w]).all())


# ------------------------------------------------------------------ the class: state across iterate() calls
class ChunkedSolver:
    """Sim3Solver's public behaviour on one candidate: iterate(n) in chunks and find(), from the per-iteration results of solve()"""

    def __init__(self, pb, sets, n1, indices1, probability=0.99, min_inliers=6, max_iterations=300, **kw):
        self.pb, self.n1, self.indices1, self.min_inliers = pb, n1, np.asarray(indices1, int), min_inliers
        self.N = len(pb["X1c"])
        self.res = solve(pb, sets, probability, min_inliers, max_iterations, **kw)
        self.max_its = self.res["budget"]
        self.iterations, self.best_inliers, self.best = 0, 0, None

    def iterate(self, n):
        """-> dict(T12 (4x4 float32 or None), no_more, inliers [n1] bool, n_inliers, converged): the bConverge overload"""
        out = dict(T12=None, no_more=False, inliers=np.zeros(self.n1, bool), n_inliers=0, converged=False)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur, improved = 0, None
        while self.iterations < self.max_its and cur < n:
            k = self.iterations
            cur += 1; self.iterations += 1
            c = self.res["counts"][k]
            if c >= self.best_inliers:
                self.best_inliers, self.best = c, k
                improved = k
                if c > self.min_inliers:
                    out.update(T12=self.T12(k), n_inliers=int(c), converged=True)
                    out["inliers"][self.indices1[self.res["inlier"]]] = True
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
        if improved is not None:
            out["T12"] = self.T12(improved)
        return out

    def T12(self, k):
        h = self.res["hyps"][k]
        T = np.eye(4, dtype=F32)
        T[:3, :3] = h["R12"] * h["s12"]                                     # sR = ms12i * mR12i, float products (:413)
        T[:3, 3] = h["t12"]
        return T

    def estimated(self):
        h = self.res["hyps"][self.best]
        return h["R12"], h["t12"], h["s12"]

    def find(self):
        return self.iterate(self.max_its)


def loop_closing_run(cs, chunk=20):
    """src/LoopClosing.cc:681-684 -> (the last iterate's answer, number of calls)"""
    calls = 0
    while True:
        r = cs.iterate(chunk)
        calls += 1
        if r["converged"] or r["no_more"]:
            return r, calls
