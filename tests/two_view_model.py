"""numpy model of TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:39-933), written from the reference text
and sharing no code with the library.  dtype = np.float32 follows the reference's operation order in the per-match arithmetic
(CheckHomography, CheckFundamental, CheckRT); dtype = np.float64 is the yardstick.  Every decomposition is numpy's (LAPACK) SVD, the sets
are explicit, rh_threshold is a knob (the reference's 0.50, :117; its older 0.40 is in its comment)."""
import numpy as np
import ransac_sets_model

TH_H = 5.991
TH_F = 3.841
TH_SCORE = 5.991
COS_LIMIT = 0.99998


def match_list(matches12, n2):
    """mvMatches12 (:53-62): (first index, second index) of the matched keypoints in index order; an entry >= n2 is no match."""
    m = np.asarray(matches12)
    i1 = np.nonzero((m >= 0) & (m < n2))[0]
    return i1.astype(np.int64), m[i1].astype(np.int64)


def draw_sets_reference(N, iterations, rand):
    """:81-96 with `rand` = a callable returning the next DUtils::Random::RandomInt(0, d-1) for a given d."""
    return ransac_sets_model.draw_sets_reference(N, iterations, rand, 8)


def random_sets(N, iterations, seed):
    r = np.random.RandomState(seed)
    return np.array([r.choice(N, 8, replace=False) for _ in range(iterations)], np.int32).reshape(iterations, 8)


def normalize(pts, dt):
    """Normalize (:753-799) over ALL keypoints of the frame -> (normalised points, T)."""
    p = np.asarray(pts, dt)
    n = len(p)
    mean = (p.sum(0, dtype=np.float64) / n).astype(dt)
    q = p - mean
    dev = (np.abs(q).sum(0, dtype=np.float64) / n).astype(dt)
    s = dt(1.0) / dev
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], dt)
    return q * s, T


def inv3(S, dt):
    """cv::invert of a 3x3 matrix as OpenCV does it for CV_32F: cofactors and determinant in double, each entry rounded once."""
    S = np.asarray(S, dt).astype(np.float64)
    s = lambda i, j: S[..., i, j]
    d = s(0, 0) * (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) - s(0, 1) * (s(1, 0) * s(2, 2) - s(1, 2) * s(2, 0)) + \
        s(0, 2) * (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / d
    T = np.empty(S.shape, np.float64)
    T[..., 0, 0] = (s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1)) * d
    T[..., 0, 1] = (s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2)) * d
    T[..., 0, 2] = (s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1)) * d
    T[..., 1, 0] = (s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2)) * d
    T[..., 1, 1] = (s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0)) * d
    T[..., 1, 2] = (s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2)) * d
    T[..., 2, 0] = (s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0)) * d
    T[..., 2, 1] = (s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1)) * d
    T[..., 2, 2] = (s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)) * d
    T[~np.isfinite(d)] = 0.0
    return T.astype(dt)


def hypotheses(kp1, kp2, i1, i2, sets, dt):
    """ComputeH21 / ComputeF21 (:231-308) of every set, denormalised (:165, :217) -> H21 [it][3][3], F21 [it][3][3]."""
    n1, T1 = normalize(kp1, dt)
    n2, T2 = normalize(kp2, dt)
    T2inv = np.linalg.inv(T2.astype(np.float64)).astype(dt)
    a = n1[i1][sets]                    # [it][8][2]
    b = n2[i2][sets]
    u1, v1, u2, v2 = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    A = np.empty((len(sets), 16, 9), dt)
    A[:, 0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    A[:, 1::2] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    Hn = np.linalg.svd(A)[2][:, 8].reshape(-1, 3, 3)
    H21 = (T2inv @ Hn @ T1).astype(dt)
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], -1).astype(dt)
    Fp = np.linalg.svd(A)[2][:, 8].reshape(-1, 3, 3)
    U, w, Vt = np.linalg.svd(Fp)
    w[:, 2] = 0
    Fn = (U * w[:, None, :]) @ Vt
    F21 = (T2.T @ Fn @ T1).astype(dt)
    return H21, F21


def chi_h(H21, H12, p1, p2, dt):
    """the two chi-squares of CheckHomography (:357-379) at sigma = 1; H [...][3][3] broadcast against the matches"""
    H = np.asarray(H21, dt)[..., None]
    Hi = np.asarray(H12, dt)[..., None]
    u1, v1, u2, v2 = [np.asarray(x, dt) for x in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
    with np.errstate(all="ignore"):
        w = dt(1.0) / (Hi[..., 2, 0, :] * u2 + Hi[..., 2, 1, :] * v2 + Hi[..., 2, 2, :])
        x = (Hi[..., 0, 0, :] * u2 + Hi[..., 0, 1, :] * v2 + Hi[..., 0, 2, :]) * w
        y = (Hi[..., 1, 0, :] * u2 + Hi[..., 1, 1, :] * v2 + Hi[..., 1, 2, :]) * w
        c1 = (u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)
        w = dt(1.0) / (H[..., 2, 0, :] * u1 + H[..., 2, 1, :] * v1 + H[..., 2, 2, :])
        x = (H[..., 0, 0, :] * u1 + H[..., 0, 1, :] * v1 + H[..., 0, 2, :]) * w
        y = (H[..., 1, 0, :] * u1 + H[..., 1, 1, :] * v1 + H[..., 1, 2, :]) * w
        c2 = (u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)
    return c1, c2


def chi_f(F21, p1, p2, dt):
    """the two chi-squares of CheckFundamental (:433-459) at sigma = 1"""
    F = np.asarray(F21, dt)[..., None]
    u1, v1, u2, v2 = [np.asarray(x, dt) for x in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
    with np.errstate(all="ignore"):
        a2 = F[..., 0, 0, :] * u1 + F[..., 0, 1, :] * v1 + F[..., 0, 2, :]
        b2 = F[..., 1, 0, :] * u1 + F[..., 1, 1, :] * v1 + F[..., 1, 2, :]
        c2 = F[..., 2, 0, :] * u1 + F[..., 2, 1, :] * v1 + F[..., 2, 2, :]
        num2 = a2 * u2 + b2 * v2 + c2
        d1 = num2 * num2 / (a2 * a2 + b2 * b2)
        a1 = F[..., 0, 0, :] * u2 + F[..., 1, 0, :] * v2 + F[..., 2, 0, :]
        b1 = F[..., 0, 1, :] * u2 + F[..., 1, 1, :] * v2 + F[..., 2, 1, :]
        c1 = F[..., 0, 2, :] * u2 + F[..., 1, 2, :] * v2 + F[..., 2, 2, :]
        num1 = a1 * u1 + b1 * v1 + c1
        d2 = num1 * num1 / (a1 * a1 + b1 * b1)
    return d1, d2


def score_from_chi(c1, c2, th, sigma, dt):
    """score and inlier flags from the two chi-squares: the running float sum of :365-384 / :443-464 in match order"""
    inv = dt(1.0) / (dt(sigma) * dt(sigma))
    c1 = c1 * inv
    c2 = c2 * inv
    with np.errstate(invalid="ignore"):
        o1, o2 = c1 > dt(th), c2 > dt(th)
    terms = np.stack([np.where(o1, dt(0), dt(TH_SCORE) - c1), np.where(o2, dt(0), dt(TH_SCORE) - c2)], -1).astype(dt)
    terms = terms.reshape(terms.shape[:-2] + (-1,))
    score = np.cumsum(terms, -1, dtype=dt)[..., -1] if terms.shape[-1] else np.zeros(terms.shape[:-1], dt)
    return score, ~o1 & ~o2


def check_homography(H21, p1, p2, sigma, dt):
    c1, c2 = chi_h(H21, inv3(H21, dt), p1, p2, dt)
    return score_from_chi(c1, c2, TH_H, sigma, dt)


def check_fundamental(F21, p1, p2, sigma, dt):
    c1, c2 = chi_f(F21, p1, p2, dt)
    return score_from_chi(c1, c2, TH_F, sigma, dt)


def argmax_first(scores):
    """:170 / :221: strictly greater wins -> the lowest iteration among equal scores; a score of 0 (or NaN) never wins"""
    best, bi = 0.0, -1
    for i, s in enumerate(np.asarray(scores)):
        if s > best:
            best, bi = s, i
    return bi, best


def check_rt(R, t, K4, p1, p2, inl, th2, dt):
    """CheckRT (:802-911) -> dict: n (nGood), parallax [deg], keep / good [N] flags, X [N][3] and the quantities the tests band on"""
    fx, fy, cx, cy = [dt(v) for v in K4]
    R = np.asarray(R, dt)
    t = np.asarray(t, dt).reshape(3)
    N = len(p1)
    Kmat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    P1 = np.c_[Kmat, np.zeros(3)].astype(dt)
    P2 = (Kmat @ np.c_[R.astype(np.float64), t.astype(np.float64)]).astype(dt)
    O2 = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(dt)
    out = dict(n=0, parallax=0.0, keep=np.zeros(N, bool), good=np.zeros(N, bool), X=np.zeros((N, 3), dt), edge=np.zeros(N, bool))
    idx = np.nonzero(inl)[0]
    if len(idx) == 0:
        return out
    q1, q2 = np.asarray(p1, dt)[idx], np.asarray(p2, dt)[idx]
    A = np.stack([q1[:, 0:1] * P1[2] - P1[0], q1[:, 1:2] * P1[2] - P1[1], q2[:, 0:1] * P2[2] - P2[0], q2[:, 1:2] * P2[2] - P2[1]], 1).astype(dt)
    v = np.linalg.svd(A)[2][:, 3]
    with np.errstate(all="ignore"):
        X = (v[:, :3] / v[:, 3:4]).astype(dt)
        fin = np.isfinite(X).all(1)
        X64 = X.astype(np.float64)
        d1 = np.sqrt((X64 * X64).sum(1)).astype(dt)
        n2 = X - O2
        n264 = n2.astype(np.float64)
        d2 = np.sqrt((n264 * n264).sum(1)).astype(dt)
        cos = ((X64 * n264).sum(1) / (d1 * d2).astype(np.float64)).astype(dt)
        low = cos.astype(np.float64) < COS_LIMIT
        X2 = (X64 @ R.astype(np.float64).T).astype(dt) + t
        keep = fin & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low)
        iz1 = dt(1.0) / X[:, 2]
        e1 = (fx * X[:, 0] * iz1 + cx - q1[:, 0]) ** 2 + (fy * X[:, 1] * iz1 + cy - q1[:, 1]) ** 2
        iz2 = dt(1.0) / X2[:, 2]
        e2 = (fx * X2[:, 0] * iz2 + cx - q2[:, 0]) ** 2 + (fy * X2[:, 1] * iz2 + cy - q2[:, 1]) ** 2
        keep &= ~(e1 > dt(th2)) & ~(e2 > dt(th2))
        # matches whose decisions hang on a threshold: reprojection errors within 1e-3 relative of th2, depths within 1e-3 of the point's
        # distance from zero, 1 - cosParallax within 1e-3 relative of 1 - 0.99998 plus four float ulps of 1 (the resolution of a float cosine)
        edge = (np.abs(e1 - th2) <= 1e-3 * th2) | (np.abs(e2 - th2) <= 1e-3 * th2) | (np.abs(X[:, 2]) <= 1e-3 * d1) | \
               (np.abs(X2[:, 2]) <= 1e-3 * d2) | (np.abs(cos.astype(np.float64) - COS_LIMIT) <= 1e-3 * (1 - COS_LIMIT) + 4 * 2.0 ** -24) | ~fin
    out["n"] = int(keep.sum())
    out["keep"][idx] = keep
    out["good"][idx] = keep & low
    out["X"][idx[keep]] = X[keep]
    out["edge"][idx] = edge
    if out["n"] > 0:
        c = np.sort(cos[keep])
        out["parallax"] = float(np.degrees(np.arccos(np.clip(np.float64(c[min(50, len(c) - 1)]), -1, 1))))
    return out


def motion_hypotheses_f(F21, K4, dt):
    """E21 = K^T F21 K and DecomposeE (:484-502, :913-933): (R1, t), (R2, t), (R1, -t), (R2, -t)"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dt)
    E = (K.T @ np.asarray(F21, dt) @ K).astype(dt)
    u, w, vt = np.linalg.svd(E)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dt)
    R1 = u @ W @ vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = u @ W.T @ vt
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def motion_hypotheses_h(H21, K4, dt):
    """Faugeras (:588-690) -> the 8 (R, t), or None when d1/d2 < 1.00001 or d2/d3 < 1.00001 (:601)"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dt)
    A = (np.linalg.inv(K.astype(np.float64)).astype(dt) @ np.asarray(H21, dt) @ K).astype(dt)
    U, w, Vt = np.linalg.svd(A)
    s = dt(np.linalg.det(U) * np.linalg.det(Vt))
    d1, d2, d3 = [dt(x) for x in w]
    with np.errstate(all="ignore"):
        if not (np.isfinite(d1 / d2) and np.isfinite(d2 / d3)) or d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            return None
    a1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    a3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [a1, a1, -a1, -a1]
    x3 = [a3, -a3, a3, -a3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    out = []
    for i in range(4):
        Rp = np.eye(3, dtype=dt)
        Rp[0, 0] = ct; Rp[0, 2] = -st[i]; Rp[2, 0] = st[i]; Rp[2, 2] = ct
        tp = np.array([x1[i], 0, -x3[i]], dt) * (d1 - d3)
        tt = U @ tp
        out.append(((s * U @ Rp @ Vt).astype(dt), (tt / np.linalg.norm(tt)).astype(dt)))
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    for i in range(4):
        Rp = np.eye(3, dtype=dt)
        Rp[0, 0] = cp; Rp[0, 2] = sp[i]; Rp[1, 1] = -1; Rp[2, 0] = sp[i]; Rp[2, 2] = -cp
        tp = np.array([x1[i], 0, x3[i]], dt) * (d1 + d3)
        tt = U @ tp
        out.append(((s * U @ Rp @ Vt).astype(dt), (tt / np.linalg.norm(tt)).astype(dt)))
    return out


def reconstruct_from(model, M, inl, K4, p1, p2, dt, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    """ReconstructH (model 1, :577-736) / ReconstructF (model 2, :475-575) from a given matrix and inlier flags -> dict: ok, hyps [(R, t)],
    n_good, sel (the hypothesis whose parallax decides, -1 = none), parallax, rt (CheckRT of sel), margin (the smallest distance, in
    points, of an integer decision from flipping) and par_margin (|parallax - min_parallax| in degrees)"""
    N = int(np.sum(inl))
    th2 = 4.0 * float(dt(sigma) * dt(sigma))
    res = dict(ok=False, hyps=[], n_good=[], sel=-1, parallax=0.0, rt=None, margin=1e9, par_margin=1e9, n_inl=N)
    hyps = motion_hypotheses_f(M, K4, dt) if model == 2 else motion_hypotheses_h(M, K4, dt)
    if hyps is None:
        return res
    rts = [check_rt(R, t, K4, p1, p2, inl, th2, dt) for R, t in hyps]
    g = [r["n"] for r in rts]
    res["hyps"], res["n_good"] = hyps, g
    if model == 2:
        mg = max(g)
        nmin = max(int(0.9 * N), min_triangulated)
        nsim = sum(x > 0.7 * mg for x in g)
        others = sorted(g)[:-1]
        res["margin"] = min([abs(mg - nmin)] + [abs(x - 0.7 * mg) for x in others] + [abs(x - mg) for x in others])
        if mg < nmin or nsim > 1:
            return res
        k = g.index(mg)
        res["sel"], res["parallax"], res["rt"] = k, rts[k]["parallax"], rts[k]
        res["par_margin"] = abs(rts[k]["parallax"] - min_parallax)
        res["ok"] = bool(rts[k]["parallax"] > min_parallax)
    else:
        best = second = 0
        bi = -1
        for i, n in enumerate(g):
            if n > best:
                second, best, bi = best, n, i
            elif n > second:
                second = n
        if bi < 0:
            return res
        res["sel"], res["parallax"], res["rt"] = bi, rts[bi]["parallax"], rts[bi]
        res["margin"] = min(abs(second - 0.75 * best), abs(best - min_triangulated), abs(best - 0.9 * N), abs(best - second))
        res["par_margin"] = abs(rts[bi]["parallax"] - min_parallax)
        res["ok"] = bool(second < 0.75 * best and rts[bi]["parallax"] >= min_parallax and best > min_triangulated and best > 0.9 * N)
    return res


def reconstruct(kp1, kp2, matches12, K4, sets, dt, sigma=1.0, rh_threshold=0.50, min_parallax=1.0, min_triangulated=50):
    """the whole of Reconstruct (:39-127).  kp1 / kp2: [n][2] pixel coordinates.  -> dict (see the keys below)"""
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    kp2 = np.asarray(kp2, np.float32).reshape(-1, 2)
    i1, i2 = match_list(matches12, len(kp2))
    N = len(i1)
    n1 = len(kp1)
    out = dict(N=N, i1=i1, i2=i2, ok=False, model=0, SH=0.0, SF=0.0, iH=-1, iF=-1, RH=None, R=None, t=None, P3D=np.zeros((n1, 3), dt),
               tri=np.zeros(n1, bool), rec=None, scores=None, H21=None, F21=None)
    if N < 8:
        return out
    p1, p2 = kp1[i1], kp2[i2]
    out["p1"], out["p2"] = p1, p2
    H21, F21 = hypotheses(kp1, kp2, i1, i2, np.asarray(sets), dt)
    sh, _ = check_homography(H21, p1, p2, sigma, dt)
    sf, _ = check_fundamental(F21, p1, p2, sigma, dt)
    out["scores"], out["H21"], out["F21"] = np.stack([sh, sf], -1), H21, F21
    iH, SH = argmax_first(sh)
    iF, SF = argmax_first(sf)
    SH, SF = dt(SH), dt(SF)
    out.update(SH=float(SH), SF=float(SF), iH=iH, iF=iF)
    if SH + SF == 0:
        return out
    RH = SH / (SH + SF)
    out["RH"] = float(RH)
    model = 1 if RH > dt(rh_threshold) else 2
    if (model == 1 and iH < 0) or (model == 2 and iF < 0):
        return out
    out["model"] = model
    M = H21[iH] if model == 1 else F21[iF]
    inl = (check_homography(M, p1, p2, sigma, dt) if model == 1 else check_fundamental(M, p1, p2, sigma, dt))[1]
    rec = reconstruct_from(model, M, inl, K4, p1, p2, dt, sigma, min_parallax, min_triangulated)
    out["rec"], out["inl"] = rec, inl
    if rec["ok"]:
        R, t = rec["hyps"][rec["sel"]]
        out.update(ok=True, R=np.asarray(R, dt), t=np.asarray(t, dt))
        out["P3D"][i1[rec["rt"]["keep"]]] = rec["rt"]["X"][rec["rt"]["keep"]]
        out["tri"][i1[rec["rt"]["good"]]] = True
    return out


def rot_angle_deg(Ra, Rb):
    """angle of Ra Rb^T from the chord |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2): well conditioned at small angles, where acos of the trace
    turns a rounding error of 1e-7 into 0.02 degrees"""
    d = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64))
    return float(np.degrees(2 * np.arcsin(min(1.0, d / (2 * np.sqrt(2))))))


def dir_angle_deg(a, b):
    a = np.asarray(a, np.float64).reshape(3); b = np.asarray(b, np.float64).reshape(3)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))
