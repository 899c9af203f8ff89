"""Extended-precision model of ONE Levenberg-Marquardt tick of the bundle adjustments.  TEST INFRASTRUCTURE ONLY.

One tick = normal equations -> Schur complement -> LDL^T of the reduced system -> point back-substitution -> x0 (+) dx, everything in
numpy longdouble (80-bit, eps 1.1e-19 on x86).  The per-edge residuals and Jacobians are the float64 oracle's per-edge entry points
(orc_ba_edge / orc_ba_edge_kb8 / orc_ba_edge_tobody, orc_iba_edge_visual / orc_iba_edge_inertial; pinned by finite differences in
test_oracle_match_ba.py / test_oracle_iba.py); everything downstream is this file's own and shares no code with the oracle's
build_system / solve_system / ldlt_solve.  The assembly is generic: camera-side unknown blocks of a given width (6 for the local BA,
15 / 6 for the inertial window), 3-vector points, visual edges (block, point, J_block, J_point, r, weight) and non-visual edges
(columns, J, r, information), so the local and the inertial window run through the same solve_tick().

A candidate result (the oracle's or the device's download after one tick) is measured by
  step error      e = max(|X1 - X1_model|, |T1 - T1_model|) / |dx_model|_inf   (rotation matrix + translation of every free keyframe,
                                                                                every point that has an edge; velocity / biases too
                                                                                in the inertial window)
  backward error  |(H + lambda I) dx - b|_inf / (|H + lambda I|_inf |dx|_inf + |b|_inf)  of the full, unreduced system, blockwise
  floor           2^-52 max|estimate| / |dx_model|_inf      (what storing a result in float64 costs)
and the device is held to e_device <= K (e_oracle + floor), see within_bound()."""
import ctypes as C
import numpy as np
import pytest

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:
    pytest.skip("numpy longdouble is not an extended-precision type on this host (eps %.3g): the one-tick BA model needs eps < 1e-18"
                % float(np.finfo(LD).eps), allow_module_level=True)
assert np.finfo(LD).eps < 1e-18

EPS64 = LD(2) ** -52
# e_device <= K (e_oracle + floor).  K started at 4 (the margin test_gpu_two_view.py gives the device in the same construction) and was raised
# by the rule the tests state: a case may exceed it only with a backward error at float64 level (<= order 2^-52), and K is then the
# smallest power of two that covers twice the largest measured ratio.  Measured on an MI355X: 63.9 (the 20 x 500 window in the world
# shifted by (1000, -2000, 500) m; 37.6 on the shifted stereo window), 17.5 (81 free keyframes, k_ba_big_*), 5.2 (48 free keyframes,
# MFMA Schur form), every other graph <= 1.7.  The shifted windows are not a solver effect: this model takes the oracle's float64
# residuals, so e_oracle does not contain what evaluating R X + t at |X| ~ 2000 m costs (3e-10 px), while the device evaluates its own;
# against a model with exact pinhole edges the oracle itself is at 6.6e-10 there (test_ba_step_model.py::test_exact_pinhole_edges...),
# the device at 8.9e-10.
K = 128
ABS_BOUND = 1e-9            # and, in the generator's own coordinates, e_device <= 1e-9 (what test_gpu_ba.py states)


def within_bound(e_candidate, e_oracle, floor, k=K):
    """The bound the device is held to (the yardstick is the float64 oracle's own step error on the same graph)."""
    return float(e_candidate) <= k * (float(e_oracle) + float(floor))


# ---------------------------------------------------------------------------------------------- small dense helpers, longdouble
def _inv3(A):
    """[m,3,3] inverses by the adjugate."""
    c0 = A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1]
    c1 = A[:, 1, 2] * A[:, 2, 0] - A[:, 1, 0] * A[:, 2, 2]
    c2 = A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]
    det = A[:, 0, 0] * c0 + A[:, 0, 1] * c1 + A[:, 0, 2] * c2
    I = np.zeros_like(A)
    I[:, 0, 0] = c0; I[:, 0, 1] = A[:, 0, 2] * A[:, 2, 1] - A[:, 0, 1] * A[:, 2, 2]; I[:, 0, 2] = A[:, 0, 1] * A[:, 1, 2] - A[:, 0, 2] * A[:, 1, 1]
    I[:, 1, 0] = c1; I[:, 1, 1] = A[:, 0, 0] * A[:, 2, 2] - A[:, 0, 2] * A[:, 2, 0]; I[:, 1, 2] = A[:, 0, 2] * A[:, 1, 0] - A[:, 0, 0] * A[:, 1, 2]
    I[:, 2, 0] = c2; I[:, 2, 1] = A[:, 0, 1] * A[:, 2, 0] - A[:, 0, 0] * A[:, 2, 1]; I[:, 2, 2] = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    return I / det[:, None, None]


def _skew(w):
    S = np.zeros(w.shape[:-1] + (3, 3), LD)
    S[..., 0, 1] = -w[..., 2]; S[..., 0, 2] = w[..., 1]; S[..., 1, 0] = w[..., 2]
    S[..., 1, 2] = -w[..., 0]; S[..., 2, 0] = -w[..., 1]; S[..., 2, 1] = w[..., 0]
    return S


def _abc(th):
    """sin(th)/th, (1-cos th)/th^2, (th-sin th)/th^3 with their series below 1e-4 (exact to longdouble there)."""
    th = np.asarray(th, LD)
    small = th < 1e-4
    t = np.where(small, LD(1), th)
    t2 = th * th
    a = np.where(small, 1 - t2 / 6 + t2 * t2 / 120, np.sin(t) / t)
    b = np.where(small, LD(0.5) - t2 / 24 + t2 * t2 / 720, (1 - np.cos(t)) / (t * t))
    c = np.where(small, LD(1) / 6 - t2 / 120 + t2 * t2 / 5040, (t - np.sin(t)) / (t * t * t))
    return a, b, c


def so3_exp(w):
    """[m,3] -> R [m,3,3], V [m,3,3] (the SE3 translation factor)."""
    w = np.asarray(w, LD)
    a, b, c = _abc(np.sqrt(np.sum(w * w, -1)))
    O = _skew(w); O2 = O @ O
    I = np.eye(3, dtype=LD)
    return I + a[..., None, None] * O + b[..., None, None] * O2, I + b[..., None, None] * O + c[..., None, None] * O2


def so3_log(R):
    R = np.asarray(R, LD)
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2     # sin(th) axis
    s = np.sqrt(np.sum(v * v, -1))
    c = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) / 2
    th = np.arctan2(s, c)
    a, _, _ = _abc(th)
    return v / a[..., None]


def quat_to_R(q):
    """[m,4] (x, y, z, w), normalised here in longdouble -> [m,3,3]."""
    q = np.asarray(q, LD)
    q = q / np.sqrt(np.sum(q * q, -1))[..., None]
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.zeros(q.shape[:-1] + (3, 3), LD)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _ldlt_solve(A, b):
    """LDL^T without pivoting, left-looking row loop; returns (x, d, max |L|)."""
    n = len(b)
    Lm = np.zeros((n, n), LD); d = np.zeros(n, LD)
    for j in range(n):
        v = Lm[j, :j] * d[:j]
        d[j] = A[j, j] - np.dot(Lm[j, :j], v)
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ v) / d[j]
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = b[i] - np.dot(Lm[i, :i], y[:i])
    y /= d
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - np.dot(Lm[i + 1:, i], x[i + 1:])
    return x, d, (float(np.abs(Lm).max()) if n else 0.0)


# ---------------------------------------------------------------------------------------------- the generic tick
def solve_tick(dims, L, vis, nonvis, lam_user, tau, leave_out=None):
    """dims [nb]: width of every camera-side unknown block.  vis: dict(block [E] (-1 = fixed), point [E], Jb [E,3,6] (the first six
    unknowns of the block), Jp [E,3,3], r [E,3], w [E]).  nonvis: list of (cols [c] into the camera-side vector, -1 = fixed; J [D,c];
    r [D]; information [D,D], robust weight included).  lambda = lam_user if > 0 else tau max diag (levenberg.cpp:171-185).
    leave_out = "schur" / "backsub": a deliberately WRONG model (one off-diagonal block pair of one point missing from the Schur
    complement / one pose's W term missing from one point's back-substitution) for the tests that prove the bound has teeth."""
    dims = np.asarray(dims, np.int64)
    off = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    nb, n = len(dims), int(off[-1])
    blk, pt = np.asarray(vis["block"], np.int64), np.asarray(vis["point"], np.int64)
    Jb, Jp, r, w = (np.asarray(vis[k], LD) for k in ("Jb", "Jp", "r", "w"))
    active = np.bincount(pt, minlength=L) > 0
    Hll = np.zeros((L, 3, 3), LD); bl = np.zeros((L, 3), LD)
    np.add.at(Hll, pt, np.einsum("eda,e,edb->eab", Jp, w, Jp))
    np.add.at(bl, pt, -np.einsum("eda,e,ed->ea", Jp, w, r))
    H = np.zeros((n, n), LD); b = np.zeros(n, LD)
    fe = np.flatnonzero(blk >= 0)
    bf, pf = blk[fe], pt[fe]
    cols6 = off[bf][:, None] + np.arange(6)
    np.add.at(H, (cols6[:, :, None], cols6[:, None, :]), np.einsum("eda,e,edb->eab", Jb[fe], w[fe], Jb[fe]))
    np.add.at(b, cols6, -np.einsum("eda,e,ed->ea", Jb[fe], w[fe], r[fe]))
    W = np.einsum("eda,e,edb->eab", Jb[fe], w[fe], Jp[fe])                       # [free edges, 6, 3]
    for cols, J, res, Om in nonvis:
        cols = np.asarray(cols, np.int64); keep = cols >= 0
        if not keep.any():
            continue
        J = np.asarray(J, LD); Om = np.asarray(Om, LD); res = np.asarray(res, LD)
        Jk, ck = J[:, keep], cols[keep]
        H[np.ix_(ck, ck)] += Jk.T @ (Om @ Jk)
        b[ck] += -(Jk.T @ (Om @ res))
    if lam_user > 0:
        lam = LD(lam_user)
    else:
        md = LD(0)
        if n:
            md = max(md, np.abs(np.diagonal(H)).max())
        if active.any():
            md = max(md, np.abs(np.einsum("laa->la", Hll[active])).max())
        lam = LD(tau) * md
    Di = np.zeros((L, 3, 3), LD)
    Di[active] = _inv3(Hll[active] + lam * np.eye(3, dtype=LD))
    # Schur complement S = Hcc + lambda I - sum_l W_l D_l^-1 W_l^T, bs = bc - sum_l W_l D_l^-1 bl
    Y = W @ Di[pf]
    bs = b.copy()
    np.add.at(bs, cols6, -np.einsum("eac,ec->ea", Y, bl[pf]))
    S6 = np.zeros((nb, nb, 6, 6), LD)
    if len(fe):
        order = np.argsort(pf, kind="stable")
        lf = pf[order]
        starts = np.flatnonzero(np.r_[True, lf[1:] != lf[:-1]])
        cnt = np.diff(np.r_[starts, len(lf)])
        c2 = cnt * cnt
        grp = np.repeat(np.arange(len(cnt)), c2)
        k = np.arange(int(c2.sum())) - np.repeat(np.cumsum(c2) - c2, c2)
        i1 = order[starts[grp] + k // cnt[grp]]; i2 = order[starts[grp] + k % cnt[grp]]
        if leave_out == "schur":
            cand = np.flatnonzero(bf[i1] != bf[i2])
            p = cand[len(cand) // 2]
            drop = ((i1 == i1[p]) & (i2 == i2[p])) | ((i1 == i2[p]) & (i2 == i1[p]))
            assert drop.sum() == 2
            i1, i2 = i1[~drop], i2[~drop]
        for c in range(0, len(i1), 200000):
            a_, b_ = i1[c:c + 200000], i2[c:c + 200000]
            np.add.at(S6, (bf[a_], bf[b_]), -np.einsum("eac,ebc->eab", Y[a_], W[b_]))
    S = H + lam * np.eye(n, dtype=LD)
    if nb:
        rows = off[:nb, None] + np.arange(6)
        S[rows[:, None, :, None], rows[None, :, None, :]] += S6
    x, d, maxL = _ldlt_solve(S, bs)
    cl = bl.copy()
    back = np.einsum("eab,ea->eb", W, x[cols6]) if len(fe) else np.zeros((0, 3), LD)
    if leave_out == "backsub":
        back[len(fe) // 2] = 0
    np.add.at(cl, pf, -back)
    xl = np.einsum("lab,lb->la", Di, cl)
    sdiag = np.abs(np.diagonal(S)).max() if n else LD(0)
    return dict(x=x, xl=xl, lam=lam, active=active, off=off, dims=dims, n=n, H=H, b=b, Hll=Hll, bl=bl, W=W, cols6=cols6, pf=pf,
                growth=float(np.abs(d).max() / sdiag) if n else 0.0, max_L=maxL,
                pivot_ratio=float(np.abs(d).max() / np.abs(d).min()) if n else 1.0,
                order=n + 3 * int(active.sum()))


def backward_error(t, dxc, dxl):
    """|(H + lambda I) dx - b|_inf / (|H + lambda I|_inf |dx|_inf + |b|_inf) of the full system, evaluated blockwise."""
    lam, act, W, cols6, pf = t["lam"], t["active"], t["W"], t["cols6"], t["pf"]
    dxc = np.asarray(dxc, LD); dxl = np.where(act[:, None], np.asarray(dxl, LD), LD(0))
    rc = t["H"] @ dxc + lam * dxc - t["b"]
    np.add.at(rc, cols6, np.einsum("eab,eb->ea", W, dxl[pf]))
    rl = np.einsum("lab,lb->la", t["Hll"], dxl) + lam * dxl - t["bl"]
    np.add.at(rl, pf, np.einsum("eab,ea->eb", W, dxc[cols6]))
    rows_c = np.abs(t["H"] + lam * np.eye(t["n"], dtype=LD)).sum(1)
    np.add.at(rows_c, cols6, np.abs(W).sum(2))
    rows_l = np.abs(t["Hll"] + lam * np.eye(3, dtype=LD)).sum(2)
    np.add.at(rows_l, pf, np.abs(W).sum(1))
    mx = lambda a: LD(np.abs(a).max()) if np.size(a) else LD(0)
    res = max(mx(rc), mx(rl[act]))
    nrm = max(mx(rows_c), mx(rows_l[act])) * max(mx(dxc), mx(dxl)) + max(mx(t["b"]), mx(t["bl"][act]))
    return float(res / nrm)


def _huber_weight(chi2, delta, dsqr):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(chi2 <= dsqr, LD(1), delta / np.sqrt(chi2))


def _huber_rho(chi2, delta, dsqr):
    with np.errstate(invalid="ignore"):                                              # (no robust kernel: delta = inf)
        return np.where(chi2 <= dsqr, chi2, 2 * np.sqrt(chi2) * delta - dsqr)


# ---------------------------------------------------------------------------------------------- local BA
def _camera_views(g):
    """Per pose: the calibration its edges use (graph_of_pose): list of dicts, index per pose."""
    if g.get("cameras"):
        views = []
        for c in g["cameras"]:
            v = {k: g[k] for k in g if k not in ("cameras", "pose_camera")}
            v.update(fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], bf=c["bf"], kb=c.get("kb"), rig2=c.get("rig2"))
            views.append(v)
        return views, np.asarray(g["pose_camera"], np.int64)
    return [g], np.zeros(g["n_poses"], np.int64)


def local_edges(g, poses):
    """float64 residual and Jacobians of every edge from the oracle's per-edge entry points."""
    import oracle_ba_bind as ob
    lib = ob.lib
    E = g["n_edges"]
    err = np.zeros((E, 3)); Jx = np.zeros((E, 3, 3)); Jt = np.zeros((E, 3, 6))
    X = np.ascontiguousarray(g["points0"], np.float64); O = np.ascontiguousarray(g["edge_obs"], np.float64)
    views, pcam = _camera_views(g)
    cgs = [ob.make_cgraph(v) for v in views]
    kbs = [np.ascontiguousarray(v["kb"], np.float64) if v.get("kb") is not None else None for v in views]
    e_ = np.zeros(3); jx = np.zeros(9); jt = np.zeros(18)
    pe, pjx, pjt = e_.ctypes.data, jx.ctypes.data, jt.ctypes.data
    pP, pX, pO = poses.ctypes.data, X.ctypes.data, O.ctypes.data
    ek, el, es = (np.asarray(g[k]).tolist() for k in ("edge_pose", "edge_point", "edge_stereo"))
    for e in range(E):
        k, st = ek[e], es[e]
        ci = int(pcam[k]); v = views[ci]
        e_[:] = 0; jx[:] = 0; jt[:] = 0
        if st == 2:
            lib.orc_ba_edge_tobody(C.byref(cgs[ci][0]), pP + 56 * k, pX + 24 * el[e], pO + 24 * e, pe, pjx, pjt)
        elif kbs[ci] is not None and st == 0:
            lib.orc_ba_edge_kb8(pP + 56 * k, pX + 24 * el[e], pO + 24 * e, v["fx"], v["fy"], v["cx"], v["cy"], kbs[ci].ctypes.data, pe, pjx, pjt)
        else:
            lib.orc_ba_edge(pP + 56 * k, pX + 24 * el[e], pO + 24 * e, st, v["fx"], v["fy"], v["cx"], v["cy"], v["bf"], pe, pjx, pjt)
        D = 3 if st == 1 else 2
        err[e, :D] = e_[:D]; Jx[e, :D] = jx.reshape(3, 3)[:D]; Jt[e, :D] = jt.reshape(3, 6)[:D]
    return err, Jx, Jt


def exact_pinhole_mono_edges(g, poses):
    """Residual and Jacobians of monocular Pinhole edges evaluated in longdouble by this file (OptimizableTypes.cpp:139-160): what
    local_edges() returns up to the float64 rounding of the oracle's evaluation.  Drop-in for local_edges on all-mono Pinhole graphs."""
    assert np.all(np.asarray(g["edge_stereo"]) == 0) and g.get("kb") is None and not g.get("cameras")
    R = quat_to_R(poses[:, :4]); t = np.asarray(poses[:, 4:], LD)
    ek = np.asarray(g["edge_pose"], np.int64)
    P = np.einsum("eab,eb->ea", R[ek], np.asarray(g["points0"], LD)[g["edge_point"]]) + t[ek]
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = (LD(g[k]) for k in ("fx", "fy", "cx", "cy"))
    E = len(ek)
    obs = np.asarray(g["edge_obs"], LD)
    err = np.zeros((E, 3), LD)
    err[:, 0] = obs[:, 0] - (fx * x / z + cx); err[:, 1] = obs[:, 1] - (fy * y / z + cy)
    pj = np.zeros((E, 3, 3), LD)                                                    # -projectJac
    pj[:, 0, 0] = -fx / z; pj[:, 0, 2] = fx * x / (z * z); pj[:, 1, 1] = -fy / z; pj[:, 1, 2] = fy * y / (z * z)
    D = np.zeros((E, 3, 6), LD)                                                     # d(T X)/d[omega, upsilon] = [-[P]x | I]
    D[:, 0, 1] = z; D[:, 0, 2] = -y; D[:, 0, 3] = 1; D[:, 1, 0] = -z; D[:, 1, 2] = x; D[:, 1, 4] = 1; D[:, 2, 0] = y; D[:, 2, 1] = -x; D[:, 2, 5] = 1
    return err, pj @ R[ek], pj @ D


def _f32(x):
    with np.errstate(over="ignore"):
        return np.float32(x)


def local_tick(g, params, leave_out=None, edges=None):
    """One tick of the local / merge / global BA on a synth_ba graph.  params: the oracle's or the device's parameter struct (same
    fields).  Returns the tick dict of solve_tick() plus chi2 (robust, before the step), free (pose index of every block) and the
    updated estimates R1 [nf,3,3], t1 [nf,3], X1 [L,3]."""
    poses = np.ascontiguousarray(g["poses0"], np.float64).copy()
    neg = poses[:, 3] < 0
    poses[neg, :4] = -poses[neg, :4]
    poses[:, :4] /= np.sqrt(np.sum(poses[:, :4] ** 2, 1))[:, None]                 # SE3Quat ctor (float64, as oracle and device do it)
    err, Jx, Jt = (edges or local_edges)(g, poses)
    ek, el = np.asarray(g["edge_pose"], np.int64), np.asarray(g["edge_point"], np.int64)
    is2 = np.asarray(g["edge_inv_sigma2"], LD)
    errL = np.asarray(err, LD)
    chi2e = is2 * np.sum(errL * errL, 1)
    st = np.asarray(g["edge_stereo"]) == 1
    # thHuber = (float)sqrt(th2), delta^2 kept as a float (Optimizer.cc:1910-1911, robust_kernel_impl.h:84)
    dm = float(_f32(np.sqrt(params.huber_mono2))); ds = float(_f32(np.sqrt(params.huber_stereo2)))
    dm2 = float(_f32(dm * dm)); ds2 = float(_f32(ds * ds))
    delta = np.where(st, LD(ds), LD(dm)); d2 = np.where(st, LD(ds2), LD(dm2))
    w = _huber_weight(chi2e, delta, d2) * is2
    has = np.bincount(ek, minlength=g["n_poses"]) > 0
    free = np.flatnonzero((np.asarray(g["pose_fixed"]) == 0) & has)
    hidx = -np.ones(g["n_poses"], np.int64); hidx[free] = np.arange(len(free))
    L = g["n_points"]
    t = solve_tick(np.full(len(free), 6), L, dict(block=hidx[ek], point=el, Jb=Jt, Jp=Jx, r=err, w=w), [],
                   float(params.user_lambda_init), float(params.tau), leave_out)
    t["chi2"] = float(np.sum(_huber_rho(chi2e, delta, d2)))
    t["free"] = free; t["n_edges"] = g["n_edges"]
    R0 = quat_to_R(poses[free, :4]); t0 = poses[free, 4:].astype(LD)
    dx = t["x"].reshape(len(free), 6)
    # VertexSE3Expmap::oplusImpl: T <- exp([omega, upsilon]) T; below 1e-5 rad SE3Quat::exp takes R = V = I + O + O^2 (se3quat.h:223-257)
    Re, Ve = so3_exp(dx[:, :3])
    tiny = np.sqrt(np.sum(dx[:, :3] ** 2, 1)) < 0.00001
    if tiny.any():
        O = _skew(dx[tiny, :3])
        Re[tiny] = np.eye(3, dtype=LD) + O + O @ O; Ve[tiny] = Re[tiny]
    t["R0"], t["t0"] = R0, t0
    t["R1"] = Re @ R0
    t["t1"] = np.einsum("hab,hb->ha", Re, t0) + np.einsum("hab,hb->ha", Ve, dx[:, 3:])
    t["X0"] = np.asarray(g["points0"], LD)
    t["X1"] = t["X0"] + np.where(t["active"][:, None], t["xl"], LD(0))
    return t


def _mx(*arrs):
    return max([LD(np.abs(a).max()) for a in arrs if np.size(a)] + [LD(0)])


def local_errors(t, poses, points):
    """Step error, backward error and float64 floor of a candidate (poses [P,7], points [L,3]) after one tick."""
    free, act = t["free"], t["active"]
    R1c = quat_to_R(np.asarray(poses)[free, :4]); t1c = np.asarray(poses, LD)[free, 4:]
    X1c = np.asarray(points, LD)
    norm = _mx(t["x"], t["xl"][act])
    e = _mx(R1c - t["R1"], t1c - t["t1"], (X1c - t["X1"])[act]) / norm
    floor = EPS64 * _mx(t["t1"], t["X1"][act], np.ones(1)) / norm
    Rd = R1c @ np.swapaxes(t["R0"], 1, 2)                                          # T1 T0^-1
    td = t1c - np.einsum("hab,hb->ha", Rd, t["t0"])
    om = so3_log(Rd)
    _, V = so3_exp(om)
    up = np.einsum("hab,hb->ha", _inv3(V), td) if len(free) else np.zeros((0, 3), LD)
    dxc = np.concatenate([om, up], 1).reshape(-1)
    return dict(e=float(e), floor=float(floor), backward=backward_error(t, dxc, X1c - t["X0"]), norm=float(norm))


# ---------------------------------------------------------------------------------------------- inertial local BA
K_R, K_T, K_V = 0, 9, 12


def inertial_tick(win, params, leave_out=None):
    """One tick of Optimizer::LocalInertialBA's optimisation on a synth_iba Window: blocks of 15 unknowns (pose 6, velocity, gyro bias,
    accelerometer bias) for keyframes with IMU states and of 6 without; EdgeMono / EdgeStereo visual edges, EdgeInertial (9 x 24,
    Huber sqrt(16.92) where the window marks it), EdgeGyroRW and EdgeAccRW (J = [-I, I]); lambda = lambda_init."""
    import oracle_iba_bind as ib
    lib = ib.lib
    a = win.arrays
    kf = np.ascontiguousarray(win.kf0, np.float64); X = np.ascontiguousarray(win.pts0, np.float64)
    n_kf, L, E, M = win.n_kf, win.n_points, win.n_edges, win.n_inertial
    imu = a["kf_imu"] != 0
    freek = np.flatnonzero(a["kf_fixed"] == 0)
    dims = np.where(imu[freek], 15, 6)
    off = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    blk = -np.ones(n_kf, np.int64); blk[freek] = np.arange(len(freek))
    prob = win.struct(ib.Problem)
    err = np.zeros((E, 3)); Jx = np.zeros((E, 3, 3)); Jp = np.zeros((E, 3, 6))
    e_ = np.zeros(3); jx = np.zeros(9); jp = np.zeros(18)
    ek, el, es = a["edge_kf"].tolist(), a["edge_point"].tolist(), a["edge_stereo"].tolist()
    O = a["edge_obs"]
    for e in range(E):
        lib.orc_iba_edge_visual(C.addressof(prob), kf.ctypes.data + 8 * ib.KF * ek[e], X.ctypes.data + 24 * el[e], O.ctypes.data + 24 * e,
                                es[e], e_.ctypes.data, jx.ctypes.data, jp.ctypes.data)
        D = 3 if es[e] == 1 else 2
        err[e, :D] = e_[:D]; Jx[e, :D] = jx.reshape(3, 3)[:D]; Jp[e, :D] = jp.reshape(3, 6)[:D]
    is2 = a["edge_inv_sigma2"].astype(LD)
    errL = err.astype(LD)
    chi2e = is2 * np.sum(errL * errL, 1)
    st = a["edge_stereo"] == 1
    # thHuberMono = sqrt(5.991) etc. are floats handed to setDelta(double); delta^2 is their double product (Optimizer.cc:4893-4896)
    dm = float(np.sqrt(np.float32(5.991))); ds = float(np.sqrt(np.float32(7.815)))
    delta = np.where(st, LD(ds), LD(dm)); d2 = np.where(st, LD(ds * ds), LD(dm * dm))
    w = _huber_weight(chi2e, delta, d2) * is2
    chi2 = np.sum(_huber_rho(chi2e, delta, d2))
    di = float(np.sqrt(16.92)); di2 = di * di
    nonvis = []
    Jrw = np.concatenate([-np.eye(3), np.eye(3)], 1)
    for m in range(M):
        k1, k2 = int(a["in_kf1"][m]), int(a["in_kf2"][m])
        er, J = ib.edge_inertial(kf[k1], kf[k2], a["in_preint"][m])
        o1 = off[blk[k1]] if blk[k1] >= 0 else None; o2 = off[blk[k2]] if blk[k2] >= 0 else None
        c1 = (lambda s, c: np.full(c, -1) if o1 is None else o1 + s + np.arange(c))
        c2 = (lambda s, c: np.full(c, -1) if o2 is None else o2 + s + np.arange(c))
        info = a["in_info"][m].reshape(9, 9).astype(LD)
        erL = er.astype(LD)
        c = erL @ info @ erL
        if a["in_robust"][m]:
            wi = _huber_weight(c, LD(di), LD(di2)); chi2 = chi2 + _huber_rho(c, LD(di), LD(di2))
        else:
            wi = LD(1); chi2 = chi2 + c
        nonvis.append((np.concatenate([c1(0, 15), c2(0, 9)]), J, er, wi * info))
        for s, key in ((15, "in_info_g"), (18, "in_info_a")):                        # G2oTypes.h:642-651, :684-687
            rw = (kf[k2, s:s + 3] - kf[k1, s:s + 3]).astype(LD)
            Om = a[key][m].reshape(3, 3).astype(LD)
            chi2 = chi2 + rw @ Om @ rw
            nonvis.append((np.concatenate([c1(s - 6, 3), c2(s - 6, 3)]), Jrw, rw, Om))
    t = solve_tick(dims, L, dict(block=blk[a["edge_kf"]], point=a["edge_point"], Jb=Jp, Jp=Jx, r=err, w=w), nonvis,
                   float(params.lambda_init), 0.0, leave_out)
    t["chi2"] = float(chi2); t["free"] = freek; t["imu"] = imu[freek]; t["n_edges"] = E + 3 * M
    # ImuCamPose::Update (G2oTypes.cc:192-220): twb += Rwb ut, Rwb <- Rwb Exp(ur); velocity and biases add
    s0 = kf[freek].astype(LD)
    R0 = s0[:, :9].reshape(-1, 3, 3)
    x = t["x"]
    o = t["off"][:-1]
    ur = x[o[:, None] + np.arange(3)]; ut = x[o[:, None] + 3 + np.arange(3)]
    rest = np.zeros((len(freek), 9), LD)
    for i in np.flatnonzero(t["imu"]):
        rest[i] = x[o[i] + 6:o[i] + 15]
    Re, _ = so3_exp(ur)
    t["s0"] = s0
    t["R1"] = R0 @ Re
    t["t1"] = s0[:, 9:12] + np.einsum("hab,hb->ha", R0, ut)
    t["rest1"] = s0[:, 12:21] + rest
    t["X0"] = X.astype(LD)
    t["X1"] = t["X0"] + np.where(t["active"][:, None], t["xl"], LD(0))
    return t


def inertial_errors(t, kf, points):
    freek, act, imu = t["free"], t["active"], t["imu"]
    c = np.asarray(kf, LD)[freek]
    R1c = c[:, :9].reshape(-1, 3, 3); t1c = c[:, 9:12]; rest = c[:, 12:21]
    X1c = np.asarray(points, LD)
    norm = _mx(t["x"], t["xl"][act])
    e = _mx(R1c - t["R1"], t1c - t["t1"], (rest - t["rest1"])[imu], (X1c - t["X1"])[act]) / norm
    floor = EPS64 * _mx(t["t1"], t["rest1"][imu], t["X1"][act], np.ones(1)) / norm
    R0 = t["s0"][:, :9].reshape(-1, 3, 3)
    ur = so3_log(np.swapaxes(R0, 1, 2) @ R1c)
    ut = np.einsum("hba,hb->ha", R0, t1c - t["s0"][:, 9:12])
    dxc = np.zeros(t["n"], LD)
    o = t["off"][:-1]
    for i in range(len(freek)):
        dxc[o[i]:o[i] + 3] = ur[i]; dxc[o[i] + 3:o[i] + 6] = ut[i]
        if imu[i]:
            dxc[o[i] + 6:o[i] + 15] = rest[i] - t["s0"][i, 12:21]
    return dict(e=float(e), floor=float(floor), backward=backward_error(t, dxc, X1c - t["X0"]), norm=float(norm))


def report(name, kernels, dev, orc, t):
    """One line per graph: kernels taken, e_device, e_oracle, ratio, both backward errors, the bound's ingredients."""
    ratio = dev["e"] / (orc["e"] + orc["floor"])
    print("[ba-step] %-34s %-58s n %4d e_dev %.3g e_orc %.3g floor %.3g ratio %.3g bwd dev %.3g orc %.3g (n eps %.3g) growth %.3g max|L| %.3g"
          % (name, kernels, t["n"], dev["e"], orc["e"], orc["floor"], ratio, dev["backward"], orc["backward"], t["order"] * float(EPS64),
             t["growth"], t["max_L"]))
    return ratio
