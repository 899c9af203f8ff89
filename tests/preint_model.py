"""IMU preintegration restated in numpy from the reference's text (src/ImuTypes.cc:30-36 NormalizeRotation, :153-178
IntegratedRotation, :225-244 Initialize, :255-310 IntegrateNewMeasurement), over a dtype: float32 (with the SVD NormalizeRotation, what
the reference computes up to OpenCV's double accumulation inside gemm) and longdouble (the yardstick).  It keeps the reference's own
shape -- a dense 9 x 9 A, a 9 x 6 B, whole-matrix products -- and shares nothing with csrc/preint_core.h, which cuts the same recursion
into 9-vector products.  Batched over chains only to be quick: every chain runs the same statements, a chain that has ended keeps
its state.

Also the edge information the inertial optimisers take from the covariance (optc::inertial_information and inv3_block,
host/Optimizer_LocalInertialBA.cc:57-88) over a dtype: float64 (what the C++ computes) and longdouble."""
import numpy as np

LD = np.longdouble
F32 = np.float32
EPS = np.float32(1e-4)
FIELDS = ("dT", "dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "avgA", "avgW", "C")


def skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    S[..., 0, 1] = -v[..., 2]; S[..., 0, 2] = v[..., 1]; S[..., 1, 0] = v[..., 2]
    S[..., 1, 2] = -v[..., 0]; S[..., 2, 0] = -v[..., 1]; S[..., 2, 1] = v[..., 0]
    return S


def normalize_rotation(R):
    """U V^T of the SVD; in longdouble (LAPACK has none) the same matrix as the limit of R <- (R + R^-T) / 2 from the float64 U V^T."""
    if R.dtype == LD:
        U, _, Vt = np.linalg.svd(R.astype(np.float64))
        X = (U @ Vt).astype(LD)
        # the polar factor of R: Newton on R itself, started close (the float64 answer is within 1e-15 of it)
        Y = R.copy()
        for _ in range(6):
            Y = (Y + np.swapaxes(_inv3(Y), -1, -2)) / 2
        assert np.max(np.abs(X - Y)) < 1e-6
        return Y
    U, _, Vt = np.linalg.svd(R)
    return (U @ Vt).astype(R.dtype)


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


def integrated_rotation(accW, dt):
    """deltaR, rightJ of IntegratedRotation(angVel, bias, dt), [B,3,3] each; accW = angVel - bias."""
    T = accW.dtype.type
    v = accW * dt[:, None]
    d2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    d = np.sqrt(d2)
    W = skew(v)
    I = np.broadcast_to(np.eye(3, dtype=accW.dtype), W.shape)
    small = d < T(EPS)
    with np.errstate(all="ignore"):
        s, c = np.sin(d), np.cos(d)
        a = (s / d)[:, None, None]; b = ((T(1) - c) / d2)[:, None, None]; e = ((d - s) / (d2 * d))[:, None, None]
        WW = W @ W
        dR_big = I + W * a + WW * b
        rJ_big = I - W * b + WW * e
    sm = small[:, None, None]
    return np.where(sm, I + W, dR_big).astype(accW.dtype), np.where(sm, I, rJ_big).astype(accW.dtype)


def initialize(B, dtype):
    z3 = lambda: np.zeros((B, 3), dtype)
    z33 = lambda: np.zeros((B, 3, 3), dtype)
    return {"dT": np.zeros(B, dtype), "dR": np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)).copy(), "dV": z3(), "dP": z3(),
            "JRg": z33(), "JVg": z33(), "JVa": z33(), "JPg": z33(), "JPa": z33(), "avgA": z3(), "avgW": z3(),
            "C": np.zeros((B, 15, 15), dtype)}


def integrate(bias, meas, nga, walk, dtype, start=None, exact_bias=False):
    """bias [B][6] (bg, ba), meas: list of B arrays [len][7] float32, nga / walk [6][6] -> dict of the fields, each with a leading B.
    start: a dict as returned (the chains continue from it) or None (Initialize).  exact_bias: the bias is taken as given, not rounded
    to float32 first (the finite differences of test_preint_model.py shift it by less than a float32 step)."""
    B = len(meas)
    lens = np.array([len(m) for m in meas])
    L = int(lens.max()) if B else 0
    M = np.zeros((B, max(L, 1), 7), dtype)
    for c, m in enumerate(meas):
        if len(m):
            M[c, :len(m)] = np.asarray(m, F32).astype(dtype)
    bias = np.asarray(bias, dtype) if exact_bias else np.asarray(bias, F32).astype(dtype)
    bg, ba = bias[:, :3], bias[:, 3:]
    nga = np.asarray(nga, F32).astype(dtype); walk = np.asarray(walk, F32).astype(dtype)
    S = initialize(B, dtype) if start is None else {k: np.array(start[k], dtype) for k in FIELDS}
    I3 = np.eye(3, dtype=dtype)
    half = dtype(0.5)
    for k in range(L):
        act = lens > k
        acc = M[:, k, 0:3] - ba
        accW = M[:, k, 3:6] - bg
        dt = M[:, k, 6]
        dt1, dt2 = dt[:, None], dt[:, None, None]
        dT, dR, dV, dP = S["dT"], S["dR"], S["dV"], S["dP"]
        N = {}
        Racc = (dR @ acc[:, :, None])[:, :, 0]
        with np.errstate(all="ignore"):
            N["avgA"] = (dT[:, None] * S["avgA"] + Racc * dt1) / (dT + dt)[:, None]
            N["avgW"] = (dT[:, None] * S["avgW"] + accW * dt1) / (dT + dt)[:, None]
        N["dP"] = dP + dV * dt1 + half * Racc * dt1 * dt1
        N["dV"] = dV + Racc * dt1
        A = np.broadcast_to(np.eye(9, dtype=dtype), (B, 9, 9)).copy()
        Bm = np.zeros((B, 9, 6), dtype)
        Wacc = skew(acc)
        A[:, 3:6, 0:3] = -(dR * dt2) @ Wacc
        A[:, 6:9, 0:3] = -(half * dR * dt2 * dt2) @ Wacc
        A[:, 6:9, 3:6] = I3 * dt2
        Bm[:, 3:6, 3:6] = dR * dt2
        Bm[:, 6:9, 3:6] = half * dR * dt2 * dt2
        N["JPa"] = S["JPa"] + S["JVa"] * dt2 - half * dR * dt2 * dt2
        N["JPg"] = S["JPg"] + S["JVg"] * dt2 - (half * dR * dt2 * dt2) @ Wacc @ S["JRg"]
        N["JVa"] = S["JVa"] - dR * dt2
        N["JVg"] = S["JVg"] - (dR * dt2) @ Wacc @ S["JRg"]
        deltaR, rightJ = integrated_rotation(accW, dt)
        N["dR"] = normalize_rotation(dR @ deltaR)
        A[:, 0:3, 0:3] = np.swapaxes(deltaR, 1, 2)
        Bm[:, 0:3, 0:3] = rightJ * dt2
        C = S["C"].copy()
        C[:, 0:9, 0:9] = A @ C[:, 0:9, 0:9] @ np.swapaxes(A, 1, 2) + Bm @ nga @ np.swapaxes(Bm, 1, 2)
        C[:, 9:15, 9:15] = C[:, 9:15, 9:15] + walk
        N["C"] = C
        N["JRg"] = np.swapaxes(deltaR, 1, 2) @ S["JRg"] - rightJ * dt2
        N["dT"] = dT + dt
        for key in FIELDS:
            v = N[key].astype(dtype)
            S[key] = np.where(act.reshape((B,) + (1,) * (v.ndim - 1)), v, S[key])
    return S


def concat(m1, m2):
    return [np.concatenate([np.asarray(a, F32).reshape(-1, 7), np.asarray(b, F32).reshape(-1, 7)]) for a, b in zip(m1, m2)]


# --------------------------------------------------------------------------------------------------------------- field groups
def groups(S):
    """The field groups the K rule is applied to, name -> array with a leading B: the vectors and Jacobians, each 3 x 3 block of
    C(0:9, 0:9), the walk block."""
    g = {k: np.asarray(S[k]) for k in FIELDS if k != "C"}
    C = np.asarray(S["C"])
    for i, a in enumerate("rvp"):
        for j, b in enumerate("rvp"):
            g["C_" + a + b] = C[:, 3 * i:3 * i + 3, 3 * j:3 * j + 3]
    g["C_walk"] = C[:, 9:15, 9:15]
    g["C_cross"] = np.concatenate([C[:, 0:9, 9:15].reshape(len(C), -1), C[:, 9:15, 0:9].reshape(len(C), -1)], axis=1)
    return g


def record_fields(rec, cov, avg):
    """The device's arrays (record [B][67] doubles, cov [B][225] or [B][15][15] float, avg [B][6]) as the dict integrate() returns."""
    rec = np.asarray(rec); B = len(rec)
    m = lambda o: rec[:, o:o + 9].reshape(B, 3, 3)
    return {"dT": rec[:, 0], "dR": m(1), "dV": rec[:, 10:13], "dP": rec[:, 13:16], "JRg": m(16), "JVg": m(25), "JVa": m(34), "JPg": m(43),
            "JPa": m(52), "avgA": np.asarray(avg)[:, 0:3], "avgW": np.asarray(avg)[:, 3:6], "C": np.asarray(cov).reshape(B, 15, 15)}


# --------------------------------------------------------------------------------------------------------------- information
def jacobi_eig(A, dtype):
    """Cyclic Jacobi as host/Optimizer_LocalInertialBA.cc:33-52 runs it -> (w, V), A = V diag(w) V^T."""
    A = np.array(A, dtype); n = len(A)
    V = np.eye(n, dtype=dtype)
    one = dtype(1)
    for _ in range(64):
        off = sum(A[i, j] * A[i, j] for i in range(n) for j in range(i + 1, n))
        if off < 1e-300:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                with np.errstate(over="ignore"):           # a tiny A[p, q]: theta^2 overflows to inf and t becomes 0, as in the C++
                    theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
                    t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one); s = t * c
                a, b = A[:, p].copy(), A[:, q].copy(); A[:, p] = c * a - s * b; A[:, q] = s * a + c * b
                a, b = A[p, :].copy(), A[q, :].copy(); A[p, :] = c * a - s * b; A[q, :] = s * a + c * b
                a, b = V[:, p].copy(), V[:, q].copy(); V[:, p] = c * a - s * b; V[:, q] = s * a + c * b
    return np.diag(A).copy(), V


def information(C, dtype):
    """C: one 15 x 15 float covariance -> (info [9][9], info_g [3][3], info_a [3][3], eigenvalues [9]) in dtype."""
    C = np.asarray(C, F32).astype(dtype)
    A = (C[:9, :9] + C[:9, :9].T) * dtype(0.5)
    w, V = jacobi_eig(A, dtype)
    wmax = np.max(np.abs(w))
    inv = np.zeros(9, dtype)
    for i in range(9):
        x = dtype(1) / w[i] if w[i] > wmax * dtype(1e-7) * 9 else dtype(0)
        inv[i] = dtype(0) if x < 1e-12 else x
    info = (V * inv[None, :]) @ V.T
    with np.errstate(all="ignore"):
        ig = _inv3(C[9:12, 9:12]).astype(F32).astype(dtype)
        ia = _inv3(C[12:15, 12:15]).astype(F32).astype(dtype)
    return info, ig, ia, w
