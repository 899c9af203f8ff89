"""Models of the shared geometry primitives that orbhip.debug_geom_probe runs alone on the device.  TEST INFRASTRUCTURE ONLY: it imports
nothing from the kernels' side.

Every op has a FAITHFUL model: the reference's formula with its branches and thresholds (Eigen's quaternion functions, g2o's SE3Quat,
Sim3 and RobustKernelHuber, src/G2oTypes.cc ExpSO3 / LogSO3 / RightJacobianSO3 / InverseRightJacobianSO3, src/ImuTypes.cc
NormalizeRotation, Pinhole / KannalaBrandt8 project / projectJac), stated ONCE over an arithmetic namespace and evaluated twice on the
exact double inputs: at 50 digits in mpmath (the expected output) and in numpy float64 (the yardstick).  The float64 run is checked
against what essential_graph_model.py, sim3_opt_model.py, pose_inertial_model.py and new_points_model.py already state
(tests/test_geom_probe_model.py::test_other_models_agree): one formula cannot be evaluated by numpy ufuncs and by mpmath from the same
vectorised text, so the text here is scalar, and the older models are its second statement instead of being re-typed.  The reference's
quirks are part of the model: R = I + Omega + Omega^2 in the small-angle branches of Sim3 and SE3Quat, the unscaled return of LogSO3
when |sin theta| < 1e-5 or the cosine is out of range, the NaN of the KB8 projectJac on the optical axis, 1 / (d sin d) of the inverse
right Jacobian.  IMU::NormalizeRotation is the exception the header documents: the reference takes U V^T of an SVD, the library two
Newton steps of the polar iteration; the faithful model states the two steps (so3_normalize), the truth is the polar factor.

The float ops (tri_project, tri_unproject, tri_svd4_null) have op-by-op float32 models, compared bit for bit.

The TRUTH, independent of any closed form (50 digits): mp.expm of the generator for the exponentials, round trips for the logarithms,
mp.diff of the un-rounded projection for the camera Jacobians, the polar factor for so3_normalize, mp.svd_r for the null vector.

Every faithful function returns (output, branch): `branch` names the path taken and `margins` collects the relative distance of every
branch argument to its threshold (0 for an exact tie)."""
import math

import mpmath
import numpy as np
from mpmath import mp

import new_points_model as npm

mp.dps = 50
f32, f64 = np.float32, np.float64
EPS = 0.00001
PI = math.pi


class _N64:
    """numpy float64 scalars: IEEE division by zero, NaN from an out-of-range acos"""
    name = "f64"
    num = staticmethod(f64)
    sqrt, sin, cos, acos, exp, log, atan2 = (staticmethod(f) for f in (np.sqrt, np.sin, np.cos, np.arccos, np.exp, np.log, np.arctan2))
    fabs = staticmethod(abs)
    r32 = staticmethod(lambda x: f64(f32(x)))                      # (double)(float)x
    sqrtf = staticmethod(lambda x: f64(np.sqrt(f32(x))))           # (double)sqrtf((float)x)

    @staticmethod
    def div(a, b):
        return f64(a) / f64(b)


class _NMP:
    name = "mp"
    num = staticmethod(mp.mpf)
    sqrt, sin, cos, acos, exp, log, atan2 = (staticmethod(f) for f in (mp.sqrt, mp.sin, mp.cos, mp.acos, mp.exp, mp.log, mp.atan2))
    fabs = staticmethod(abs)
    r32 = staticmethod(lambda x: mp.mpf(float(f32(float(x)))))
    sqrtf = staticmethod(lambda x: mp.mpf(float(np.sqrt(f32(float(x))))))

    @staticmethod
    def div(a, b):
        if b == 0:
            return mp.nan if (a == 0 or mp.isnan(a)) else (mp.inf if a > 0 else -mp.inf)
        return a / b


N64, NMP = _N64, _NMP


def _rel(x, thr):
    """relative distance of a branch argument to its threshold"""
    x, thr = float(x), float(thr)
    return abs(x - thr) / max(abs(thr), 1e-300) if thr != 0 else abs(x)


# ------------------------------------------------------------------------------------------------ quaternions, Eigen
def quat_to_R(N, q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], "-"


def R_to_quat(N, R, margins=None):
    """Eigen::Quaterniond(Matrix3d): branch 'trace', else 'i0' / 'i1' / 'i2' by the largest diagonal element (the first on a tie)"""
    t = R[0] + R[4] + R[8]
    half = N.num(0.5)
    q = [None] * 4
    if margins is not None:
        margins.append(("trace", abs(float(t))))
    if t > 0:
        t = N.sqrt(t + 1)
        q[3] = half * t
        t = half / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
        return q, "trace"
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    if margins is not None:
        margins.append(("diag01", _rel(R[4], R[0])))
        margins.append(("diag2", _rel(R[8], R[4 * i] if i < 2 else max(R[0], R[4]))))
    j, k = (i + 1) % 3, (i + 2) % 3
    t = N.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1)
    q[i] = half * t
    t = half / t
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q, "i%d" % i


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rot(N, q, v):
    u = _cross(q[:3], v)
    u = [c + c for c in u]
    c2 = _cross(q[:3], u)
    return [v[i] + q[3] * u[i] + c2[i] for i in range(3)], "-"


def quat_mul(N, a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], "-"


def quat_norm_rot(N, q):
    """SE3Quat::normalizeRotation"""
    br = "flip" if q[3] < 0 else ("w0" if q[3] == 0 else "keep")
    if q[3] < 0:
        q = [-c for c in q]
    n = N.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q], br


def huber(N, e, delta, dsqr):
    """RobustKernelHuber::robustify: rho, rho'"""
    if e <= dsqr:
        return [e, N.num(1)], ("at" if e == dsqr else "below")
    s = N.sqrt(e)
    return [2 * s * delta - dsqr, delta / s], "above"


# ------------------------------------------------------------------------------------------------ 3x3 helpers
def _skew(N, w):
    z = N.num(0)
    return [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]


def _mm(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _mv(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def _eye(N):
    return [N.num(1.0 if i % 4 == 0 else 0.0) for i in range(9)]


def _rodrigues(N, w, a, b):
    W = _skew(N, w)
    W2 = _mm(W, W)
    I = _eye(N)
    return [I[i] + a * W[i] + b * W2[i] for i in range(9)]


def _inv3(N, A):
    c0, c1, c2 = A[4] * A[8] - A[5] * A[7], A[5] * A[6] - A[3] * A[8], A[3] * A[7] - A[4] * A[6]
    idet = 1 / (A[0] * c0 + A[1] * c1 + A[2] * c2)
    return [c0 * idet, (A[2] * A[7] - A[1] * A[8]) * idet, (A[1] * A[5] - A[2] * A[4]) * idet,
            c1 * idet, (A[0] * A[8] - A[2] * A[6]) * idet, (A[2] * A[3] - A[0] * A[5]) * idet,
            c2 * idet, (A[1] * A[6] - A[0] * A[7]) * idet, (A[0] * A[4] - A[1] * A[3]) * idet]


# ------------------------------------------------------------------------------------------------ SO(3), G2oTypes.cc / ImuTypes.cc
def so3_normalize(N, R, steps=2):
    """the library's stand-in for U V^T: `steps` Newton steps R <- (R + R^-T) / 2"""
    R = list(R)
    half = N.num(0.5)
    for _ in range(steps):
        I = _inv3(N, R)
        R = [half * (R[3 * i + j] + I[3 * j + i]) for i in range(3) for j in range(3)]
    return R, "-"


def so3_exp(N, w, eps=1e-5, normalize=True, margins=None):
    d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    d = N.sqrt(d2)
    if margins is not None:
        margins.append(("d", _rel(d, eps)))
    if d < eps:
        R, br = _rodrigues(N, w, N.num(1), N.num(0.5)), "small"
    else:
        R, br = _rodrigues(N, w, N.sin(d) / d, (1 - N.cos(d)) / d2), "large"
    if normalize:
        R = so3_normalize(N, R)[0]
    return R, br


def so3_exp_imu(N, w, margins=None):
    return so3_exp(N, w, 1e-4, False, margins)


def so3_log(N, R, margins=None):
    tr = R[0] + R[4] + R[8]
    w = [(R[7] - R[5]) / 2, (R[2] - R[6]) / 2, (R[3] - R[1]) / 2]
    c = (tr - 1) * N.num(0.5)
    if margins is not None:                     # an exact +-1 is intended; otherwise at least an ulp outside or well inside
        margins.append(("cos", 0.0 if abs(float(c)) == 1.0 else 1.0))
    if c > 1 or c < -1:
        return w, "out_of_range"
    theta = N.acos(c)
    s = N.sin(theta)
    if margins is not None:
        margins.append(("sin", _rel(abs(s), 1e-5)))
    if N.fabs(s) < 1e-5:
        return w, "unscaled"
    return [theta * x / s for x in w], "scaled"


def so3_inv_right_jac(N, v, margins=None):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = N.sqrt(d2)
    if margins is not None:
        margins.append(("d", _rel(d, 1e-5)))
    if d < 1e-5:
        return _eye(N), "small"
    return _rodrigues(N, v, N.num(0.5), 1 / d2 - N.div(1 + N.cos(d), 2 * d * N.sin(d))), "large"


def so3_right_jac(N, v, margins=None):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = N.sqrt(d2)
    if margins is not None:
        margins.append(("d", _rel(d, 1e-5)))
    if d < 1e-5:
        return _eye(N), "small"
    return _rodrigues(N, v, -(1 - N.cos(d)) / d2, (d - N.sin(d)) / (d2 * d)), "large"


# ------------------------------------------------------------------------------------------------ SE3Quat
def se3_oplus(N, u, pose, margins=None):
    """VertexSE3Expmap::oplusImpl: SE3Quat::exp(u) * pose"""
    theta = N.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    O = _skew(N, u[:3])
    O2 = _mm(O, O)
    I = _eye(N)
    if margins is not None:
        margins.append(("theta", _rel(theta, EPS)))
    if theta < EPS:
        R = [I[i] + O[i] + O2[i] for i in range(9)]
        V, br = R, "small"
    else:
        sn, cs = N.sin(theta), N.cos(theta)
        a, b, c = sn / theta, (1 - cs) / (theta * theta), (theta - sn) / (theta * theta * theta)
        R = [I[i] + a * O[i] + b * O2[i] for i in range(9)]
        V, br = [I[i] + b * O[i] + c * O2[i] for i in range(9)], "large"
    qe, b2 = R_to_quat(N, R)
    te = _mv(V, u[3:6])
    qe = quat_norm_rot(N, qe)[0]
    rt = quat_rot(N, qe, pose[4:7])[0]
    qn = quat_norm_rot(N, quat_mul(N, qe, pose[:4])[0])[0]
    return qn + [te[i] + rt[i] for i in range(3)], br + "/" + b2


def se3_mul(N, a, b):
    rt = quat_rot(N, a[:4], b[4:7])[0]
    q = quat_norm_rot(N, quat_mul(N, a[:4], b[:4])[0])[0]
    return q + [a[4 + i] + rt[i] for i in range(3)], "-"


# ------------------------------------------------------------------------------------------------ g2o::Sim3
def _s3_abc(N, sigma, theta, s, small_sigma, small_theta):
    if small_sigma:
        C = N.num(1)
        if small_theta:
            return N.num(1) / 2, N.num(1) / 6, C
        th2 = theta * theta
        return (1 - N.cos(theta)) / th2, (theta - N.sin(theta)) / (th2 * theta), C
    C = (s - 1) / sigma
    if small_theta:
        sg2 = sigma * sigma
        return ((sigma - 1) * s + 1) / sg2, ((N.num(0.5) * sg2 - sigma + 1) * s) / (sg2 * sigma), C
    a, b, th2 = s * N.sin(theta), s * N.cos(theta), theta * theta
    c = th2 + sigma * sigma
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) * 1 / th2, C


def s3_exp(N, u, margins=None):
    sigma = u[6]
    theta = N.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    O = _skew(N, u[:3])
    O2 = _mm(O, O)
    s = N.exp(sigma)
    ss, st = bool(N.fabs(sigma) < EPS), bool(theta < EPS)
    if margins is not None:
        margins.append(("sigma", _rel(abs(sigma), EPS)))
        margins.append(("theta", _rel(theta, EPS)))
    A, B, C = _s3_abc(N, sigma, theta, s, ss, st)
    ra = rb = N.num(1)
    if not st:
        ra, rb = N.sin(theta) / theta, (1 - N.cos(theta)) / (theta * theta)
    I = _eye(N)
    R = [I[i] + ra * O[i] + rb * O2[i] for i in range(9)]
    q, b2 = R_to_quat(N, R)
    W = [A * O[i] + B * O2[i] + C * I[i] for i in range(9)]
    return q + _mv(W, u[3:6]) + [s], ("ss" if ss else "sl") + ("ts" if st else "tl") + "/" + b2


def _lu_solve3(N, W, t, margins=None):
    """Eigen's PartialPivLU of a 3x3: the first row of largest magnitude in the column.  Branch: column-0 and column-1 exchange"""
    M = [[W[3 * i], W[3 * i + 1], W[3 * i + 2], t[i]] for i in range(3)]
    a = [abs(M[i][0]) for i in range(3)]
    p = 0
    for i in (1, 2):
        if a[i] > a[p]:
            p = i
    if margins is not None:
        margins.append(("pivot0", min(_rel(a[i], a[p]) for i in range(3) if i != p)))          # 0.0: an exact tie, the first row wins
    M[0], M[p] = M[p], M[0]
    for r in (1, 2):
        l = M[r][0] / M[0][0]
        for j in (1, 2, 3):
            M[r][j] = M[r][j] - l * M[0][j]
    p1 = 2 if abs(M[2][1]) > abs(M[1][1]) else 1
    if margins is not None:
        margins.append(("pivot1", _rel(abs(M[2][1]), abs(M[1][1])) if abs(M[2][1]) != abs(M[1][1]) else 0.0))
    M[1], M[p1] = M[p1], M[1]
    l = M[2][1] / M[1][1]
    M[2][2] = M[2][2] - l * M[1][2]
    M[2][3] = M[2][3] - l * M[1][3]
    x2 = M[2][3] / M[2][2]
    x1 = (M[1][3] - M[1][2] * x2) / M[1][1]
    x0 = (M[0][3] - M[0][1] * x1 - M[0][2] * x2) / M[0][0]
    return [x0, x1, x2], "p%d%d" % (p, p1)


def s3_log(N, S, margins=None):
    s = S[7]
    sigma = N.log(s)
    R = quat_to_R(N, S[:4])[0]
    d = N.num(0.5) * (R[0] + R[4] + R[8] - 1)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    ss, st = bool(N.fabs(sigma) < EPS), bool(d > 1 - EPS)
    if margins is not None:
        margins.append(("sigma", _rel(abs(sigma), EPS)))
        margins.append(("d", _rel(d, 1 - EPS)))
    if st:
        theta, f = N.num(0), N.num(0.5)
    else:
        theta = N.acos(d)
        f = theta / (2 * N.sqrt(1 - d * d))
    om = [f * x for x in dR]
    A, B, C = _s3_abc(N, sigma, theta, s, ss, st)
    O = _skew(N, om)
    O2 = _mm(O, O)
    I = _eye(N)
    W = [A * O[i] + B * O2[i] + C * I[i] for i in range(9)]
    ups, piv = _lu_solve3(N, W, S[4:7], margins)
    return om + ups + [sigma], ("ss" if ss else "sl") + ("ts" if st else "tl") + "/" + piv


def s3_mul(N, a, b):
    rt = quat_rot(N, a[:4], b[4:7])[0]
    return quat_mul(N, a[:4], b[:4])[0] + [a[7] * rt[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]], "-"


def s3_inverse(N, a):
    q = [-a[0], -a[1], -a[2], a[3]]
    m = -1 / a[7]
    return q + quat_rot(N, q, [m * a[4], m * a[5], m * a[6]])[0] + [1 / a[7]], "-"


def s3_map(N, S, X):
    r = quat_rot(N, S[:4], X)[0]
    return [S[7] * r[i] + S[4 + i] for i in range(3)], "-"


# ------------------------------------------------------------------------------------------------ GeometricCamera in double
def cam_project(N, c):
    """(fx fy cx cy model k0..k3 P): Pinhole.cpp:41-47, KannalaBrandt8.cpp:52-69 (float atan2f results, then double)"""
    fx, fy, cx, cy, model = c[0], c[1], c[2], c[3], int(c[4])
    k, P = c[5:9], c[9:12]
    if model == 1:
        x2y2 = P[0] * P[0] + P[1] * P[1]
        theta = N.r32(N.atan2(N.sqrtf(x2y2), N.r32(P[2])))
        psi = N.r32(N.atan2(N.r32(P[1]), N.r32(P[0])))
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9
        return [fx * r * N.cos(psi) + cx, fy * r * N.sin(psi) + cy], "kb8"
    return [N.div(fx * P[0], P[2]) + cx, N.div(fy * P[1], P[2]) + cy], "pinhole"


def _kb8_f_fd(N, k, theta):
    t2 = theta * theta
    t3, t4 = t2 * theta, t2 * t2
    t5, t6 = t4 * theta, t2 * t4
    t7, t8 = t6 * theta, t4 * t4
    t9 = t8 * theta
    return (theta + t3 * k[0] + t5 * k[1] + t7 * k[2] + t9 * k[3],
            1 + 3 * k[0] * t2 + 5 * k[1] * t4 + 7 * k[2] * t6 + 9 * k[3] * t8)


def cam_project_jac(N, c):
    """Pinhole.cpp:81-91, KannalaBrandt8.cpp:166-195: 0 / 0 on the optical axis, kept"""
    fx, fy, model = c[0], c[1], int(c[4])
    k, (x, y, z) = c[5:9], c[9:12]
    if model == 1:
        x2, y2, z2 = x * x, y * y, z * z
        r2 = x2 + y2
        r = N.sqrt(r2)
        r3 = r2 * r
        f, fd = _kb8_f_fd(N, k, N.atan2(r, z))
        D = r2 * (r2 + z2)
        return [fx * (N.div(fd * z * x2, D) + N.div(f * y2, r3)), fx * (N.div(fd * z * y * x, D) - N.div(f * y * x, r3)), N.div(-fx * fd * x, r2 + z2),
                fy * (N.div(fd * z * y * x, D) - N.div(f * y * x, r3)), fy * (N.div(fd * z * y2, D) + N.div(f * x2, r3)), N.div(-fy * fd * y, r2 + z2)], "kb8"
    zero = N.num(0)
    return [fx / z, zero, -fx * x / (z * z), zero, fy / z, -fy * y / (z * z)], "pinhole"


def cam_project_smooth(c):
    """the projection without its float roundings, at 50 digits: what mp.diff differentiates"""
    fx, fy, cx, cy, model = c[0], c[1], c[2], c[3], int(c[4])
    k = c[5:9]

    def f(x, y, z):
        if model == 1:
            r = mp.sqrt(x * x + y * y)
            fr = _kb8_f_fd(NMP, k, mp.atan2(r, z))[0]
            return [fx * fr * x / r + cx, fy * fr * y / r + cy]
        return [fx * x / z + cx, fy * y / z + cy]
    return f


# ------------------------------------------------------------------------------------------------ float ops, op by op (bit for bit)
def tri_project(ctype, p, P):
    """GeometricCamera::project(cv::Point3f) in float: Pinhole.cpp:34-37, KannalaBrandt8.cpp:28-45"""
    p, P = [f32(v) for v in p], [f32(v) for v in P]
    with np.errstate(all="ignore"):
        if ctype == 0:
            return np.array([p[0] * P[0] / P[2] + p[2], p[1] * P[1] / P[2] + p[3]], f32)
        x2y2 = P[0] * P[0] + P[1] * P[1]
        theta = npm.atan2f(np.sqrt(x2y2), P[2])
        psi = npm.atan2f(P[1], P[0])
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + p[4] * t3 + p[5] * t5 + p[6] * t7 + p[7] * t9
        s, c = npm.sincos_signed(f64(psi))
        return np.array([p[0] * r * f32(c) + p[2], p[1] * r * f32(s) + p[3]], f32)


def tri_unproject(ctype, p, u, v, info=None):
    """GeometricCamera::unproject in float: Pinhole.cpp:57-60, KannalaBrandt8.cpp:103-130; info: {'branch', 'steps'}"""
    p, u, v = [f32(x) for x in p], f32(u), f32(v)
    one = f32(1)
    with np.errstate(all="ignore"):
        pwx, pwy = (u - p[2]) / p[0], (v - p[3]) / p[1]
        if ctype == 0:
            return np.array([pwx, pwy, one], f32)
        scale = one
        theta_d = np.sqrt(pwx * pwx + pwy * pwy)
        lim = f32(PI / 2)
        clamped = bool(theta_d > lim)
        theta_d = min(max(-lim, theta_d), lim)
        steps = 0
        if f64(theta_d) > 1e-8:
            theta = theta_d
            for _ in range(10):
                steps += 1
                t2 = theta * theta
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t4 * t4
                k0, k1, k2, k3 = p[4] * t2, p[5] * t4, p[6] * t6, p[7] * t8
                fix = (theta * (one + k0 + k1 + k2 + k3) - theta_d) / (one + f32(3) * k0 + f32(5) * k1 + f32(7) * k2 + f32(9) * k3)
                theta = theta - fix
                if abs(fix) < f32(1e-6):
                    break
            s, c = npm.sincos_signed(f64(theta))
            scale = f32(s / c) / theta_d
        if info is not None:
            info["branch"] = ("tiny" if steps == 0 else "newton") + ("/clamped" if clamped else "")
            info["steps"] = steps
        return np.array([pwx * scale, pwy * scale, one], f32)


def tri_svd4_null(At):
    """At [4][4], At[i] = column i of A"""
    return npm.jacobi_null4(np.asarray(At, f32).reshape(4, 4).T)


def atan2f_boundary_distance(y, x):
    """relative distance of the 50-digit atan2 of two floats to the nearest float32 rounding boundary"""
    t = mp.atan2(mp.mpf(float(f32(y))), mp.mpf(float(f32(x))))
    if t == 0:
        return 1.0
    r = f32(float(t))
    lo, hi = np.nextafter(r, f32(-np.inf)), np.nextafter(r, f32(np.inf))
    return float(min(abs(t - (mp.mpf(float(r)) + mp.mpf(float(lo))) / 2), abs(t - (mp.mpf(float(r)) + mp.mpf(float(hi))) / 2)) / abs(t))


# ------------------------------------------------------------------------------------------------ truth, 50 digits
def _M3(R):
    return mp.matrix(3, 3) if R is None else mp.matrix([[mp.mpf(R[3 * i + j]) for j in range(3)] for i in range(3)])


def _flat(M):
    return [M[i, j] for i in range(M.rows) for j in range(M.cols)]


def truth_so3_exp(w):
    return _flat(mp.expm(_M3(_skew(NMP, [mp.mpf(x) for x in w]))))


def _gen4(om, ups, sigma):
    G = mp.zeros(4, 4)
    O = _skew(NMP, [mp.mpf(x) for x in om])
    for i in range(3):
        for j in range(3):
            G[i, j] = O[3 * i + j]
        G[i, i] += mp.mpf(sigma)
        G[i, 3] = mp.mpf(ups[i])
    return G


def _mat4(q, t, s):
    """[[s R(q), t], [0, 1]] with Eigen's toRotationMatrix on q as it stands"""
    R = quat_to_R(NMP, [mp.mpf(x) for x in q])[0]
    M = mp.eye(4)
    for i in range(3):
        for j in range(3):
            M[i, j] = mp.mpf(s) * R[3 * i + j]
        M[i, 3] = mp.mpf(t[i])
    return M


def _top(M):
    return [M[i, j] for i in range(3) for j in range(4)]


def truth_se3_oplus(u, pose):
    """expm(generator(u)) T(pose) as 3 x 4; a result (q, t) is compared as se3_as_matrix(result)"""
    return _top(mp.expm(_gen4(u[:3], u[3:6], 0)) * _mat4(pose[:4], pose[4:7], 1))


def se3_as_matrix(T):
    return _top(_mat4(T[:4], T[4:7], 1))


def truth_s3_exp(u):
    return _top(mp.expm(_gen4(u[:3], u[3:6], u[6])))


def s3_as_matrix(S):
    return _top(_mat4(S[:4], S[4:7], S[7]))


def roundtrip_s3_log(u):
    """expm(generator(u)): compared with s3_as_matrix(S) of the input S of the logarithm that returned u"""
    return truth_s3_exp(u)


def roundtrip_so3_log(w):
    return truth_so3_exp(w)


def truth_polar(R):
    U, S, V = mp.svd_r(_M3(R))
    return _flat(U * V)


def truth_null4(At):
    """unit null vector (up to sign) of A, A's column i = At[i], and the gap sigma_3 / sigma_2"""
    A = mp.matrix([[mp.mpf(float(At[4 * j + i])) for j in range(4)] for i in range(4)])
    U, S, V = mp.svd_r(A)
    k = min(range(4), key=lambda i: S[i])
    return [V[k, j] for j in range(4)], [S[i] for i in range(4)]


def truth_cam_jac(c):
    f = cam_project_smooth([mp.mpf(x) for x in c])
    P = [mp.mpf(x) for x in c[9:12]]
    J = []
    for r in range(2):
        for a in range(3):
            n = tuple(1 if i == a else 0 for i in range(3))
            J.append(mp.diff(lambda x, y, z: f(x, y, z)[r], tuple(P), n))
    return J


# ------------------------------------------------------------------------------------------------ running a model over a case table
FAITHFUL = {
    "quat_to_R": lambda N, a, m: quat_to_R(N, a), "R_to_quat": lambda N, a, m: R_to_quat(N, a, m),
    "quat_rot": lambda N, a, m: quat_rot(N, a[:4], a[4:7]), "quat_mul": lambda N, a, m: quat_mul(N, a[:4], a[4:8]),
    "quat_norm_rot": lambda N, a, m: quat_norm_rot(N, a), "huber": lambda N, a, m: huber(N, a[0], a[1], a[2]),
    "se3_oplus": lambda N, a, m: se3_oplus(N, a[:6], a[6:13], m), "se3_mul": lambda N, a, m: se3_mul(N, a[:7], a[7:14]),
    "so3_exp": lambda N, a, m: so3_exp(N, a, 1e-5, True, m), "so3_exp_imu": lambda N, a, m: so3_exp_imu(N, a, m),
    "so3_log": lambda N, a, m: so3_log(N, a, m), "so3_right_jac": lambda N, a, m: so3_right_jac(N, a, m),
    "so3_inv_right_jac": lambda N, a, m: so3_inv_right_jac(N, a, m), "so3_normalize": lambda N, a, m: so3_normalize(N, a),
    "s3_exp": lambda N, a, m: s3_exp(N, a, m), "s3_log": lambda N, a, m: s3_log(N, a, m),
    "s3_mul": lambda N, a, m: s3_mul(N, a[:8], a[8:16]), "s3_inverse": lambda N, a, m: s3_inverse(N, a),
    "s3_map": lambda N, a, m: s3_map(N, a[:8], a[8:11]), "cam_project": lambda N, a, m: cam_project(N, a),
    "cam_project_jac": lambda N, a, m: cam_project_jac(N, a),
}


def _to_float(v):
    if isinstance(v, mp.mpf):
        return float("nan") if mp.isnan(v) else float(v)
    return float(v)


def run_faithful(op, inputs, want_margins=False):
    """-> expected (list of rows of mpf), f64 rows [n, w] float64, branches (from the 50-digit run), branches64, margins per item"""
    fn = FAITHFUL[op]
    exp, y64, br, br64, mg = [], [], [], [], []
    with np.errstate(all="ignore"):
        for row in np.asarray(inputs, f64):
            m = [] if want_margins else None
            o, b = fn(NMP, [mp.mpf(float(x)) for x in row], m)
            exp.append([mp.mpf(v) for v in o]); br.append(b); mg.append(m)
            o, b = fn(N64, [f64(x) for x in row], None)
            y64.append([float(v) for v in o]); br64.append(b)
    return exp, np.array(y64, f64), br, br64, mg


def errors(cand, expected):
    """per item: max |cand - expected| over the finite entries of expected, the floor 2^-52 max |expected|, and whether the NaN / Inf
    pattern of the candidate equals the expected one"""
    e, fl, same = [], [], []
    for c, x in zip(np.asarray(cand, f64), expected):
        worst, big, ok = mp.mpf(0), mp.mpf(0), True
        for cv, xv in zip(c, x):
            xv = mp.mpf(xv)
            if mp.isnan(xv) or mp.isinf(xv):
                ok = ok and ((mp.isnan(xv) and math.isnan(cv)) or (mp.isinf(xv) and math.isinf(cv) and (cv > 0) == (xv > 0)))
                continue
            if not math.isfinite(cv):
                ok = False
                continue
            worst, big = max(worst, abs(mp.mpf(float(cv)) - xv)), max(big, abs(xv))
        e.append(float(worst)); fl.append(float(big) * 2.0 ** -52); same.append(ok)
    return np.array(e), np.array(fl), np.array(same)


def angle_to(v, n):
    """angle between the lines of v and n"""
    v = [mp.mpf(float(x)) for x in v]
    d = abs(sum(a * b for a, b in zip(v, n))) / (mp.sqrt(sum(a * a for a in v)) * mp.sqrt(sum(b * b for b in n)))
    return float(mp.acos(min(d, mp.mpf(1))))
