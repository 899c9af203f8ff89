"""The per-match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:479-724) as a model, written from the reference
text in plain Python with np.float32 / np.float64 scalars: one operation per expression, every rounding where the C++ types put it.

  new_point(...)      the float model: outcome code + world point of one match -- the yardstick of the device kernel;
  new_point_f64(...)  a straightforward float64 restatement with np.linalg.svd: outcome + the smallest relative distance of any decision
                      quantity to its threshold (the model's own check, and the filter of the crafted matches).

The two camera functions are the oracle's exported orc_camera_project_f / orc_camera_unproject_f; the 4x4 null vector restates
OpenCV 3.4's JacobiSVDImpl_<float> itself.  cv::Mat arithmetic: Mat::dot / cv::norm accumulate in double; `Rwc * xn` and the rows of
`Rcw.row(i).dot(x) + tcw(i)` are sums in double rounded once (the rounding points of KannalaBrandt8::matchAndtriangulate's restatement,
oracle/match_oracle.c); `Twc.R * x3Dc + Twc.t` (no transposed operand) is the small-matrix path: a float sum, then one rounding of
double(t) + double(c) (host/cvmath.h mul_add); `s * row - row` is a float multiply and a float subtract; Mat / scalar multiplies by
the float reciprocal.  cosf / atan2f are the library's fixed sequences (a Cody-Waite reduction with fdlibm kernels in double, double
atan2), both rounded to float.  Parity against an OpenCV build is unpinned.

Outcome codes: 0 no match, 1 triangulated, 2 KF1's stereo depth, 3 KF2's stereo depth, 4 low parallax and no stereo (:622), 5 w == 0
(:605), 6 empty stereo point, 7 z1 <= 0, 8 z2 <= 0, 9 reprojection in KF1, 10 in KF2, 11 a zero distance, 12 far point, 13 scale ratio."""
import math
from fractions import Fraction

import numpy as np

import oracle_match_bind as om

f32, f64 = np.float32, np.float64

PAIR_DTYPE = np.dtype([("cam1", "<f4", (2, 8)), ("cam2", "<f4", (2, 8)), ("cam1_type", "<i4", (2,)), ("cam2_type", "<i4", (2,)),
                       ("nleft1", "<i4"), ("nleft2", "<i4"), ("Tcw1", "<f4", (2, 12)), ("Tcw2", "<f4", (2, 12)), ("Twc1", "<f4", (12,)),
                       ("Twc2", "<f4", (12,)), ("Ow1", "<f4", (2, 3)), ("Ow2", "<f4", (2, 3)), ("mb1", "<f4"), ("mb2", "<f4"), ("mbf", "<f4"),
                       ("ratio_factor", "<f4"), ("far_points", "<i4"), ("th_far_points", "<f4")])

# wrong rules the scenes must tell from the model (tests/test_new_points_model.py)
VARIANTS = ("mbf2", "if_not_else_if", "unproject_un", "ratio_inverted")


def _fma(a, b, c):
    """fma of three doubles, exactly rounded (int / int of a Fraction is correctly rounded)"""
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return f64(r.numerator / r.denominator)


def sincos_signed(x):
    """the library's stand-in for sin / cos (oracle/match_oracle.c sincos_signed, csrc/cam_project_f32.h tri_sincos_signed)"""
    x = f64(x)
    TWO_OVER_PI = f64(6.36619772367581382433e-01)
    PIO2_HI, PIO2_LO = f64(1.57079632679489655800e+00), f64(6.12323399573676603587e-17)
    S = [f64(v) for v in (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
                          -2.50507602534068634195e-08, 1.58969099521155010221e-10)]
    Cc = [f64(v) for v in (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
                           2.08757232129817482790e-09, -1.13596475577881948265e-11)]
    dk = f64(np.rint(x * TWO_OVER_PI))
    k = int(dk)
    r = _fma(-dk, PIO2_HI, x)
    r = _fma(-dk, PIO2_LO, r)
    z = r * r
    ps = _fma(z, S[5], S[4])
    for c in (S[3], S[2], S[1], S[0]):
        ps = _fma(z, ps, c)
    s = _fma(r * z, ps, r)
    pc = _fma(z, Cc[5], Cc[4])
    for c in (Cc[3], Cc[2], Cc[1], Cc[0]):
        pc = _fma(z, pc, c)
    c = _fma(z * z, pc, _fma(z, f64(-0.5), f64(1.0)))
    return ((s, c), (c, -s), (-s, -c), (-c, s))[k & 3]


def atan2f(y, x):
    return f32(math.atan2(float(f32(y)), float(f32(x))))


def cos_stereo(mb, depth):
    """cos(2*atan2(mb/2, mvDepth[idx])) (:583, :585): float operands pick std::atan2(float, float) and std::cos(float)"""
    a = atan2f(f32(mb) / f32(2), depth)
    t = f32(2) * a
    return f32(sincos_signed(f64(t))[1])


def jacobi_null4(A):
    """last row of Vt of cv::SVD::compute(A 4x4 CV_32F, FULL_UV): OpenCV 3.4 lapack.cpp JacobiSVDImpl_<float> restated (one-sided Jacobi on
    the rows of A^T in float, norms and dot products accumulated in double, eps = 2 FLT_EPSILON, at most 30 sweeps, hypot(p, beta) as
    sqrt(p*p + beta*beta), rows sorted by decreasing singular value with the reference's selection sort)"""
    A = np.asarray(A, f32).reshape(4, 4)
    At = [[f32(A[j, i]) for j in range(4)] for i in range(4)]
    Vt = [[f32(1.0 if i == k else 0.0) for k in range(4)] for i in range(4)]
    W = []
    for i in range(4):
        sd = f64(0)
        for k in range(4):
            sd = sd + f64(At[i][k]) * f64(At[i][k])
        W.append(sd)
    eps = f32(np.finfo(f32).eps) * f32(2)
    for _ in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                a, b, p = W[i], W[j], f64(0)
                for k in range(4):
                    p = p + f64(At[i][k]) * f64(At[j][k])
                if abs(p) <= f64(eps) * np.sqrt(a * b):
                    continue
                p = p * f64(2)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * f64(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * f64(s) * f64(2)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * f64(2))))
                    s = f32(p / (gamma * f64(c) * f64(2)))
                a = b = f64(0)
                for k in range(4):
                    t0 = c * At[i][k] + s * At[j][k]
                    t1 = -s * At[i][k] + c * At[j][k]
                    At[i][k], At[j][k] = t0, t1
                    a = a + f64(t0) * f64(t0)
                    b = b + f64(t1) * f64(t1)
                W[i], W[j] = a, b
                changed = True
                for k in range(4):
                    t0 = c * Vt[i][k] + s * Vt[j][k]
                    t1 = -s * Vt[i][k] + c * Vt[j][k]
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    for i in range(4):
        sd = f64(0)
        for k in range(4):
            sd = sd + f64(At[i][k]) * f64(At[i][k])
        W[i] = np.sqrt(sd)
    for i in range(3):
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return np.array(Vt[3], f32)


def triangulation_matrix(xn1, xn2, T1, T2):
    """A of :594-598: row = xn * Tcw.row(2) - Tcw.row(0 / 1), a float multiply and a float subtract per element"""
    A = np.zeros((4, 4), f32)
    for j in range(4):
        A[0, j] = f32(xn1[0]) * f32(T1[8 + j]) - f32(T1[j])
        A[1, j] = f32(xn1[1]) * f32(T1[8 + j]) - f32(T1[4 + j])
        A[2, j] = f32(xn2[0]) * f32(T2[8 + j]) - f32(T2[j])
        A[3, j] = f32(xn2[1]) * f32(T2[8 + j]) - f32(T2[4 + j])
    return A


def _row_dot(T, r, x):
    s = f64(T[4 * r]) * f64(x[0]) + f64(T[4 * r + 1]) * f64(x[1]) + f64(T[4 * r + 2]) * f64(x[2]) + f64(T[4 * r + 3])
    return f32(s)


def _dist(x, O):
    a, b, c = f32(x[0]) - f32(O[0]), f32(x[1]) - f32(O[1]), f32(x[2]) - f32(O[2])
    return f32(np.sqrt(f64(a) * f64(a) + f64(b) * f64(b) + f64(c) * f64(c)))


def unproject_stereo(cam, Twc, u, v, z):
    """KeyFrame::UnprojectStereo (KeyFrame.cc:821-837); None = the empty cv::Mat"""
    z = f32(z)
    if not z > 0:
        return None
    invfx, invfy = f32(1.0) / f32(cam[0]), f32(1.0) / f32(cam[1])
    x = (f32(u) - f32(cam[2])) * z * invfx
    y = (f32(v) - f32(cam[3])) * z * invfy
    out = np.zeros(3, f32)
    for i in range(3):
        t = f32(Twc[4 * i]) * x + f32(Twc[4 * i + 1]) * y + f32(Twc[4 * i + 2]) * z
        out[i] = f32(f64(t) + f64(Twc[4 * i + 3]))
    return out


def _reproject(stereo, ctype, cam, kfcam, mbf, T, x3D, z, u, v, ur, sigma2):
    x, y = _row_dot(T, 0, x3D), _row_dot(T, 1, x3D)
    invz = f32(f64(1.0) / f64(z))
    if not stereo:
        uv = om.camera_project_f(ctype, cam, np.array([x, y, z], f32))
        eX, eY = f32(uv[0]) - f32(u), f32(uv[1]) - f32(v)
        return not f64(eX * eX + eY * eY) > f64(5.991) * f64(sigma2)
    u1 = f32(kfcam[0]) * x * invz + f32(kfcam[2])
    u1_r = u1 - f32(mbf) * invz
    v1 = f32(kfcam[1]) * y * invz + f32(kfcam[3])
    eX, eY, eR = u1 - f32(u), v1 - f32(v), u1_r - f32(ur)
    return not f64(eX * eX + eY * eY + eR * eR) > f64(7.8) * f64(sigma2)


def _ulp_shift(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf), dtype=f32)
    return x


def new_point(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2, variant=None, cs_shift=0, mbf2=None):
    """One match.  P: a PAIR_DTYPE record; lv = (sigma2_1, scale1, sigma2_2, scale2) float32 arrays; k = (x, y, octave) of the keypoint the
    loop reads, raw = (x, y) of mvKeys[idx].  variant: one of VARIANTS (a WRONG rule, for the tests of the scenes); cs_shift: move the
    stereo cosine by that many float ulps (the one place a libm result decides); mbf2: KF2's own mbf (variant 'mbf2' only).
    Returns (code, x3D float32[3] -- zeros unless the code is 1..3)."""
    with np.errstate(all="ignore"):
        return _new_point(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2, variant, cs_shift, mbf2)


def _new_point(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2, variant, cs_shift, mbf2):
    zero = np.zeros(3, f32)
    rig1, rig2 = P["nleft1"] != -1, P["nleft2"] != -1
    assert rig1 == rig2, "a mixed rig / single-camera pair: the reference reuses stale matrices"
    ur1, ur2 = f32(ur1), f32(ur2)
    bStereo1, bStereo2 = (not rig1) and ur1 >= 0, (not rig2) and ur2 >= 0
    c1 = 1 if rig1 and idx1 >= P["nleft1"] else 0
    c2 = 1 if rig2 and idx2 >= P["nleft2"] else 0
    T1, T2, cam1, cam2 = P["Tcw1"][c1], P["Tcw2"][c2], P["cam1"][c1], P["cam2"][c2]
    type1, type2 = int(P["cam1_type"][c1]), int(P["cam2_type"][c2])
    xn1 = om.camera_unproject_f(type1, cam1, f32(k1[0]), f32(k1[1]))
    xn2 = om.camera_unproject_f(type2, cam2, f32(k2[0]), f32(k2[1]))
    ray1, ray2 = np.zeros(3, f32), np.zeros(3, f32)
    for i in range(3):
        ray1[i] = f32(f64(T1[i]) * f64(xn1[0]) + f64(T1[4 + i]) * f64(xn1[1]) + f64(T1[8 + i]) * f64(xn1[2]))
        ray2[i] = f32(f64(T2[i]) * f64(xn2[0]) + f64(T2[4 + i]) * f64(xn2[1]) + f64(T2[8 + i]) * f64(xn2[2]))
    dot = f64(ray1[0]) * f64(ray2[0]) + f64(ray1[1]) * f64(ray2[1]) + f64(ray1[2]) * f64(ray2[2])
    n1 = np.sqrt(f64(ray1[0]) * f64(ray1[0]) + f64(ray1[1]) * f64(ray1[1]) + f64(ray1[2]) * f64(ray1[2]))
    n2 = np.sqrt(f64(ray2[0]) * f64(ray2[0]) + f64(ray2[1]) * f64(ray2[1]) + f64(ray2[2]) * f64(ray2[2]))
    cosRays = f32(dot / (n1 * n2))
    cosStereo = cosRays + f32(1)
    cs1 = cs2 = cosStereo
    if bStereo1:
        cs1 = _ulp_shift(cos_stereo(P["mb1"], depth1), cs_shift)
    if bStereo2 and (not bStereo1 or variant == "if_not_else_if"):
        cs2 = _ulp_shift(cos_stereo(P["mb2"], depth2), cs_shift)
    cosStereo = cs2 if cs2 < cs1 else cs1
    if cosRays < cosStereo and cosRays > 0 and (bStereo1 or bStereo2 or f64(cosRays) < f64(0.9998)):
        v = jacobi_null4(triangulation_matrix(xn1, xn2, T1, T2))
        if v[3] == 0:
            return 5, zero
        inv = f32(f64(1.0) / f64(v[3]))
        x3D = np.array([v[0] * inv, v[1] * inv, v[2] * inv], f32)
        code = 1
    elif bStereo1 and cs1 < cs2:
        r = k1 if variant == "unproject_un" else raw1
        x3D = unproject_stereo(P["cam1"][0], P["Twc1"], r[0], r[1], depth1)
        code = 2
    elif bStereo2 and cs2 < cs1:
        r = k2 if variant == "unproject_un" else raw2
        x3D = unproject_stereo(P["cam2"][0], P["Twc2"], r[0], r[1], depth2)
        code = 3
    else:
        return 4, zero
    if x3D is None:
        return 6, zero
    z1 = _row_dot(T1, 2, x3D)
    if z1 <= 0:
        return 7, zero
    z2 = _row_dot(T2, 2, x3D)
    if z2 <= 0:
        return 8, zero
    if not _reproject(bStereo1, type1, cam1, P["cam1"][0], P["mbf"], T1, x3D, z1, k1[0], k1[1], ur1, lv[0][int(k1[2])]):
        return 9, zero
    if not _reproject(bStereo2, type2, cam2, P["cam2"][0], mbf2 if variant == "mbf2" else P["mbf"], T2, x3D, z2, k2[0], k2[1], ur2,
                      lv[2][int(k2[2])]):
        return 10, zero
    d1, d2 = _dist(x3D, P["Ow1"][c1]), _dist(x3D, P["Ow2"][c2])
    if d1 == 0 or d2 == 0:
        return 11, zero
    if P["far_points"] and (d1 >= f32(P["th_far_points"]) or d2 >= f32(P["th_far_points"])):
        return 12, zero
    ratioDist = d2 / d1
    ratioOctave = f32(lv[1][int(k1[2])]) / f32(lv[3][int(k2[2])])
    rf = f32(P["ratio_factor"])
    if variant == "ratio_inverted":
        bad = ratioDist * rf > ratioOctave and ratioDist < ratioOctave * rf
    else:
        bad = ratioDist * rf < ratioOctave or ratioDist > ratioOctave * rf
    if bad:
        return 13, zero
    return code, x3D


# ------------------------------------------------------------------ float64 restatement
def _unproject64(ctype, p, u, v):
    p = np.asarray(p, f64)
    x, y = (u - p[2]) / p[0], (v - p[3]) / p[1]
    if ctype == 0:
        return np.array([x, y, 1.0])
    td = min(max(-math.pi / 2, math.hypot(x, y)), math.pi / 2)
    s = 1.0
    if td > 1e-8:
        th = td
        for _ in range(10):
            t2 = th * th
            fix = (th * (1 + p[4] * t2 + p[5] * t2 ** 2 + p[6] * t2 ** 3 + p[7] * t2 ** 4) - td) / \
                  (1 + 3 * p[4] * t2 + 5 * p[5] * t2 ** 2 + 7 * p[6] * t2 ** 3 + 9 * p[7] * t2 ** 4)
            th -= fix
            if abs(fix) < 1e-6:                              # precision(1e-6) of KannalaBrandt8.h: the float model stops there too
                break
        s = math.tan(th) / td
    return np.array([x * s, y * s, 1.0])


def new_point_f64(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2):
    """The same loop body in float64 with np.linalg.svd.  Returns (code, x3D, margin): margin = the smallest relative distance of a
    decision quantity the match met to its threshold.  Cosines are compared as 1 - cos (a cosine near 1 cannot be 1 % away from another),
    cos > 0 as |cos|, depths as |z| / distance to the centre, w == 0 as |w| < 1e-9 of the unit null vector (a zero in float is a point at
    infinity here) and a zero distance as one below 1e-4 (the float triangulation's own error): the constructions of those two are exact,
    synth_new_points.py, and carry no margin."""
    with np.errstate(all="ignore"):
        return _new_point_f64(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2)


def _new_point_f64(P, lv, idx1, idx2, k1, raw1, ur1, depth1, k2, raw2, ur2, depth2):
    margin = [np.inf]

    def near(q, thr, scale=None):
        s = abs(thr) if scale is None else scale
        margin[0] = min(margin[0], abs(q - thr) / s if s > 0 else np.inf)

    rig = P["nleft1"] != -1
    st1, st2 = (not rig) and ur1 >= 0, (not rig) and ur2 >= 0
    c1 = 1 if rig and idx1 >= P["nleft1"] else 0
    c2 = 1 if rig and idx2 >= P["nleft2"] else 0
    T1, T2 = P["Tcw1"][c1].astype(f64).reshape(3, 4), P["Tcw2"][c2].astype(f64).reshape(3, 4)
    cam1, cam2 = P["cam1"][c1].astype(f64), P["cam2"][c2].astype(f64)
    type1, type2 = int(P["cam1_type"][c1]), int(P["cam2_type"][c2])
    xn1, xn2 = _unproject64(type1, cam1, float(k1[0]), float(k1[1])), _unproject64(type2, cam2, float(k2[0]), float(k2[1]))
    r1, r2 = T1[:, :3].T @ xn1, T2[:, :3].T @ xn2
    cr = float(r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2)))
    cs1 = cs2 = cr + 1
    if st1:
        cs1 = math.cos(2 * math.atan2(float(P["mb1"]) / 2, float(depth1)))
    elif st2:
        cs2 = math.cos(2 * math.atan2(float(P["mb2"]) / 2, float(depth2)))
    cs = min(cs1, cs2)
    if st1 or st2:
        near(1 - cr, 1 - cs)
    near(cr, 0.0, 1.0)
    if not (st1 or st2):
        near(1 - cr, 1 - 0.9998)
    zero = np.zeros(3)
    if cr < cs and cr > 0 and (st1 or st2 or cr < 0.9998):
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        v = np.linalg.svd(A)[2][3]
        if abs(v[3]) < 1e-9:
            return 5, zero, margin[0]
        x = v[:3] / v[3]
        code = 1
    elif st1 and cs1 < cs2:
        if not depth1 > 0:
            return 6, zero, margin[0]
        cam = P["cam1"][0].astype(f64); Twc = P["Twc1"].astype(f64).reshape(3, 4)
        x = Twc[:, :3] @ np.array([(raw1[0] - cam[2]) * depth1 / cam[0], (raw1[1] - cam[3]) * depth1 / cam[1], depth1], f64) + Twc[:, 3]
        code = 2
    elif st2 and cs2 < cs1:
        if not depth2 > 0:
            return 6, zero, margin[0]
        cam = P["cam2"][0].astype(f64); Twc = P["Twc2"].astype(f64).reshape(3, 4)
        x = Twc[:, :3] @ np.array([(raw2[0] - cam[2]) * depth2 / cam[0], (raw2[1] - cam[3]) * depth2 / cam[1], depth2], f64) + Twc[:, 3]
        code = 3
    else:
        return 4, zero, margin[0]
    O1, O2 = P["Ow1"][c1].astype(f64), P["Ow2"][c2].astype(f64)
    d1, d2 = float(np.linalg.norm(x - O1)), float(np.linalg.norm(x - O2))
    X1, X2 = T1[:, :3] @ x + T1[:, 3], T2[:, :3] @ x + T2[:, 3]
    near(X1[2], 0.0, max(d1, 1e-300))
    if X1[2] <= 0:
        return 7, zero, margin[0]
    near(X2[2], 0.0, max(d2, 1e-300))
    if X2[2] <= 0:
        return 8, zero, margin[0]
    for which, (st, ctype, cam, kf, X, k, ur, s2) in enumerate(((st1, type1, cam1, P["cam1"][0].astype(f64), X1, k1, ur1, lv[0][int(k1[2])]),
                                                                (st2, type2, cam2, P["cam2"][0].astype(f64), X2, k2, ur2, lv[2][int(k2[2])]))):
        if not st:
            uv = om.kb8_project_np((ctype, cam), X)
            e2, thr = (uv[0] - k[0]) ** 2 + (uv[1] - k[1]) ** 2, 5.991 * float(s2)
        else:
            u = kf[0] * X[0] / X[2] + kf[2]; v_ = kf[1] * X[1] / X[2] + kf[3]
            e2, thr = (u - k[0]) ** 2 + (v_ - k[1]) ** 2 + (u - float(P["mbf"]) / X[2] - float(ur)) ** 2, 7.8 * float(s2)
        near(e2, thr)
        if e2 > thr:
            return 9 + which, zero, margin[0]
    if d1 < 1e-4 or d2 < 1e-4:                              # a zero in float: within the triangulation's own error of the centre
        return 11, zero, margin[0]
    if P["far_points"]:
        near(d1, float(P["th_far_points"])); near(d2, float(P["th_far_points"]))
        if d1 >= P["th_far_points"] or d2 >= P["th_far_points"]:
            return 12, zero, margin[0]
    rd, ro, rf = d2 / d1, float(lv[1][int(k1[2])]) / float(lv[3][int(k2[2])]), float(P["ratio_factor"])
    near(rd * rf, ro); near(rd, ro * rf)
    if rd * rf < ro or rd > ro * rf:
        return 13, zero, margin[0]
    return code, x, margin[0]


# ------------------------------------------------------------------ one pair, a chain of pairs
def run_pair(pr, variant=None, cs_shift=0, f64_too=False):
    """Every match of one pair (synth_new_points.py layout).  Returns dict(outcome uint8 [n1], x3D float32 [n1][3], n_created, has_mp1,
    has_mp2 -- the flags after AddMapPoint (:715-716), from pr['mp1'] / pr['mp2'] when present)."""
    n1 = len(pr["kp1"])
    out = np.zeros(n1, np.uint8); x3 = np.zeros((n1, 3), f32)
    mp1 = np.array(pr.get("mp1", np.zeros(n1, np.uint8)), np.uint8); mp2 = np.array(pr.get("mp2", np.zeros(len(pr["kp2"]), np.uint8)), np.uint8)
    res64 = {}
    for i in np.flatnonzero(pr["matches12"] >= 0):
        a = match_args(pr, int(i))
        c, x = new_point(*a, variant=variant, cs_shift=cs_shift, mbf2=pr.get("mbf2"))
        out[i] = c; x3[i] = x
        if 1 <= c <= 3:
            mp1[i] = 1; mp2[pr["matches12"][i]] = 1
        if f64_too:
            res64[int(i)] = new_point_f64(*a)
    r = dict(outcome=out, x3D=x3, n_created=int(np.sum((out >= 1) & (out <= 3))), has_mp1=mp1, has_mp2=mp2)
    if f64_too:
        r["f64"] = res64
    return r


def match_args(pr, i):
    j = int(pr["matches12"][i])
    k1, k2 = pr["kp1"][i], pr["kp2"][j]
    raw1, raw2 = pr.get("kp1_raw", pr["kp1"])[i], pr.get("kp2_raw", pr["kp2"])[j]
    return (pr["P"], pr["lv"], i, j, (k1["x"], k1["y"], k1["octave"]), (raw1["x"], raw1["y"]), pr["ur1"][i], pr["depth1"][i],
            (k2["x"], k2["y"], k2["octave"]), (raw2["x"], raw2["y"]), pr["ur2"][j], pr["depth2"][j])


def libm_sensitive(pr, i):
    """the one licence of the device comparison: a stereo match whose outcome or point changes when the stereo cosine moves one float ulp"""
    j = int(pr["matches12"][i])
    if pr["P"]["nleft1"] != -1 or not (pr["ur1"][i] >= 0 or pr["ur2"][j] >= 0):
        return False
    a = match_args(pr, i)
    c0, x0 = new_point(*a)
    for sh in (-1, 1):
        c, x = new_point(*a, cs_shift=sh)
        if c != c0 or x.tobytes() != x0.tobytes():
            return True
    return False
