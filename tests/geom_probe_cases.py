"""Inputs of tests/test_gpu_geom_probe.py: at most 512 items per op, built by code with fixed seeds.  TEST INFRASTRUCTURE ONLY.

CASES[op] = Case(inputs [n, in_width] float64, labels, truth): labels[i] names the branch item i must take (None: the op has none; 'a|b':
either), as geom_probe_model's faithful functions name them; truth lists the items that also go through the 50-digit truth check.
tests/test_geom_probe_model.py asserts the labels, the branch coverage and the margins: every branch argument is an intended exact
value (a tie, a cosine of exactly +-1) or at least 1e-9 relative away from its threshold.

Rotations: angles 0, 1e-9, 0.9e-5, 1.1e-5, 0.9e-4, 1.1e-4, 1, 2 pi / 3 -+ 1e-3, 3.0, pi - 1e-3, pi - 1e-7 and pi, about x, y, z, six
diagonals and five random axes.  R_to_quat leaves its trace branch above 120 degrees and then picks the largest diagonal element, i.e.
the axis' largest component; equal components (the diagonals) are exact ties R[0] == R[4] etc., the first index wins.

s3_log: the pivot outcomes 'p<r><c>' (r: the row exchanged with row 0, c: the row taken for column 1).  Small sigma and d > 1 - 1e-5
(theta below 4.5e-3): W = I + O(theta), no exchange is reachable from a unit quaternion; test_geom_probe_model.py::
test_s3_log_small_small_never_pivots searches 2000 random Sim3 and finds none (the two crafted non-unit items below are no rotations).  Large sigma and small theta: reachable, because the reference's B = (sigma^2 / 2 - sigma + 1)
s / sigma^3 of that branch (sim3.h:199) grows like 1 / sigma^3 instead of tending to 1 / 6, so B Omega^2 is of order one for a small
|sigma|; kept, as the library keeps it.  In the three reachable branches all six outcomes occur and each is drawn until it has 8 items.
Exact ties: a rotation about
x gives a1 == a2 (== 0) in column 0; a NON-ZERO tie a0 == a1 cannot be had from a rotation (the entries come out of libm), so one item
is a crafted non-unit quaternion (0, 0, 2^-10, 2^9 t) in the small-small branch, where W = [[a, -a, 0], [a, a, 0], [0, 0, 1]] with
a = fl(1 - fl(fl(t^2) / 6)) == t / 2 bit for bit: every operation up to the comparison rounds once whether contracted or not.  Both
orders of two equal pivots solve the system equally well, so only the last bit tells them apart: the item's translation is chosen so
that upsilon_0 of the first-row order differs in its last bit from the second-row order, whether a * x1 + t0 is contracted or not, and
the GPU test compares this one item bit for bit (the CPU test proves the claim in exact rational arithmetic).  A second
crafted item (2^-10, 0, 0, 2^9 t) has an exact ZERO on the diagonal of column 1, where only the exchange keeps the solve finite."""
import math
from collections import namedtuple

import numpy as np

import geom_probe_model as gm

Case = namedtuple("Case", "inputs labels truth")
f32, f64 = np.float32, np.float64
PI = math.pi
EPS = 1e-5
ANGLES = [0.0, 1e-9, 0.9e-5, 1.1e-5, 0.9e-4, 1.1e-4, 1.0, 2 * PI / 3 - 1e-3, 2 * PI / 3 + 1e-3, 3.0, PI - 1e-3, PI - 1e-7, PI]


def _unit(v):
    v = np.asarray(v, f64)
    return v / np.sqrt(np.sum(v * v))


def _axes():
    rng = np.random.default_rng(20240)
    fixed = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 1), (-1, 1, 1)]
    return [_unit(a) for a in fixed] + [_unit(rng.normal(size=3)) for _ in range(5)]


AXES = _axes()
ROT = [(th, ax) for ax in AXES for th in ANGLES]              # 182 (angle, axis)


def rot_R(th, ax):
    """c I + s [a]x + (1 - c) a a^T: equal axis components give exactly equal diagonal elements"""
    c, s = math.cos(th), math.sin(th)
    a = ax
    R = np.empty(9)
    for i in range(3):
        for j in range(3):
            R[3 * i + j] = (1 - c) * a[i] * a[j] + (c if i == j else 0.0)
    R[1] -= s * a[2]; R[2] += s * a[1]; R[3] += s * a[2]; R[5] -= s * a[0]; R[6] -= s * a[1]; R[7] += s * a[0]
    return R


def rot_q(th, ax):
    return np.concatenate([math.sin(th / 2) * ax, [math.cos(th / 2)]])


def rq_label(th, ax):
    """the branch of Eigen's Quaterniond(Matrix3d) on a rotation by th about ax"""
    if th < 2 * PI / 3:
        return "trace"
    a2 = [ax[0] * ax[0], ax[1] * ax[1], ax[2] * ax[2]]
    i = 0
    if a2[1] > a2[0]:
        i = 1
    if a2[2] > a2[i]:
        i = 2
    return "i%d" % i


def _every(n, k):
    """k indices spread over range(n)"""
    return sorted(set(int(round(x)) for x in np.linspace(0, n - 1, k)))


def _rand_q(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.sqrt(np.sum(q * q, 1))[:, None]


def _build():
    C = {}
    rng = np.random.default_rng(951)
    rotvec = np.array([th * ax for th, ax in ROT])
    quats = np.array([rot_q(th, ax) for th, ax in ROT])
    mats = np.array([rot_R(th, ax) for th, ax in ROT])
    n = len(ROT)

    # ---- quaternions
    C["quat_to_R"] = Case(np.vstack([quats, quats * rng.uniform(0.5, 2, (n, 1))]), None, [])
    C["quat_rot"] = Case(np.hstack([np.vstack([quats, _rand_q(rng, 64)]), rng.normal(size=(n + 64, 3)) * 10]), None, [])
    C["quat_mul"] = Case(np.hstack([np.vstack([quats, _rand_q(rng, 64)]), np.vstack([quats[::-1], _rand_q(rng, 64)])]), None, [])
    qn = np.vstack([quats, -quats, quats[::3] * 3.5, _rand_q(rng, 32), [[0.6, 0, 0.8, 0], [1, 2, 3, 0], [0, 0, -2, 0], [0, 0, 0, -1], [0, 0, 0, 2]]])
    C["quat_norm_rot"] = Case(qn, ["flip" if w < 0 else ("w0" if w == 0 else "keep") for w in qn[:, 3]], [])

    # ---- R_to_quat: the rotations, 24 more per non-trace branch near each axis, and explicit ties
    R_in, R_lab = list(mats), [rq_label(th, ax) for th, ax in ROT]
    for i in range(3):
        for _ in range(24):
            ax = _unit(np.eye(3)[i] * rng.choice([-1, 1]) + rng.uniform(-0.35, 0.35, 3))
            th = rng.uniform(2.3, 3.12)
            R_in.append(rot_R(th, ax)); R_lab.append(rq_label(th, ax))
    for th in (2.3, 2.8, 3.1, PI):                       # about z: R[0] == R[4] == cos th below R[8] = 1
        R_in.append(rot_R(th, AXES[2])); R_lab.append("i2")
    for th in (2.3, 2.8, 3.1, PI):                       # R[0] == R[4] the largest: the first wins
        R_in.append(rot_R(th, AXES[3])); R_lab.append("i0")
    C["R_to_quat"] = Case(np.array(R_in), R_lab, [])

    # ---- huber: delta as the callers round it, e below / at / one ulp above dsqr, 0, far above
    hub = []
    for th2 in (5.991, 7.815, 1.0, 10.0):
        delta = float(f32(math.sqrt(th2)))
        dsqr = float(f32(delta * delta))
        for delta_, dsqr_ in ((delta, dsqr), (math.sqrt(th2), th2)):
            for e in (0.0, 0.5 * dsqr_, np.nextafter(dsqr_, 0), dsqr_, np.nextafter(dsqr_, np.inf), 1.5 * dsqr_, 10 * dsqr_, 1e6):
                hub.append([e, delta_, dsqr_])
    hub = np.array(hub)
    C["huber"] = Case(hub, ["at" if e == d else ("below" if e < d else "above") for e, _, d in hub], [])

    # ---- SE3
    poses = np.hstack([_rand_q(rng, n), rng.normal(size=(n, 3)) * 5])
    C["se3_oplus"] = Case(np.hstack([rotvec, rng.normal(size=(n, 3)), poses]),
                          [("small" if th < EPS else "large") + "/" + ("trace" if th < EPS else rq_label(th, ax)) for th, ax in ROT], _every(n, 24))
    C["se3_mul"] = Case(np.hstack([quats, rng.normal(size=(n, 3)), poses]), None, [])

    # ---- SO(3)
    C["so3_exp"] = Case(rotvec, ["small" if th < 1e-5 else "large" for th, _ in ROT], _every(n, 24))
    C["so3_exp_imu"] = Case(rotvec, ["small" if th < 1e-4 else "large" for th, _ in ROT], _every(n, 12))
    jv = np.vstack([rotvec, [(PI - 1e-6) * ax for ax in AXES], [[PI, 0, 0]]])
    jl = ["small" if th < 1e-5 else "large" for th, _ in ROT] + ["large"] * (len(AXES) + 1)
    C["so3_right_jac"] = Case(jv, jl, _every(n + len(AXES), 24))
    C["so3_inv_right_jac"] = Case(jv, jl, [])                          # the product Jr Jr^-1 is checked on so3_right_jac's truth items
    lg, ll = [], []
    for k, (th, ax) in enumerate(ROT):
        if th == PI and k // len(ANGLES) >= 3:          # at pi the cosine is -1 exactly about x, y, z only; elsewhere its rounding would pick the branch
            continue
        lg.append(rot_R(th, ax))
        ll.append("unscaled" if math.sin(th) < 1e-5 else "scaled")
    for th in (0.9e-5, 1.1e-5):
        for ax in AXES[:6]:
            lg.append(rot_R(PI - th, ax)); ll.append("unscaled" if th < 1e-5 else "scaled")
    lg += [np.eye(3).ravel(), np.diag([1.0, -1, -1]).ravel(), np.diag([-1.0, 1, -1]).ravel()]; ll += ["unscaled"] * 3          # cosine exactly +-1
    lg += [np.diag([1, 1, 1 + 2.0 ** -51]).ravel(), np.diag([1, -1, -1 - 2.0 ** -51]).ravel()]; ll += ["out_of_range"] * 2     # one ulp outside
    C["so3_log"] = Case(np.array(lg), ll, _every(len(lg) - 17, 24))

    # ---- so3_normalize: rotation + delta N, N of unit Frobenius norm
    sn, sl = [], []
    for k, (th, ax) in enumerate([(0.0, AXES[0]), (1.0, AXES[9]), (3.0, AXES[10]), (PI - 1e-3, AXES[6]), (2.0, AXES[11]), (0.3, AXES[12]),
                                  (1e-4, AXES[13]), (2.5, AXES[1]), (PI, AXES[2]), (1.5, AXES[7]), (0.7, AXES[4]), (2.9, AXES[8])]):
        Rx = np.array([float(v) for v in gm.truth_so3_exp(th * ax)])
        for delta in (1e-15, 6e-8, 1e-5, 1e-3):
            N = rng.normal(size=9)
            sn.append(Rx + delta * N / np.sqrt(np.sum(N * N))); sl.append("%g" % delta)
    C["so3_normalize"] = Case(np.array(sn), sl, list(range(len(sn))))

    # ---- Sim3
    u7, ul = [], []
    for sigma in (0.0, 0.9e-5, -0.9e-5, 1.1e-5, -1.1e-5, 1e-3, 0.5, -0.5, 3.0, -3.0):
        for th in (0.0, 1e-9, 0.9e-5, 1.1e-5, 1.0, 2.5, 3.0):
            for ax in (AXES[9], AXES[(len(u7) // 3) % 9], AXES[10 + len(u7) % 4]):
                u7.append(np.concatenate([th * ax, rng.normal(size=3) * 3, [sigma]]))
                ul.append(("ss" if abs(sigma) < EPS else "sl") + ("ts" if th < EPS else "tl") + "/" + ("trace" if th < EPS else rq_label(th, ax)))
    C["s3_exp"] = Case(np.array(u7), ul, _every(len(u7), 32))
    sims = np.hstack([np.vstack([quats, _rand_q(rng, 64)]), rng.normal(size=(n + 64, 3)) * 4, np.exp(rng.uniform(-3, 3, (n + 64, 1)))])
    C["s3_mul"] = Case(np.hstack([sims, sims[::-1]]), None, [])
    C["s3_inverse"] = Case(sims, None, [])
    C["s3_map"] = Case(np.hstack([sims, rng.normal(size=(len(sims), 3)) * 10]), None, [])
    C["s3_log"] = _s3_log_cases()

    # ---- cameras in double: (fx fy cx cy model k[4] P)
    cams = [[458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0, 0],                                                    # EuRoC pinhole
            [190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 1,
             0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182],       # TUM-VI KB8
            [458.654, 457.296, 367.215, 248.375, 1, -0.0133, 0.0205, -0.0121, 0.0028]]                              # EuRoC-like fisheye k
    pts = [[0, 0, 2.0], [1e-12, 0, 1.0], [0, 1e-12, 3.0], [-1e-12, 1e-12, 0.5], [math.tan(math.radians(89)), 0, 1.0],
           [0.6 * math.tan(math.radians(89)), -0.8 * math.tan(math.radians(89)), 1.0], [0.3, -0.2, -1.0], [-2.0, 1.0, -0.5], [0, 0, -1.0]]
    pts += [list(p) for p in np.hstack([rng.normal(size=(40, 2)) * 1.5, rng.uniform(0.3, 8, (40, 1))])]
    cp = np.array([c + p for c in cams for p in pts])
    lab = ["kb8" if r[4] == 1 else "pinhole" for r in cp]
    C["cam_project"] = Case(cp, lab, [])
    C["cam_project_jac"] = Case(cp, lab, [i for i in _every(len(cp), 40) if not (cp[i, 9] == 0 and cp[i, 10] == 0)][:30])

    # ---- cameras in float: (p[8] P) and (p[8] u v), all values float-exact
    fcams = [np.array(f32([c[0], c[1], c[2], c[3], c[5], c[6], c[7], c[8]]), f64) for c in cams]
    fpts = np.array(f32(pts), f64)
    C["tri_project_pinhole"] = Case(np.array([np.concatenate([fcams[0], p]) for p in fpts]), None, [])
    C["tri_project_kb8"] = Case(np.array([np.concatenate([c, p]) for c in fcams[1:] for p in fpts]), None, [])
    C["tri_unproject_pinhole"] = Case(np.array([np.concatenate([fcams[0], f64(f32(uv))]) for uv in rng.uniform(0, 700, (32, 2))]), None, [])
    unit = np.array(f32([1, 1, 0, 0, 0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673]), f64)       # theta_d = |(u, v)|
    uk, ukl = [], []
    for cam in fcams[1:]:
        for r, phi in zip(rng.uniform(0.05, 1.45, 40), rng.uniform(0, 2 * PI, 40)):                           # theta_d = r < pi / 2
            uv = (cam[2] + cam[0] * r * math.cos(phi), cam[3] + cam[1] * r * math.sin(phi))
            uk.append(np.concatenate([cam, f64(f32(uv))])); ukl.append("newton")
        uk.append(np.concatenate([cam, cam[2:4]])); ukl.append("tiny")                                      # the principal point
        for uv in ((cam[2] + 2 * cam[0], cam[3]), (cam[2] - 3 * cam[0], cam[3] + 3 * cam[1]), (0.0, 1e4)):   # beyond the pi / 2 clamp
            uk.append(np.concatenate([cam, f64(f32(uv))])); ukl.append("newton/clamped")
    for td, lb in ((0.0, "tiny"), (0.9e-8, "tiny"), (1.1e-8, "newton"), (1e-4, "newton"), (0.5, "newton"), (1.5, "newton"), (1.5707, "newton")):
        uk.append(np.concatenate([unit, f64(f32([td, 0]))])); ukl.append(lb)
        uk.append(np.concatenate([unit, f64(f32([0, -td]))])); ukl.append(lb)
    # strong distortion: the Newton iteration's slowest inputs (test_geom_probe_model.py prints the step counts)
    hard = np.array(f32([1, 1, 0, 0, -0.3, 0.1, -0.02, 0.002]), f64)
    for td in (0.3, 0.6, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3):
        uk.append(np.concatenate([hard, f64(f32([td, 0]))])); ukl.append("newton")
    # all ten Newton steps: found by a random search over k and theta_d (30000 draws; coefficients far from any real lens)
    ten = np.array(f32([1, 1, 0, 0, 0.11289330571889877, -0.10578923672437668, -0.028128741309046745, -0.03340231627225876]), f64)
    uk.append(np.concatenate([ten, f64(f32([1.2108377685902596, 0]))])); ukl.append("newton")
    C["tri_unproject_kb8"] = Case(np.array(uk), ukl, [])

    # ---- tri_svd4_null: in[4 i + k] = At[i][k], At[i] = column i of A
    sv, svl = [], []

    def add(A, lb):
        sv.append(np.array(f32(np.asarray(A).T.ravel()), f64)); svl.append(lb)

    def ortho():
        return np.linalg.qr(rng.normal(size=(4, 4)))[0]
    for d in ((4, 3, 2, 1), (1, 2, 3, 4), (2, 0.5, 3, 1), (1, 1, 1, 1), (3, 0, 2, 1)):
        add(np.diag(d), "diagonal")
    for _ in range(16):
        add(ortho() @ np.diag([rng.uniform(2, 4), rng.uniform(1, 2), rng.uniform(0.3, 1), rng.uniform(1e-5, 1e-3)]) @ ortho().T, "gap")
    for _ in range(6):
        M = rng.normal(size=(4, 4))
        add(M, "random"); add(M[:, ::-1], "random")                    # column norms in both orders: both signs of beta at the first pair
    for _ in range(6):
        M = rng.normal(size=(4, 4))
        M[:, rng.permutation(4)[:2]] = 0                                # two zero columns: a tie at zero, the sort's order decides
        add(M, "rank2")
    for _ in range(4):
        add(ortho() @ np.diag([2, 2, 1, 0.5]), "equal")                # columns = scaled orthonormal rows: ties among the norms
        add(ortho() @ np.diag([3, 2, 1, 1]), "equal_smallest")
    add(np.diag([3, 2, 1, 1]), "equal_smallest"); add(np.diag([1, 1, 3, 2]), "equal_smallest"); add(np.zeros((4, 4)), "rank2")
    C["tri_svd4_null"] = Case(np.array(sv), svl, [i for i, l in enumerate(svl) if l == "gap"])
    return C


ZERO_PIVOT_T = 2.4494897427831783
TIE_T0, TIE_T1 = 2.534, 0.393         # the tie item's translation: see test_geom_probe_model.py::test_pivot_tie_is_exact


def tie_t():
    """t with fl(1 + fl((1/6) fl(-t t))) == t / 2 bit for bit, next to the root 1.3723 of t^2 / 6 + t / 2 = 1"""
    t = f64((-3 + math.sqrt(33)) / 2)
    sixth = f64(1.0) / f64(6.0)
    cand = [t]
    up = dn = t
    for _ in range(4000):
        up, dn = np.nextafter(up, f64(2)), np.nextafter(dn, f64(1))
        cand += [up, dn]
    for c in cand:
        if f64(1) + sixth * (-(c * c)) == f64(0.5) * c:
            return float(c)
    raise AssertionError("no exact tie near the root")


def s3_log_draw(rng, small_sigma, small_theta):
    """one random Sim3 of the given branch pair"""
    th = rng.uniform(1e-4, 4.0e-3) if small_theta else rng.uniform(0.2, 3.1)
    if rng.uniform() < 0.25 and small_theta:
        th = 0.0
    sigma = rng.choice([0.0, 0.5e-5, -0.9e-5]) if small_sigma else rng.choice([-1, 1]) * math.exp(rng.uniform(math.log(1.1e-5), math.log(3.0)))
    q = rot_q(th, _unit(rng.normal(size=3)))
    return np.concatenate([q, rng.normal(size=3) * 3, [math.exp(sigma)]])


def _s3_log_cases():
    rng = np.random.default_rng(77031)
    S, L, truth = [], [], []
    for ss in (True, False):
        for st in (True, False):
            name = ("ss" if ss else "sl") + ("ts" if st else "tl")
            want = {"p01": 8} if ss and st else {p: 8 for p in ("p01", "p11", "p21", "p02", "p12", "p22")}
            for _ in range(20000):
                if not any(want.values()):
                    break
                x = s3_log_draw(rng, ss, st)
                m = []
                _, br = gm.s3_log(gm.N64, [f64(v) for v in x], m)
                piv = br.split("/")[1]
                if br.split("/")[0] == name and want.get(piv, 0) > 0 and min(v for _, v in m) >= 1e-6:
                    want[piv] -= 1
                    S.append(x); L.append(br)
            assert not any(want.values()), (name, want)
    truth = _every(len(S), 48)
    # the issue's three: 3.1 rad about z, y, x -> (0 <-> 1, none), (0 <-> 2, none), (none, 1 <-> 2); about x also a1 == a2 == 0 in column 0
    for ax, lb in ((AXES[2], "p11"), (AXES[1], "p21"), (AXES[0], "p02")):
        for s in (1.0, math.exp(0.7)):
            S.append(np.concatenate([rot_q(3.1, ax), [0.3, -1.2, 2.0], [s]])); L.append(("ss" if s == 1 else "sl") + "tl/" + lb)
    for th in (1.0, 2.0e-3):                                  # a1 == a2 == 0 without an exchange
        S.append(np.concatenate([rot_q(th, AXES[0]), [1.0, 2.0, -3.0], [1.0]])); L.append("ss" + ("ts" if th < 4e-3 else "tl") + "/p01")
    # column 1 with an EXACT zero on the diagonal after column 0: (x, 0, 0, w) gives W = [[1, 0, 0], [0, b, -t / 2], [0, t / 2, b]] with
    # b = fl(1 - fl(fl(t^2) / 6)) == 0 for t = 2.4494897427831783 (next to sqrt 6): without the exchange the solve divides by zero
    S.append(np.array([2.0 ** -10, 0, 0, ZERO_PIVOT_T * 2.0 ** 9, 0.5, 1.25, -2.0, 1.0])); L.append("ssts/p02")
    t = tie_t()                                               # the non-zero tie a0 == a1: the first row stays
    S.append(np.array([0, 0, 2.0 ** -10, t * 2.0 ** 9, TIE_T0, TIE_T1, 2.25, 1.0])); L.append("ssts/p01")
    return Case(np.array(S), L, truth)


CASES = _build()
TIE_ITEM = len(CASES["s3_log"].inputs) - 1
assert all(len(c.inputs) <= 512 for c in CASES.values())
N_TRUTH = sum(len(c.truth) for c in CASES.values())
