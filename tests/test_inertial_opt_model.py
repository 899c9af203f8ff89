"""CPU tests of the numpy model of Optimizer::InertialOptimization (tests/inertial_opt_model.py): its Jacobians against central
differences of its own error for all eight vertex blocks, the bordered block-tridiagonal solve against a dense one, recovery of the
truth on noise-free data, float64 and extended precision making the same accept / reject decisions over the decisive prefix, and
fixed / unconnected unknowns staying bit-identical."""
import numpy as np
import inertial_opt_cases as ic
import inertial_opt_model as iom
import synth_inertial_opt as sio

LD = np.longdouble


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip(np.asarray(Ra, float).reshape(3, 3)[:, 2] @ np.asarray(Rb, float)[:, 2], -1, 1))))


def test_jacobians_agree_with_central_differences():
    mp = sio.make_map(11, 6, mono=True, noise=1.0)
    rng = np.random.default_rng(0)
    mp["glob"][10:16] = rng.normal(0, 0.02, 6)
    mp["glob"][9] = 1.7                                     # away from 1: the scale block is d e / d s (see below)
    P = iom.Problem(mp, LD)
    vel = P.vel0 + rng.normal(0, 0.1, P.vel0.shape)
    glob = P.glob0.copy()
    e, J = iom.edge_error(P, vel, glob, jac=True)
    h = LD(1e-8)
    free = dict(free_vel_bias=1, free_gdir=1, free_scale=1)

    def fd(fn, dim):
        cols = []
        for j in range(dim):
            d = np.zeros(dim, LD); d[j] = h
            cols.append((fn(d) - fn(-d)) / (2 * h))
        return np.stack(cols, -1)

    for ed in range(len(P.e2)):
        k1, k2 = int(P.e1[ed]), int(P.e2[ed])

        def vfun(k):
            def f(d):
                v = vel.copy(); v[k] = v[k] + d
                return iom.edge_error(P, v, glob)[ed]
            return f

        def pfun(k):
            def f(d):
                R, p = iom.update_pose(P.R, P.p, k, d)
                return iom.edge_error(P, vel, glob, R=R, p=p)[ed]
            return f

        def gfun(sl):
            def f(d):
                xb = np.zeros(9, LD); xb[sl] = d
                return iom.edge_error(P, vel, iom.update_glob(glob, xb, free))[ed]
            return f

        def sfun(d):                                        # the reference's scale Jacobian is the derivative by s itself, not by the
            g = glob.copy(); g[9] = g[9] + d[0]             # exponent of VertexScale's update s exp(d): the two agree at s = 1 only
            return iom.edge_error(P, vel, g)[ed]
        for name, fn, dim in (("p1", pfun(k1), 6), ("v1", vfun(k1), 3), ("bg", gfun(slice(0, 3)), 3), ("ba", gfun(slice(3, 6)), 3),
                              ("p2", pfun(k2), 6), ("v2", vfun(k2), 3), ("gd", gfun(slice(6, 8)), 2), ("s", sfun, 1)):
            F = fd(fn, dim)
            err = float(np.abs(F - J[name][ed]).max())
            assert err <= 1e-8 * (1 + float(np.abs(J[name][ed]).max())), (ed, name, err)        # measured: <= 4e-11


def test_block_solve_equals_dense_solve():
    for fam, n, gaps in (("a_mono_prior", 12, ()), ("a_stereo", 7, (3,)), ("b", 5, ()), ("a_fixed", 6, ()), ("d", 6, ())):
        mp = ic.make(fam, n, 2, gaps)
        if gaps:
            mp["link"][n - 1] = 0                           # and a keyframe without any edge
        prm = ic.params(fam)
        P = iom.Problem(mp, np.float64)
        chi, D, O, B, C, rv, rb = iom.build(P, P.vel0, P.glob0, prm)
        lam = 1e3
        xv, xb = iom.solve_system(P, prm, lam, D, O, B, C, rv, rb)
        H, b, act, cols = iom.dense_system(P, prm, lam, D, O, B, C, rv, rb)
        x = np.linalg.solve(H, b)
        want_v = np.zeros((n, 3)); want_b = np.zeros(9)
        if len(act):
            want_v[act] = x[:3 * len(act)].reshape(-1, 3)
        want_b[cols] = x[3 * len(act):]
        scale = np.abs(x).max()
        assert np.abs(xv - want_v).max() <= 1e-9 * scale and np.abs(xb - want_b).max() <= 1e-9 * scale, fam      # measured: <= 3e-13
        assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max())


def test_overload_a_recovers_the_truth_on_noise_free_data():
    mp = sio.make_map(3, 10, mono=True)
    r = iom.optimize(mp, iom.default_params(0, mono=True, priorG=0, priorA=0), np.float64)
    T = mp["truth"]
    # bounds: the residual errors measured on this case (scale 2e-9 relative, angle 5e-6 deg, bg 1.1e-9, ba 9.6e-7, velocities 1.7e-8), x 10
    assert abs(r["glob"][9] / T["scale"] - 1) <= 2e-8
    assert _angle(r["glob"][0:9], T["Rwg"]) <= 5e-5
    assert np.abs(r["glob"][10:13] - T["bg"]).max() <= 1.1e-8 and np.abs(r["glob"][13:16] - T["ba"]).max() <= 1e-5
    assert np.abs(r["kf"][:, 12:15] - T["vel"]).max() <= 2e-7
    assert r["chi_last"] <= 1e-6 * r["chi_first"]


def test_overload_d_recovers_scale_and_direction():
    mp = sio.refine_start(sio.make_map(5, 12, mono=True, scale_true=1.0), 15.0, 1.4)
    r = iom.optimize(mp, iom.default_params(3), np.float64)
    T = mp["truth"]
    # measured: scale error 2e-13 relative, angle 0 deg (below arccos' resolution) after the 10 Gauss-Newton iterations
    assert r["reason"] == iom.END_ITERATIONS and r["iterations"] == 10
    assert abs(r["glob"][9] / T["scale"] - 1) <= 1e-9 and _angle(r["glob"][0:9], T["Rwg"]) <= 1e-5


def test_float64_and_extended_precision_decide_alike_over_the_decisive_prefix():
    for c in ic.FULL_CASES:
        mp, r64, rld = ic.model_runs(c[0], c[1], c[2], None, ())
        pre = iom.decisive_prefix(rld["trace"])
        assert pre >= 5, (c, pre)
        for it in range(pre):
            assert r64["trace"][it]["accepted"] == rld["trace"][it]["accepted"], (c, it)


def test_fixed_and_unconnected_unknowns_stay_bit_identical():
    mp = ic.make("a_mono_prior", 10, 3, (5,))
    mp["link"][9] = 0                                       # keyframe 9 has no edge at all
    mp["kf"][9, 12:15] = [0.125, -0.25, 0.5]
    r = iom.optimize(mp, ic.params("a_mono_prior"), np.float64)
    assert r["kf"][9, 12:15].tobytes() == mp["kf"][9, 12:15].tobytes()
    assert np.abs(r["kf"][:9, 12:15] - mp["kf"][:9, 12:15]).max() > 0              # both sides of the gap moved
    rf = iom.optimize(mp, ic.params("a_fixed"), np.float64)
    assert rf["kf"].tobytes() == np.asarray(mp["kf"], np.float64).tobytes() and rf["glob"][10:16].tobytes() == mp["glob"][10:16].tobytes()
    assert rf["glob"][0:10].tobytes() != mp["glob"][0:10].tobytes()
    rb = iom.optimize(ic.make("b", 8, 3), ic.params("b"), np.float64)
    assert rb["glob"][0:10].tobytes() == ic.make("b", 8, 3)["glob"][0:10].tobytes()
