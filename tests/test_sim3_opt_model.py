"""Keeps the OptimizeSim3 model (tests/sim3_opt_model.py) honest on the CPU: its analytic Jacobian against finite differences, convergence
on noise-free data, g2o's numerical Jacobian against the analytic one over a committed seed set, and the two preconditions the GPU
comparison (tests/test_gpu_sim3_opt.py) rests on."""
import numpy as np
import pytest

import sim3_opt_model as m
import synth_sim3 as s

# Largest distance in (q, t, s) between solve(..., "numeric") -- the reference's 1e-9 central differences -- and solve(..., "analytic")
# over synth_sim3.NUMERIC_SET, as measured (printed by test_numeric_vs_analytic, recorded in DESIGN 4c): 1.15e-8.  The bound is 10x
# that; the margin covers seeds that are not in the set.
NUMERIC_VS_ANALYTIC_MEASURED = 1.15e-8
NUMERIC_VS_ANALYTIC_BOUND = 10 * NUMERIC_VS_ANALYTIC_MEASURED


def _random_state(r, fix_scale):
    S = m.sim3_exp(np.r_[r.normal(size=3) * 0.3, r.normal(size=3) * 0.5, 0.0 if fix_scale else r.uniform(-0.6, 0.6)])
    return S


@pytest.mark.parametrize("kb8", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_analytic_jacobian_matches_central_differences(kb8, fix_scale):
    """Both edge types, both cameras, random states; step 1e-6 on the SMOOTH projection (for KannalaBrandt8 the projection itself rounds
    theta and psi to float: at that step its differences are quantisation noise, which is why projectJac's formula is used)."""
    r = np.random.RandomState(11 + 2 * kb8 + fix_scale)
    worst = 0.0
    for trial in range(5):
        pb = s.make_pair(7000 + trial, n=30, kb8=kb8, fix_scale=fix_scale, exact=True)
        S = m.sim3_mul(_random_state(r, fix_scale), pb["sim3_true"]) if trial else pb["sim3"]
        S = m.sim3_mul(m.sim3_exp(np.r_[r.normal(size=3) * 0.05, r.normal(size=3) * 0.05, 0]), pb["sim3_true"]) if trial % 2 else S
        J12, J21 = m.jacobians_analytic(pb, S)

        def err(Sx):
            return (pb["obs1"] - m.project_smooth(pb["cam1"], m.sim3_map(Sx, pb["P2c"])),
                    pb["obs2"] - m.project_smooth(pb["cam2"], m.sim3_map(m.sim3_inverse(Sx), pb["P1c"])))
        h = 1e-6
        for d in range(7):
            u = np.zeros(7); u[d] = h
            a = err(m.oplus(pb, S, u.copy())); b = err(m.oplus(pb, S, -u))
            for J, ea, eb in ((J12, a[0], b[0]), (J21, a[1], b[1])):
                num = (ea - eb) / (2 * h)
                ok = np.all(np.isfinite(num), 1) & (np.abs(J[:, :, d]).max(1) < 1e6)       # points behind a camera project anywhere
                # central difference: truncation h^2 |f'''| + rounding eps |f| / h ~ 1e-16 * 1e3 px / 1e-6 = 1e-7 -> relative 1e-6 of |J|
                scale = 1.0 + np.abs(J[ok][:, :, d]).max()
                worst = max(worst, np.abs(num[ok] - J[ok][:, :, d]).max() / scale)
        if fix_scale:
            assert not J12[:, :, 6].any() and not J21[:, :, 6].any()
    print("analytic vs step-1e-6 central difference, worst relative deviation: %.3e" % worst)
    assert worst < 1e-6


@pytest.mark.parametrize("kb8", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_noise_free_data_returns_the_truth(kb8, fix_scale):
    """Exact inputs, no noise, no outliers.  Pinhole: the model ends at the true Sim3 to 1e-8 (ten near-Gauss-Newton iterations from a
    few degrees off converge quadratically; what is left is rounding).  KannalaBrandt8: the projection rounds theta to float (6e-8 rad,
    ~3e-5 px), which bounds the accuracy: 1e-6."""
    pb = s.make_pair(8000 + 2 * kb8 + fix_scale, n=80, kb8=kb8, fix_scale=fix_scale, noise=0.0, exact=True)
    out = m.solve(pb)
    assert out["n_in"] == 80 and out["n_bad"] == 0 and not out["flag"].any() and out["iters2"] == 5
    d = m.sim3_distance(out["sim3"], pb["sim3_true"])
    print("noise-free distance to the truth: %.3e" % d)
    assert d < (1e-6 if kb8 else 1e-8)


def test_numeric_vs_analytic():
    """The reference's numerical Jacobian (step 1e-9) against the analytic one the device uses.  Pinhole only: for KannalaBrandt8 the
    reference differentiates a projection that rounds theta and psi to float (KannalaBrandt8.cpp:52-69); with a 1e-9 step that derivative
    is quantisation noise (0 or +-1 float ulp / 2e-9), so there is nothing to compare with -- KB8 parity with the reference is unpinnable."""
    worst = 0.0
    for spec in s.NUMERIC_SET:
        pb = s.make_pair(**spec)
        a = m.solve(pb, "analytic"); b = m.solve(pb, "numeric")
        np.testing.assert_array_equal(a["flag"], b["flag"])
        assert (a["n_in"], a["n_corr"], a["n_bad"], a["iters2"]) == (b["n_in"], b["n_corr"], b["n_bad"], b["iters2"]), spec
        d = m.sim3_distance(a["sim3"], b["sim3"])
        print("numeric vs analytic %s: %.3e" % (spec, d))
        worst = max(worst, d)
    print("numeric vs analytic, largest distance in (q, t, s): %.3e (bound %.3e)" % (worst, NUMERIC_VS_ANALYTIC_BOUND))
    assert worst <= NUMERIC_VS_ANALYTIC_BOUND


@pytest.mark.parametrize("kb8", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_gpu_batch_preconditions(kb8, fix_scale):
    """What tests/test_gpu_sim3_opt.py relies on when it demands identical flags and 1e-9: on every committed GPU input no decisive chi2
    lies within a relative 1e-6 of th2, and a summation-order perturbation moves (q, t, s) by less than 1e-10 and no flag.  The
    perturbations are the rows reversed and five fixed random permutations (synth_sim3.summation_orders): near convergence a Pinhole
    problem's last LM steps are ~1e-9 long and whether one is taken hangs on the rounding of chi2, which one reordering alone does not
    always expose.  A seed that violates either is replaced (synth_sim3.BATCH_SEEDS, CLASS_SCENES), the bounds stay."""
    import sim3_golden_cases
    probs = s.gpu_batch(kb8, fix_scale)
    if not kb8 and not fix_scale:                          # the golden pairs and the class-method scenes ride along once
        probs = probs + sim3_golden_cases.cases() + [s.class_problem(s.make_keyframes(**spec))[0] for spec in s.CLASS_SCENES.values()]
    for k, pb in enumerate(probs):
        a = m.solve(pb)
        assert a["margin"] > 1e-6, (k, a["margin"])
        for order in s.summation_orders(len(pb["P1c"])):
            r = m.solve(pb, order=order)
            np.testing.assert_array_equal(a["flag"], r["flag"])
            assert (a["n_in"], a["n_bad"]) == (r["n_in"], r["n_bad"])
            d = m.sim3_distance(a["sim3"], r["sim3"])
            assert d < 1e-10, (k, d)


def test_sim3_exp_branches():
    """g2o::Sim3(Vector7d): each of the four branches is taken and agrees with exp(u / 2)^2.  The general branch does so to rounding;
    a branch below a 1e-5 threshold drops terms of first order in sigma or theta (C = 1 instead of 1 + sigma / 2 + ..., R = I + Omega +
    Omega^2), so it agrees to 1e-5 |upsilon| -- the reference's approximation, kept."""
    r = np.random.RandomState(5)
    for th, sg in ((3e-6, 3e-6), (3e-6, 0.2), (0.2, 3e-6), (0.2, 0.2)):
        ax = r.normal(size=3); ax /= np.linalg.norm(ax)
        u = np.r_[ax * th, r.normal(size=3), sg]
        E = m.sim3_exp(u)
        assert abs(E[7] - np.exp(sg)) < 1e-15
        H = m.sim3_exp(u / 2)
        tol = 1e-5 * max(1.0, np.linalg.norm(u[3:6])) if min(th, sg) < 1e-5 else 1e-12
        assert m.sim3_distance(E, m.sim3_mul(H, H)) < tol
