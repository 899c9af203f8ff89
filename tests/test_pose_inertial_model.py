"""CPU checks of the inertial pose-only optimisation's model (tests/pose_inertial_model.py) against independent arithmetic, and of
the new C ABI's exports.  No GPU."""
import ctypes
import os
import numpy as np
import pytest
import oracle_iba_bind as oib
import pose_inertial_model as pm
import synth_pose_inertial as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_inertial_symbols_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "liborbhip.so"))
    for s in ("orbhip_pose_inertial_optimization_device", "orbhip_pose_inertial_optimization_host"):
        assert hasattr(lib, s), s


@pytest.mark.parametrize("kind", ["mono", "stereo", "rig"])
def test_visual_edges_match_the_oracle(kind):
    fr, _ = sp.make_frame(3, kind, 0, n_points=40, behind=False)
    cam = sp.camera(kind)
    err, _, Jp = pm.visual(cam, fr["state"], fr["Xw"], fr["obs"], fr["kind"])
    for i in range(len(fr["Xw"])):
        e, _, J = oib.edge_visual(cam, fr["state"], fr["Xw"][i], fr["obs"][i], int(fr["kind"][i]))
        np.testing.assert_allclose(err[i], e, rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(Jp[i], J, rtol=1e-10, atol=1e-8)


def _fd(fun, s, p, which, k, h=1e-6):
    """central difference of fun along unknown k of `which` ('s' or 'p') through ImuCamPose::Update / '+='"""
    dx = np.zeros(15); dx[k] = h
    if which == "s":
        return (fun(oib.kf_update(s, dx), p) - fun(oib.kf_update(s, -dx), p)) / (2 * h)
    return (fun(s, oib.kf_update(p, dx)) - fun(s, oib.kf_update(p, -dx))) / (2 * h)


def test_prior_edge_jacobian_by_finite_differences():
    fr, _ = sp.make_frame(4, "mono", 1)
    p = fr["prev"]
    _, J = pm.prior_edge(p, fr["prior"])
    for k in range(15):
        num = _fd(lambda s_, p_: pm.prior_edge(p_, fr["prior"], jac=False)[0], None, p, "p", k)
        np.testing.assert_allclose(J[:, k], num, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["mono", "stereo"])       # (KannalaBrandt8 projects through float angles: no finite differences)
def test_whole_residual_jacobian_by_finite_differences(mode, kind):
    """The normal equations' H, b equal J^T J, -J^T r of the whitened residual differentiated numerically (all edges, no kernel)."""
    fr, _ = sp.make_frame(5, kind, mode, n_points=30, behind=False)
    cam = sp.camera(kind)
    s, p = fr["state"], (fr["prev"] if mode == 1 else None)
    r = pm.residual(fr, cam, mode, s, p)
    nx = 15 if mode == 0 else 30
    J = np.zeros((len(r), nx))
    for k in range(nx):
        J[:, k] = _fd(lambda s_, p_: pm.residual(fr, cam, mode, s_, p_), s, p, "s" if k < 15 else "p", k % 15)
    H, b, _ = pm.normal_equations(fr, cam, mode, s, p, np.ones(len(fr["Xw"]), bool), robust_vis=False, robust_prior=False)
    Hn = J.T @ J
    assert np.linalg.norm(H - Hn) <= 2e-5 * np.linalg.norm(Hn)
    np.testing.assert_allclose(b, -J.T @ r, rtol=2e-5, atol=2e-5 * np.abs(J.T @ r).max())


def test_marginalize_is_the_schur_complement():
    rng = np.random.default_rng(6)
    A = rng.normal(0, 1, (30, 30))
    H = A @ A.T + 30 * np.eye(30)
    M = pm.marginalize(H, 0, 14)
    S = H[15:, 15:] - H[15:, :15] @ np.linalg.solve(H[:15, :15], H[:15, 15:])
    np.testing.assert_allclose(M[15:, 15:], S, rtol=1e-10, atol=1e-10)
    assert np.all(M[:15, :] == 0) and np.all(M[:, :15] == 0)
    M2 = pm.marginalize(H, 15, 29)                      # the kernel's ordering (current frame first)
    S2 = H[:15, :15] - H[:15, 15:] @ np.linalg.solve(H[15:, 15:], H[15:, :15])
    np.testing.assert_allclose(M2[:15, :15], S2, rtol=1e-10, atol=1e-10)


def test_constraint_pose_imu_is_psd_and_keeps_a_psd_input():
    rng = np.random.default_rng(7)
    A = rng.normal(0, 1, (15, 15))
    Hin = A @ A.T
    np.testing.assert_allclose(pm.constraint_pose_imu(Hin), Hin, rtol=0, atol=1e-12 * np.abs(Hin).max())
    Hind = A + A.T                                        # indefinite: the negative part is removed
    Hc = pm.constraint_pose_imu(Hind)
    assert np.linalg.eigvalsh(Hc).min() > -1e-12 * np.abs(Hc).max()
    np.testing.assert_allclose(pm.constraint_pose_imu(Hc), Hc, rtol=0, atol=1e-12 * np.abs(Hc).max())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_noise_free_frame_returns_the_true_state(mode, kind):
    fr, true = sp.make_frame(8, kind, mode, noise_free=True)
    r = pm.solve(fr, sp.camera(kind), mode)
    np.testing.assert_allclose(r["state"], true, rtol=0, atol=1e-9)
    assert not r["outlier"].any() and r["ret"] == len(fr["Xw"]) and r["rounds"] == 4 and r["iterations"] == 40


def test_few_edges_stop_after_the_first_round():
    fr, _ = sp.make_frame(9, "mono", 0, n_points=5, n_close=0, behind=False)
    r = pm.solve(fr, sp.camera("mono"), 0)
    assert r["rounds"] == 1 and r["iterations"] == 10


@pytest.mark.parametrize("mode", [0, 1])
def test_a_point_behind_the_camera_is_rejected_by_its_depth_alone(mode):
    """The mirrored map point projects to its observed pixel: its chi2 stays under the gate, only isDepthPositive makes it an outlier."""
    fr, _ = sp.make_frame(12, "mono", mode)
    j = fr["behind"]
    assert j >= 0
    r = pm.solve(fr, sp.camera("mono"), mode)
    assert r["outlier"][j] and not r["depth_ok"][j] and r["chi2"][j] < 5.991


def test_close_points_use_the_wider_gate():
    """Close edges with gate < chi2 <= 1.5 gate stay inliers; far edges in that band are outliers."""
    seen_close = seen_far = 0
    for seed in range(20, 40):
        fr, _ = sp.make_frame(seed, "mono", 1, n_close=150, outlier_frac=0.0)
        r = pm.solve(fr, sp.camera("mono"), 1)
        c32 = r["chi2"].astype(np.float32)
        band = (c32 > np.float32(5.991)) & (c32 <= np.float32(1.5 * float(np.float32(5.991)))) & r["depth_ok"]
        close = fr["close"].astype(bool)
        assert not r["outlier"][band & close].any() and r["outlier"][band & ~close].all()
        seen_close += int((band & close).sum()); seen_far += int((band & ~close).sum())
    assert seen_close > 0 and seen_far > 0
