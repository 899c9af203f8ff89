"""Device batch of the inertial pose-only optimisations (orbhip_pose_inertial_optimization_device / _host) against the CPU model
(tests/pose_inertial_model.py): identical outlier flags, return values, rounds and GN iterations; state within 1e-8; the new prior's
H within 1e-6 (relative Frobenius); a second run byte-identical."""
import numpy as np
import pytest
import pose_inertial_model as pm
import synth_pose_inertial as sp

pytestmark = pytest.mark.gpu


def _run(ctx, frames, kind, mode, rec_init, max_edges=None):
    import torch
    import orbhip
    F = len(frames)
    n = np.array([len(fr["Xw"]) for fr in frames], np.int32)
    M = max(int(n.max()) if F else 1, 1) if max_edges is None else max_edges
    Xw = np.zeros((F, M, 3)); obs = np.zeros((F, M, 3)); is2 = np.zeros((F, M)); knd = np.zeros((F, M), np.uint8)
    cl = np.zeros((F, M), np.uint8)
    for f, fr in enumerate(frames):
        k = n[f]
        Xw[f, :k] = fr["Xw"]; obs[f, :k] = fr["obs"]; is2[f, :k] = fr["inv_sigma2"]; knd[f, :k] = fr["kind"]; cl[f, :k] = fr["close"]
    st = lambda key: np.stack([np.asarray(fr[key], np.float64).reshape(-1) for fr in frames])
    prior = np.stack([np.concatenate([fr["prior"], fr["prior_H"]]) for fr in frames]) if mode == 1 else None
    arrs = [Xw, obs, is2, knd, cl, n, st("prev"), st("preint"), st("info"), st("info_g"), st("info_a")]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
    tp = torch.from_numpy(prior).cuda() if prior is not None else None
    outs = []
    for _ in range(2):
        state = torch.from_numpy(st("state")).cuda()
        out = torch.full((F, M), 9, dtype=torch.uint8, device="cuda")
        ret = torch.full((F,), -9, dtype=torch.int32, device="cuda")
        H = torch.zeros((F, 225), dtype=torch.float64, device="cuda")
        stats = torch.full((F, 4), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        orbhip.pose_inertial_optimization_device(ctx, mode, rec_init, sp.rig(kind), F, M, *[x.data_ptr() for x in t],
                                                 None if tp is None else tp.data_ptr(), state.data_ptr(), out.data_ptr(),
                                                 ret.data_ptr(), H.data_ptr(), stats.data_ptr())
        ctx.synchronize()
        outs.append([a.cpu().numpy() for a in (state, out, ret, H, stats)])
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes(), "second run differs"
    return outs[0]


def _check(frames, kinds, mode, rec_init, res):
    state, out, ret, H, stats = res
    for f, fr in enumerate(frames):
        r = pm.solve(fr, sp.camera(kinds[f] if isinstance(kinds, list) else kinds), mode, rec_init)
        k = len(fr["Xw"])
        np.testing.assert_array_equal(out[f, :k].astype(bool), r["outlier"], err_msg="frame %d" % f)
        assert (out[f, k:] == 9).all()
        assert ret[f] == r["ret"], (f, ret[f], r["ret"])
        assert tuple(stats[f]) == (r["rounds"], r["iterations"], r["fails"], r["n_bad"]), (f, stats[f], r)
        np.testing.assert_allclose(state[f], r["state"], rtol=0, atol=1e-8)
        Hm = r["H"]
        assert np.linalg.norm(H[f].reshape(15, 15) - Hm) <= 1e-6 * np.linalg.norm(Hm), (f, np.linalg.norm(H[f].reshape(15, 15) - Hm))


@pytest.mark.parametrize("rec_init", [False, True])
@pytest.mark.parametrize("kind", ["mono", "stereo", "rig"])
@pytest.mark.parametrize("mode", [0, 1])
def test_device_batch_matches_the_model(gpu_ctx, mode, kind, rec_init):
    frames = [sp.make_frame(100 + 7 * i, kind, mode, n_points=[300, 120, 40, 25][i % 4])[0] for i in range(8)]
    _check(frames, kind, mode, rec_init, _run(gpu_ctx, frames, kind, mode, rec_init))


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_cases(gpu_ctx, mode):
    """0 visual edges (the < 10 edges break after round 1), a frame pushed into recovery (few edges, many outliers), close points and
    a point behind the camera (every synthetic frame holds one)."""
    frames = [sp.make_frame(200, "stereo", mode, n_points=0)[0], sp.make_frame(201, "mono", mode, n_points=4, n_close=2)[0],
              sp.make_frame(202, "mono", mode, n_points=35, outlier_frac=0.5, n_close=10)[0],
              sp.make_frame(203, "stereo", mode, n_points=60, n_close=30)[0]]
    res = _run(gpu_ctx, frames, "stereo", mode, False, max_edges=64)
    assert tuple(res[4][0][:2]) == (1, 10)
    assert pm.solve(frames[2], sp.camera("stereo"), mode)["recovered"]          # the recovery branch ran on frame 2
    _check(frames, "stereo", mode, False, res)


def test_ragged_batch_of_256_frames(gpu_ctx):
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 400, 256); sizes[:4] = [0, 2500, 1200, 7]
    for mode in (0, 1):
        frames = [sp.make_frame(300 + i, "stereo", mode, n_points=int(sizes[i]))[0] for i in range(256)]
        _check(frames, "stereo", mode, False, _run(gpu_ctx, frames, "stereo", mode, False))


def test_chain_of_frames(gpu_ctx):
    """One trajectory: LastKeyFrame on the first frame, then LastFrame on 24 more.  Frame i's preintegration spans the true states of
    frames i-1 and i; its previous state and prior are frame i-1's output (state and H), device and model each fed their own."""
    import orbhip
    rig = sp.rig("rig")
    cam = sp.camera("rig")
    fr, true = sp.make_frame(400, "rig", 0)
    st, out, ret, H, stats = orbhip.pose_inertial_optimization_host(gpu_ctx, 0, False, rig, fr)
    r = pm.solve(fr, cam, 0)
    np.testing.assert_array_equal(out.astype(bool), r["outlier"])
    np.testing.assert_allclose(st, r["state"], rtol=0, atol=1e-8)
    dev, mod = (st, H), (r["state"], r["H"])
    for i in range(1, 25):
        fr, true = sp.make_frame(400 + i, "rig", 1, prev_true=true)
        fd, fm = dict(fr), dict(fr)
        fd["prev"], fd["prior"], fd["prior_H"] = dev[0].copy(), dev[0].copy(), dev[1].reshape(-1).copy()
        fm["prev"], fm["prior"], fm["prior_H"] = mod[0].copy(), mod[0].copy(), mod[1].reshape(-1).copy()
        st, out, ret, H, stats = orbhip.pose_inertial_optimization_host(gpu_ctx, 1, False, rig, fd)
        r = pm.solve(fm, cam, 1)
        np.testing.assert_array_equal(out.astype(bool), r["outlier"], err_msg="frame %d" % i)
        assert ret == r["ret"] and tuple(stats) == (r["rounds"], r["iterations"], r["fails"], r["n_bad"]), i
        np.testing.assert_allclose(st, r["state"], rtol=0, atol=1e-8, err_msg="frame %d" % i)
        assert np.linalg.norm(H - r["H"]) <= 1e-6 * np.linalg.norm(r["H"]), i
        assert np.abs(st[9:12] - true[9:12]).max() < 0.05, i             # the chain tracks the trajectory
        dev, mod = (st, H), (r["state"], r["H"])


def test_host_form_rejects_a_right_camera_edge_without_a_second_camera(gpu_ctx):
    import orbhip
    fr, _ = sp.make_frame(500, "mono", 0, n_points=20)
    fr["kind"] = fr["kind"].copy(); fr["kind"][3] = 2
    with pytest.raises(orbhip.OrbHipError):
        orbhip.pose_inertial_optimization_host(gpu_ctx, 0, False, sp.rig("mono"), fr)
