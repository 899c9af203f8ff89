"""HIP-vs-oracle parity of the local-BA solver (rows B1-B8) through the C ABI.
Tolerance (BASELINE.json north_star): RMSE <= 1e-4 on poses and points vs the CPU path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


@pytest.fixture(scope="module", params=["pairs", "mfma"])
def ba_ctx(request, gpu_ctx):
    """Both forms of the Schur complement: the per-block-pair kernels (k_ba_schur_rows / k_ba_schur_big, the default) on the session context and the
    FP64-MFMA panel GEMM (k_ba_schur_gemm, orbhip_ctx_set_ba_schur_mode(ctx, 2): what config #4 names and what the landmark-sharded
    mode runs) on a context of its own -- the mode is a property of the context, so the two never interfere."""
    import orbhip
    if request.param == "pairs":
        yield gpu_ctx
        return
    ctx = orbhip.Context(0)
    orbhip.ba_set_schur_mode(ctx, 2)
    yield ctx
    ctx.close()


def _check(gpu_ctx, graphs, params=None, tol=TOL):
    import orbhip
    import oracle_ba_bind as ob
    bb = orbhip.BaBatch(gpu_ctx, graphs)
    bb.solve(params)
    poses, points, outl, stats = bb.download()
    bb.close()
    op = None
    if params is not None:
        op = ob.default_params()
        for f, _ in ob.Params._fields_:
            setattr(op, f, getattr(params, f))
    for i, g in enumerate(graphs):
        rc, o_poses, o_pts, o_out, o_st, o_chi2, o_depth = ob.solve_with_gate_values(g, op)
        assert stats[i]["discarded"] == o_st["discarded"]
        if o_st["discarded"]:
            np.testing.assert_array_equal(poses[i], g["poses0"])
            continue
        assert _rmse(poses[i][:, 4:], o_poses[:, 4:]) <= tol, ("pose t", i, stats[i], o_st)
        assert _rmse(poses[i][:, :4], o_poses[:, :4]) <= tol, ("pose q", i)
        assert _rmse(points[i], o_pts) <= tol, ("points", i)
        assert stats[i]["iterations_run"] == o_st["iterations_run"], (stats[i], o_st)
        assert stats[i]["lm_trials"] == o_st["lm_trials"], (stats[i], o_st)
        assert abs(stats[i]["chi2_initial"] - o_st["chi2_initial"]) <= 1e-6 * abs(o_st["chi2_initial"])
        assert abs(stats[i]["chi2_final"] - o_st["chi2_final"]) <= 1e-6 * abs(o_st["chi2_final"])
        # outlier flags may differ only for edges whose chi2 / depth sits numerically ON the gate: the two solves agree to ~1e-9 in
        # the estimates (asserted per LM tick, against an extended-precision model, in test_gpu_ba_step.py: the measured figures are
        # in its docstring), i.e. to ~f/z * 1e-9 px in a residual and ~1e-6 relative in a chi2 near the gate (the same bound the
        # total chi2 is held to above); every other flag must agree
        prm = op if op is not None else ob.default_params()
        gm = prm.gate_mono2 if prm.gate_mono2 > 0 else prm.huber_mono2
        gs = prm.gate_stereo2 if prm.gate_stereo2 > 0 else prm.huber_stereo2
        gate = np.where(np.asarray(g["edge_stereo"]) == 1, gs, gm)
        on_gate = (np.abs(o_chi2 - gate) <= 1e-6 * gate) | (np.abs(o_depth) <= 1e-7)
        diff = outl[i] != o_out
        assert not np.any(diff & ~on_gate), ("outlier flags", i, np.flatnonzero(diff & ~on_gate)[:8], o_chi2[diff & ~on_gate][:8])
    return stats


def test_ba_small_mono(ba_ctx):
    gpu_ctx = ba_ctx
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=s) for s in range(4)]
    _check(gpu_ctx, graphs)


def test_ba_full_size_mono(ba_ctx):
    gpu_ctx = ba_ctx
    """BASELINE config #4: 50 KF x 2000 points x 10 obs, 2 fixed KFs, 5 % outliers."""
    import synth_ba
    graphs = [synth_ba.make_graph(seed=s) for s in (1, 2)]
    st = _check(gpu_ctx, graphs)
    assert all(s["iterations_run"][0] == 5 for s in st)


def test_ba_stereo_and_mixed(ba_ctx):
    gpu_ctx = ba_ctx
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=7, stereo_frac=1.0),
              synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=8, stereo_frac=0.4)]
    _check(gpu_ctx, graphs)


def _two_pinholes():
    return [dict(fx=458.0, fy=458.0, cx=320.0, cy=240.0, bf=458.0 * 0.11, stereo_frac=0.3),
            dict(fx=380.0, fy=395.0, cx=300.0, cy=255.0, bf=380.0 * 0.07, stereo_frac=0.3)]


def test_ba_per_keyframe_calibration_two_pinholes(ba_ctx):
    """the reference gives every edge its keyframe's own camera (Optimizer.cc:1961, :1990-1994).  One window whose
    keyframes alternate between two Pinhole calibrations (mono and stereo edges), in a batch with a single-calibration graph: within
    1e-4 of the oracle with the same LM trials; solving it with camera 0 for everybody must NOT agree (the table is really used)."""
    gpu_ctx = ba_ctx
    import synth_ba
    cams = _two_pinholes()
    g = synth_ba.make_graph(n_kf=14, n_pts=400, obs=6, seed=21, cameras=cams, pose_camera=[i % 2 for i in range(14)])
    g1 = synth_ba.make_graph(n_kf=9, n_pts=120, obs=5, seed=22)
    st = _check(gpu_ctx, [g, g1])
    assert st[0]["chi2_final"] < 0.5 * st[0]["chi2_initial"]
    import orbhip
    wrong = dict(g); wrong.pop("cameras"); wrong.pop("pose_camera")
    bb = orbhip.BaBatch(gpu_ctx, [wrong]); bb.solve(); _, _, _, sw = bb.download(); bb.close()
    assert sw[0]["chi2_final"] > 1.5 * st[0]["chi2_final"]


def test_ba_per_keyframe_calibration_pinhole_and_fisheye_rig(ba_ctx):
    """A window that mixes a Pinhole keyframe set with keyframes of a KannalaBrandt8 two-camera rig (their own mTrl / mpCamera2,
    Optimizer.cc:2021-2023): monocular KB8 edges, second-camera edges with twin chains, and Pinhole mono / stereo edges in ONE graph."""
    gpu_ctx = ba_ctx
    import synth_ba
    kb = (-0.0034, 0.0007, -0.002, 0.0002)
    q = np.array([0.0, 0.02, 0.0, 1.0]); q /= np.linalg.norm(q)
    rig = dict(Trl=(q[0], q[1], q[2], q[3], -0.1, 0.0, 0.0), cam=(190.0, 190.0, 254.0, 256.0), kb=(0.003, 0.0009, -0.002, 0.0003))
    cams = [dict(fx=458.0, fy=458.0, cx=320.0, cy=240.0, bf=458.0 * 0.11, stereo_frac=0.5),
            dict(fx=190.9, fy=190.3, cx=254.9, cy=256.8, bf=0.0, kb=kb, rig2=rig)]
    g = synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=23, cameras=cams, pose_camera=[0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0], right_frac=0.5)
    assert (g["edge_stereo"] == 2).sum() > 100 and (g["edge_stereo"] == 1).sum() > 100
    _check(gpu_ctx, [g])


def test_ba_ragged_batch(ba_ctx):
    gpu_ctx = ba_ctx
    """Graphs of different sizes in one batch, incl. a point seen only by fixed KFs."""
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=5, n_pts=30, obs=3, seed=11),
              synth_ba.make_graph(n_kf=20, n_pts=500, obs=8, seed=12),
              synth_ba.make_graph(n_kf=9, n_pts=77, obs=5, seed=13, n_fixed=3)]
    g = graphs[2]
    keep = ~((g["edge_point"] == 5) & (g["pose_fixed"][g["edge_pose"]] == 0))     # point 5: fixed-KF edges only
    for k in ("edge_pose", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        g[k] = g[k][keep]
    g["n_edges"] = int(keep.sum())
    _check(gpu_ctx, graphs)


@pytest.mark.parametrize("rows", [1, 0])
def test_ba_batches_of_eight_and_more_both_pair_kernels(gpu_ctx, rows, monkeypatch):
    """From 8 windows per call on the pair lists run four pairs per wave: k_ba_schur_rows (one workgroup per row of the block matrix,
    pose i's W D^-1 in LDS; the default) or, with ORBHIP_BA_SCHUR_ROWS=0 and for rows of more than 1024 blocks, k_ba_schur_big<16>.
    A ragged batch (different sizes, stereo, a point seen by fixed keyframes only, a window without a free keyframe, a window of
    the full bench size) against the oracle through both."""
    import synth_ba
    monkeypatch.setenv("ORBHIP_BA_SCHUR_ROWS", str(rows))
    graphs = [synth_ba.make_graph(n_kf=5, n_pts=30, obs=3, seed=211),
              synth_ba.make_graph(n_kf=20, n_pts=500, obs=8, seed=212),
              synth_ba.make_graph(n_kf=9, n_pts=77, obs=5, seed=213, n_fixed=3),
              synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=214, stereo_frac=1.0),
              synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=215, stereo_frac=0.4),
              synth_ba.make_graph(n_kf=4, n_pts=50, obs=3, seed=216, n_fixed=4),
              synth_ba.make_graph(seed=217),
              synth_ba.make_graph(n_kf=30, n_pts=900, obs=12, seed=218),
              synth_ba.make_graph(n_kf=4, n_pts=25, obs=3, seed=219, n_fixed=2),
              synth_ba.make_graph(n_kf=40, n_pts=700, obs=25, seed=220)]
    g = graphs[2]
    # one point keeps its fixed-keyframe edges only; it must keep two of them (a single mono edge leaves Hll singular, and what a
    # solver makes of that is rounding noise -- g2o's included)
    fixed_e = g["pose_fixed"][g["edge_pose"]] != 0
    nfix = np.bincount(g["edge_point"], weights=fixed_e, minlength=g["n_points"])
    nfree = np.bincount(g["edge_point"], weights=~fixed_e, minlength=g["n_points"])
    pt = int(np.flatnonzero((nfix >= 2) & (nfree >= 1))[0])
    keep = ~((g["edge_point"] == pt) & ~fixed_e)
    for k in ("edge_pose", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        g[k] = g[k][keep]
    g["n_edges"] = int(keep.sum())
    _check(gpu_ctx, graphs)


def test_ba_row_kernel_falls_back_when_a_row_exceeds_its_lds(gpu_ctx):
    """A keyframe that observes more than 1024 landmarks: its W D^-1 blocks do not fit the row kernel's LDS, the whole batch takes
    k_ba_schur_big<16>."""
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=4, n_pts=1300, obs=4, seed=230 + k) for k in range(8)]
    assert max(np.bincount(g["edge_pose"]).max() for g in graphs) > 1024
    _check(gpu_ctx, graphs)


def test_ba_all_keyframes_fixed(ba_ctx):
    """No free keyframe at all (the map-merge LBA as the reference writes it puts edges on the FIXED keyframes only, Optimizer.cc:6292 /
    :6424): no reduced system, the points are refined against fixed poses.  Next to a normal graph in the same batch."""
    import orbhip
    import synth_ba
    gpu_ctx = ba_ctx
    import oracle_ba_bind as ob
    g = synth_ba.make_graph(n_kf=8, n_pts=150, obs=6, seed=5, stereo_frac=0.3, outlier_frac=0.03, pose_noise=(0.0003, 0.001))
    g["pose_fixed"] = np.ones(8, np.uint8)
    prm = ob.merge_params(); prm.iters2 = 0                               # premise of the merge parity (see test_ba_merge_variant): >= 2 edges per point survive
    out1 = ob.solve(g, prm)[3]
    assert np.bincount(g["edge_point"][out1 == 0], minlength=g["n_points"]).min() >= 2
    st = _check(gpu_ctx, [g], orbhip.ba_merge_params())
    assert st[0]["chi2_final"] < st[0]["chi2_initial"] and not st[0]["discarded"]
    st = _check(gpu_ctx, [g, synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=6)])
    assert not st[0]["discarded"]


def test_ba_discards_when_mostly_outliers(ba_ctx):
    gpu_ctx = ba_ctx
    import synth_ba
    g = synth_ba.make_graph(n_kf=8, n_pts=120, obs=5, seed=21, outlier_frac=0.9)
    st = _check(gpu_ctx, [g])
    assert st[0]["discarded"] == 1


def test_ba_inertial_lambda_and_short_schedule(ba_ctx):
    gpu_ctx = ba_ctx
    """user lambda init = 100 (pMap->IsInertial(), Optimizer.cc:1837-1838) and a 2+3 schedule."""
    import orbhip
    import synth_ba
    p = orbhip.ba_default_params()
    p.user_lambda_init = 100.0
    p.iters1, p.iters2 = 2, 3
    _check(gpu_ctx, [synth_ba.make_graph(n_kf=10, n_pts=200, obs=6, seed=31)], p)


def test_ba_abort_flag(gpu_ctx):
    import orbhip
    import synth_ba
    g = synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=3)
    bb = orbhip.BaBatch(gpu_ctx, [g])
    flag = np.ones(1, np.uint8)
    assert bb.solve(abort=flag) == orbhip.E_ABORTED       # Optimizer.cc:2041-2043: return before optimizing
    bb.close()


def test_ba_convenience_entry_point(gpu_ctx):
    """orbhip_ba_solve_batch == create + solve + download."""
    import ctypes as C
    import orbhip
    import synth_ba
    g = synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=5)
    bb = orbhip.BaBatch(gpu_ctx, [g])
    bb.solve()
    poses, points, outl, stats = bb.download()
    bb.close()
    bb2 = orbhip.BaBatch(gpu_ctx, [g])          # only to reuse the struct packing
    arr = (orbhip.BaGraph * 1)()
    k = bb2._keep[0]
    arr[0] = orbhip.BaGraph(g["n_poses"], g["n_points"], g["n_edges"], *[a.ctypes.data for a in k],
                            g["fx"], g["fy"], g["cx"], g["cy"], g["bf"])
    P = g["poses0"].copy(); X = g["points0"].copy()
    pp = (C.c_void_p * 1)(P.ctypes.data); px = (C.c_void_p * 1)(X.ctypes.data)
    prm = orbhip.ba_default_params()
    rc = orbhip.lib.orbhip_ba_solve_batch(gpu_ctx.h, C.cast(arr, C.c_void_p), 1, C.byref(prm), None,
                                          C.cast(pp, C.c_void_p), C.cast(px, C.c_void_p), None, None)
    assert rc == 0
    np.testing.assert_array_equal(P, poses[0])
    np.testing.assert_array_equal(X, points[0])
    bb2.close()


def test_ba_merge_variant(ba_ctx):
    gpu_ctx = ba_ctx
    """Map-merge local BA (Optimizer.cc:6255-6800): first-pass outliers excluded, robust kernel dropped for the
    second pass, Huber 5.99 / gate 5.991, no bail-out.  Parity is asserted on graphs where every point keeps >= 2
    observations after the exclusion; a point left with ONE monocular edge makes Hll + lambda*I (lambda ~ 1e-44)
    numerically singular in g2o as well, and what follows (inf/NaN in the Schur complement, failed solve
    'accepted' through a negative computeScale) depends on the operation order -- only sanity is checked there."""
    import orbhip
    import oracle_ba_bind as ob
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=20, n_pts=300, obs=10, seed=41, outlier_frac=0.03),
              synth_ba.make_graph(n_kf=24, n_pts=400, obs=12, seed=42, outlier_frac=0.05, stereo_frac=0.5)]
    for g in graphs:                                                     # guard the premise of the parity claim
        prm = ob.merge_params(); prm.iters2 = 0
        out1 = ob.solve(g, prm)[3]                                        # first-pass classification == the exclusion set
        kept = np.bincount(g["edge_point"][out1 == 0], minlength=g["n_points"])
        assert kept[np.bincount(g["edge_point"], minlength=g["n_points"]) > 0].min() >= 2
    st = _check(gpu_ctx, graphs, orbhip.ba_merge_params())
    st_default = _check(gpu_ctx, graphs)
    assert st[0]["chi2_final"] != st_default[0]["chi2_final"]            # it is a different optimisation
    # mostly-outlier graph: the tracking LBA discards it, the merge variant never does; no hang, flags produced
    gbad = synth_ba.make_graph(n_kf=8, n_pts=120, obs=5, seed=43, outlier_frac=0.9)
    bb = orbhip.BaBatch(gpu_ctx, [gbad])
    bb.solve(orbhip.ba_merge_params())
    _, _, outl, stats = bb.download()
    bb.close()
    assert stats[0]["discarded"] == 0 and outl[0].sum() > 0.5 * len(outl[0])


def test_ba_kannala_brandt_camera(ba_ctx):
    gpu_ctx = ba_ctx
    """Monocular edges through KannalaBrandt8 (rows B2 / B3: KannalaBrandt8.cpp:52-69 project, :166-195 projectJac)."""
    import synth_ba
    kb = (-0.0034, 0.0007, -0.0021, 0.0002)
    graphs = [synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=71, kb8=kb),
              synth_ba.make_graph(n_kf=10, n_pts=200, obs=5, seed=72, kb8=kb, stereo_frac=0.3)]   # stereo edges stay pinhole (types_six_dof_expmap)
    _check(gpu_ctx, graphs)


def test_ba_second_camera_tobody_edges(ba_ctx):
    gpu_ctx = ba_ctx
    """EdgeSE3ProjectXYZToBody (rows B2 / B3): observations in the second camera of a rigid fisheye pair (mTrl, mpCamera2),
    mixed with left-camera KannalaBrandt8 edges; plus a pinhole second camera."""
    import orbhip
    import synth_ba
    kb = (-0.0034, 0.0007, -0.0021, 0.0002)
    rig = dict(Trl=(0.004, -0.012, 0.002, 0.99991, -0.101, 0.0007, 0.0012), cam=(190.4, 190.6, 252.7, 255.0), kb=(0.0031, 0.0007, -0.0019, 0.0003))
    rig_pin = dict(Trl=(0.0, 0.01, 0.0, 0.99995, -0.11, 0.0, 0.0), cam=(458.0, 458.0, 320.0, 240.0), kb=None)
    graphs = [synth_ba.make_graph(n_kf=12, n_pts=300, obs=6, seed=91, kb8=kb, rig2=rig),
              synth_ba.make_graph(n_kf=10, n_pts=200, obs=5, seed=92, rig2=rig_pin, right_frac=0.8)]
    assert all((g["edge_stereo"] == 2).sum() > 300 for g in graphs)
    _check(gpu_ctx, graphs)
    _check(gpu_ctx, graphs[:1], orbhip.ba_merge_params())         # depth gate of the level-1 classification uses the right camera's z
    # type-2 edges without a rig are rejected
    bad = dict(graphs[0]); bad["rig2"] = None
    with pytest.raises(orbhip.OrbHipError):
        orbhip.BaBatch(gpu_ctx, [bad])


def test_ba_large_window_and_dense_observations(ba_ctx):
    gpu_ctx = ba_ctx
    """Corner shapes of BOTH Schur kernels (ba_ctx): 70 free keyframes (ld = 480 -- MFMA form: 5 points per LDS stage, 165 tile
    chunks = three workgroups per point range; pair form: 2485 pair lists), points seen by almost every keyframe (MFMA form: stages cut
    by the 85-block limit, not by the point count; pair form: lists as long as the point count), next to a small graph."""
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=72, n_pts=500, obs=12, seed=51),
              synth_ba.make_graph(n_kf=40, n_pts=90, obs=37, seed=52, outlier_frac=0.02),
              synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=53)]
    stats = _check(gpu_ctx, graphs)
    assert not any(s["discarded"] for s in stats)


def _solve_sharded_in_process(device, graphs, world, params=None, abort_rank=None):
    """`world` ranks as threads of this process (own context / stream / batch / exchange buffer each, one GPU): the exchange
    callback is an all-gather between the threads' buffers.  The solver code path is the multi-process one."""
    import threading
    import torch
    import orbhip
    ctxs = [orbhip.Context(device) for _ in range(world)]
    bbs = [orbhip.BaBatch(ctxs[r], graphs, rank=r, world=world) for r in range(world)]
    stride = bbs[0].exchange_doubles
    assert all(b.exchange_doubles == stride for b in bbs)
    bufs = [torch.zeros(world * stride, dtype=torch.float64, device="cuda") for _ in range(world)]
    for r in range(world):
        bbs[r].set_exchange_buffer(bufs[r].data_ptr(), world * stride)
    torch.cuda.synchronize()
    bar = threading.Barrier(world)
    stages = [[] for _ in range(world)]
    errs = []

    def make_exchange(r):
        def exchange(stage, count):
            stages[r].append(stage)
            bar.wait(timeout=60)
            for o in range(world):
                if o != r:
                    bufs[o][r * stride: r * stride + count].copy_(bufs[r][r * stride: r * stride + count])
            torch.cuda.synchronize()
            bar.wait(timeout=60)
        return exchange

    def run(r):
        try:
            ab = None
            if abort_rank is not None:
                ab = np.zeros(1, np.uint8)
                ab[0] = 1 if r == abort_rank else 0
            bbs[r].solve_sharded(make_exchange(r), params, ab)
        except BaseException as e:
            errs.append(e)
            bar.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errs, errs
    outs = [b.download() for b in bbs]
    for b in bbs:
        b.close()
    for c in ctxs:
        c.close()
    return outs, stages


@pytest.mark.parametrize("world", [2, 3])
def test_ba_landmark_sharded_matches_single_rank(gpu_ctx, world):
    """SURVEY 8e optional mode: points sharded over `world` ranks, Schur block all-gathered every trial.  Every rank must report
    the same stats and poses; points / outlier flags of the ranks tile the full arrays; result == the unsharded GPU solve and the
    oracle within the BA tolerance."""
    import orbhip
    import oracle_ba_bind as ob
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=14, n_pts=310, obs=7, seed=61, stereo_frac=0.3),
              synth_ba.make_graph(n_kf=8, n_pts=101, obs=5, seed=62)]
    outs, stages = _solve_sharded_in_process(0, graphs, world)
    assert all(st == stages[0] for st in stages) and stages[0][-1] == 4 and stages[0].count(2) == stages[0].count(3)
    bb = orbhip.BaBatch(gpu_ctx, graphs)
    bb.solve()
    poses1, points1, outl1, stats1 = bb.download()
    bb.close()
    for i, g in enumerate(graphs):
        L, E = g["n_points"], g["n_edges"]
        pts = np.array(g["points0"], np.float64).copy(); out = np.zeros(E, np.uint8)
        for r in range(world):
            poses_r, points_r, outl_r, stats_r = outs[r]
            assert stats_r[i] == outs[0][3][i], (r, stats_r[i], outs[0][3][i])
            np.testing.assert_array_equal(poses_r[i], outs[0][0][i])
            p0, p1 = r * L // world, (r + 1) * L // world
            pts[p0:p1] = points_r[i][p0:p1]
            e_sel = (g["edge_point"] >= p0) & (g["edge_point"] < p1)
            out[e_sel] = outl_r[i][e_sel]
        st = outs[0][3][i]
        assert st["iterations_run"] == stats1[i]["iterations_run"] and st["lm_trials"] == stats1[i]["lm_trials"], (st, stats1[i])
        assert _rmse(outs[0][0][i], poses1[i]) < 1e-9 and _rmse(pts, points1[i]) < 1e-9
        assert st["n_outliers"] == stats1[i]["n_outliers"] and int(np.sum(out != outl1[i])) == 0
        rc, o_poses, o_pts, o_out, o_st = ob.solve(g, None)
        assert _rmse(outs[0][0][i][:, 4:], o_poses[:, 4:]) <= TOL and _rmse(pts, o_pts) <= TOL


def test_ba_landmark_sharded_abort_and_discard(gpu_ctx):
    """The abort flag of ONE rank stops every rank at the same trial; the >= 50 % outlier rule uses the counts of all ranks."""
    import synth_ba
    g = synth_ba.make_graph(n_kf=8, n_pts=120, obs=5, seed=21, outlier_frac=0.9)
    outs, stages = _solve_sharded_in_process(0, [g], 2)
    assert all(o[3][0]["discarded"] == 1 for o in outs)
    for o in outs:
        np.testing.assert_array_equal(o[0][0], g["poses0"])
    g2 = synth_ba.make_graph(n_kf=6, n_pts=40, obs=4, seed=3)
    outs, stages = _solve_sharded_in_process(0, [g2], 2, abort_rank=1)
    assert stages[0] == stages[1] and stages[0].count(3) == 1            # one trial, then both ranks stop
    assert outs[0][3][0] == outs[1][3][0]


_SHARD_WORKER = r"""
import os, sys, json
sys.path.insert(0, os.path.join(ROOT, "orb-slam3-mac_amd", "python"))
import numpy as np, torch, torch.distributed as dist
import orbhip, shard, synth_ba
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(0)
graphs = [synth_ba.make_graph(n_kf=12, n_pts=240, obs=6, seed=81), synth_ba.make_graph(n_kf=7, n_pts=90, obs=4, seed=82)]
ctx = orbhip.Context(0)
bb = orbhip.BaBatch(ctx, graphs, rank=rank, world=world)
stride = bb.exchange_doubles
xbuf = torch.zeros(world * stride, dtype=torch.float64, device="cuda")
bb.set_exchange_buffer(xbuf.data_ptr(), world * stride)
bb.solve_sharded(shard.make_ba_exchange(xbuf, stride))
poses, points, outl, stats = bb.download()
# the points of the other ranks: one all-gather of the owned slices
full = []
for i, g in enumerate(graphs):
    L = g["n_points"]
    parts = [None] * world
    dist.all_gather_object(parts, points[i][rank * L // world:(rank + 1) * L // world])
    full.append(np.concatenate(parts))
if rank == 0:
    single = orbhip.BaBatch(ctx, graphs); single.solve(); p1, q1, o1, s1 = single.download(); single.close()
    for i in range(len(graphs)):
        assert stats[i]["lm_trials"] == s1[i]["lm_trials"] and stats[i]["iterations_run"] == s1[i]["iterations_run"], (stats[i], s1[i])
        assert np.sqrt(np.mean((poses[i] - p1[i]) ** 2)) < 1e-9 and np.sqrt(np.mean((full[i] - q1[i]) ** 2)) < 1e-9
    print("SHARD_OK", json.dumps(stats[0]))
bb.close(); ctx.close()
dist.barrier()
dist.destroy_process_group()
"""


def test_ba_landmark_sharded_two_processes_torch_distributed(tmp_path):
    """Two processes (torch.distributed, gloo rendezvous on 127.0.0.1, both on this box's one GPU) run shard.make_ba_exchange --
    the code path the multi-GPU bench leg uses with backend nccl (= RCCL)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text("ROOT = %r\n" % root + _SHARD_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29621", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29621", str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=400)
    assert r.returncode == 0 and "SHARD_OK" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("robust", [True, False])
def test_ba_global_bundle_adjustment_params(gpu_ctx, robust):
    """Optimizer::BundleAdjustment (Optimizer.cc:62-330): one optimize(N) pass, only the first keyframe fixed, optional robust
    kernel, no outlier stage / bail-out -- the same solver under orbhip_ba_global_params, checked against the oracle."""
    import orbhip
    import oracle_ba_bind as ob
    import synth_ba
    # one fixed keyframe: stereo observations pin the scale, so the problem is well posed and trajectories must agree
    graphs = [synth_ba.make_graph(n_kf=25, n_pts=400, obs=8, seed=102, n_fixed=1, outlier_frac=0.04, stereo_frac=0.3),
              synth_ba.make_graph(n_kf=9, n_pts=150, obs=5, seed=103, n_fixed=1, outlier_frac=0.0, stereo_frac=1.0)]
    # monocular map initialisation (2 keyframes, one fixed): the scale is a free gauge, the reduced system is singular along it and
    # any two implementations wander differently along that direction -- only the cost is comparable
    ginit = synth_ba.make_graph(n_kf=2, n_pts=120, obs=2, seed=101, n_fixed=1, outlier_frac=0.0)
    p = orbhip.ba_global_params(20 if robust else 10, robust)
    bb = orbhip.BaBatch(gpu_ctx, graphs + [ginit])
    bb.solve(p)
    poses, points, outl, stats = bb.download()
    bb.close()
    for i, g in enumerate(graphs):
        rc, o_poses, o_pts, o_out, o_st = ob.solve(g, ob.global_params(20 if robust else 10, robust))
        assert stats[i]["discarded"] == 0 and o_st["discarded"] == 0
        assert stats[i]["iterations_run"] == o_st["iterations_run"] and stats[i]["iterations_run"][1] == 0, (stats[i], o_st)
        assert stats[i]["lm_trials"] == o_st["lm_trials"]
        assert _rmse(poses[i], o_poses) <= TOL and _rmse(points[i], o_pts) <= TOL
        assert abs(stats[i]["chi2_final"] - o_st["chi2_final"]) <= 1e-6 * abs(o_st["chi2_final"])
    rc, o_poses, o_pts, o_out, o_st = ob.solve(ginit, ob.global_params(20 if robust else 10, robust))
    st = stats[len(graphs)]
    assert st["discarded"] == 0 and st["iterations_run"][1] == 0
    assert np.isfinite(st["chi2_final"]) and st["chi2_final"] < st["chi2_initial"] and o_st["chi2_final"] < o_st["chi2_initial"]
    assert np.all(np.isfinite(poses[len(graphs)])) and np.all(np.isfinite(points[len(graphs)]))


def test_ba_golden_fixture_without_oracle(gpu_ctx):
    """The HIP solver against the committed vectors of tests/golden/ba_golden.npz (made by the oracle, tools/gen_golden.py) -- no
    live oracle involved: poses / points within 1e-4 RMSE (they agree to ~1e-9), identical outlier flags and LM counts."""
    import os
    import orbhip
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ba_golden.npz"))
    g = {k[2:]: gold[k] for k in gold.files if k.startswith("g_")}
    for k in ("n_poses", "n_points", "n_edges"):
        g[k] = int(g[k])
    for k in ("fx", "fy", "cx", "cy", "bf"):
        g[k] = float(g[k])
    bb = orbhip.BaBatch(gpu_ctx, [g])
    bb.solve()
    poses, points, outl, stats = bb.download()
    bb.close()
    assert _rmse(poses[0], gold["poses"]) <= TOL and _rmse(points[0], gold["points"]) <= TOL
    assert _rmse(poses[0], gold["poses"]) <= 1e-7, "closer than the tolerance in practice: a drift worth looking at"
    np.testing.assert_array_equal(outl[0], gold["outlier"])
    assert stats[0]["iterations_run"] == gold["iterations_run"].tolist() and stats[0]["lm_trials"] == int(gold["lm_trials"])


@pytest.mark.parametrize("n_kf,n_pts", [(122, 2500), (202, 3000)])
def test_ba_more_than_80_free_keyframes(gpu_ctx, n_kf, n_pts):
    """The reference takes every covisible keyframe into the window (Optimizer.cc:1703-1819; the merge variant two whole
    neighbourhoods): 120 and 200 free keyframes -- a reduced system of 720 / 1200 unknowns, built per 6x6 block and factored by
    the global-memory blocked LDL^T -- against the oracle; a smaller window in the same batch takes the same path."""
    import synth_ba
    graphs = [synth_ba.make_graph(n_kf=n_kf, n_pts=n_pts, obs=10, seed=300 + n_kf),
              synth_ba.make_graph(n_kf=9, n_pts=120, obs=5, seed=301 + n_kf)]
    st = _check(gpu_ctx, graphs)
    assert st[0]["iterations_run"][0] == 5


def test_ba_rejected_graph_reports_through_last_error(gpu_ctx):
    """A graph the host-side checks reject comes back as ORBHIP_E_BADARG with its reason in orbhip_last_error() (the BA messages used
    to go to a string of their own that nothing read).  2 poses, 4 points, edge_stereo[0] = 3; no kernel is launched."""
    import orbhip
    import synth_ba
    g = dict(synth_ba.make_graph(n_kf=2, n_pts=4, obs=2, seed=11, n_fixed=1, outlier_frac=0.0))
    assert (g["n_poses"], g["n_points"]) == (2, 4) and g["n_edges"] > 0
    g["edge_stereo"] = np.array(g["edge_stereo"], np.uint8).copy()
    g["edge_stereo"][0] = 3
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.BaBatch(gpu_ctx, [g])
    assert ei.value.code == orbhip.E_BADARG
    assert "edge_stereo" in orbhip.lib.orbhip_last_error().decode()


def test_pose_optimization_rejected_call_reports_through_last_error(gpu_ctx):
    """orbhip_pose_optimization_device with per-edge second-camera flags (d_right) but no second camera (cam2 == NULL):
    ORBHIP_E_BADARG, the message names cam2; no kernel is launched."""
    import torch
    import orbhip
    F, M = 1, 4
    Xw = torch.zeros((F, M, 3), dtype=torch.float64, device="cuda"); obs = torch.zeros((F, M, 3), dtype=torch.float64, device="cuda")
    w = torch.ones((F, M), dtype=torch.float64, device="cuda"); n = torch.full((F,), M, dtype=torch.int32, device="cuda")
    pose = torch.tensor([[0, 0, 0, 1, 0, 0, 0]], dtype=torch.float64, device="cuda")
    right = torch.zeros((F, M), dtype=torch.uint8, device="cuda")
    out = torch.zeros((F, M), dtype=torch.uint8, device="cuda"); ninl = torch.zeros((F,), dtype=torch.int32, device="cuda")
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.pose_optimization_device(gpu_ctx, Xw.data_ptr(), obs.data_ptr(), w.data_ptr(), n.data_ptr(), F, M, (458.0, 458.0, 320.0, 240.0, 50.0),
                                        pose.data_ptr(), out.data_ptr(), ninl.data_ptr(), rig2=None, d_right=right.data_ptr())
    assert ei.value.code == orbhip.E_BADARG
    assert "cam2" in orbhip.lib.orbhip_last_error().decode()
