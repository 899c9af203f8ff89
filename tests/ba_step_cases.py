"""The graphs of the one-tick BA tests (test_ba_step_model.py on the CPU, test_gpu_ba_step.py / test_gpu_iba_step.py on the device) and
their reference data: the extended-precision model's tick and the float64 oracle's result after the same tick, computed once per
process.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import ba_step_model as bm

# ---------------------------------------------------------------------------------------------- local BA
# free keyframes against the 32-column panels of ba_ldlt.h (n = 6 nf): a single partial panel, the exact multiples at 16 / 32 / 48 / 64 /
# 80 free keyframes, one past and one short of each; then the global-memory path (n = 486 is 15 panels + 6 columns)
SIZES_SMALL = [1, 2, 5, 6, 15, 16, 17, 31, 32, 33, 48, 63, 64, 79, 80]
SIZES_BIG = [81, 86, 122, 202]
BATCH_SIZES = [1, 7, 8, 9, 65]
SHIFT = np.array([1000.0, -2000.0, 500.0])
_KB = (-0.0034, 0.0007, -0.0021, 0.0002)


def _mk(**kw):
    import synth_ba
    return synth_ba.make_graph(**kw)


def _size_graph(nf):
    n_kf = nf + 2
    if nf > 100:                                             # the sizes test_gpu_ba.py runs its two largest windows at
        # (202: a seed on which the float64 oracle itself stays at 2e-12 of the model; others reach 6e-11 at this order)
        return _mk(n_kf=n_kf, n_pts=2500 if nf < 200 else 3000, obs=10, seed=1000 + nf if nf < 200 else 4)
    return _mk(n_kf=n_kf, n_pts=max(30, min(1500, 20 * n_kf)), obs=min(8, n_kf), seed=1000 + nf)


def _keep_edges(g, keep):
    for k in ("edge_pose", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        g[k] = g[k][keep]
    g["n_edges"] = int(keep.sum())
    return g


def _point_with(g, n_fixed_min, n_free_min):
    fixed_e = g["pose_fixed"][g["edge_pose"]] != 0
    nfix = np.bincount(g["edge_point"], weights=fixed_e, minlength=g["n_points"])
    nfree = np.bincount(g["edge_point"], weights=~fixed_e, minlength=g["n_points"])
    return int(np.flatnonzero((nfix >= n_fixed_min) & (nfree >= n_free_min))[0]), fixed_e


def _fixed_only_point():
    g = _mk(n_kf=9, n_pts=77, obs=5, seed=13, n_fixed=3)
    pt, fixed_e = _point_with(g, 2, 1)                      # keeps two fixed-keyframe edges (one mono edge alone leaves Hll singular)
    g = _keep_edges(g, ~((g["edge_point"] == pt) & ~fixed_e))
    assert np.all(g["pose_fixed"][g["edge_pose"][g["edge_point"] == pt]] != 0)
    return g


def _one_free_two_fixed():
    g = _mk(n_kf=9, n_pts=77, obs=5, seed=14, n_fixed=3)
    pt, fixed_e = _point_with(g, 2, 1)
    of_pt = g["edge_point"] == pt
    drop = np.zeros(g["n_edges"], bool)
    drop[np.flatnonzero(of_pt & ~fixed_e)[1:]] = True        # one free observation stays
    drop[np.flatnonzero(of_pt & fixed_e)[2:]] = True         # two fixed ones stay
    g = _keep_edges(g, ~drop)
    assert (g["edge_point"] == pt).sum() == 3
    return g


def _kf_four_obs():
    g = _mk(n_kf=10, n_pts=200, obs=6, seed=15)
    k = 5
    drop = np.zeros(g["n_edges"], bool)
    drop[np.flatnonzero(g["edge_pose"] == k)[4:]] = True
    g = _keep_edges(g, ~drop)
    assert (g["edge_pose"] == k).sum() == 4 and np.bincount(g["edge_point"], minlength=g["n_points"]).min() >= 2
    return g


def _point_seen_by_all():
    g = _mk(n_kf=10, n_pts=100, obs=10, seed=16)
    free = np.flatnonzero(g["pose_fixed"] == 0)
    per_pt = np.zeros((g["n_points"], g["n_poses"]), bool); per_pt[g["edge_point"], g["edge_pose"]] = True
    assert per_pt[:, free].all(1).any()
    return g


def _no_free_kf():
    g = _mk(n_kf=8, n_pts=150, obs=6, seed=5, stereo_frac=0.3, outlier_frac=0.03, pose_noise=(0.0003, 0.001))
    g["pose_fixed"] = np.ones(8, np.uint8)
    return g


def _two_pinholes():
    cams = [dict(fx=458.0, fy=458.0, cx=320.0, cy=240.0, bf=458.0 * 0.11, stereo_frac=0.3),
            dict(fx=380.0, fy=395.0, cx=300.0, cy=255.0, bf=380.0 * 0.07, stereo_frac=0.3)]
    return _mk(n_kf=14, n_pts=400, obs=6, seed=21, cameras=cams, pose_camera=[i % 2 for i in range(14)])


def _pinhole_and_fisheye_rig():
    q = np.array([0.0, 0.02, 0.0, 1.0]); q /= np.linalg.norm(q)
    rig = dict(Trl=(q[0], q[1], q[2], q[3], -0.1, 0.0, 0.0), cam=(190.0, 190.0, 254.0, 256.0), kb=(0.003, 0.0009, -0.002, 0.0003))
    cams = [dict(fx=458.0, fy=458.0, cx=320.0, cy=240.0, bf=458.0 * 0.11, stereo_frac=0.5),
            dict(fx=190.9, fy=190.3, cx=254.9, cy=256.8, bf=0.0, kb=(-0.0034, 0.0007, -0.002, 0.0002), rig2=rig)]
    g = _mk(n_kf=12, n_pts=300, obs=6, seed=23, cameras=cams, pose_camera=[0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0], right_frac=0.5)
    assert (g["edge_stereo"] == 2).sum() > 100 and (g["edge_stereo"] == 1).sum() > 100
    return g


def _rig(kb):
    if kb:
        return dict(Trl=(0.004, -0.012, 0.002, 0.99991, -0.101, 0.0007, 0.0012), cam=(190.4, 190.6, 252.7, 255.0), kb=(0.0031, 0.0007, -0.0019, 0.0003))
    return dict(Trl=(0.0, 0.01, 0.0, 0.99995, -0.11, 0.0, 0.0), cam=(458.0, 458.0, 320.0, 240.0), kb=None)


def _twin_edges(g):
    """the rig graphs put a left and a right observation on one (pose, point) pair"""
    key = g["edge_pose"].astype(np.int64) * g["n_points"] + g["edge_point"]
    assert len(np.unique(key)) < len(key)
    return g


def _shifted(g):
    """World moved by SHIFT, poses and points consistently: X + s, t - R s."""
    g = dict(g)
    R = np.asarray(bm.quat_to_R(g["poses0"][:, :4]), np.float64)
    P = g["poses0"].copy()
    P[:, 4:] = P[:, 4:] - R @ SHIFT
    g["poses0"] = P
    g["points0"] = g["points0"] + SHIFT
    return g


def _stereo04():
    return _mk(n_kf=12, n_pts=300, obs=6, seed=8, stereo_frac=0.4)


_POOL_SHAPES = [(5, 30, 3), (9, 77, 5), (12, 100, 6), (4, 25, 3), (7, 60, 4), (20, 200, 8), (3, 30, 3), (15, 120, 6)]


def _pool(i):
    n_kf, n_pts, obs = _POOL_SHAPES[i % len(_POOL_SHAPES)]
    return _mk(n_kf=n_kf, n_pts=n_pts, obs=obs, seed=2000 + i, stereo_frac=(0.0, 0.4, 1.0)[i % 3] if i % 2 else 0.0)


# name -> (graph builder, parameter spec).  spec: kind = default / merge / global / global_plain, lam = user_lambda_init,
# shifted = held by the K bound alone (not in the generator's own coordinates)
CASES = {}
for _nf in SIZES_SMALL + SIZES_BIG:
    CASES["nf%d" % _nf] = ((lambda nf=_nf: _size_graph(nf)), dict(nf=_nf))
CASES.update({
    "stereo_1.0": (lambda: _mk(n_kf=12, n_pts=300, obs=6, seed=7, stereo_frac=1.0), {}),
    "stereo_0.4": (_stereo04, {}),
    "kb8": (lambda: _mk(n_kf=12, n_pts=300, obs=6, seed=71, kb8=_KB), {}),
    "kb8_stereo": (lambda: _mk(n_kf=10, n_pts=200, obs=5, seed=72, kb8=_KB, stereo_frac=0.3), {}),
    "rig_fisheye": (lambda: _twin_edges(_mk(n_kf=12, n_pts=300, obs=6, seed=91, kb8=_KB, rig2=_rig(True))), {}),
    "rig_pinhole": (lambda: _twin_edges(_mk(n_kf=10, n_pts=200, obs=5, seed=92, rig2=_rig(False), right_frac=0.8)), {}),
    "two_pinholes": (_two_pinholes, {}),
    "pinhole_and_fisheye_rig": (_pinhole_and_fisheye_rig, {}),
    "fixed_only_point": (_fixed_only_point, {}),
    "one_free_two_fixed": (_one_free_two_fixed, {}),
    "kf_four_obs": (_kf_four_obs, {}),
    "point_seen_by_all": (_point_seen_by_all, {}),
    "global_robust": (lambda: _mk(n_kf=25, n_pts=400, obs=8, seed=102, n_fixed=1, outlier_frac=0.04, stereo_frac=0.3), dict(kind="global")),
    "global_plain": (lambda: _mk(n_kf=25, n_pts=400, obs=8, seed=102, n_fixed=1, outlier_frac=0.04, stereo_frac=0.3), dict(kind="global_plain")),
    "no_free_kf": (_no_free_kf, dict(nf=0)),
    "merge": (lambda: _mk(n_kf=20, n_pts=300, obs=10, seed=41, outlier_frac=0.03), dict(kind="merge")),
    "lam100": (_stereo04, dict(lam=100.0)),
    "lam1e4": (_stereo04, dict(lam=1e4)),
    "lam1e6": (_stereo04, dict(lam=1e6)),
    "shift_mono": (lambda: _shifted(_mk(n_kf=20, n_pts=500, obs=8, seed=12)), dict(shifted=True)),
    "shift_stereo": (lambda: _shifted(_stereo04()), dict(shifted=True)),
    "full_size": (lambda: _mk(seed=1), dict(nf=48)),
})
for _i in range(max(BATCH_SIZES)):
    CASES["pool%d" % _i] = ((lambda i=_i: _pool(i)), {})
for _i in range(8):
    CASES["wide%d" % _i] = ((lambda i=_i: _mk(n_kf=4, n_pts=1300, obs=4, seed=230 + i)), {})

_graphs, _refs = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = CASES[name][0]()
    return _graphs[name]


def local_params(name, device=False):
    """One tick: iters1 = 1, iters2 = 0, no_discard = 1 on the parameter set the case names."""
    spec = CASES[name][1]
    kind = spec.get("kind", "default")
    if device:
        import orbhip
        p = {"default": orbhip.ba_default_params, "merge": orbhip.ba_merge_params, "global": lambda: orbhip.ba_global_params(1, True),
             "global_plain": lambda: orbhip.ba_global_params(1, False)}[kind]()
    else:
        import oracle_ba_bind as ob
        p = {"default": ob.default_params, "merge": ob.merge_params, "global": lambda: ob.global_params(1, True),
             "global_plain": lambda: ob.global_params(1, False)}[kind]()
    p.iters1, p.iters2, p.no_discard = 1, 0, 1
    if "lam" in spec:
        p.user_lambda_init = spec["lam"]
    return p


def local_reference(name):
    """-> dict(tick = the model's tick, oracle = the oracle's errors against it, stats = the oracle's stats), cached."""
    if name not in _refs:
        import oracle_ba_bind as ob
        g = graph(name)
        p = local_params(name)
        rc, poses, pts, _, st = ob.solve(g, p)
        t = bm.local_tick(g, p)
        _refs[name] = dict(tick=t, oracle=bm.local_errors(t, poses, pts), stats=st, oracle_poses=poses, oracle_points=pts)
    return _refs[name]


def local_kernels(names, schur_mode, rows_env):
    """Which Schur / LDL^T kernels a batch of these graphs takes: the conditions of orbhip_ba_batch_solve's dispatcher restated."""
    nfs = [int(local_reference(n)["tick"]["n"]) // 6 for n in names]
    G = len(names)
    big = any(nf > 80 for nf in nfs)
    pair = big or schur_mode != 2
    if max(nfs) == 0:
        schur = "no reduced system"
    elif pair:
        rowmax = 0
        for n in names:
            g = graph(n); t = local_reference(n)["tick"]
            hid = -np.ones(g["n_poses"], int); hid[t["free"]] = 1
            rowmax = max(rowmax, int(np.bincount(g["edge_pose"][hid[g["edge_pose"]] >= 0], minlength=1).max()))
        if G >= 8 and rowmax <= 1024 and rows_env != 0:
            schur = "k_ba_schur_rows"
        elif G >= 8:
            schur = "k_ba_schur_big<16>"
        else:
            schur = "k_ba_schur_big<64>"
    else:
        schur = "k_ba_schur_gemm+bschur+finish"
    n = 6 * max(nfs)
    ldlt = "k_ba_big_* (%d panels + %d)" % (n // 32, n % 32) if big else "k_ba_ldlt (%d full panels + %d)" % (n // 32, n % 32)
    return schur + " / " + ldlt


# ---------------------------------------------------------------------------------------------- inertial local BA
# n_opt optimizable keyframes = a reduced system of order 15 n_opt through ba_ldlt.h (32 = the cap: 480 unknowns)
IBA_CASES = {
    "opt1": (dict(seed=201, n_opt=1, n_fixed_vis=4, n_points=80), False),
    "opt2": (dict(seed=202, n_opt=2, n_fixed_vis=3, n_points=80), False),
    "opt3": (dict(seed=22, n_opt=3, n_fixed_vis=2, n_points=60), False),
    "opt7": (dict(seed=207, n_opt=7, n_fixed_vis=8, n_points=250), False),
    "opt8": (dict(seed=21, n_opt=8, n_fixed_vis=10, n_points=300), False),
    "opt8_mono": (dict(seed=208, n_opt=8, n_fixed_vis=10, n_points=300, stereo_frac=0.0), False),
    "opt8_stereo": (dict(seed=209, n_opt=8, n_fixed_vis=10, n_points=300, stereo_frac=1.0), False),
    "opt8_no_covisible": (dict(seed=210, n_opt=8, n_fixed_vis=0, n_points=300), False),
    "opt7_covisible_with_imu": (dict(seed=211, n_opt=7, n_fixed_vis=8, n_points=250, covisible_imu=True), False),
    "opt10_fisheye_rig": (dict(seed=26, n_opt=10, n_fixed_vis=30, n_points=900, fisheye_rig=True), False),
    "opt16": (dict(seed=216, n_opt=16, n_fixed_vis=12, n_points=500), False),
    "opt17": (dict(seed=217, n_opt=17, n_fixed_vis=12, n_points=500), False),
    "opt25_large": (dict(seed=31, n_opt=25, n_fixed_vis=40, n_points=1200, large=True), True),
    "opt32_large": (dict(seed=232, n_opt=32, n_fixed_vis=20, n_points=1000, large=True), True),
}
for _i in range(4):
    IBA_CASES["small%d" % _i] = (dict(seed=70 + _i, n_opt=3 + _i, n_fixed_vis=2 + _i, n_points=60 + 30 * _i), False)
_wins, _irefs = {}, {}


def window(name):
    if name not in _wins:
        import synth_iba
        kw = dict(IBA_CASES[name][0])
        covisible_imu = kw.pop("covisible_imu", False)
        w = synth_iba.make_window(**kw)
        if covisible_imu:                                    # the covisible fixed keyframes carry IMU states too (kf_imu = 1, still fixed)
            w.arrays["kf_imu"][:] = 1
        _wins[name] = w
    return _wins[name]


def iba_params(name, device=False):
    large = IBA_CASES[name][1]
    if device:
        import orbhip
        p = orbhip.iba_default_params(large)
    else:
        import oracle_iba_bind as ib
        p = ib.default_params(large)
    p.iterations = 1
    return p


def iba_reference(name):
    if name not in _irefs:
        import oracle_iba_bind as ib
        w = window(name)
        p = iba_params(name)
        kf, pts, _, st = ib.solve(w, p)
        t = bm.inertial_tick(w, p)
        _irefs[name] = dict(tick=t, oracle=bm.inertial_errors(t, kf, pts), stats=st, oracle_kf=kf, oracle_points=pts)
    return _irefs[name]
