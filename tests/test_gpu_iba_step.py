"""ONE Levenberg-Marquardt tick of the device's inertial local BA (iterations = 1) against the extended-precision model of
tests/ba_step_model.py: k_iba_solve's normal equations (visual, EdgeInertial, EdgeGyroRW, EdgeAccRW), Schur complement, the reduced
LDL^T of order 15 n_opt (through ba_ldlt.h, up to 480) and the back-substitution, through every team size, the one-shot call and
the resident batch.  Same metrics and the same bound as test_gpu_ba_step.py: e_device <= K (e_oracle + floor) and e_device <= 1e-9
for every window.

K = 128 (ba_step_model.K; set by the local BA's shifted windows, see test_gpu_ba_step.py).  Measured on an MI355X, e_device /
(e_oracle + floor): between 0.2 and 1.7 on every window, team size and entry point (largest 1.66, a 4-keyframe window on the
single-workgroup path); e_device <= 1.9e-13, backward errors <= 1e-17 -- the inertial step would hold K = 4."""
import numpy as np
import pytest
import ba_step_model as bm
import ba_step_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import orbhip
    ctx = orbhip.Context(0)
    yield orbhip, ctx
    ctx.close()


def _check(names, got, what):
    kfs, pts, _, stats = got
    failures = []
    for i, n in enumerate(names):
        ref = bc.iba_reference(n)
        t, orc, st = ref["tick"], ref["oracle"], stats[i]
        assert t["n"] == 15 * bc.IBA_CASES[n][0]["n_opt"]
        dev = bm.inertial_errors(t, kfs[i], pts[i])
        bm.report("%s[%d/%d]" % (n, i, len(names)), what, dev, orc, t)
        assert st["iterations_run"] == 1 and st["lm_trials"] == 1 and st["failed"] == 0, (n, st)
        assert abs(st["err"] - t["chi2"]) <= t["n_edges"] * 2.0 ** -52 * t["chi2"], (n, st["err"], t["chi2"])
        if not bm.within_bound(dev["e"], orc["e"], orc["floor"]):
            failures.append((n, "K bound", dev, orc))
        if not dev["e"] <= bm.ABS_BOUND:
            failures.append((n, "1e-9", dev, orc))
    assert not failures, failures


def _solve(hip, names):
    orbhip, ctx = hip
    wins = [bc.window(n) for n in names]
    structs = [w.struct(orbhip.IbaWindow) for w in wins]
    got = orbhip.inertial_ba_solve_batch(ctx, structs, [w.kf0 for w in wins], [w.pts0 for w in wins], bc.iba_params(names[0], device=True))
    return got, "k_iba_solve team %d" % orbhip.inertial_ba_last_team_size()


@pytest.mark.parametrize("name", [n for n in bc.IBA_CASES if not n.startswith("small")])
def test_one_tick_window_sizes_and_content(hip, name):
    """n_opt = 1, 2, 3, 7, 8, 16, 17, 25, 32 (the cap); mono / stereo / both; with and without covisible fixed keyframes (the fixed
    previous keyframe carries IMU states, the covisible ones do not); the two-fisheye rig; the `large` parameters."""
    got, what = _solve(hip, [name])
    _check([name], got, what)


@pytest.mark.parametrize("team", [1, 2, 5, 16])
def test_one_tick_every_team_size(hip, team, monkeypatch):
    orbhip, _ = hip
    monkeypatch.setenv("ORBHIP_IBA_TEAM", str(team))
    names = ["opt3", "opt8", "opt10_fisheye_rig", "opt17"]
    got, what = _solve(hip, names)
    assert orbhip.inertial_ba_last_team_size() == team
    _check(names, got, what)


def test_one_tick_many_windows_take_the_single_workgroup_path(hip):
    orbhip, _ = hip
    names = ["small%d" % (i % 4) for i in range(160)]
    got, what = _solve(hip, names)
    assert orbhip.inertial_ba_last_team_size() == 1
    _check(names, got, what)


def test_one_tick_resident_batch(hip):
    orbhip, ctx = hip
    names = ["opt2", "opt7", "opt8_stereo", "opt16"]
    wins = [bc.window(n) for n in names]
    structs = [w.struct(orbhip.IbaWindow) for w in wins]
    b = orbhip.IbaBatch(ctx, structs, [w.kf0 for w in wins], [w.pts0 for w in wins])
    try:
        b.solve(bc.iba_params(names[0], device=True))
        _check(names, b.download(), "resident batch, team %d" % orbhip.inertial_ba_last_team_size())
    finally:
        b.close()
