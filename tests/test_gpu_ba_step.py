"""ONE Levenberg-Marquardt tick of the device's local BA (orbhip.BaBatch with iters1 = 1, iters2 = 0, no_discard = 1: the download is
x0 (+) dx) against the extended-precision model of tests/ba_step_model.py, graph by graph.

test_gpu_ba.py compares with the oracle after the whole LM schedule (RMSE <= 1e-4), and LM forgives a wrong step; this file looks at
what a single tick computes -- normal equations, Schur complement (k_ba_schur_big<64> / <16>, k_ba_schur_rows, k_ba_schur_gemm +
k_ba_bschur + k_ba_schur_finish), reduced LDL^T (k_ba_ldlt with full and partial panels, the k_ba_big_* global-memory path) and
k_ba_backsub_points -- through every size-chosen form.

The bound, for EVERY graph: e_device <= K (e_oracle + floor), e_oracle being the float64 oracle's own step error against the model on the
same graph (computed live; nothing is measured against the code under test) and floor the cost of storing a result in float64; and,
in the generator's own coordinates, e_device <= 1e-9.  chi2_initial agrees with the model's to E 2^-52 relative (E edges).

K = 128 (ba_step_model.K, where the rule that set it is written down).  Measured on an MI355X, e_device / (e_oracle + floor) over the
550 graph solves of this file and test_gpu_iba_step.py: 63.9 and 37.6 on the two shifted windows (e_device 8.9e-10 / 5.5e-10, backward
error 1.2e-13 / 1.0e-13 against the oracle's 1.7e-13 / 7.2e-14: the float64 evaluation of R X + t at 2000 m, which the yardstick does
not contain -- test_ba_step_model.py::test_exact_pinhole_edges_and_what_the_yardstick_does_not_see puts the oracle itself at 6.6e-10
there), 17.5 on 81 free keyframes (k_ba_big_*, e_device 4.5e-12 where the oracle on 80 / 86 free keyframes is at 2.5e-12 / 1.8e-12),
5.2 on 48 free keyframes through the MFMA form (1.9e-13), every other local-BA graph <= 1.3; largest e_device in the generator's
coordinates 4.5e-12.  Every backward error is at or below the oracle's level (<= 2.4e-15 unshifted against order 2^-52 >= 1e-13).

Sensitivity, checked once outside the tree: with k_ba_schur_rows made to drop ONE block pair (poses 0, 1) of ONE point per graph, the
three batches of this file that take that kernel (8, 9, 65 graphs, default pair lists) fail with step errors up to 0.14 and backward
errors of 1e-3, and every graph through the other forms passes; of test_gpu_ba.py only
test_ba_batches_of_eight_and_more_both_pair_kernels[1] notices, by 2.5e-6 relative in the chi2_final of its 5-keyframe graph, whose
RMSE, iteration and trial-count criteria still hold."""
import numpy as np
import pytest
import ba_step_model as bm
import ba_step_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["pairs", "mfma"])
def ba_ctx(request, gpu_ctx):
    """Both forms of the Schur complement (see test_gpu_ba.py): the pair-list kernels on the session context, the FP64-MFMA panel GEMM
    (orbhip_ctx_set_ba_schur_mode(ctx, 2)) on a context of its own."""
    import orbhip
    if request.param == "pairs":
        yield gpu_ctx, 0
        return
    ctx = orbhip.Context(0)
    orbhip.ba_set_schur_mode(ctx, 2)
    yield ctx, 2
    ctx.close()


def _one_tick(ctx, names, schur_mode=0, rows_env=None):
    """The batch `names` through one tick on the device; every graph of it against the model and the bound."""
    import orbhip
    graphs = [bc.graph(n) for n in names]
    kinds = {bc.CASES[n][1].get("kind", "default") for n in names} | {bc.CASES[n][1].get("lam") for n in names}
    assert len(kinds) == 2, "one parameter set per batch"
    bb = orbhip.BaBatch(ctx, graphs)
    bb.solve(bc.local_params(names[0], device=True))
    poses, points, _, stats = bb.download()
    bb.close()
    kernels = bc.local_kernels(names, schur_mode, rows_env)
    failures = []
    for i, n in enumerate(names):
        ref = bc.local_reference(n)
        t, orc, st = ref["tick"], ref["oracle"], stats[i]
        dev = bm.local_errors(t, poses[i], points[i])
        bm.report("%s[%d/%d]" % (n, i, len(names)), kernels, dev, orc, t)
        assert st["lm_trials"] == 1 and st["iterations_run"] == [1, 0] and st["discarded"] == 0, (n, st)
        assert abs(st["chi2_initial"] - t["chi2"]) <= t["n_edges"] * 2.0 ** -52 * t["chi2"], (n, st["chi2_initial"], t["chi2"])
        if not bm.within_bound(dev["e"], orc["e"], orc["floor"]):
            failures.append((n, "K bound", dev, orc))
        if not bc.CASES[n][1].get("shifted") and not dev["e"] <= bm.ABS_BOUND:
            failures.append((n, "1e-9", dev, orc))
    assert not failures, failures


@pytest.mark.parametrize("nf", bc.SIZES_SMALL)
def test_one_tick_reduced_system_sizes(ba_ctx, nf):
    """n = 6 nf against the 32-column panels of ba_ldlt.h, one graph per call."""
    ctx, mode = ba_ctx
    assert bc.local_reference("nf%d" % nf)["tick"]["n"] == 6 * nf
    _one_tick(ctx, ["nf%d" % nf], mode)


@pytest.mark.parametrize("nf", bc.SIZES_BIG)
def test_one_tick_more_than_80_free_keyframes(gpu_ctx, nf):
    """The k_ba_big_* path (pair lists whatever the context's mode)."""
    assert bc.local_reference("nf%d" % nf)["tick"]["n"] == 6 * nf
    _one_tick(gpu_ctx, ["nf%d" % nf])


@pytest.mark.parametrize("G", bc.BATCH_SIZES)
def test_one_tick_ragged_batches(ba_ctx, G):
    """The pair kernels change form at 8 graphs and round the grid to multiples of 8; k_ba_pretrial / k_ba_control work in blocks of
    64.  Through the default pair lists and Schur mode 2."""
    ctx, mode = ba_ctx
    _one_tick(ctx, ["pool%d" % i for i in range(G)], mode)


@pytest.mark.parametrize("G", [8, 9, 65])
def test_one_tick_ragged_batches_without_the_row_kernel(gpu_ctx, G, monkeypatch):
    monkeypatch.setenv("ORBHIP_BA_SCHUR_ROWS", "0")
    _one_tick(gpu_ctx, ["pool%d" % i for i in range(G)], 0, rows_env=0)


def test_one_tick_row_kernel_falls_back(gpu_ctx):
    """A keyframe with more than 1024 landmarks: k_ba_schur_big<16> for the whole batch."""
    names = ["wide%d" % i for i in range(8)]
    assert max(np.bincount(bc.graph(n)["edge_pose"]).max() for n in names) > 1024
    _one_tick(gpu_ctx, names)


def test_one_tick_one_big_graph_takes_the_batch_along(gpu_ctx):
    """ONE graph with more than 80 free keyframes: the whole batch takes the global-memory path, small graphs included."""
    _one_tick(gpu_ctx, ["pool0", "nf86", "pool1", "pool2", "pool6"])


CONTENT = ["stereo_1.0", "stereo_0.4", "kb8", "kb8_stereo", "rig_fisheye", "rig_pinhole", "two_pinholes", "pinhole_and_fisheye_rig",
           "fixed_only_point", "one_free_two_fixed", "kf_four_obs", "point_seen_by_all", "global_robust", "global_plain", "no_free_kf",
           "merge", "full_size"]


@pytest.mark.parametrize("name", CONTENT)
def test_one_tick_edge_content(ba_ctx, name):
    ctx, mode = ba_ctx
    _one_tick(ctx, [name], mode)


@pytest.mark.parametrize("name", ["stereo_0.4", "lam100", "lam1e4", "lam1e6"])
def test_one_tick_lambda(ba_ctx, name):
    """tau max diag (effectively 0) and user_lambda_init = 100 (the inertial value), 1e4, 1e6 (lambda dominates the diagonals)."""
    ctx, mode = ba_ctx
    _one_tick(ctx, [name], mode)


@pytest.mark.parametrize("name", ["shift_mono", "shift_stereo"])
def test_one_tick_shifted_world(ba_ctx, name):
    """The world moved by (1000, -2000, 500) m: the oracle's own error grows with it, which is what the yardstick and the floor are
    for; held by the K bound alone."""
    ctx, mode = ba_ctx
    _one_tick(ctx, [name], mode)
