"""Device batch of Optimizer::InertialOptimization (orbhip_inertial_optimization_device / _host) against the numpy model
(tests/inertial_opt_model.py) in float64 and in extended precision.

One-step tests (iterations 1 and 2) and full runs: the same iterations, LM trials, end reason and accept / reject decisions as the model,
and the project's K rule on Rwg, scale, biases, velocities, chi2 and lambda: the device's
error against the extended-precision model is at most K = 128 times the float64 model's; where that is zero, the floor is the largest
float64-model error over the cases of the overload; both carry the storage floor 2^-52 max|value| of tests/ba_step_model.py's rule.
Full runs whose models go on past the decisive prefix (the last iteration of most maps with priors gains nothing and ends in Terminate)
are held to the model over the prefix -- chi2 and lambda of every iteration -- and past it to what follows from the prefix's definition:
the same end reason, between one and three further iterations, an end state within the K rule plus the steps those iterations may take
or leave (inertial_opt_cases.past_prefix_slack), a final chi2 not above the float64 model's by more than the rule plus 3e-9 chi2.
The measured ratios are printed.  Further: a second run is byte-identical, rows
beyond each map and all fixed quantities keep their sentinel / input bytes, a NaN map ends alone, a GN map without edges reports
"solver failed", the argument checks."""
import numpy as np
import pytest
import inertial_opt_cases as ic
import inertial_opt_model as iom
import synth_inertial_opt as sio

pytestmark = pytest.mark.gpu
LENGTHS = [1, 2, 3, 10, 63, 64, 65, 100, 257]
SENT = 777.25


def _params(family, iterations=None):
    import orbhip
    ov, mono, fixed, pg, pa = ic.FAMILIES[family]
    p = orbhip.inertial_opt_params(ov, mono, fixed, pg, pa)
    if iterations is not None:
        p.iterations = iterations
    return p


def _run(ctx, maps, p, pad=3):
    """Two launches on fresh copies; asserts that they agree byte for byte and that the rows behind the batch keep their sentinel.
    -> kf [K][21], glob [m][16], stats [m][8], trace [m][iterations][2] (NaN = not written)."""
    import torch
    import orbhip
    off, kf, link, preint, info, glob = sio.pack(maps)
    K_, m = int(off[-1]), len(maps)
    kfp = np.full((K_ + pad, 21), SENT); kfp[:K_] = kf
    globp = np.full((m + 1, 16), SENT); globp[:m] = glob
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    t_off, t_link, t_pre, t_info = dev(off), dev(np.concatenate([link, np.ones(pad, np.uint8)])), dev(preint), dev(info)
    outs = []
    for _ in range(2):
        t_kf, t_glob = dev(kfp), dev(globp)
        t_st = torch.full((m + 1, 8), SENT, dtype=torch.float64, device="cuda")
        t_tr = torch.full((m + 1, max(p.iterations, 1), 2), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        orbhip.inertial_optimization_device(ctx, p, m, t_off.data_ptr(), t_kf.data_ptr(), t_link.data_ptr(), t_pre.data_ptr(),
                                            t_info.data_ptr(), t_glob.data_ptr(), t_st.data_ptr(), t_tr.data_ptr())
        ctx.synchronize()
        outs.append([a.cpu().numpy() for a in (t_kf, t_glob, t_st, t_tr)])
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes(), "second run differs"
    o_kf, o_glob, o_st, o_tr = outs[0]
    assert (o_kf[K_:] == SENT).all() and (o_glob[m:] == SENT).all() and (o_st[m:] == SENT).all() and np.isnan(o_tr[m:]).all()
    # poses are never written; without free velocities and biases nothing of a keyframe is
    assert o_kf[:K_, 0:12].tobytes() == kf[:, 0:12].tobytes()
    if not p.free_vel_bias:
        assert o_kf[:K_].tobytes() == kf.tobytes() and o_glob[:m, 10:16].tobytes() == glob[:, 10:16].tobytes()
    if not p.free_gdir:
        assert o_glob[:m, 0:9].tobytes() == glob[:, 0:9].tobytes()
    if not p.free_scale:
        assert o_glob[:m, 9].tobytes() == glob[:, 9].tobytes()
    return o_kf[:K_], o_glob[:m], o_st[:m], o_tr[:m, :p.iterations], off


def _compare(cases, res, full):
    """cases: [(family, n, seed, iterations, gaps)] in batch order."""
    kf, glob, st, tr, off = res
    floors = ic.floors_of(cases)
    worst = {}
    for i, c in enumerate(cases):
        mp, r64, rld = ic.model_runs(*c)
        tag = "%s n=%d seed=%d" % c[:3]
        gn = bool(ic.params(c[0])["gauss_newton"])
        pre = len(rld["trace"]) if gn else iom.decisive_prefix(rld["trace"])
        whole = pre == len(rld["trace"]) and pre == len(r64["trace"])
        trd = tr[i]
        if whole or not full:
            assert (int(st[i, 0]), int(st[i, 1]), int(st[i, 2])) == (rld["iterations"], rld["trials"], rld["reason"]), (tag, st[i], rld["iterations"], rld["trials"], rld["reason"])
        # decisions and lambda over the decisive prefix: an iteration's lambda is lambda_before * factor for an accepted trial and
        # * 2^(q(q+1)/2) for q rejected ones, so equal lambdas (to rounding) are equal decisions
        for it in range(pre):
            lam_m = float(rld["trace"][it]["lam"])
            assert np.isfinite(trd[it, 0]) and abs(trd[it, 1] - lam_m) <= 1e-6 * abs(lam_m), (tag, it, trd[it], lam_m)
            chi_m = float(rld["trace"][it]["chi"])
            assert abs(trd[it, 0] - chi_m) <= 1e-6 * abs(chi_m) + 1e-9, (tag, it, trd[it], chi_m)
        slack = None
        if full and not whole:
            # the run goes on past the decisive prefix, where decisions are rounding noise: it ends as the model does (every such
            # iteration gains far less than the 1e-3 of LM's stop test, so Terminate comes within three of them), after at least the
            # prefix's trials, and its end state is the model's up to the steps those iterations may take or leave
            slack = ic.past_prefix_slack(r64, rld, pre)
            assert rld["reason"] == r64["reason"] == iom.END_TERMINATE and int(st[i, 2]) == iom.END_TERMINATE, (tag, st[i])
            assert pre + 1 <= int(st[i, 0]) <= pre + ic.PAST_PREFIX_ITERATIONS, (tag, st[i], pre)
            assert int(st[i, 1]) >= sum(r["trials"] for r in rld["trace"][:pre]) + 1, (tag, st[i])
            print("past the prefix: %s prefix %d, iterations device %d / float64 %d / extended %d, trials %d / %d / %d"
                  % (tag, pre, st[i, 0], r64["iterations"], rld["iterations"], st[i, 1], r64["trials"], rld["trials"]))
        a, b = int(off[i]), int(off[i + 1])
        dev = ic.group_values(kf[a:b], glob[i], st[i, 4], st[i, 5])
        ok, rep = ic.k_rule(dev, r64, rld, floors[ic.OVERLOAD_OF[c[0]]], slack)
        for g, (ed, bound, e64) in rep.items():
            if slack is not None:
                continue                                    # the ratios reported are those of runs the rule alone bounds
            ratio = ed / (bound / ic.K) if bound > 0 else 0.0
            w = worst.setdefault((ic.OVERLOAD_OF[c[0]], g), [0.0, tag])
            if ratio > w[0]:
                w[0], w[1] = ratio, tag
        assert ok, (tag, {g: v for g, v in rep.items() if v[0] > v[1]})
    for (ov, g), (ratio, tag) in sorted(worst.items()):
        print("K-rule ratio overload %s %-5s %8.3f  (%s)" % (ov, g, ratio, tag))


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("family", list(ic.FAMILIES))
def test_one_step(gpu_ctx, family, iterations):
    import orbhip
    lens = LENGTHS + [orbhip.inertial_opt_lds_keyframes()]
    if family == "a_mono":                                  # no priors: 9 (n - 1) equations for 3 n + 9 unknowns are rank deficient below n = 4
        lens = [n for n in lens if n >= 10]
    cases = [(family, n, 3, iterations, ()) for n in lens]
    maps = [ic.model_runs(*c)[0] for c in cases]
    _compare(cases, _run(gpu_ctx, maps, _params(family, iterations)), full=False)


@pytest.mark.parametrize("family", list(ic.FAMILIES))
def test_full_runs(gpu_ctx, family):
    cases = [(f, n, s, None, ()) for f, n, s in ic.FULL_CASES if f == family]
    cases += [(family, n, 4, None, ()) for n in ((10, 65) if family != "a_mono_prior" else (3, 65, 257))]
    for c in cases[:len([1 for f, _, _ in ic.FULL_CASES if f == family])]:
        assert iom.decisive_prefix(ic.model_runs(*c)[2]["trace"]) >= 5, c
    maps = [ic.model_runs(*c)[0] for c in cases]
    res = _run(gpu_ctx, maps, _params(family))
    _compare(cases, res, full=True)
    # the final chi2 is not above the float64 model's by more than the rule allows -- every case; where the run goes on past the
    # decisive prefix, plus the less than 1e-9 chi2 that each of at most three such iterations can gain
    floors = ic.floors_of(cases)
    for i, c in enumerate(cases):
        _, r64, rld = ic.model_runs(*c)
        e64 = abs(float(np.longdouble(r64["chi_last"]) - rld["chi_last"]))
        base = (e64 if e64 > 0 else floors[ic.OVERLOAD_OF[family]]["chi"]) + 2.0 ** -52 * abs(float(rld["chi_last"]))
        pre = iom.decisive_prefix(rld["trace"])
        gn = bool(ic.params(family)["gauss_newton"])
        extra = 0.0 if gn or pre == len(rld["trace"]) == len(r64["trace"]) else ic.past_prefix_slack(r64, rld, pre)["chi"]
        assert res[2][i, 4] <= float(r64["chi_last"]) + ic.K * base + extra, (c, res[2][i, 4], float(r64["chi_last"]), base, extra)


def _ragged():
    lens = [1, 2, 3, 10, 63, 64, 65, 100, 257]
    cases = [("a_mono_prior", lens[i % 9], 10 + i, 2, ()) for i in range(64)]
    cases[5] = ("a_mono_prior", 10, 15, 2, (5,))            # a gap: two chains
    maps = [ic.model_runs(*c)[0] for c in cases]
    return cases, maps


def test_ragged_batch_gap_and_no_edges(gpu_ctx):
    cases, maps = _ragged()
    noedge = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in maps[9].items()}
    noedge["link"][:] = 0
    maps = maps[:9] + [noedge] + maps[10:]
    res = _run(gpu_ctx, maps, _params("a_mono_prior", 2))
    keep = [i for i in range(64) if i != 9]
    sub = (np.concatenate([res[0][res[4][i]:res[4][i + 1]] for i in keep]), res[1][keep], res[2][keep], res[3][keep],
           np.concatenate([[0], np.cumsum([len(maps[i]["kf"]) for i in keep])]))
    _compare([cases[i] for i in keep], sub, full=False)
    # the map without edges: its velocities never become active; what moves is what the priors and lambda alone move
    _, r64, rld = maps[9], iom.optimize(noedge, ic.params("a_mono_prior", 2), np.float64), iom.optimize(noedge, ic.params("a_mono_prior", 2), ic.LD)
    a, b = int(res[4][9]), int(res[4][10])
    assert res[0][a:b, 12:15].tobytes() == np.asarray(noedge["kf"])[:, 12:15].tobytes()
    assert (int(res[2][9, 0]), int(res[2][9, 1]), int(res[2][9, 2])) == (rld["iterations"], rld["trials"], rld["reason"])
    # the gap map: the keyframes on both sides of the cut are solved, as two chains
    assert int(res[2][5, 6]) == 8


def test_nan_map_ends_alone(gpu_ctx):
    cases, maps = _ragged()
    clean = _run(gpu_ctx, maps, _params("a_mono_prior", 2))
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in maps[17].items()}
    bad["preint"][1, 11] = np.nan
    dirty = _run(gpu_ctx, maps[:17] + [bad] + maps[18:], _params("a_mono_prior", 2))
    assert int(dirty[2][17, 2]) == iom.END_NONFINITE and int(dirty[2][17, 0]) == 0
    a, b = int(clean[4][17]), int(clean[4][18])
    assert dirty[0][a:b, 12:15].tobytes() == np.asarray(bad["kf"])[:, 12:15].tobytes()          # velocities as they came
    assert dirty[1][17].tobytes() == np.asarray(bad["glob"]).tobytes()
    for i in range(64):
        if i != 17:
            x, y = int(clean[4][i]), int(clean[4][i + 1])
            assert dirty[0][x:y].tobytes() == clean[0][x:y].tobytes() and dirty[1][i].tobytes() == clean[1][i].tobytes(), i
            assert dirty[2][i].tobytes() == clean[2][i].tobytes()


def test_gn_without_edges_reports_solver_failed(gpu_ctx):
    mp = ic.make("d", 6, 1)
    mp["link"][:] = 0
    kf, glob, st, tr, _ = _run(gpu_ctx, [mp, ic.make("d", 6, 2)], _params("d"))
    assert int(st[0, 2]) == iom.END_SOLVER and int(st[0, 0]) == 1
    assert glob[0].tobytes() == np.asarray(mp["glob"]).tobytes() and kf[:6].tobytes() == np.asarray(mp["kf"]).tobytes()
    assert int(st[1, 2]) == iom.END_ITERATIONS and int(st[1, 0]) == 10


def test_4096_keyframes_three_iterations(gpu_ctx):
    c = ("a_mono_prior", 4096, 1, 3, ())
    _compare([c], _run(gpu_ctx, [ic.model_runs(*c)[0]], _params("a_mono_prior", 3)), full=False)


def test_host_form_equals_device_form(gpu_ctx):
    import orbhip
    c = ("a_mono", 10, 1, None, ())
    mp = ic.model_runs(*c)[0]
    p = _params("a_mono")
    kf, glob, st, tr, _ = _run(gpu_ctx, [mp], p)
    hkf, hglob, hst, htr = orbhip.inertial_optimization_host(gpu_ctx, p, mp, trace=True)
    assert hkf.tobytes() == kf.tobytes() and hglob.tobytes() == glob[0].tobytes() and hst.tobytes() == st[0].tobytes()
    assert np.array_equal(htr, tr[0], equal_nan=True)


def test_argument_checks(gpu_ctx):
    import torch
    import orbhip
    mp = ic.make("a_mono", 4, 1)
    off, kf, link, preint, info, glob = sio.pack([mp])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    t = [dev(a) for a in (off, kf, link, preint, info, glob)]
    ptr = [x.data_ptr() for x in t]
    call = lambda p, maps, o=None: orbhip.lib.orbhip_inertial_optimization_device(gpu_ctx.h, orbhip.C.byref(p), maps, o or ptr[0], *ptr[1:], None, None)   # noqa: E731
    p = _params("a_mono")
    assert call(p, 0) == 0
    assert call(p, -1) == -1
    nothing = _params("a_fixed"); nothing.free_gdir = 0; nothing.free_scale = 0
    assert call(nothing, 1) == -1
    assert call(p, 1, dev(np.array([4, 0], np.int32)).data_ptr()) == -1
    assert call(p, 1, dev(np.array([0, 4097], np.int32)).data_ptr()) == -1
    gpu_ctx.synchronize()
    assert torch.equal(t[1].cpu(), torch.from_numpy(kf))
