"""IMU preintegration on the device (orbhip_preintegrate_device / _host, csrc/preint_kernels.hip) in both forms against the longdouble
model (tests/preint_model.py).

K rule (ba_step_model.within_bound, K = 128): every field group -- dT, dR, dV, dP, each Jacobian, avgA, avgW, each 3 x 3 block of
C(0:9, 0:9), the walk block -- obeys e_device <= K (e_float32_model + 2^-24 max|group|), per chain.  Chain lengths 0, 1, 2, 63, 64, 65,
127, 128, 129, 257, 2000; batches of 1, 63, 64, 65, 130 ragged chains with empty ones first, last and in the middle; a full symmetric
Nga; acceleration equal to its bias; both sides of IntegratedRotation's branch.  Also: a continued chain equals the chain integrated in
one go and reruns are equal, byte for byte; a NaN stays in its chain; the information from the device's own covariance obeys the K rule
against the longdouble restatement (floor 2^-52 max|info|; lengths 2 and 2000 sampled as preint_cases.INFO_DT says, so that no
eigenvalue lies within a factor 8 of the cut); the device arrays feed orbhip_inertial_optimization_device directly with the
result of a solve fed from host copies; argument errors return their codes and write nothing.

Measured on an MI355X, e_device / (e_float32_model + floor) per field group, the largest over all cases, lane form / wave form:
dT 0.86 / 0.86, dR 0.88 / 0.88, dV 1.77 / 2.41, dP 4.81 / 4.81, JRg 1.43 / 1.97, JVg 1.03 / 1.04, JVa 1.45 / 1.45, JPg 1.31 / 1.31,
JPa 1.53 / 1.53, avgA 4.35 / 4.35, avgW 4.44 / 4.44, C_rr 2.36 / 3.09, C_rv 2.65 / 2.65, C_rp 3.51 / 3.25, C_vr 2.60 / 2.60, C_vv 1.83 /
1.83, C_vp 2.24 / 2.24, C_pr 3.41 / 2.63, C_pv 2.58 / 2.58, C_pp 1.99 / 1.99, walk block 1.00 / 1.00, the blocks between 0 / 0 (exact
zeros).  The largest of a case: lengths 4.44 (avgW), batches of 63, 64, 65 3.71 and of 130 4.35 (avgA), full Nga 4.81
(dP), acceleration equal to its bias 1.09 / 0.97, the branch case 1.28.  The information (every chain with measurements of the
lengths, the batch of 65 and the full-Nga case): lengths 0.94 / 0.95, batch of 65 0.99 / 1.00, full Nga 0.91 / 0.89 (the device runs
the float64 model's operations).  K = 128 leaves a factor 26."""
import functools
import numpy as np
import pytest
import ba_step_model as bsm
import preint_cases as pc
import preint_model as pm

pytestmark = pytest.mark.gpu

FORMS = {"lane": 1, "wave": 2}
NGA, WALK = pc.calib_nga(), pc.calib_nga(pc.NGW, pc.NAW)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (bias list, meas list, nga, longdouble fields, float32 fields), computed once."""
    nga = NGA
    if name == "lengths":
        pairs = [pc.single(n) for n in pc.LENGTHS]
        bias, meas = [p[0][0] for p in pairs], [p[1][0] for p in pairs]
    elif name.startswith("batch"):
        bias, meas = pc.batch(int(name[5:]))
    elif name == "full_nga":
        bias, meas = pc.batch(5, seed=3)
        meas[1] = pc.chain(1, 91); meas[3] = pc.chain(66, 92)
        nga = pc.full_nga()
    elif name == "acc_bias":
        b, m = pc.acc_equals_bias_chain()
        bias, meas = [b, pc.bias(5)], [m, pc.chain(20, 5)]
    elif name == "branch":
        b, m = pc.branch_chain()
        bias, meas = [b], [m]
    else:
        raise KeyError(name)
    ref, f32 = pc.models(bias, meas, nga, WALK)
    return bias, meas, nga, ref, f32


CASES = ["lengths"] + ["batch%d" % b for b in pc.BATCHES] + ["full_nga", "acc_bias", "branch"]


def run_device(ctx, bias, meas, nga, form, start=None, want_info=False):
    """-> dict of numpy outputs (record, cov, avg and, with want_info, info / info_g / info_a) and the device tensors."""
    import torch
    import orbhip
    n = len(meas)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(m) for m in meas])
    flat = np.concatenate([np.asarray(m, np.float32).reshape(-1, 7) for m in meas] + [np.zeros((1, 7), np.float32)])
    rec = np.full((n, 67), 7.5); cov = np.full((n, 225), 7.5, np.float32); avg = np.full((n, 6), 7.5, np.float32)
    cont = np.zeros(n, np.uint8)
    for c in range(n):
        if start is not None and start[c] is not None:
            rec[c], cov[c], avg[c] = start[c]; cont[c] = 1
        rec[c, 61:67] = np.asarray(bias[c], np.float32)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         (("off", off), ("meas", flat), ("cont", cont), ("rec", rec), ("cov", cov), ("avg", avg))}
    t["info"] = torch.full((n, 81), 7.5, dtype=torch.float64, device="cuda")
    t["ig"] = torch.full((n, 9), 7.5, dtype=torch.float64, device="cuda")
    t["ia"] = torch.full((n, 9), 7.5, dtype=torch.float64, device="cuda")
    p = orbhip.preint_params(nga=nga, nga_walk=WALK, force_form=form, want_info=want_info)
    torch.cuda.synchronize()
    orbhip.preintegrate_device(ctx, p, n, t["off"].data_ptr(), t["meas"].data_ptr(), t["cont"].data_ptr() if start is not None else None,
                               t["rec"].data_ptr(), t["cov"].data_ptr(), t["avg"].data_ptr(), t["info"].data_ptr(), t["ig"].data_ptr(),
                               t["ia"].data_ptr())
    ctx.synchronize()
    return {k: t[k].cpu().numpy() for k in ("rec", "cov", "avg", "info", "ig", "ia")}, t


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CASES)
def test_k_rule_and_reruns(gpu_ctx, name, form):
    bias, meas, nga, ref, f32 = case(name)
    out, _ = run_device(gpu_ctx, bias, meas, nga, FORMS[form])
    again, _ = run_device(gpu_ctx, bias, meas, nga, FORMS[form])
    for k in ("rec", "cov", "avg"):
        assert out[k].tobytes() == again[k].tobytes(), "rerun differs in " + k
    assert out["rec"][:, 61:67].astype(np.float32).tobytes() == np.asarray(bias, np.float32).tobytes()      # the bias is never written
    assert (out["info"] == 7.5).all() and (out["ig"] == 7.5).all()                                          # no info was asked for
    dev = pm.record_fields(out["rec"], out["cov"], out["avg"])
    worst = 0.0
    for g, (ed, ef, fl) in pc.k_rule_ratios(dev, ref, f32).items():
        ratio = ed / (ef + fl) if ed else 0.0
        worst = max(worst, ratio)
        print("%s %s %-8s e_dev %.3e e_f32 %.3e floor %.3e ratio %.2f" % (name, form, g, ed, ef, fl, ratio))
        assert bsm.within_bound(ed, ef, fl), (name, form, g, ed, ef, fl)
    print("%s %s worst ratio %.2f" % (name, form, worst))
    # a fresh chain of length 0 yields Initialize's values
    for c, m in enumerate(meas):
        if len(m) == 0:
            want = np.zeros(61); want[1] = want[5] = want[9] = 1
            assert np.array_equal(out["rec"][c, :61], want) and not out["cov"][c].any() and not out["avg"][c].any()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("split", [1, 64, 65])
def test_continue_equals_one_go(gpu_ctx, split, form):
    bias, meas = pc.single(129)
    b2 = [bias[0], pc.bias(9)]
    whole = [meas[0], pc.chain(30, 9)]
    one, _ = run_device(gpu_ctx, b2, whole, NGA, FORMS[form])
    first, _ = run_device(gpu_ctx, b2, [meas[0][:split], whole[1][:0]], NGA, FORMS[form])
    start = [(first["rec"][c], first["cov"][c], first["avg"][c]) for c in range(2)]
    second, _ = run_device(gpu_ctx, b2, [meas[0][split:], whole[1]], NGA, FORMS[form], start=start)
    for k in ("rec", "cov", "avg"):
        assert one[k].tobytes() == second[k].tobytes(), k
    # a chain that continues with nothing keeps its record; one that starts fresh beside it is not disturbed
    third, _ = run_device(gpu_ctx, b2, [meas[0][:0], whole[1]], NGA, FORMS[form], start=[start[0], None])
    assert third["rec"][0].tobytes() == first["rec"][0].tobytes() and third["cov"][0].tobytes() == first["cov"][0].tobytes()
    assert third["rec"][1].tobytes() == one["rec"][1].tobytes() and third["cov"][1].tobytes() == one["cov"][1].tobytes()


@pytest.mark.parametrize("form", list(FORMS))
def test_nan_stays_in_its_chain(gpu_ctx, form):
    bias, meas = pc.batch(65)
    clean, _ = run_device(gpu_ctx, bias, meas, NGA, FORMS[form])
    sick = [m.copy() for m in meas]
    victim = next(c for c, m in enumerate(meas) if len(m) > 10)
    sick[victim][5, 1] = np.nan
    got, _ = run_device(gpu_ctx, bias, sick, NGA, FORMS[form])
    others = np.arange(65) != victim
    for k in ("rec", "cov", "avg"):
        assert got[k][others].tobytes() == clean[k][others].tobytes(), k
    assert np.isnan(got["rec"][victim, 10:13]).any() and np.isnan(got["cov"][victim]).any()


def _info_case(name):
    """Every chain of the case that has measurements (a chain of length 0 has C = 0 and no information)."""
    if name == "lengths":
        bias, meas = pc.info_lengths()
        return bias, meas, NGA
    bias, meas, nga, _, _ = case(name)
    keep = [c for c, m in enumerate(meas) if len(m) > 0]
    return [bias[c] for c in keep], [meas[c] for c in keep], nga


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["lengths", "batch65", "full_nga"])
def test_information_from_the_device_covariance(gpu_ctx, name, form):
    bias, meas, nga = _info_case(name)
    assert any(len(m) == 1 for m in meas)                                 # the length-1 chain: three exactly singular directions
    if name == "lengths":
        assert sorted(len(m) for m in meas) == [n for n in pc.LENGTHS if n > 0]
    out, _ = run_device(gpu_ctx, bias, meas, nga, FORMS[form], want_info=True)
    worst = 0.0
    for c in range(len(meas)):
        C = out["cov"][c].reshape(15, 15)
        ref, rg, ra, w = pm.information(C, pm.LD)
        thr = 9e-7 * float(np.max(np.abs(w)))
        assert not ((np.abs(w) > thr / 8) & (np.abs(w) < thr * 8)).any(), (name, c, w)       # the case's condition: no eigenvalue near the cut
        if len(meas[c]) == 1:
            assert int((w <= thr).sum()) == 3
        f64, g64, a64, _ = pm.information(C, np.float64)
        for tag, d, r, o in (("info", out["info"][c].reshape(9, 9), ref, f64), ("info_g", out["ig"][c].reshape(3, 3), rg, g64),
                             ("info_a", out["ia"][c].reshape(3, 3), ra, a64)):
            ed = float(np.max(np.abs(d.astype(pm.LD) - r))); eo = float(np.max(np.abs(o.astype(pm.LD) - r)))
            fl = 2.0 ** -52 * float(np.max(np.abs(r)))
            ratio = ed / (eo + fl) if ed else 0.0
            worst = max(worst, ratio)
            assert bsm.within_bound(ed, eo, fl), (name, form, c, tag, ed, eo, fl)
    print("%s %s information worst ratio %.2f" % (name, form, worst))


def test_feeds_the_inertial_optimiser_without_a_host_visit(gpu_ctx):
    """preintegrate_device with want_info -> inertial_optimization_device on the same device arrays; the same solve fed from host copies
    of those arrays gives the same bytes."""
    import torch
    import orbhip
    n = 9
    bias = [pc.bias(40)] * n
    meas = [pc.chain(0, 0)] + [pc.chain(40, 40 + k) for k in range(1, n)]
    out, t = run_device(gpu_ctx, bias, meas, NGA, 0, want_info=True)
    rng = np.random.default_rng(4)
    kf = np.zeros((n, 21)); kf[:, 0] = kf[:, 4] = kf[:, 8] = 1
    kf[:, 9:12] = np.cumsum(rng.normal(0, 0.1, (n, 3)), axis=0); kf[:, 12:15] = rng.normal(0, 0.3, (n, 3))
    kf[:, 15:21] = np.asarray(bias[0], np.float64)
    link = np.ones(n, np.uint8); link[0] = 0
    glob = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0] + [float(v) for v in bias[0]])
    off = np.array([0, n], np.int32)
    prm = orbhip.inertial_opt_params(1)
    prm.iterations = 5

    def solve(d_preint, d_info):
        a = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (("off", off), ("kf", kf), ("link", link), ("glob", glob))}
        st = torch.zeros((1, 8), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        orbhip.inertial_optimization_device(gpu_ctx, prm, 1, a["off"].data_ptr(), a["kf"].data_ptr(), a["link"].data_ptr(), d_preint.data_ptr(),
                                            d_info.data_ptr(), a["glob"].data_ptr(), st.data_ptr())
        gpu_ctx.synchronize()
        return a["kf"].cpu().numpy(), a["glob"].cpu().numpy(), st.cpu().numpy()
    direct = solve(t["rec"], t["info"])
    copies = solve(torch.from_numpy(out["rec"].copy()).cuda(), torch.from_numpy(out["info"].copy()).cuda())
    assert direct[2][0, 0] >= 1 and direct[2][0, 1] >= 1 and np.isfinite(direct[0]).all()      # iterations and LM trials ran
    for a, b in zip(direct, copies):
        assert a.tobytes() == b.tobytes()


def test_host_entry_matches_the_device_entry(gpu_ctx):
    import orbhip
    bias, meas, nga, _, _ = case("batch63")
    for form in FORMS.values():
        dev, _ = run_device(gpu_ctx, bias, meas, nga, form, want_info=True)
        rec, cov, avg, info, ig, ia = orbhip.preintegrate_host(gpu_ctx, orbhip.preint_params(nga=nga, nga_walk=WALK, force_form=form), bias, meas)
        live = np.array([len(m) > 0 for m in meas])
        assert rec.tobytes() == dev["rec"].tobytes() and cov.reshape(-1, 225).tobytes() == dev["cov"].tobytes() and avg.tobytes() == dev["avg"].tobytes()
        assert info.reshape(-1, 81)[live].tobytes() == dev["info"][live].tobytes() and ig.reshape(-1, 9)[live].tobytes() == dev["ig"][live].tobytes()


def test_argument_errors_write_nothing(gpu_ctx):
    import torch
    import orbhip
    n = 3
    rec = torch.full((n, 67), 7.5, dtype=torch.float64, device="cuda"); cov = torch.full((n, 225), 7.5, device="cuda")
    avg = torch.full((n, 6), 7.5, device="cuda"); info = torch.full((n, 99), 7.5, dtype=torch.float64, device="cuda")
    meas = torch.zeros((20, 7), device="cuda")
    good = torch.tensor([0, 5, 5, 9], dtype=torch.int32, device="cuda"); bad = torch.tensor([0, 5, 4, 9], dtype=torch.int32, device="cuda")
    neg = torch.tensor([-1, 5, 6, 9], dtype=torch.int32, device="cuda")
    p = orbhip.preint_params()
    torch.cuda.synchronize()
    ip = info.data_ptr()

    def call(params, chains, off, m, r, c, a, i=ip):
        with pytest.raises(orbhip.OrbHipError) as e:
            orbhip.preintegrate_device(gpu_ctx, params, chains, off, m, None, r, c, a, i, i + 8 * 81 * n, i + 8 * 90 * n)
        assert e.value.code == -1
    call(p, -1, good.data_ptr(), meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    call(p, n, bad.data_ptr(), meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    call(p, n, neg.data_ptr(), meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    call(p, n, None, meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    call(p, n, good.data_ptr(), None, rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    call(p, n, good.data_ptr(), meas.data_ptr(), None, cov.data_ptr(), avg.data_ptr())
    call(p, n, good.data_ptr(), meas.data_ptr(), rec.data_ptr(), None, avg.data_ptr())
    call(p, n, good.data_ptr(), meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), None)
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.preintegrate_device(gpu_ctx, p, n, good.data_ptr(), meas.data_ptr(), None, rec.data_ptr(), cov.data_ptr(), avg.data_ptr(), None, None, None)
    assert e.value.code == -1
    q = orbhip.preint_params(force_form=7)
    call(q, n, good.data_ptr(), meas.data_ptr(), rec.data_ptr(), cov.data_ptr(), avg.data_ptr())
    gpu_ctx.synchronize()
    for x in (rec, cov, avg, info):
        assert bool((x == 7.5).all())
    # chains == 0 succeeds and launches nothing; without want_info the info arrays may be absent
    orbhip.preintegrate_device(gpu_ctx, p, 0, None, None, None, None, None, None)
    orbhip.preintegrate_device(gpu_ctx, orbhip.preint_params(want_info=False), n, good.data_ptr(), meas.data_ptr(), None, rec.data_ptr(),
                               cov.data_ptr(), avg.data_ptr())
    gpu_ctx.synchronize()
    assert bool((info == 7.5).all()) and not bool((rec[:, :61] == 7.5).all())


def test_host_entry_argument_errors_write_nothing(gpu_ctx):
    """orbhip_preintegrate_host runs the same argument rules (one function for both entries) on its host arrays."""
    import ctypes as C
    import orbhip
    n = 3
    rec = np.full((n, 67), 7.5); cov = np.full((n, 225), 7.5, np.float32); avg = np.full((n, 6), 7.5, np.float32)
    info = np.full((n, 81), 7.5); ig = np.full((n, 9), 7.5); ia = np.full((n, 9), 7.5)
    meas = np.zeros((20, 7), np.float32)
    good, bad, neg = (np.array(v, np.int32) for v in ([0, 5, 5, 9], [0, 5, 4, 9], [-1, 5, 6, 9]))
    p = orbhip.preint_params()
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(params, chains, off, m, r, c, a, i=info, g=ig, h=ia):
        return orbhip.lib.orbhip_preintegrate_host(gpu_ctx.h, C.byref(params), chains, ptr(off), ptr(m), None, ptr(r), ptr(c), ptr(a), ptr(i), ptr(g), ptr(h))
    assert call(p, -1, good, meas, rec, cov, avg) == -1
    assert call(p, n, bad, meas, rec, cov, avg) == -1
    assert call(p, n, neg, meas, rec, cov, avg) == -1
    assert call(p, n, None, meas, rec, cov, avg) == -1
    assert call(p, n, good, None, rec, cov, avg) == -1
    assert call(p, n, good, meas, None, cov, avg) == -1
    assert call(p, n, good, meas, rec, None, avg) == -1
    assert call(p, n, good, meas, rec, cov, None) == -1
    assert call(p, n, good, meas, rec, cov, avg, None, None, None) == -1
    assert call(orbhip.preint_params(force_form=7), n, good, meas, rec, cov, avg) == -1
    for x in (rec, cov, avg, info, ig, ia):
        assert (x == 7.5).all()
    assert call(p, 0, None, None, None, None, None, None, None, None) == 0
    assert call(orbhip.preint_params(want_info=False), n, good, meas, rec, cov, avg, None, None, None) == 0
    assert (info == 7.5).all() and not (rec[:, :61] == 7.5).all()
