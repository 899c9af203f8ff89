"""orbhip_two_view_reconstruct_device / _host against the numpy model (tests/two_view_model.py) on the batch of tests/synth_two_view.py:
scoring (exact up to the order of a float sum), hypotheses (against the float64 model, yardstick = the float32 model's own distance from
it, computed live), winners and decisions, outputs, reset values and untouched rows, the extract -> match -> reconstruct chain with
device-drawn sets, byte-identical second runs.

Motion hypotheses are compared as (R, t) pairs and as multisets of nGood, not by their number: the numbering depends on the signs a
singular value decomposition happens to give its vectors (numpy's differ from OpenCV's too), the set of hypotheses does not.

Measured on an MI355X, the 24-pair batch under rh_threshold 0.50 (every figure is printed before its assertion):
  (4) chi-squares within 1e-3 of their threshold: 1.3e-4 of 4.5 M evaluations (cap 1 %); scores within the bound on every hypothesis
  (5) score gap to the float64 model / best score: device p95 6.4e-6, max 1.3e-3; float32 numpy model p95 8.1e-6, max 9.5e-4 (bound: 4 x)
  (6) every winner equal except iter_f of the 8-match pair (3e-14 below the best: one exit); every nGood, decision and parallax equal
  (7) R21 / t21 within 0.0002 degrees of the float64 model; vP3D within 4.5e-6 relative; no flag differs, no match inside a band
  chain (8 pairs, 58-79 matches): (4) 4.3e-4, (5) device p95 6.5e-6 max 3.1e-3, float32 model p95 8.4e-6 max 3.4e-3"""
import numpy as np
import pytest
import ransac_sets_model as rs
import two_view_model as tv
import synth_two_view as sy

pytestmark = pytest.mark.gpu

ITER = 200
BAND = 1e-3
POISON = 0x5A


def _kp_array(orbhip, rows, max_n):
    a = np.zeros((len(rows), max_n), orbhip.KP_DTYPE)
    for p, xy in enumerate(rows):
        a[p, :len(xy)]["x"] = xy[:, 0]
        a[p, :len(xy)]["y"] = xy[:, 1]
    return a


def _run_device(ctx, pairs, max_n, rh, draw_sets, seed=0, sets=None, spare=2, d_inputs=None, iters=ITER):
    """pairs: list of dicts (kp1, kp2, matches12).  One rh_threshold per call.  Runs twice (byte-identical) -> dict of numpy outputs.
    d_inputs: (d_kp1, d_n1, d_kp2, d_n2, stride, d_m12) device addresses to use instead of uploading."""
    import torch
    import orbhip
    P = len(pairs)
    keep = []
    if d_inputs is None:
        kp1 = _kp_array(orbhip, [s["kp1"] for s in pairs], max_n); kp2 = _kp_array(orbhip, [s["kp2"] for s in pairs], max_n)
        n1 = np.array([len(s["kp1"]) for s in pairs], np.int32); n2 = np.array([len(s["kp2"]) for s in pairs], np.int32)
        m12 = np.full((P, max_n), -1, np.int32)
        for p, s in enumerate(pairs):
            m12[p, :n1[p]] = s["matches12"]
        keep = [torch.from_numpy(a.view(np.uint8) if a.dtype == orbhip.KP_DTYPE else a).cuda() for a in (kp1, n1, kp2, n2, m12)]
        d_inputs = (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), max_n, keep[4].data_ptr())
    prm = orbhip.tvr_params(iters, 1.0, rh, draw_sets, seed)
    outs = []
    for _ in range(2):
        Q = P + spare
        d_sets = torch.full((Q, iters, 8), -7, dtype=torch.int32, device="cuda")
        if sets is not None:
            d_sets[:P] = torch.from_numpy(np.ascontiguousarray(sets, np.int32)).cuda()
        ok = torch.full((Q,), POISON, dtype=torch.uint8, device="cuda")
        R = torch.full((Q, 9), 7.5, dtype=torch.float32, device="cuda"); t = torch.full((Q, 3), 7.5, dtype=torch.float32, device="cuda")
        P3D = torch.full((Q, max_n, 3), 7.5, dtype=torch.float32, device="cuda")
        tri = torch.full((Q, max_n), POISON, dtype=torch.uint8, device="cuda")
        st = torch.full((Q, 72), POISON, dtype=torch.uint8, device="cuda")
        hs = torch.full((Q, iters, 2), 7.5, dtype=torch.float32, device="cuda")
        hm = torch.full((Q, iters, 2, 9), 7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        orbhip.two_view_reconstruct_device(ctx, d_inputs[0], d_inputs[1], d_inputs[2], d_inputs[3], d_inputs[4], d_inputs[5], P, max_n, sy.K4,
                                           prm, d_sets.data_ptr(), ok.data_ptr(), R.data_ptr(), t.data_ptr(), P3D.data_ptr(), tri.data_ptr(),
                                           st.data_ptr(), hs.data_ptr(), hm.data_ptr())
        ctx.check_status()
        outs.append(dict(sets=d_sets.cpu().numpy(), ok=ok.cpu().numpy(), R=R.cpu().numpy(), t=t.cpu().numpy(), P3D=P3D.cpu().numpy(),
                         tri=tri.cpu().numpy(), stats=st.cpu().numpy().view(orbhip.TVR_STATS_DTYPE).reshape(Q), scores=hs.cpu().numpy(),
                         mats=hm.cpu().numpy()))
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), "second run differs in " + k
    return outs[0]


def _models(pairs, rhs, sets):
    m64 = [tv.reconstruct(s["kp1"], s["kp2"], s["matches12"], sy.K4, sets[p], np.float64, rh_threshold=rhs[p]) for p, s in enumerate(pairs)]
    m32 = [tv.reconstruct(s["kp1"], s["kp2"], s["matches12"], sy.K4, sets[p], np.float32, rh_threshold=rhs[p]) for p, s in enumerate(pairs)]
    return m64, m32


def _gaps(scores, m64):
    """|score - float64 model's score| / the pair's best float64 score of that model, over every (pair, iteration, model) -> flat array;
    NaN on both sides counts as agreement, on one side as an infinite gap"""
    out = []
    for p, o in enumerate(m64):
        if o["scores"] is None:
            continue
        a, b = np.asarray(scores[p], np.float64), np.asarray(o["scores"], np.float64)
        best = np.maximum(np.nanmax(np.where(np.isfinite(b), b, 0), axis=0), 1e-30)
        g = np.abs(a - b) / best
        both = np.isnan(a) & np.isnan(b)
        g[both] = 0
        g[np.isnan(g)] = np.inf
        out.append(g.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


def _check_all(pairs, rhs, names, dev, sets, truth=True):
    """checks (4)-(7) of the feature's acceptance list for one device run"""
    P = len(pairs)
    m64, m32 = _models(pairs, rhs, sets)
    f32 = np.float32
    # ---- (4) scoring is the reference's: the float32 model's CheckHomography / CheckFundamental on the device's own matrices
    inband = total = 0
    for p, o in enumerate(m64):
        N = o["N"]
        if N < 8:
            assert np.all(dev["scores"][p] == 0) and np.all(dev["mats"][p] == 0), names[p]
            continue
        for model, th in ((0, tv.TH_H), (1, tv.TH_F)):
            M = dev["mats"][p, :, model].reshape(ITER, 3, 3)
            c1, c2 = tv.chi_h(M, tv.inv3(M, f32), o["p1"], o["p2"], f32) if model == 0 else tv.chi_f(M, o["p1"], o["p2"], f32)
            sc, _ = tv.score_from_chi(c1, c2, th, 1.0, f32)
            nb = (np.abs(c1.astype(np.float64) - th) <= BAND * th).astype(int) + (np.abs(c2.astype(np.float64) - th) <= BAND * th).astype(int)
            inband += int(nb.sum()); total += 2 * nb.size
            d = dev["scores"][p, :, model]
            assert np.array_equal(np.isnan(d), np.isnan(sc)), (names[p], model)
            fin = np.isfinite(sc)
            tol = N * 2.0 ** -24 * np.abs(sc[fin].astype(np.float64)) + th * BAND * nb.sum(-1)[fin] + 1e-30
            err = np.abs(d[fin].astype(np.float64) - sc[fin])
            assert np.all(err <= tol), (names[p], model, float(np.max(err - tol)))
    share = inband / max(total, 1)
    print("(4) chi-squares within 1e-3 of their threshold: %.3g of %d evaluations" % (share, total))
    assert share <= 0.01
    # ---- (5) the hypotheses are right: device scores against the float64 model's, yardstick = the float32 model's own gap
    g_dev = _gaps(dev["scores"], m64)
    g_f32 = _gaps([o["scores"] for o in m32 if o["scores"] is not None], [o for o in m64 if o["scores"] is not None])
    p95_d, max_d = np.percentile(g_dev, 95), g_dev.max()
    p95_m, max_m = np.percentile(g_f32, 95), g_f32.max()
    print("(5) score gap to the float64 model / best score: device p95 %.3g max %.3g; float32 model p95 %.3g max %.3g" % (p95_d, max_d, p95_m, max_m))
    assert p95_d <= 4 * max(p95_m, 1e-4) and max_d <= 4 * max_m
    live_gap = 4 * max_m
    # ---- (6) winners and decisions
    exits_w = exits_d = 0
    for p, o in enumerate(m64):
        st = dev["stats"][p]
        N = o["N"]
        assert st["n_matches"] == N, names[p]
        if N < 8:
            assert st["model"] == 0 and st["iter_h"] == -1 and st["iter_f"] == -1 and dev["ok"][p] == 0, names[p]
            continue
        for key, ref, col in (("iter_h", o["iH"], 0), ("iter_f", o["iF"], 1)):
            if st[key] != ref:
                s64 = o["scores"][:, col]
                best = np.nanmax(s64)
                assert st[key] >= 0 and (best - s64[st[key]]) / best <= live_gap, (names[p], key, int(st[key]), ref)
                exits_w += 1
                print("(6) %s: %s %d where the float64 model has %d (its score of the device's winner is %.3g below its best)"
                      % (names[p], key, st[key], ref, (best - s64[st[key]]) / best))
        SH, SF = f32(st["score_h"]), f32(st["score_f"])
        model = 0 if SH + SF == 0 else (1 if SH / (SH + SF) > f32(rhs[p]) else 2)
        if model and st["iter_h" if model == 1 else "iter_f"] < 0:
            model = 0
        assert st["model"] == model, names[p]
        if o["RH"] is not None and abs(o["RH"] - rhs[p]) > 1e-3:
            assert st["model"] == o["model"], (names[p], st["model"], o["model"], o["RH"])
        if model == 0:
            assert dev["ok"][p] == 0
            continue
        # the model's decision on the device's winning matrix
        M = dev["mats"][p, st["iter_h" if model == 1 else "iter_f"], model - 1].reshape(3, 3)
        inl = (tv.check_homography(M, o["p1"], o["p2"], 1.0, f32) if model == 1 else tv.check_fundamental(M, o["p1"], o["p2"], 1.0, f32))[1]
        assert st["n_inliers"] == int(inl.sum()), (names[p], int(st["n_inliers"]), int(inl.sum()))
        rec = tv.reconstruct_from(model, M, inl, sy.K4, o["p1"], o["p2"], f32)
        tol = max(1, int(0.01 * N))
        ng_d = sorted(int(x) for x in st["n_good"][:st["n_hyp"]])
        ng_m = sorted(rec["n_good"])
        print("(6) %-16s N %3d model %d inliers %3d nGood device %s model %s parallax %.3f / %.3f ok %d / %d" %
              (names[p], N, model, st["n_inliers"], list(st["n_good"][:st["n_hyp"]]), rec["n_good"], st["parallax"], rec["parallax"], dev["ok"][p], rec["ok"]))
        assert len(ng_d) == len(ng_m) and all(abs(a - b) <= tol for a, b in zip(ng_d, ng_m)), (names[p], ng_d, ng_m)
        if bool(dev["ok"][p]) != rec["ok"] or (st["hyp_index"] >= 0) != (rec["sel"] >= 0):
            assert rec["margin"] <= tol or rec["par_margin"] <= 0.01, (names[p], dev["ok"][p], rec["ok"], rec["margin"], rec["par_margin"])
            exits_d += 1
            continue
        if rec["sel"] >= 0:
            assert abs(int(st["n_good"][st["hyp_index"]]) - rec["n_good"][rec["sel"]]) <= tol, names[p]
            assert abs(st["parallax"] - rec["parallax"]) <= max(0.01, 1e-3 * rec["parallax"]), (names[p], st["parallax"], rec["parallax"])
        # ---- (7) outputs
        n1 = len(pairs[p]["kp1"])
        if rec["ok"]:
            R, t = dev["R"][p].reshape(3, 3), dev["t"][p]
            Rm, tm = rec["hyps"][rec["sel"]]
            assert abs(np.linalg.norm(t.astype(np.float64)) - 1) <= 1e-6, names[p]
            assert tv.rot_angle_deg(R, Rm) <= 0.01 and tv.dir_angle_deg(t, tm) <= 0.01, (names[p], tv.rot_angle_deg(R, Rm), tv.dir_angle_deg(t, tm))
            if o["ok"] and m32[p]["ok"]:
                dR, dt_ = tv.rot_angle_deg(R, o["R"]), tv.dir_angle_deg(t, o["t"])
                lR, lt = tv.rot_angle_deg(m32[p]["R"], o["R"]), tv.dir_angle_deg(m32[p]["t"], o["t"])
                print("(7) %-16s device vs float64 model R %.4f t %.4f deg; float32 model vs float64 R %.4f t %.4f deg" % (names[p], dR, dt_, lR, lt))
                assert dR <= max(4 * lR, 0.01) and dt_ <= max(4 * lt, 0.01), names[p]
                if truth and np.linalg.norm(pairs[p]["t"]) > 0:
                    assert tv.rot_angle_deg(R, pairs[p]["R"]) <= 1.5 * tv.rot_angle_deg(o["R"], pairs[p]["R"]) + 0.05, names[p]
                    assert tv.dir_angle_deg(t, pairs[p]["t"]) <= 1.5 * tv.dir_angle_deg(o["t"], pairs[p]["t"]) + 0.05, names[p]
            i1 = o["i1"]
            tri_m = np.zeros(n1, bool); tri_m[i1[rec["rt"]["good"]]] = True
            edge = np.zeros(n1, bool); edge[i1[rec["rt"]["edge"]]] = True
            tri_d = dev["tri"][p, :n1].astype(bool)
            assert edge.sum() <= max(1, 0.01 * N), (names[p], int(edge.sum()))
            assert np.array_equal(tri_d[~edge], tri_m[~edge]), (names[p], int((tri_d != tri_m).sum()))
            both = tri_d & tri_m
            Xm = np.zeros((n1, 3)); Xm[i1[rec["rt"]["keep"]]] = rec["rt"]["X"][rec["rt"]["keep"]]
            Xd = dev["P3D"][p, :n1].astype(np.float64)
            rel = np.linalg.norm(Xd[both] - Xm[both], axis=1) / np.linalg.norm(Xm[both], axis=1)
            print("(7) %-16s %d triangulated, vP3D relative difference max %.3g" % (names[p], int(both.sum()), rel.max() if len(rel) else 0))
            assert np.all(rel <= 1e-3), names[p]
            unmatched = np.ones(n1, bool); unmatched[i1] = False
            assert not tri_d[unmatched].any() and not Xd[unmatched].any(), names[p]
    print("(6) exits used: winners %d, decisions %d" % (exits_w, exits_d))
    assert exits_w <= 1 and exits_d <= 1
    # failures leave the reset values; rows beyond n1 and pairs beyond the batch are untouched
    for p in range(P):
        n1 = len(pairs[p]["kp1"])
        if not dev["ok"][p]:
            assert dev["ok"][p] == 0 and not dev["R"][p].any() and not dev["t"][p].any(), names[p]
            assert not dev["P3D"][p, :n1].any() and not dev["tri"][p, :n1].any(), names[p]
        else:
            assert dev["ok"][p] == 1
        assert np.all(dev["P3D"][p, n1:] == 7.5) and np.all(dev["tri"][p, n1:] == POISON), names[p]
    assert np.all(dev["ok"][P:] == POISON) and np.all(dev["R"][P:] == 7.5) and np.all(dev["t"][P:] == 7.5)
    assert np.all(dev["P3D"][P:] == 7.5) and np.all(dev["tri"][P:] == POISON) and np.all(dev["scores"][P:] == 7.5) and np.all(dev["sets"][P:] == -7)
    assert np.all(dev["stats"][P:].view(np.uint8) == POISON)
    return m64


@pytest.mark.parametrize("rh", [0.50, 0.40])
def test_batch_against_the_model(gpu_ctx, rh):
    """the whole committed batch in ONE call (>= 24 pairs: general, planes, low parallax, edge cases, ragged counts, max_n 8192 with 5000
    keypoints per frame), caller's sets, under the reference's rh_threshold 0.50 and under 0.40 (which sends the planar and the
    low-parallax pairs down ReconstructH)"""
    entries = sy.batch()
    names = [e[0] for e in entries]; pairs = [e[1] for e in entries]
    Ns = [len(tv.match_list(s["matches12"], len(s["kp2"]))[0]) for s in pairs]
    sets = np.stack([sy.model_sets(names[p], Ns[p], ITER) for p in range(len(pairs))])
    dev = _run_device(gpu_ctx, pairs, 8192, rh, False, sets=sets)
    assert np.array_equal(dev["sets"][:len(pairs)], sets)
    _check_all(pairs, [rh] * len(pairs), names, dev, sets)
    models = [int(m) for m in dev["stats"]["model"][:len(pairs)]]
    print(dict(zip(names, zip(dev["ok"][:len(pairs)].tolist(), models))))
    assert len(pairs) >= 24 and dev["ok"][:len(pairs)].sum() >= 3
    if rh == 0.40:
        assert sum(m == 1 for m in models) >= 8 and sum(bool(o) and m == 1 for o, m in zip(dev["ok"], models)) >= 5      # ReconstructH ran and succeeded


def test_capacity_and_arguments(gpu_ctx):
    import torch
    import orbhip
    z = torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    prm = orbhip.tvr_params(ITER)
    args = lambda max_n, p: (gpu_ctx, z, z, z, z, max_n, z, 1, max_n, sy.K4, p, z, z, z, z, z, z)
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.two_view_reconstruct_device(*args(8193, prm))
    assert e.value.code == orbhip.E_CAPACITY
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.two_view_reconstruct_device(*args(16, orbhip.tvr_params(1025)))
    assert e.value.code == orbhip.E_CAPACITY
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.two_view_reconstruct_device(*args(16, orbhip.tvr_params(0)))
    assert e.value.code == orbhip.E_BADARG


def test_host_form_equals_device_form(gpu_ctx):
    """orbhip_two_view_reconstruct_host on one pair = the batched call on that pair, bit for bit; with draw_sets it returns the sets"""
    import orbhip
    name, sc, rh = sy.batch()[0]
    N = len(tv.match_list(sc["matches12"], len(sc["kp2"]))[0])
    sets = sy.model_sets(name, N, ITER)
    dev = _run_device(gpu_ctx, [sc], 2048, rh, False, sets=sets[None])
    kp1 = _kp_array(orbhip, [sc["kp1"]], len(sc["kp1"]))[0]; kp2 = _kp_array(orbhip, [sc["kp2"]], len(sc["kp2"]))[0]
    ok, R, t, P3D, tri, st, s_out = orbhip.two_view_reconstruct_host(gpu_ctx, kp1, kp2, sc["matches12"], sy.K4, orbhip.tvr_params(ITER, 1.0, rh, False), sets)
    n1 = len(kp1)
    assert ok == bool(dev["ok"][0]) and ok
    assert R.tobytes() == dev["R"][0].tobytes() and t.tobytes() == dev["t"][0].tobytes()
    assert P3D.tobytes() == dev["P3D"][0, :n1].tobytes() and np.array_equal(tri, dev["tri"][0, :n1].astype(bool))
    assert st.tobytes() == dev["stats"][0].tobytes() and np.array_equal(s_out, sets)
    r2 = orbhip.two_view_reconstruct_host(gpu_ctx, kp1, kp2, sc["matches12"], sy.K4, orbhip.tvr_params(ITER, 1.0, rh, True, 5))
    s2 = r2[6]
    assert s2.min() >= 0 and s2.max() < N and all(len(set(row)) == 8 for row in s2.tolist())


def _check_sets(sets, Ns):
    for p, N in enumerate(Ns):
        if N < 8:
            assert np.all(sets[p] == -1), p
            continue
        s = np.sort(sets[p], axis=1)
        assert s.min() >= 0 and s.max() < N and np.all(s[:, 1:] != s[:, :-1]), p


def test_device_drawn_sets_are_the_models(gpu_ctx):
    """the 8-draw sets exactly (tests/ransac_sets_model.py): one pair's match list cut to N = 7 (no set), 8 and 9 (every draw meets a
    moved slot or the last one) and 20 matches; 300 iterations take the prepare kernel's 256 threads on a second trip; seed 5 and a seed
    above 2^63"""
    name, sc, rh = sy.batch()[0]
    valid = tv.match_list(sc["matches12"], len(sc["kp2"]))[0]
    Ns = (7, 8, 9, 20)
    assert len(valid) >= max(Ns)
    pairs = []
    for N in Ns:
        m12 = np.full(len(sc["matches12"]), -1, np.int32)
        m12[valid[:N]] = np.asarray(sc["matches12"])[valid[:N]]
        pairs.append(dict(sc, matches12=m12))
    for seed in (5, 2 ** 63 + 7):
        dev = _run_device(gpu_ctx, pairs, 2048, rh, True, seed=seed, iters=300)
        _check_sets(dev["sets"], Ns)
        for p, N in enumerate(Ns):
            assert np.array_equal(dev["sets"][p], rs.device_sets(seed, p, N, 300, 8)), (seed, N)


def test_chain_extract_match_reconstruct(gpu_ctx):
    """Extractor.extract_device -> search_for_initialization_device -> two_view_reconstruct_device(draw_sets = 1) with no host copy in
    between; the sets the device drew are read back, checked, and (4)-(7) run with them"""
    import torch
    import orbhip
    B, W, H = 9, 640, 480
    imgs = orbhip.synth_frames(W, H, B, seed=991, first=0)
    d = torch.from_numpy(imgs).cuda()
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7); ext.reserve(W, H, B)
    mk = ext.max_keypoints
    kp, desc, cnt, _ = ext.results_device()
    prev = torch.zeros((B, mk, 2), dtype=torch.float32, device="cuda")
    m12 = torch.full((B, mk), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
    P = B - 1
    assert mk <= 8192
    d_in = (kp, cnt, kp + mk * 28, cnt + 4, mk, m12.data_ptr())

    def chain(seed):
        ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
        orbhip.prev_matched_init_device(gpu_ctx, kp, mk, P, mk, prev.data_ptr())
        orbhip.search_for_initialization_device(gpu_ctx, kp, desc, cnt, kp + mk * 28, desc + mk * 32, cnt + 4, P, mk, mk, (0.0, 0.0, float(W), float(H)),
                                                100, 0.9, True, prev.data_ptr(), m12.data_ptr(), nm.data_ptr())
        return _run_device(gpu_ctx, [None] * P, mk, 0.5, True, seed=seed, d_inputs=d_in)
    dev = chain(3)
    dev_same = chain(3)
    dev_other = chain(4)
    for k in dev:
        assert dev[k].tobytes() == dev_same[k].tobytes(), k
    # the model's inputs: what the chain left on the device
    gpu_ctx.synchronize()
    counts = _from_device(cnt, B * 4).view(np.int32)
    kps = _from_device(kp, B * mk * 28).view(orbhip.KP_DTYPE).reshape(B, mk)
    m = m12.cpu().numpy()
    pairs = []
    for p in range(P):
        a, b = kps[p, :counts[p]], kps[p + 1, :counts[p + 1]]
        pairs.append(dict(kp1=np.c_[a["x"], a["y"]].astype(np.float32), kp2=np.c_[b["x"], b["y"]].astype(np.float32), matches12=m[p, :counts[p]]))
    Ns = [len(tv.match_list(s["matches12"], len(s["kp2"]))[0]) for s in pairs]
    print("chain: matches per pair", Ns, "ok", dev["ok"][:P].tolist())
    assert max(Ns) >= 8
    _check_sets(dev["sets"], Ns)
    assert any(not np.array_equal(dev["sets"][p], dev_other["sets"][p]) for p in range(P) if Ns[p] >= 8)
    sets = np.where(dev["sets"][:P] < 0, 0, dev["sets"][:P])
    _check_all(pairs, [0.5] * P, ["chain_%d" % p for p in range(P)], dev, sets, truth=False)
    ext.close()


def _from_device(addr, nbytes):
    """nbytes at a raw device address -> numpy uint8"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dst = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(dst.ctypes.data, addr, nbytes, 2) == 0
    return dst


@pytest.mark.parametrize("case", ["general", "planar", "fisheye"])
def test_class_through_host_smoke(tmp_path, case):
    """lib/host_smoke tvr: GeometricCamera::ReconstructWithTwoViews -> TwoViewReconstruction::Reconstruct on the GPU, against the float64
    model fed the sets the class drew (the class has the reference's fixed rh_threshold 0.50)"""
    import os
    import subprocess
    sc = sy.scene("plane_a", 1) if case == "planar" else sy.scene("general", 1)
    cam, cam_type, keys = sy.K4, 0, sc
    if case == "fisheye":
        cam, cam_type = sy.KB8_CAM, 1
        keys = dict(sc, kp1=sy.kb8_distort(sc["kp1"].astype(np.float64), cam).astype(np.float32),
                    kp2=sy.kb8_distort(sc["kp2"].astype(np.float64), cam).astype(np.float32))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fin, fout = str(tmp_path / "tvr.in"), str(tmp_path / "tvr.out")
    sy.write_flat(fin, dict(kp1=keys["kp1"], kp2=keys["kp2"], matches=keys["matches12"], cam_type=np.array([cam_type]), cam=np.array(cam, np.float32)))
    r = subprocess.run([os.path.join(root, "orb-slam3-mac_amd", "lib", "host_smoke"), "tvr", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and "tvr:" in r.stdout, r.stdout[-3000:]
    out = sy.read_flat(fout)
    n1 = len(sc["kp1"])
    assert out["sizes"].tolist() == [n1, n1, n1]
    sets = out["sets"].reshape(ITER, 8)
    o64 = tv.reconstruct(sc["kp1"], sc["kp2"], sc["matches12"], sy.K4, sets, np.float64)
    o32 = tv.reconstruct(sc["kp1"], sc["kp2"], sc["matches12"], sy.K4, sets, np.float32)
    assert bool(out["ok"][0]) == o64["ok"], (case, out["ok"], o64["ok"])
    if case == "fisheye":
        assert np.abs(out["un1"].reshape(-1, 2) - sc["kp1"]).max() <= 1e-3
    if not o64["ok"]:
        assert out["R21"].size == 0 and out["t21"].size == 0 and not out["P3D"].any() and not out["tri"].any()
        return
    R, t = out["R21"].reshape(3, 3), out["t21"]
    dR, dt_ = tv.rot_angle_deg(R, o64["R"]), tv.dir_angle_deg(t, o64["t"])
    lR, lt = tv.rot_angle_deg(o32["R"], o64["R"]), tv.dir_angle_deg(o32["t"], o64["t"])
    print("class %s: against the float64 model R %.4f t %.4f deg; float32 model R %.4f t %.4f deg" % (case, dR, dt_, lR, lt))
    assert dR <= max(4 * lR, 0.01) and dt_ <= max(4 * lt, 0.01)
    assert abs(np.linalg.norm(t.astype(np.float64)) - 1) <= 1e-6
    assert tv.rot_angle_deg(R, sc["R"]) <= 1.5 * tv.rot_angle_deg(o64["R"], sc["R"]) + 0.05
    assert tv.dir_angle_deg(t, sc["t"]) <= 1.5 * tv.dir_angle_deg(o64["t"], sc["t"]) + 0.05
    tri = out["tri"].astype(bool)
    assert (tri != o64["tri"]).sum() <= max(1, 0.01 * o64["N"])
