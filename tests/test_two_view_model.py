"""The numpy model of TwoViewReconstruction::Reconstruct (tests/two_view_model.py) on the committed scenes (tests/synth_two_view.py):
what the float64 model returns per family, float32 against float64, and the two caps the GPU tests lean on, established for the models
alone: a float32 and a float64 chi-square of one and the same matrix fall on different sides of their threshold only within a relative
1e-3 of it, and such values are at most 1 % of all (pair, iteration, match, direction) evaluations."""
import numpy as np
import two_view_model as tv
import synth_two_view as sy

ITER = 200


def _run(name, sc, rh, dt):
    N = len(tv.match_list(sc["matches12"], len(sc["kp2"]))[0])
    return tv.reconstruct(sc["kp1"], sc["kp2"], sc["matches12"], sy.K4, sy.model_sets(name, N, ITER), dt, rh_threshold=rh)


def test_float64_model_on_the_committed_scenes():
    res = {name: (_run(name, sc, rh, np.float64), sc) for name, sc, rh in sy.batch()}
    assert len(res) >= 24
    for name, (o, sc) in res.items():
        fam = name.rsplit("_", 1)[0]
        if fam == "general":
            assert o["model"] == 2 and 0.09 <= o["RH"] <= 0.18, (name, o["RH"])
        if fam in ("plane_a", "plane_b"):                                  # rh_threshold 0.40: the H branch, success on every seed
            assert o["model"] == 1 and 0.45 <= o["RH"] <= 0.48 and o["ok"], (name, o["RH"], o["ok"])
        if fam == "plane_a_rh50":                                          # the reference's 0.50: planar scenes go to F
            assert o["model"] == 2 and not o["ok"], name
        if fam == "plane_far":                                             # Faugeras' twin solution has as many good points: false
            assert o["model"] == 1 and not o["ok"] and o["rec"]["n_good"][1] > 0.75 * o["rec"]["n_good"][0], name
        if fam in ("lowpar", "lowpar_h"):
            assert not o["ok"], name
        if o["ok"] and fam in ("general", "plane_a", "plane_b"):
            eR, et = tv.rot_angle_deg(o["R"], sc["R"]), tv.dir_angle_deg(o["t"], sc["t"])
            assert eR <= 1.0 and et <= 3.0, (name, eR, et)
            assert abs(np.linalg.norm(o["t"]) - 1) < 1e-12
    ok = {n: o["ok"] for n, (o, _) in res.items()}
    assert [ok["general_%d" % s] for s in (1, 2, 4, 8)] == [True, False, True, True]
    g2 = res["general_2"][0]["rec"]
    assert max(g2["n_good"]) < 0.9 * g2["n_inl"]                           # the failing seed fails on maxGood < 0.9 N
    lp = res["lowpar_1"][0]["rec"]
    assert sum(g > 0.7 * max(lp["n_good"]) for g in lp["n_good"]) > 1      # F branch on low parallax: no clear winner
    lh = res["lowpar_h_1"][0]
    assert lh["model"] == 1 and 0.05 <= lh["rec"]["parallax"] <= 0.3       # H branch on low parallax: 0.1-0.2 degrees
    for name in ("zero_matches", "seven_matches"):
        o = res[name][0]
        assert o["N"] in (0, 7) and not o["ok"] and o["model"] == 0 and not o["tri"].any() and not o["P3D"].any()
    assert res["eight_matches"][0]["N"] == 8 and not res["eight_matches"][0]["ok"]
    assert not res["all_wrong"][0]["ok"]
    ident = res["identical"][0]
    assert not ident["ok"] and abs(ident["RH"] - 0.5) < 1e-6              # SH and SF maximal: 2 * 5.991 per match each
    assert abs(ident["SH"] - 2 * tv.TH_SCORE * ident["N"]) < 1e-3 * ident["SH"]
    sc = res["identical"][1]
    o40 = _run("identical", sc, 0.40, np.float64)
    assert o40["model"] == 1 and not o40["ok"] and o40["rec"]["hyps"] == []   # d1/d2 < 1.00001: ReconstructH returns before CheckRT
    assert len(res["ragged_small"][1]["kp1"]) != len(res["ragged_small"][1]["kp2"])
    assert len(res["big_5000"][1]["kp1"]) == 5000


def test_float32_and_float64_models_agree():
    """every success flag and every winner index; a winner may differ only where the float64 model scores the other winner within the
    float32-against-float64 score gap of the batch of its own best (the eight-match pair: every set is the same eight points), once"""
    runs = [(name, _run(name, sc, rh, np.float32), _run(name, sc, rh, np.float64)) for name, sc, rh in sy.batch()]
    gaps = []
    for name, a, b in runs:
        if b["scores"] is not None:
            best = np.maximum(np.nanmax(b["scores"], axis=0), 1e-30)
            g = np.abs(a["scores"].astype(np.float64) - b["scores"]) / best
            gaps.append(g[np.isfinite(g)])
    gaps = np.concatenate(gaps)
    print("float32 against float64 score gap / best: p95 %.3g max %.3g" % (np.percentile(gaps, 95), gaps.max()))
    exits = 0
    for name, a, b in runs:
        assert a["ok"] == b["ok"] and a["model"] == b["model"], name
        for key, col in (("iH", 0), ("iF", 1)):
            if a[key] != b[key]:
                s = b["scores"][:, col]
                assert (np.nanmax(s) - s[a[key]]) / np.nanmax(s) <= gaps.max(), (name, key, a[key], b[key])
                exits += 1
    assert exits <= 1


def test_threshold_band_caps_hold_for_the_models():
    band = 1e-3
    inband = total = flips = 0
    for name, sc, rh in sy.batch():
        o = _run(name, sc, rh, np.float32)
        if o["scores"] is None:
            continue
        for M, fn, th in ((o["H21"], lambda m, d: tv.chi_h(m, tv.inv3(m, np.float32).astype(d), o["p1"], o["p2"], d), tv.TH_H),
                          (o["F21"], lambda m, d: tv.chi_f(m, o["p1"], o["p2"], d), tv.TH_F)):
            c32 = fn(M, np.float32)
            c64 = fn(M, np.float64)                                        # the same matrices, the arithmetic in double
            for a, b in zip(c32, c64):
                with np.errstate(invalid="ignore"):
                    nb = np.abs(b - th) <= band * th
                    inband += int(nb.sum()); total += b.size
                    flips += int((((a > np.float32(th)) != (b > th)) & ~nb & np.isfinite(b)).sum())
    share = inband / total
    print("in-band share %.3g of %d evaluations, flips outside the band %d" % (share, total, flips))
    assert flips == 0
    assert share <= 0.01
