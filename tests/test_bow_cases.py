"""CPU: the crafted BoW-matcher and triangulation-matcher cases of bow_cases.py are the cases they claim to be.  The model (bow_model.py) equals
the C oracle bit for bit on every case in every form that accepts it; every keyframe feature / KF1 keypoint has the declared outcome, gate bits,
flags and match; the totals table holds every outcome, gate bit, flag and path; float64 decides every triangulation row as float32 does except
the named boundary rows; the FMA rows are FMA-sensitive; the path prediction names a case at every switch size."""
import numpy as np
import pytest

import bow_cases as bc
import bow_model as bm
import oracle_match_bind as om


def _ids(cs):
    return [c["name"] for c in cs]


BOW, TRI = bc.bow_cases(), bc.tri_cases()


@pytest.mark.parametrize("check_ori", [True, False], ids=["ori", "no-ori"])
@pytest.mark.parametrize("c", BOW, ids=_ids(BOW))
def test_bow_model_equals_the_oracle(c, check_ori):
    m = bc.run_bow_model(c, check_ori)
    n, ref = bc.run_bow_oracle(c, check_ori)
    assert m["nm"] == n
    np.testing.assert_array_equal(m["m"], ref)
    if c["form"] == "frame":                      # the rig oracle with Nleft == -1 takes the one-camera branch: the frame form exactly
        n2, ref2 = om.search_by_bow_rig(c, -1, c["ratio"], check_ori)
        assert n2 == n
        np.testing.assert_array_equal(ref2, ref)


@pytest.mark.parametrize("c", BOW, ids=_ids(BOW))
def test_every_keyframe_feature_is_what_it_is_named_for(c):
    for ori in (True, False):
        m = bc.run_bow_model(c, ori)
        for i, lab in enumerate(c["labels"]):
            oc, fl, match, match_r = c["expect"][i]
            if not ori:
                fl = fl - {"rot_removed"}
            got = (bm.BOW_OUTCOMES[m["outcome"][i]], frozenset(f for f in bm.BOW_FLAGS if m["flags"][i] & bm.BF[f]),
                   None if m["match"][i] < 0 else int(m["match"][i]), None if m["match_r"][i] < 0 else int(m["match_r"][i]))
            assert got == (oc, fl, match, match_r), (c["name"], lab, got, c["expect"][i])
            # the declared match is what the output array holds, unless the rotation check removed it
            kept = not (ori and "rot_removed" in fl)
            for j in (match, match_r):
                if j is not None:
                    have = (m["m"][i] == j) if c["form"] == "kf" else (m["m"][j] == i)
                    assert have == kept, (c["name"], lab)
            if oc != "accept":
                assert (m["m"][i] == -1) if c["form"] == "kf" else not (m["m"] == i).any(), (c["name"], lab)
    if "expected_counts" in c:
        for oc, cnt in c["expected_counts"].items():
            assert sum(e[0] == oc for e in c["expect"]) == cnt, (c["name"], oc)


@pytest.mark.parametrize("mono", [False, True], ids=["uright", "no-uright"])
@pytest.mark.parametrize("check_ori", [True, False], ids=["ori", "no-ori"])
@pytest.mark.parametrize("c", TRI, ids=_ids(TRI))
def test_tri_model_equals_the_oracles(c, check_ori, mono):
    m = bm.search_for_triangulation(c, check_ori, mono)
    n, ref = om.search_for_triangulation(c, check_ori, mono)
    assert m["nm"] == n
    np.testing.assert_array_equal(m["m"], ref)
    if not mono:                                   # the general oracle's Pinhole form (it always reads the uRight arrays)
        n2, ref2 = om.search_for_triangulation_general(c, check_ori)
        assert n2 == n
        np.testing.assert_array_equal(ref2, ref)


@pytest.mark.parametrize("c", TRI, ids=_ids(TRI))
def test_every_kf1_keypoint_is_what_it_is_named_for(c):
    for ori in (True, False):
        m = bm.search_for_triangulation(c, ori, mono=not c["stereo"])
        for i, lab in enumerate(c["labels"]):
            oc, gates, fl, match = c["expect"][i]
            if not ori:
                fl = fl - {"rot_removed"}
            got = (bm.TRI_OUTCOMES[m["outcome"][i]], frozenset(g for g in bm.TRI_GATES if m["gates"][i] & bm.TG[g]),
                   frozenset(f for f in bm.TRI_FLAGS if m["flags"][i] & bm.TF[f]), None if m["match"][i] < 0 else int(m["match"][i]))
            assert got == (oc, gates, fl, match), (c["name"], lab, got, c["expect"][i])
            assert m["m"][i] == (-1 if match is None or (ori and "rot_removed" in fl) else match), (c["name"], lab)


def totals():
    tot = {}

    def add(k, n=1):
        tot[k] = tot.get(k, 0) + n
    for c in BOW:
        add("cases:bow")
        add("features:frame-side:bow", len(c["kp_f"]))
        for e in c["expect"]:
            add("features:bow")
            add("outcome:" + e[0])
            for f in e[1]:
                add("flag:" + f)
        nleft = c.get("nleft", -1) if c["form"] == "rig" else -1
        shared = set(c["nid_k"].tolist()) & set(c["sizes"])
        for n in shared:
            add("path:" + bm.node_path(c["sizes"][n], nleft))
    for c in TRI:
        add("cases:tri")
        add("features:kf2:tri", len(c["kp2"]))
        for e in c["expect"]:
            add("features:tri")
            add("tri:outcome:" + e[0])
            for g in e[1]:
                add("gate:" + g)
            for f in e[2]:
                add("flag:" + f)
    return tot


def test_totals_table():
    tot = totals()
    assert tot == bc.TOTALS, dict(sorted(tot.items()))
    want = ["outcome:" + o for o in bm.BOW_OUTCOMES] + ["flag:" + f for f in bm.BOW_FLAGS + bm.TRI_FLAGS] + ["gate:" + g for g in bm.TRI_GATES] + \
           ["tri:outcome:" + o for o in bm.TRI_OUTCOMES] + ["path:" + p for p in bm.PATHS]
    assert all(tot.get(k, 0) > 0 for k in want), [k for k in want if not tot.get(k)]
    sizes = ["cases:bow", "cases:tri", "features:bow", "features:tri", "features:frame-side:bow", "features:kf2:tri"]
    assert set(tot) == set(want + sizes)
    # no case can leave unnoticed: every one moves the case count, and the names are the ones listed
    assert sorted(c["name"] for c in BOW + TRI) == sorted(bc.CASE_NAMES)


def test_paths_are_predicted_at_every_switch_size():
    """the model's path per shared node equals the declared function of size and Nleft, and the sizes on the switch points are all present"""
    seen = {}
    for c in BOW:
        m = bc.run_bow_model(c, False)
        nleft = c.get("nleft", -1) if c["form"] == "rig" else -1
        assert set(m["paths"]) == set(c["nid_k"].tolist()) & set(c["sizes"]), c["name"]
        for n, p in m["paths"].items():
            S = c["sizes"][n]
            assert p == ("lane" if nleft >= 0 or S < 32 else "wave" if S <= 512 else "wave+tail") and m["tails"][n] == (p == "wave+tail")
            if c["form"] != "rig":
                seen.setdefault(S, set()).add((c["form"], p))
    for S, p in ((1, "lane"), (31, "lane"), (32, "wave"), (33, "wave"), (63, "wave"), (64, "wave"), (65, "wave"), (511, "wave"), (512, "wave"),
                 (513, "wave+tail"), (600, "wave+tail")):
        assert seen.get(S) == {("frame", p), ("kf", p)}, (S, seen.get(S))
    rig40 = [c for c in BOW if c["form"] == "rig" and 40 in c["sizes"].values()]
    assert rig40 and all(set(bc.run_bow_model(c, False)["paths"].values()) == {"lane"} for c in rig40)


def test_float64_decides_as_float32_except_the_named_boundary_rows():
    diff = set()
    for c in TRI:
        a = bm.search_for_triangulation(c, False, not c["stereo"], bm.F32); b = bm.search_for_triangulation(c, False, not c["stereo"], bm.F64)
        for i, lab in enumerate(c["labels"]):
            if any(a[k][i] != b[k][i] for k in ("outcome", "gates", "flags", "match")):
                diff.add("%s:%s" % (c["name"], lab))
    assert diff == set(bc.F64_EXCEPTIONS), (sorted(diff - bc.F64_EXCEPTIONS), sorted(bc.F64_EXCEPTIONS - diff))


def test_fma_rows_are_fma_sensitive():
    """the module's claim.  Epipolar distance: for each sum of Pinhole.cpp:130-141 but the inert one, row fma_chi_<sum> flips when a product is
    fused into THAT sum alone, and when every sum is fused; lb is inert on every row (its second product is y1 * 0).  Epipole: N_FMA_ROWS rows
    flip when either square of :1097 is fused, both squares are covered, and no other row of that case flips."""
    c = bc.by_name("tri-chi-boundary")
    covered = set()
    for i, lab in enumerate(c["labels"]):
        j = int(np.flatnonzero(c["nid2"] == c["nid1"][i])[0])
        th = 3.84 * float(c["sigma2"][c["kp2"]["octave"][j]])
        plain, singles, every = bc.epipolar_forms(c["kp1"]["x"][i], c["kp1"]["y"][i], c["F12"], c["kp2"]["x"][j], c["kp2"]["y"][j])
        assert (plain < th) == (c["expect"][i][0] == "accept"), lab
        for name in bc.FMA_INERT_SUMS:
            k = bc.EPI_SUMS.index(name)
            assert singles[2 * k] == plain and singles[2 * k + 1] == plain, (lab, name)
        if lab.startswith("fma_chi_"):
            k = bc.EPI_SUMS.index(lab[len("fma_chi_"):])
            assert any((plain < th) != (v < th) for v in singles[2 * k:2 * k + 2]) and (plain < th) != (every < th), lab
            covered.add(bc.EPI_SUMS[k])
    assert covered == set(bc.EPI_SUMS) - set(bc.FMA_INERT_SUMS) and len(covered) >= 4
    c = bc.by_name("tri-epipole-boundary")
    n = 0
    squares = set()
    for i, lab in enumerate(c["labels"]):
        j = int(np.flatnonzero(c["nid2"] == c["nid1"][i])[0])
        th = float(np.float32(np.float32(100) * c["scale"][c["kp2"]["octave"][j]]))
        plain, fused = bc.epipole_forms(c["ep"], c["kp2"]["x"][j], c["kp2"]["y"][j])
        assert (plain < th) == (c["expect"][i][0] == "all_gated"), lab
        flips = any((plain < th) != (v < th) for v in fused)
        assert flips == lab.startswith("fma"), lab
        n += flips
        squares |= {k for k, v in enumerate(fused) if (plain < th) != (v < th)}
    assert n == bc.N_FMA_ROWS and squares == {0, 1}


def test_ratio_rows_sit_on_an_integer_product():
    for ratio in (0.7, 0.75):
        b2, N = bc.ratio_row(ratio)
        assert float(np.float32(ratio) * np.float32(b2)) == N and N + 1 < bm.TH_LOW
