"""The crafted stereo lists (stereo_cases.py) on the CPU: the C oracle against the plain-Python model (stereo_model.py) on every frame,
the outcome histogram the lists must reach, and the proof that they tell every wrong rule of the model from the oracle."""
import functools
import numpy as np
import pytest

import stereo_cases as sc
import stereo_model as sm

OUT = {k: i for i, k in enumerate(sm.OUTCOMES)}


@functools.lru_cache(maxsize=None)
def modelled(geom, wrong=None):
    res = {}
    for fr in sc.frames(geom):
        o = sc.oracle_results(geom)[fr["name"]]
        res[fr["name"]] = sm.stereo_model(o["pyrL"], o["pyrR"], sc.scale_table(sc.GEOMS[geom][2]), fr["kpL"], fr["dL"], fr["kpR"], fr["dR"],
                                          sc.MB, sc.MBF, wrong=wrong)
    return res


def _equal(o, m):
    (kept, ur, dp), _, _ = m
    return kept == o["kept"] and ur.tobytes() == o["ur"].tobytes() and dp.tobytes() == o["dp"].tobytes()


@pytest.mark.parametrize("geom", list(sc.GEOMS))
def test_oracle_equals_model_on_every_crafted_frame(geom):
    for fr in sc.frames(geom):
        o = sc.oracle_results(geom)[fr["name"]]; m = modelled(geom)[fr["name"]]
        (kept, ur, dp), outcome, _ = m
        assert kept == o["kept"], fr["name"]
        assert ur.tobytes() == o["ur"].tobytes() and dp.tobytes() == o["dp"].tobytes(), fr["name"]
        matched = np.isin(outcome, [OUT["accepted"], OUT["accepted_clamped"]])
        assert ((o["sad"] >= 0) == matched).all() and ((ur >= 0) == matched).all(), fr["name"]
        # the extraction underneath is a real one: the lists replace something
        assert len(o["realL"][0]) > 50 and len(o["realR"][0]) > 50, fr["name"]


def test_every_outcome_and_flag_is_reached():
    """The minimums are conditions on the case set, not measurements: every outcome code and every flag at least 3 times, accepted and
    removed-by-the-median at least 50 times each; the two unreachable branches never."""
    ms = [m for g in sc.GEOMS for m in modelled(g).values()]
    oc, fl = sm.histogram([m[1] for m in ms], [m[2] for m in ms])
    print("outcomes", oc); print("flags", fl)
    for k in sm.UNREACHABLE:
        assert oc[k] == 0, k
    for k, n in oc.items():
        if k not in sm.UNREACHABLE:
            assert n >= (50 if k in ("accepted", "median_removed") else 3), (k, n, oc)
    for k, n in fl.items():
        assert n >= 3, (k, n, fl)


def test_counts_ballots_and_median_sizes():
    """What the blocks promise beyond the histogram: the left / right counts, a wave whose 64 lanes all reach the refinement, a wave in
    which only lane 63 does, equal best distances at right indices 63 | 64, accepted sets of 1, 2, an odd and an even size, a frame in
    which the cut removes everything and frames in which it removes nothing."""
    frames = [fr for g in sc.GEOMS for fr in sc.frames(g)]
    ms = {}
    for g in sc.GEOMS:
        ms.update(modelled(g))
    assert {0, 1, 63, 64, 65, 128, 200} <= {len(fr["kpL"]) for fr in frames}
    assert {0, 1, 64, 65, 129} <= {len(fr["kpR"]) for fr in frames}
    refined = {n: m[1] >= OUT["strip_left"] for n, m in ms.items()}                 # reached the one-lane-at-a-time refinement
    assert refined["full128"][:64].all() and refined["full128"][64:].all()
    assert refined["full65"].all()                                                  # a full ballot, then lane 0 alone
    assert np.flatnonzero(refined["lane63"]).tolist() == [63]
    tie = 1 << sm.FLAGS.index("tie_across_64")
    for n in ("mix200_qvga8", "neg65", "mix65_qqvga4"):
        fr = next(f for f in frames if f["name"] == n)
        dist = lambda i, j: int(np.unpackbits(fr["dL"][i] ^ fr["dR"][j]).sum())
        assert any(dist(i, 63) == dist(i, 64) < 75 for i in np.flatnonzero(ms[n][2] & tie)), n
    V = {n: int(np.isin(m[1], [OUT["accepted"], OUT["accepted_clamped"], OUT["median_removed"]]).sum()) for n, m in ms.items()}
    kept = {n: m[0][0] for n, m in ms.items()}
    assert V["one"] == 1 and V["s_one"] == 1 and V["lane63"] == 1 and V["two63"] == 2
    assert any(v > 2 and v % 2 for v in V.values()) and any(v > 2 and v % 2 == 0 for v in V.values())
    assert V["same64"] > 20 and kept["same64"] == 0                                 # median 0: 0 < 0 fails, everything goes
    assert kept["two63"] == 2 and kept["one"] == 1                                  # nothing goes
    assert V["noleft"] == 0 and V["noright"] == 0


@pytest.mark.parametrize("wrong", sm.WRONG_RULES)
def test_each_wrong_rule_disagrees_with_the_oracle(wrong):
    caught = [fr["name"] for g in sc.GEOMS for fr in sc.frames(g) if not _equal(sc.oracle_results(g)[fr["name"]], modelled(g, wrong)[fr["name"]])]
    print(wrong, "caught by", caught)
    assert caught, wrong


def test_generator_refuses_unsafe_lists():
    fr = dict(sc.frames("qvga8")[0])
    for field, value in (("x", 3.0), ("y", 238.0), ("octave", 8), ("x", np.nan)):
        kp = fr["kpL"].copy()
        i = int(np.flatnonzero(modelled("qvga8")[fr["name"]][1] == OUT["accepted"])[0])          # a keypoint with a candidate in its window
        kp[field][i] = value
        with pytest.raises(AssertionError):
            sc.check_safe(dict(fr, kpL=kp), sc.NFEAT)
    kp = fr["kpR"].copy(); kp["x"][0] = -6.0
    with pytest.raises(AssertionError):
        sc.check_safe(dict(fr, kpR=kp), sc.NFEAT)
    with pytest.raises(AssertionError):
        sc.check_safe(fr, len(fr["kpL"]) - 1)
