"""CPU: the crafted projection-matcher cases of sbp_cases.py are the cases they claim to be.  The model (sbp_model.py) equals the C oracle bit
for bit on every case; every query has the declared outcome, gate bits, accept flags and keypoint; the totals table holds every outcome, gate
bit and flag; the replay form's hand-back is predicted as named; float64 decides every row as float32 does, except the named boundary rows."""
import numpy as np
import pytest

import sbp_cases as sc
import sbp_model as sm


def _ids(cs):
    return [c["name"] for c in cs]


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("c", sc.all_cases(), ids=_ids(sc.all_cases()))
def test_model_equals_the_oracle(c, stereo):
    if not stereo and c["ur"] is None:
        return                                               # (rig frames carry no uRight: one form only)
    m, o = sc.run_model(c, stereo=stereo), sc.run_oracle(c, stereo)
    if c["kind"] == "fuse":
        np.testing.assert_array_equal(m["bi"], o[0]); np.testing.assert_array_equal(m["bd"], o[1])
    else:
        assert m["nm"] == o[0]
        np.testing.assert_array_equal(m["tm"], o[1])


def _declared(c):
    gates = [None if e[1] is None else sum(sm.G[g] for g in e[1]) for e in c["expect"]]
    flags = [sum(sm.F[f] for f in e[2]) for e in c["expect"]]
    return [sm.OUTCOMES.index(e[0]) for e in c["expect"]], gates, flags


@pytest.mark.parametrize("c", sc.all_cases(), ids=_ids(sc.all_cases()))
def test_every_query_is_what_it_is_named_for(c):
    m = sc.run_model(c)
    out, gates, flags = _declared(c)
    for t, lab in enumerate(c["labels"]):
        got = (sm.OUTCOMES[m["outcome"][t]], int(m["gates"][t]) if gates[t] is not None else None, int(m["flags"][t]) if "flags" in m else 0)
        assert got == (c["expect"][t][0], gates[t], flags[t] if "flags" in m else 0), (c["name"], lab, got, c["expect"][t])
        match = c["expect"][t][3]
        if c["kind"] == "fuse":
            assert m["bi"][t] == (-1 if match is None else match), (c["name"], lab)
        elif match is not None:
            assert m["tm"][match] == t, (c["name"], lab, match)
        if c["expect"][t][0] != "accept":
            assert c["kind"] == "fuse" or not (m["tm"] == t).any(), (c["name"], lab)
    if c["handback"] is not None:
        assert m["handback"] == bool(c["handback"]) and (not c["handback"] or c["handback"] in m["reasons"]), (c["name"], m["reasons"])


def totals():
    tot = {}
    for c in sc.all_cases():
        for e in c["expect"]:
            for k in ["outcome:" + e[0]] + ["gate:" + g for g in (e[1] or ())] + ["flag:" + f for f in e[2]]:
                tot[k] = tot.get(k, 0) + 1
        if c["handback"]:
            tot["handback:" + c["handback"]] = tot.get("handback:" + c["handback"], 0) + 1
    return tot


def test_totals_table():
    tot = totals()
    assert tot == sc.TOTALS, tot
    want = ["outcome:" + o for o in sm.OUTCOMES] + ["gate:" + g for g in sm.GATES] + ["flag:" + f for f in sm.FLAGS] + \
           ["handback:" + r for r in sm.HANDBACK_REASONS]
    assert all(tot.get(k, 0) > 0 for k in want), [k for k in want if not tot.get(k)]
    # every pair the replay form could see is predicted to stay unless it is named to hand back
    named = {c["name"] for c in sc.all_cases() if c["handback"]}
    found = {c["name"] for c in sc.all_cases() if c["kind"] in ("frame", "map") and sc.run_model(c)["handback"]}
    assert named == found, named ^ found


def test_float64_decides_as_float32_except_the_named_boundary_rows():
    diff = set()
    for c in sc.all_cases():
        a, b = sc.run_model(c, sm.F32), sc.run_model(c, sm.F64)
        keys = ("outcome", "gates", "nstatic") + (("bi", "bd") if c["kind"] == "fuse" else ("flags",))
        for t, lab in enumerate(c["labels"]):
            same = all(a[k][t] == b[k][t] for k in keys)
            if c["kind"] != "fuse":
                same = same and np.array_equal(np.flatnonzero(a["tm"] == t), np.flatnonzero(b["tm"] == t))
            if not same:
                diff.add("%s:%s" % (c["name"], lab))
    assert diff == set(sc.F64_EXCEPTIONS), (sorted(diff - sc.F64_EXCEPTIONS), sorted(sc.F64_EXCEPTIONS - diff))


def test_second_geometry_moves_cells_and_windows():
    """the undistorted-style bounds put at least one keypoint into another cell, and one query's c0 or r1 elsewhere, than min = 0 would"""
    g = sc.GEOMS["undist"]; zero = (0.0, 0.0, g[2], g[3])
    moved_kp = moved_q = 0
    for c in sc.cases():
        if c["geom"] != "undist" or not len(c["kp"]):
            continue
        moved_kp += int((sm.build_grid(c["kp"], g)[1] != sm.build_grid(c["kp"], zero)[1]).sum())
        for t in range(len(c["q"])):
            (a0, _, _, a3), ea = sm.window(c["q"], t, g); (b0, _, _, b3), eb = sm.window(c["q"], t, zero)
            moved_q += int(ea is None and eb is None and (a0 != b0 or a3 != b3))
    assert moved_kp > 0 and moved_q > 0


def test_fma_rows_are_fma_sensitive():
    """the module's claim: N_FMA_ROWS rows per fuse-chi case whose decision one fused multiply-add would flip"""
    for geom in sc.GEOMS:
        c = sc.by_name("fuse-chi-%s" % geom)
        n = 0
        for t, lab in enumerate(c["labels"]):
            i = int(np.argmin(np.abs(c["kp"]["x"] - c["q"]["u"][t]) + np.abs(c["kp"]["y"] - c["q"]["v"][t])))
            ex, ey = np.float32(c["q"]["u"][t] - c["kp"]["x"][i]), np.float32(c["q"]["v"][t] - c["kp"]["y"][i])
            st = c["ur"][i] >= 0
            er = np.float32(c["q"]["ur"][t] - c["ur"][i]) if st else None
            plain, fused = sc.chi_forms(ex, ey, er, c["sig"][c["kp"]["octave"][i]])
            th = 7.8 if st else 5.99
            flips = any((plain > th) != (v > th) for v in fused)
            assert flips == lab.startswith("fma"), (geom, lab)
            n += flips
        assert n == sc.N_FMA_ROWS


def test_handed_back_accessor_is_exported():
    import orbhip
    assert hasattr(orbhip.lib, "orbhip_debug_sbp_handed_back") and orbhip.lib.orbhip_debug_sbp_handed_back.argtypes is not None
    assert callable(orbhip.debug_sbp_handed_back)
