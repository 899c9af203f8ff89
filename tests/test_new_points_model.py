"""The model of LocalMapping::CreateNewMapPoints (tests/new_points_model.py) is the yardstick of the device kernel: these tests hold the
model itself to account -- its linear triangulation against the oracle's KannalaBrandt8::matchAndtriangulate bit for bit, its decisions
against a float64 restatement -- and the scenes of tests/synth_new_points.py to what they promise: every outcome code reached, the
reference's odd rules told from their plausible neighbours."""
import numpy as np
import pytest

import new_points_model as npm
import oracle_match_bind as om
import synth_new_points as sy

KINDS = ("mono", "stereo", "rig")


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_null_vector_and_point_equal_the_oracle_bit_for_bit():
    """orc_kb8_match_and_triangulate is the same linear system with absolute poses (KannalaBrandt8.cpp:240-332): wherever it accepts, its
    world point is the model's A -> Jacobi null vector -> v * (float)(1 / w), bit for bit.  KB8-first pairs: rig scenes."""
    rng = np.random.default_rng(77)
    n = 0
    for seed in range(40):
        c = om.make_tri_general_case(rng, 60, 60, "rig")
        P = om.tri_case_poses(c, seed)
        g = c["geom"]
        for j in range(len(c["kp2"])):
            i = int(rng.integers(0, len(c["kp1"])))
            r1, r2 = int(i >= g["nleft1"]), int(j >= g["nleft2"])
            cam1, cam2 = np.ascontiguousarray(g["cam1"][r1]), np.ascontiguousarray(g["cam2"][r2])
            T1, T2 = np.ascontiguousarray(P["Tcw1"][r1]), np.ascontiguousarray(P["Tcw2"][r2])
            k1, k2 = c["kp1"][i], c["kp2"][j]
            x = np.zeros(3, np.float32)
            ok = om.lib.orc_kb8_match_and_triangulate(cam1.ctypes.data, 1, cam2.ctypes.data, float(k1["x"]), float(k1["y"]), float(k2["x"]), float(k2["y"]),
                                                      T1.ctypes.data, T2.ctypes.data, 1e9, 1e9, x.ctypes.data)
            if not ok:
                continue
            xn1, xn2 = om.camera_unproject_f(1, cam1, k1["x"], k1["y"]), om.camera_unproject_f(1, cam2, k2["x"], k2["y"])
            v = npm.jacobi_null4(npm.triangulation_matrix(xn1, xn2, T1, T2))
            inv = np.float32(np.float64(1.0) / np.float64(v[3]))
            mine = np.array([v[0] * inv, v[1] * inv, v[2] * inv], np.float32)
            assert np.array_equal(_bits(mine), _bits(x)), (seed, i, j, mine, x)
            n += 1
    assert n >= 200, n


def test_null_vector_is_a_null_vector():
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(4, 4)).astype(np.float32)
        v = npm.jacobi_null4(A).astype(np.float64)
        ref = np.linalg.svd(A.astype(np.float64))[2][3]
        assert abs(abs(v @ ref) - 1) < 1e-4 and abs(np.linalg.norm(v) - 1) < 1e-5


def test_stereo_cosine_is_the_float_chain():
    for mb, d in ((0.11, 3.0), (0.11, 0.4), (0.5, 40.0), (0.11, -1.0), (0.11, 0.0)):
        c = npm.cos_stereo(np.float32(mb), np.float32(d))
        assert c.dtype == np.float32
        assert abs(float(c) - np.cos(2 * np.arctan2(np.float32(mb) / 2, np.float32(d)))) < 2e-7


@pytest.mark.parametrize("kind", KINDS)
def test_crafted_matches_agree_with_the_float64_restatement(kind):
    """every crafted match: the model's outcome is the float64 restatement's, whose decision quantities are all >= 1 % off their thresholds"""
    seen = set()
    for p, pr in enumerate(sy.scene(kind)):
        r = npm.run_pair(pr, f64_too=True)
        for i in pr["crafted"]:
            code, x, margin = r["f64"][i]
            assert code == r["outcome"][i], (kind, p, i, code, r["outcome"][i])
            assert margin >= sy.MARGIN or code in (5, 11), (kind, p, i, code, margin)
            if 1 <= code <= 3:
                assert np.allclose(x, r["x3D"][i], rtol=2e-3, atol=2e-3), (kind, p, i, x, r["x3D"][i])
            seen.add(int(code))
    assert seen >= {1, 4, 5, 7, 8, 9, 10, 11, 12, 13} | ({2, 3, 6} if kind == "stereo" else set()), seen


@pytest.mark.parametrize("kind", KINDS)
def test_random_matches_agree_off_the_thresholds(kind):
    """the matches nobody crafted: model and restatement agree wherever no decision quantity lies within 1e-4 relative of its threshold"""
    checked = 0
    for p, pr in enumerate(sy.scene(kind)):
        r = npm.run_pair(pr, f64_too=True)
        for i, (code, x, margin) in r["f64"].items():
            if margin > 1e-4 and i not in pr["crafted"]:
                assert code == r["outcome"][i], (kind, p, i, code, r["outcome"][i], margin)
                checked += 1
    assert checked > 700, checked


def test_every_outcome_is_reached():
    total = np.zeros(14, int)
    for kind in KINDS:
        counts = np.zeros(14, int)
        for pr in sy.scene(kind):
            counts += np.bincount(npm.run_pair(pr)["outcome"], minlength=14)
        print("%-6s outcome counts 0..13: %s" % (kind, counts.tolist()))
        total += counts
    assert np.all(total[1:] > 0), total.tolist()


def _differs(a, b):
    return int(np.sum((a["outcome"] != b["outcome"]) | np.any(_bits(a["x3D"]) != _bits(b["x3D"]), axis=1)))


@pytest.mark.parametrize("variant", npm.VARIANTS)
def test_scenes_tell_the_wrong_rules_from_the_model(variant):
    """KF2's own mbf at :681, `if` for `else if` at :584, mvKeysUn in UnprojectStereo, the ratio test inverted: each changes an outcome or a
    point of the stereo scene (the ratio test: of every scene)"""
    for kind in KINDS if variant == "ratio_inverted" else ("stereo",):
        n = sum(_differs(npm.run_pair(pr, variant=variant), npm.run_pair(pr)) for pr in sy.scene(kind))
        print(variant, kind, n)
        assert n >= 3, (variant, kind, n)


@pytest.mark.parametrize("kind", KINDS)
def test_flags_carried_to_the_next_neighbour_change_its_matches(kind):
    """the chain scene: neighbour 2's SearchForTriangulation against the flags neighbour 1's points set is not the all-at-once search"""
    pairs = sy.chain_world(kind)
    chain, mp1 = sy.chain_reference(kind)
    at_once, _ = sy.chain_reference(kind, carry=False)
    assert np.array_equal(chain[0]["matches12"], at_once[0]["matches12"])
    assert not np.array_equal(chain[1]["matches12"], at_once[1]["matches12"])
    created0 = np.flatnonzero((chain[0]["outcome"] >= 1) & (chain[0]["outcome"] <= 3))
    assert len(created0) > 10 and np.all(chain[1]["matches12"][created0] == -1) and np.any(at_once[1]["matches12"][created0] >= 0)
    assert mp1.sum() == sum(c["n_created"] for c in chain)


@pytest.mark.parametrize("kind", ("stereo",))
def test_scenes_stay_inside_the_libm_cap(kind):
    """the device comparison may leave out a stereo match whose outcome flips with one float ulp of its stereo cosine: at most 1 % of a
    scene's stereo matches, none of the crafted ones"""
    stereo = flip = 0
    for pr in sy.scene(kind):
        for i in np.flatnonzero(pr["matches12"] >= 0):
            if pr["ur1"][i] >= 0 or pr["ur2"][pr["matches12"][i]] >= 0:
                stereo += 1
                s = npm.libm_sensitive(pr, int(i))
                assert not (s and int(i) in pr["crafted"])
                flip += s
    print("stereo matches %d, libm-sensitive %d" % (stereo, flip))
    assert stereo > 300 and flip <= 0.01 * stereo
