"""CPU: the closed form of DistributeOctTree (tests/octree_table_model.py) against the oracle's list-based octree, kept indices in order."""
import numpy as np
import pytest


import octree_table_model as M


def _oracle(c):
    import oracle_bind
    return oracle_bind.octree(c["xs"], c["ys"], c["ss"], 16, 16 + c["W"], 16, 16 + c["H"], c["N"])


def _model(c, dmax=None, info=None):
    return M.octree_table(c["xs"], c["ys"], c["ss"], 16, 16 + c["W"], 16, 16 + c["H"], c["N"], dmax=dmax, info=info)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["uniform", "clustered", "tight_blocks"])
def test_random_cases_match_the_oracle(kind):
    n_ini, quotas, passes, finals = set(), set(), 0, 0
    for seed in range(80):
        c = M.random_case(kind, seed)
        info = {}
        got, want = _model(c, info=info), _oracle(c)
        assert np.array_equal(got, want), (kind, seed, info)
        n_ini.add(int(round(c["W"] / c["H"]))); quotas.add(c["N"])
        passes, finals = max(passes, info["T"]), max(finals, info["final_iters"])
    assert n_ini == {1, 2, 3, 4} and min(quotas) == 12 and max(quotas) == 1000
    assert passes >= 3 and finals >= 1


def test_depth_limit_gives_up_or_agrees():
    """With tables down to depth dmax the closed form either says so (None: the iterative form takes the list) or gives the oracle's list."""
    gave_up = agreed = 0
    for kind in range(3):
        for seed in range(0, 80, 2):
            c = M.random_case(kind, seed)
            for dmax in (3, 5):
                got = _model(c, dmax=dmax)
                if got is None:
                    gave_up += 1
                else:
                    agreed += 1
                    assert np.array_equal(got, _oracle(c)), (kind, seed, dmax)
    assert gave_up > 10 and agreed > 10


def test_hand_made_cases_match_the_oracle_and_are_what_they_say():
    cases = M.hand_cases()
    infos = {}
    for name, c in cases.items():
        infos[name] = {}
        got, want = _model(c, info=infos[name]), _oracle(c)
        assert np.array_equal(got, want), (name, infos[name])
    assert len(_oracle(cases["empty"])) == 0 and len(_oracle(cases["one_key"])) == 1
    assert infos["two_keys_deep"]["depth"] == 5 and len(_oracle(cases["two_keys_deep"])) == 6
    assert infos["two_keys_last_table"]["depth"] == 3 and M.table_depth(1, [20]) == 3 and _model(cases["two_keys_last_table"], dmax=3) is not None
    assert list(_oracle(cases["equal_scores"])) == [12, 8, 4, 0]                      # first key of each node, n4 .. n1
    assert infos["quirk_one_quadrant"]["quirk"]
    for n in (2, 3, 4):
        c = cases["empty_root_nini%d" % n]
        hx = np.float32(c["W"]) / np.float32(n)
        assert len(set((c["xs"].astype(np.float32) / hx).astype(int))) == n - 1
    i = infos["quota_exact_full_pass"]
    assert not i["final"] and not i["quirk"] and len(_oracle(cases["quota_exact_full_pass"])) >= cases["quota_exact_full_pass"]["N"]
    assert infos["quota_mid_final"]["final"] and infos["quota_mid_final"]["mid_stop"]
    assert infos["final_tie"]["tie"] and infos["final_two_iterations"]["final_iters"] >= 2
    assert infos["tight_block_deep"]["depth"] >= 8 and _model(cases["tight_block_deep"], dmax=7) is None
    assert len(cases["many_keys"]["xs"]) > 2048


# ------------------------------------------------------------------ premises of the device tests (tests/octree_device_cases.py)
def test_device_random_lists_are_legal_and_balanced():
    """Of the 240 lists the device runs all but those that overfill a FAST cell (at most 12); the tables of a one-level extractor give up on at
    least 30 of them and complete at least 150, so that k_octree_tab and k_octree_redo both do real work.  The split lists are what they say."""
    import octree_device_cases as D
    ran, skipped, flagged = D.check_random_balance()
    assert (ran, skipped, flagged) == (229, 11, 45)
    D.check_split_cases()


@pytest.mark.parametrize("level", [0, 3, 7])
def test_device_redo_lists_are_placed(level):
    import octree_device_cases as D
    flagged = D.check_redo_lists(level)
    cases, dmax = D.redo_lists(level)
    assert dmax == 5 and len(flagged) == 10
    for p in cases:                                                      # the closed form at full depth agrees with the oracle on every one
        got = M.octree_table(p["xs"], p["ys"], p["ss"], 16, 16 + p["W"], 16, 16 + p["H"], p["N"])
        assert np.array_equal(np.stack([p["xs"][got], p["ys"][got], p["ss"][got]], 1).reshape(-1, 3), p["want"]), p["name"]


def test_device_gather_lists_take_the_second_path():
    import octree_device_cases as D
    for level in range(D.GATHER_SHAPE["nlevels"]):
        D.check_gather_lists(level)


def test_pipeline_images_have_levels_deeper_than_the_tables():
    """From the oracle's candidates and the closed form: which levels of the constructed frames the depth-5 tables give up on.  Level 0 and at
    least two higher levels are covered, every constructed frame has one, the ordinary frames none; and the 700 x 480 pair changes nIni."""
    import orbhip
    import octree_device_cases as D
    imgs = D.pipeline_images(orbhip.synth_frames)
    deep = {f: D.flagged_levels(imgs[f])[0] for f in sorted(D.PIPE_CONSTRUCTED) + list(D.PIPE_ORDINARY)}
    assert all(deep[f] for f in D.PIPE_CONSTRUCTED), deep
    covered = set().union(*deep.values())
    assert 0 in covered and len(covered - {0}) >= 2, deep
    assert all(not deep[f] for f in D.PIPE_ORDINARY), deep
    wide = D.wide_pair(orbhip.synth_frames)
    for f in range(2):
        lv, n_ini = D.flagged_levels(wide[f])
        assert n_ini[0] == 1 and n_ini[3:] == [2] * 5
    assert any(l >= 3 for l in lv), lv                                   # a two-root level of the constructed frame goes to the iterative form


# ------------------------------------------------------------------ the case set can fail
@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_case_set_tells_a_wrong_closed_form_from_the_right_one(mutation):
    """Each test-only mutation of the model (one order rule wrong) must disagree with the oracle on the lists the device tests run: on at least
    20 of them, and in every detection area it can show in -- every one for the digit and the tie rule, those with more than one root for the root
    rule (with one root there is nothing to reverse)."""
    import octree_device_cases as D
    groups, _ = D.random_groups()
    cases = [p for v in groups.values() for p in v] + D.split_cases() + [p for level in D.REDO_LEVELS for p in D.redo_lists(level)[0]]
    wrong = {}
    for p in cases:
        got = M.octree_table(p["xs"], p["ys"], p["ss"], 16, 16 + p["W"], 16, 16 + p["H"], p["N"], mutate=mutation)
        if not np.array_equal(np.stack([p["xs"][got], p["ys"][got], p["ss"][got]], 1).reshape(-1, 3), p["want"]):
            wrong[(p["W"], p["H"])] = wrong.get((p["W"], p["H"]), 0) + 1
    areas = {(p["W"], p["H"]) for p in cases}
    assert len(areas) == 7
    if mutation == "no_root_reversal":
        assert all(D.n_ini_of(*a) == 1 for a in areas - set(wrong)), wrong       # no effect without a second root
        areas = {a for a in areas if D.n_ini_of(*a) > 1}
        assert len(areas) == 3
    assert areas <= set(wrong), (mutation, wrong)
    assert sum(wrong.values()) >= 20, (mutation, wrong)
