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
