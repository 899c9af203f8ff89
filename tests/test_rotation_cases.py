"""Every (matcher, profile, seed) of rotation_cases.py is the case it claims to be -- asserted from the oracle alone, so that the device
test that runs the same cases (test_gpu_rotation.py) is known to take both 0.1 * max1 cut-offs of ComputeThreeMaxima, the case of more
than three filled bins and the all-zero histogram."""
import numpy as np
import pytest
import rotation_cases as rc

CASES = [(m, s) for m in rc.MATCHERS for s in rc.SEEDS[m]]


def _run(matcher, profile, seed):
    c, b = rc.make_case(matcher, profile, seed)
    n_off, m_off = rc.oracle(matcher, c, False)
    n_on, m_on = rc.oracle(matcher, c, True)
    return b, n_off, rc.matched_second(matcher, m_off), n_on, rc.matched_second(matcher, m_on)


@pytest.mark.parametrize("matcher,seed", CASES)
def test_one_bin_removes_nothing(matcher, seed):
    b, n_off, s_off, n_on, s_on = _run(matcher, "one", seed)
    assert n_off > 50 and n_on == n_off
    np.testing.assert_array_equal(s_on, s_off)


@pytest.mark.parametrize("profile", ["tail", "third", "four"])
@pytest.mark.parametrize("matcher,seed", CASES)
def test_surviving_bins(matcher, seed, profile):
    b, n_off, s_off, n_on, s_on = _run(matcher, profile, seed)
    filled = len(set(b[s_off].tolist()))
    assert filled == (4 if profile == "four" else 3), filled           # every bin of the profile holds a match before the check
    assert len(set(b[s_on].tolist())) == rc.SURVIVING_BINS[profile]
    assert n_on < n_off and len(s_on) < len(s_off)                      # the check removed at least one match
    assert set(s_on.tolist()) <= set(s_off.tolist())


@pytest.mark.parametrize("matcher,seed", CASES)
def test_empty_pair(matcher, seed):
    b, n_off, s_off, n_on, s_on = _run(matcher, "empty", seed)
    assert n_off == 0 and n_on == 0 and len(s_off) == 0 and len(s_on) == 0


def test_four_has_a_tie_for_a_kept_place():
    """At least one 'four' case has equal counts at the border of what is kept (second / third or third / fourth place): the scan's
    strict > keeps the lower bin.  Counted where the histogram IS the match list (SearchByBoW, SearchForTriangulation: no match is
    displaced after its entry was made)."""
    ties = 0
    for m in ("bow", "bow_kf", "tri", "tri_general"):
        for s in rc.SEEDS[m]:
            b, n_off, s_off, n_on, s_on = _run(m, "four", s)
            cnt = np.sort(np.bincount(b[s_off], minlength=30))[::-1]
            if cnt[1] == cnt[2] or cnt[2] == cnt[3]:
                ties += 1
                lo = min(k for k in (1, 5, 9, 11) if np.count_nonzero(b[s_off] == k) == cnt[2])
                assert lo in set(b[s_on].tolist())                      # of two equal bins the lower one is among the kept
    assert ties >= 1
