"""csrc/ransac_common.h in a stand-alone program (tests/ransac_common_check.cc, its own main) built with g++ -fsanitize=address,undefined
and run as a program: the sets of ransac_draw_set<K> against tests/ransac_sets_model.py for every K the solvers use, and
ransac_iteration_budget against the two solver models, both exactly.  No GPU, no library, nothing preloaded."""
import itertools
import math
import os
import subprocess
import numpy as np
import pytest

import mlpnp_model
import ransac_sets_model as rs
import sim3_solver_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ITERATIONS = 300
KEYS = ((0, 0), (5, 3), (2 ** 63 + 7, 11))                                     # (seed, item)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ransac_common") / "ransac_common_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(ROOT, "orb-slam3-mac_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "ransac_common_check.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]

    def run(requests):
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        return [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    return run


@pytest.mark.parametrize("k", (3, 6, 8))
def test_sets_are_the_models(check, k):
    """n = 0 .. k+3 (n < k: all -1; n = k and k+1: every draw meets a moved slot or the last one), 20, 129 and 300; three (seed, item)
    keys, one of them with a seed above 2^63; 300 iterations each"""
    cases = [(seed, item, n) for n in list(range(k + 4)) + [20, 129, 300] for seed, item in KEYS]
    got = np.array(check(["S %d %d %d %d %d" % (k, seed, item, n, ITERATIONS) for seed, item, n in cases]), np.int32)
    assert got.shape == (len(cases) * ITERATIONS, k)
    for c, (seed, item, n) in enumerate(cases):
        want = rs.device_sets(seed, item, n, ITERATIONS, k)
        assert np.array_equal(got[c * ITERATIONS:(c + 1) * ITERATIONS], want), (k, seed, item, n)
        if n >= k:                                                              # the model itself: k distinct indices of 0..n-1
            s = np.sort(want, axis=1)
            assert s.min() >= 0 and s.max() < n and (s[:, 1:] != s[:, :-1]).all(), (k, n)
        else:
            assert (want == -1).all()


NS = (5, 6, 7, 8, 9, 12, 20, 50, 129, 200, 300, 1000, 8192)
GRID = list(itertools.product(NS, (6, 8, 20), (0.5, 0.99, 0.999), (300, 1024)))
EPSILON = 0.4


def _quotient(eps, probability):
    return math.log(1 - probability) / math.log(1 - float(eps) ** 3) if float(eps) < 1 else 0.0


def test_budget_is_the_models(check):
    """both callers' forms of epsilon over n x min_inliers x probability x cap: n < nMin (0), n == nMin (1), quotients beyond the cap
    (saturation).  Equality is demanded: no quotient of the grid lies within 5e-3 of an integer, so the last bit of a log cannot decide"""
    sim3 = check(["B %d %d %r %d" % (n, mi, p, cap) for n, mi, p, cap in GRID])
    pnp = check(["P %d %d %r %r %d" % (n, mi, EPSILON, p, cap) for n, mi, p, cap in GRID])
    seen, nearest = set(), 1.0
    for (n, mi, p, cap), b3, (nmin, bp) in zip(GRID, sim3, pnp):
        assert b3 == [sim3_solver_model.iteration_budget(n, p, mi, cap)], (n, mi, p, cap)
        assert (nmin, bp) == mlpnp_model.ransac_parameters(n, p, mi, cap, 6, EPSILON), (n, mi, p, cap)
        for lo, eps, b in ((mi, F32(mi) / F32(n), b3[0]), (nmin, max(F32(EPSILON), F32(nmin) / F32(n)), bp)):
            seen.add("none" if n < lo else "one" if n == lo else "capped" if b == cap else "open")
            if n > lo:
                q = _quotient(eps, p)
                if q < cap + 1:
                    nearest = min(nearest, abs(q - round(q)))
    assert seen == {"none", "one", "capped", "open"}
    print("closest quotient to an integer: %.3e" % nearest)
    assert nearest >= 5e-3
