"""The RANSAC sets of TwoViewReconstruction (k = 8), Sim3Solver (k = 3) and MLPnPsolver (k = 6), modelled once: per iteration k draws
without replacement from 0..n-1, the drawn slot refilled with the last one.  draw_sets_reference takes the reference's RandomInt as a
callable (what the host classes draw from rand()); device_sets is the counter-based generator of csrc/ransac_common.h (what the library
draws on the device)."""
import numpy as np

_M64 = (1 << 64) - 1


def _sets(n, iterations, k, draw):
    """draw(it, j, d) -> an index in [0, d)"""
    sets = np.full((iterations, k), -1, np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(k):
            r = draw(it, j, len(avail))
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def draw_sets_reference(n, iterations, randint, k):
    """randint(d) = DUtils::Random::RandomInt(0, d - 1), asked k times per iteration; n >= k is the caller's to see to"""
    return _sets(n, iterations, k, lambda it, j, d: randint(d))


def _mix(x):
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64; x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64; x ^= x >> 31
    return x


def device_draw(seed, item, it, j, avail):
    """ransac_draw: floor(u * avail) from the upper 32 bits of a splitmix64 finaliser keyed by (seed, item, iteration, draw)"""
    h = _mix((_mix((seed + 0x9E3779B97F4A7C15 * (item + 1)) & _M64) + 0xD1B54A32D192ED03 * (it + 1) + 0x8CB92BA72F3D8DD7 * (j + 1)) & _M64)
    return ((h >> 32) * avail) >> 32


def device_sets(seed, item, n, iterations, k):
    """ransac_draw_set<k> for iterations 0..iterations-1 of item `item` (its INDEX in the call): the same index gives the same sets, alone
    or inside a batch; -1 for n < k"""
    if n < k:
        return np.full((iterations, k), -1, np.int32)
    return _sets(n, iterations, k, lambda it, j, d: device_draw(seed, item, it, j, d))
