"""Hand-written KeyFrameDatabase cases, each a tiny world and script with the exact lists the reference's text gives for the LAST Detect...
call.  Values are dyadic so that every score is exact by hand: a shared word with values (v, w) adds |v - w| - v - w to the sum, and the
score is -sum / 2.  tests/test_kfdb_model.py asserts the expectations against kfdb_model.py; tests/test_gpu_kfdb.py runs the same cases on
the device."""
import numpy as np


def world_of(vectors, maps, neigh=None, n_slots=None, bad_maps=()):
    n = len(vectors)
    W = [np.array(sorted(v), np.int32) for v in vectors]
    V = [np.array([v[w] for w in sorted(v)], np.float64) for v in vectors]
    return dict(seed=0, n_slots=n if n_slots is None else n_slots, n=n, vocab=64, n_maps=max(maps) + 1, words=W, values=V, map=list(maps),
                neigh=[list(neigh.get(k, [])) if neigh else [] for k in range(n)], bad_maps=list(bad_maps))


def query(qid, qmap, mode, vec, connected=(), n_candidates=3):
    return dict(op="detect", mode=mode, id=qid, map=qmap, words=np.array(sorted(vec), np.int32),
                values=np.array([vec[w] for w in sorted(vec)], np.float64), connected=list(connected), n_candidates=n_candidates)


Q4 = {1: .25, 2: .25, 3: .25, 4: .25}
ONE, S875, S75, HALF = 0x3F800000, 0x3F600000, 0x3F400000, 0x3F000000       # float32 bits of 1, 0.875, 0.75, 0.5


def _adds(n):
    return [("add", k) for k in range(n)]


def cases():
    """name -> (world, ops, expected fields of the last detect's record, expected (slot, field index, value) state entries)"""
    c = {}
    # connected keyframes: words reset at each encounter -> 1, not marked (stored id stays 0), not listed
    w = world_of([{1: .5, 2: .5}, {1: .5, 3: .5}], [0, 0])
    c["connected"] = (w, _adds(2) + [query(5, 0, 0, {1: .5, 2: .5}, connected=[0])],
                      dict(sharing=[(1, 1, 1, HALF)], touched=[(0, 1)], max_common=1, scored=[(1, HALF, HALF, 1)], loop=[1], merge=[], reloc=[]),
                      [(0, 0, 0), (0, 1, 1), (1, 0, 5), (1, 1, 1)])
    # id 0 against fresh keyframes: the stored id already equals it -> nothing listed, the words still count
    c["id_zero"] = (w, _adds(2) + [query(0, 0, 0, {1: .5, 2: .5})],
                    dict(sharing=[], touched=[(0, 2), (1, 1)], max_common=0, scored=[], loop=[], merge=[], reloc=[]), [(0, 1, 2), (1, 1, 1)])
    # a repeated id: the second call lists nothing and the words grow on top of the old count
    c["repeated_id"] = (w, _adds(2) + [query(7, 0, 1, {1: .5, 2: .5}), query(7, 0, 1, {1: .5, 3: .5})],
                        dict(sharing=[], touched=[(0, 3), (1, 3)], max_common=0, scored=[], loop=[], merge=[], reloc=[]), [(0, 4, 3), (1, 4, 3), (0, 3, 7)])
    # a stale score: query 1 scores N = slot 0 with 1.0; query 2 lists N below the threshold, so N shows 1.0 to its covisible X = slot 1
    w = world_of([{10: .5, 11: .5}, {20: .25, 21: .25, 22: .25, 23: .25}], [0, 0], neigh={1: [0]})
    c["stale_score"] = (w, _adds(2) + [query(1, 0, 0, {10: .5, 11: .5}), query(2, 0, 0, {10: .125, 20: .25, 21: .25, 22: .25, 23: .125})],
                        dict(sharing=[(0, 1, 0, 0), (1, 4, 1, S875)], touched=[], max_common=4, scored=[(1, S875, 0x3FF00000, 0)], loop=[0], merge=[], reloc=[]),
                        [(0, 2, ONE), (0, 0, 2), (1, 2, S875)])
    # a neighbour without a slot (index 2 >= n_slots) is passed over; the next neighbour still counts
    w = world_of([dict(Q4), {1: .25, 2: .25, 3: .25, 4: .125, 9: .125}, {1: 1.0}], [0, 0, 0], neigh={0: [2, 1]}, n_slots=2)
    c["neighbour_without_slot"] = (w, _adds(2) + [query(3, 0, 1, Q4)],
                                   dict(sharing=[(0, 4, 1, ONE), (1, 4, 1, S875)], touched=[], max_common=4,
                                        scored=[(0, ONE, 0x3FF00000, 0), (1, S875, S875, 1)], loop=[], merge=[], reloc=[0]), [])
    # equal acc_score from duplicate vectors: the stable sort keeps list order, which is add order (slot 2 was added first)
    w = world_of([dict(Q4), {1: .25, 2: .25, 3: .25, 4: .125, 9: .125}, dict(Q4)], [0, 0, 0])
    c["ties"] = (w, [("add", 2), ("add", 1), ("add", 0), query(4, 0, 0, Q4)],
                 dict(sharing=[(2, 4, 1, ONE), (1, 4, 1, S875), (0, 4, 1, ONE)], touched=[], max_common=4,
                      scored=[(2, ONE, ONE, 2), (1, S875, S875, 1), (0, ONE, ONE, 0)], loop=[2, 0, 1], merge=[], reloc=[]), [])
    # truncation: maxCommonWords 4, 5, 6 give minCommonWords 3, 4, 4 (0.8f product, truncated); the comparison is strict
    for m, at_min in ((4, 3), (5, 4), (6, 4)):
        qv = {k: 1.0 / 8 for k in range(1, 9)}
        full = {k: 1.0 / 8 for k in range(1, m + 1)}; full[40] = 1.0 - m / 8.0
        low = {k: 1.0 / 8 for k in range(1, at_min + 1)}; low[41] = 1.0 - at_min / 8.0
        up = {k: 1.0 / 8 for k in range(1, at_min + 2)}; up[42] = 1.0 - (at_min + 1) / 8.0
        w = world_of([full, low, up], [0, 0, 0])
        bits = lambda k: int(np.float32(k / 8.0).view(np.uint32))
        c["truncation_%d" % m] = (w, _adds(3) + [query(6, 0, 1, qv)],
                                  dict(sharing=[(0, m, 1, bits(m)), (1, at_min, 0, 0), (2, at_min + 1, 1, bits(at_min + 1))], touched=[], max_common=m,
                                       scored=[(0, bits(m), bits(m), 0), (2, bits(at_min + 1), bits(at_min + 1), 2)], loop=[], merge=[],
                                       reloc=[0, 2] if (at_min + 1) / 8.0 > 0.75 * m / 8.0 else [0]), [])
    # the 0.75 filter at equality: acc 0.75 against best 1.0 is not retained, 0.875 is
    w = world_of([dict(Q4), {1: .25, 2: .25, 3: .125, 4: .125, 9: .25}, {1: .25, 2: .25, 3: .25, 4: .125, 9: .125}], [0, 0, 0])
    c["filter_at_equality"] = (w, _adds(3) + [query(8, 0, 1, Q4)],
                               dict(sharing=[(0, 4, 1, ONE), (1, 4, 1, S75), (2, 4, 1, S875)], touched=[], max_common=4,
                                    scored=[(0, ONE, ONE, 0), (1, S75, S75, 1), (2, S875, S875, 2)], loop=[], merge=[], reloc=[0, 2]), [])
    # a merge candidate in a bad map is dropped, one in a good map is kept
    w = world_of([dict(Q4), {1: .25, 2: .25, 3: .25, 4: .125, 9: .125}, {1: .25, 2: .25, 3: .125, 4: .125, 9: .25}], [1, 2, 0], bad_maps=[1])
    c["merge_in_bad_map"] = (w, _adds(3) + [query(9, 0, 0, Q4)],
                             dict(sharing=[(0, 4, 1, ONE), (1, 4, 1, S875), (2, 4, 1, S75)], touched=[], max_common=4,
                                  scored=[(0, ONE, ONE, 0), (1, S875, S875, 1), (2, S75, S75, 2)], loop=[2], merge=[1], reloc=[]), [])
    # nNumCandidates = 1 reached on the loop list first: the walk goes on until the merge list has its one
    w = world_of([dict(Q4), {1: .25, 2: .25, 3: .25, 4: .125, 9: .125}, {1: .25, 2: .25, 3: .125, 4: .125, 9: .25}], [0, 0, 1])
    c["one_list_full"] = (w, _adds(3) + [query(9, 0, 0, Q4, n_candidates=1)],
                          dict(sharing=[(0, 4, 1, ONE), (1, 4, 1, S875), (2, 4, 1, S75)], touched=[], max_common=4,
                               scored=[(0, ONE, ONE, 0), (1, S875, S875, 1), (2, S75, S75, 2)], loop=[0], merge=[2], reloc=[]), [])
    empty = dict(sharing=[], touched=[], max_common=0, scored=[], loop=[], merge=[], reloc=[])
    c["empty_database"] = (w, [query(9, 0, 0, Q4)], empty, [])
    c["no_shared_word"] = (w, _adds(3) + [query(9, 0, 1, {30: .5, 31: .5})], empty, [(0, 3, 0)])
    return c
