"""The software-pipelined all-pairs 2-NN matcher (k_bf2nn_mfma, both instances) against the oracle at the shapes where a two-stage
pipeline over 32-column half tiles and 64-row tiles can go wrong: an odd number of half tiles, exactly one, none; neighbours in the
first and the last half tile and astride a half-tile (31 / 32) and a tile (63 / 64) boundary; the extremes of the accumulator that
starts from 0 instead of |a| (distances 0 and 256 with |a| in {0, 256}); ties across the two accumulators and the two tile buffers."""
import numpy as np
import pytest

from test_gpu_match import _bf, _bf_check, _flip

pytestmark = pytest.mark.gpu

MAX_N = 320
NB = [0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 161, 320]
NA = [1, 32, 33, 255, 256, 257, 320]
INT_MAX = np.iinfo(np.int32).max


def _anchors(nb):
    """Pairs of train rows (j1 < j2) that will be some queries' two nearest rows: astride the half-tile boundary (31, 32), astride the
    tile boundary (63, 64), one in the first and one in the last half tile; no row in two pairs."""
    used, out = set(), []
    for j1, j2 in ((31, 32), (63, 64)):
        if j2 < nb:
            out.append((j1, j2)); used |= {j1, j2}
    first = next((j for j in range(min(32, nb)) if j not in used), None)
    last = next((j for j in range(nb - 1, max(32 * ((nb - 1) // 32), 0) - 1, -1) if j not in used and j != first), None) if nb else None
    if first is not None and last is not None and first < last:
        out.append((first, last))
    elif not out and nb >= 2:
        out.append((0, nb - 1))
    return out


def _planted_pair(rng, na, nb, accept_single):
    """Random descriptors; train rows j1, j2 of every anchor pair differ in 10 known bits, and every query is a copy of one anchor's j1
    with x of those bits and y other bits inverted: its two nearest rows are j1 and j2 at distances x + y and 10 - x + y (everything else
    sits ~128 away), the nearer one in either row, with ties (x = 5) and both outcomes of the ratio test."""
    A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    anchors = _anchors(nb)
    if not anchors:
        return A, B
    diff = {}
    for j1, j2 in anchors:
        diff[j1] = rng.choice(256, 10, replace=False)
        B[j2] = _flip(B[j1], diff[j1])
    for q in range(na):
        j1, _ = anchors[q % len(anchors)]
        if na == 1:
            x, y = (0, 1) if accept_single else (4, 2)                 # 1 < 0.7 * 11; 6 < 0.7 * 8 is false
        else:
            x, y = [(0, 1), (4, 2), (10, 0), (5, 0), (7, 1), (2, 3)][(q // len(anchors)) % 6] if q < 24 else (int(rng.integers(0, 11)), int(rng.integers(0, 4)))
        rest = np.setdiff1d(np.arange(256), diff[j1])
        A[q] = _flip(B[j1], np.concatenate([diff[j1][:x], rng.choice(rest, y, replace=False)]))
    return A, B


@pytest.fixture(scope="module")
def crossed_shapes():
    """Every nA x nB of the lists above, plus pairs with nA = 0: (sizes, A list, B list, oracle results), computed once on the CPU.
    Before anything goes to the GPU: in every shape with nB >= 2 the oracle accepts some queries and rejects some (a shape with one
    query has one outcome: those alternate over the nB list and both outcomes occur)."""
    import oracle_match_bind as om
    rng = np.random.default_rng(606)
    sizes = [(a, b) for a in NA for b in NB] + [(0, b) for b in (0, 1, 33, 320)]
    da, db, ora = [], [], []
    single = []
    for a, b in sizes:
        A, B = _planted_pair(rng, a, b, accept_single=(NB.index(b) % 2 == 0) if b in NB else True)
        da.append(A); db.append(B)
        oi, od, oa = om.bf2nn(A, B, 0.7)
        ora.append((oi, od, oa))
        if b >= 2 and a >= 2:
            assert 0 < int(oa.sum()) < a, (a, b, int(oa.sum()))
        if b >= 2 and a == 1:
            single.append(int(oa[0]))
        if b >= 2 and a >= 32:                                          # the planted rows are the neighbours found, in both orders
            anchors = _anchors(b)
            got = {(int(i), int(j)) for i, j in oi}
            for j1, j2 in anchors:
                assert (j1, j2) in got and (j2, j1) in got, (a, b, j1, j2)
    assert 0 in single and 1 in single
    return sizes, da, db, ora


def test_anchor_rows_cover_boundaries_and_outer_half_tiles():
    """The planted rows (CPU only): 31 / 32 and 63 / 64 wherever the frame has them, one row of the first half tile and one of the last."""
    for nb in NB:
        an = _anchors(nb)
        rows = [j for p in an for j in p]
        assert len(rows) == len(set(rows)) and all(0 <= j < nb for j in rows)
        if nb >= 2:
            assert an
        if nb >= 33:
            assert (31, 32) in an
        if nb >= 65:
            assert (63, 64) in an
        if nb >= 34:
            assert any(j < 32 for j in rows) and any(j >= 32 * ((nb - 1) // 32) for j in rows), nb


def test_bf2nn_pipeline_crossed_shapes_one_launch(gpu_ctx, crossed_shapes):
    """One launch over all pairs: indices, distances and accept flags equal the oracle; rows >= nA keep their sentinels (checked in _bf)."""
    sizes, da, db, ora = crossed_shapes
    got = _bf(gpu_ctx, da, db, MAX_N, 0.7)
    for p, (a, b) in enumerate(sizes):
        np.testing.assert_array_equal(got[p][0], ora[p][0], err_msg="idx nA %d nB %d" % (a, b))
        np.testing.assert_array_equal(got[p][1], ora[p][1], err_msg="dist nA %d nB %d" % (a, b))
        np.testing.assert_array_equal(got[p][2], ora[p][2], err_msg="accept nA %d nB %d" % (a, b))
        if b == 0 and a:
            assert (got[p][0] == -1).all() and (got[p][1] == INT_MAX).all() and not got[p][2].any()


def test_bf2nn_pipeline_accumulator_extremes(gpu_ctx):
    """The accumulator holds Hamming - |a| in [-256, 256]: queries all-zeros (|a| = 0), all-ones (|a| = 256) and random against train rows
    all-zeros, all-ones, each query's copy (distance 0) and each query's complement (distance 256), over three half tiles and alone;
    one train row gives second = INT_MAX, index -1, accept 0."""
    rng = np.random.default_rng(77)
    zeros, ones = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    A = np.concatenate([zeros, ones, rng.integers(0, 256, (38, 32), dtype=np.uint8)])
    da = [A, A, A, A, A[:2], A[:2], A[:2], A[:2], A, A, A[:2], A[:2]]
    db = [np.concatenate([zeros, ones, A, ~A]),              # 82 rows: copy and complement of every query
          np.concatenate([~A, ones, zeros]),                 # complements first: the distance-256 rows at the low indices
          ~A, A,                                             # 256 apart from its own row in the first, 0 in the second
          zeros, ones, np.concatenate([ones, ones]), np.concatenate([zeros, zeros]),
          A[2:3], ~A[2:3], A[0:1], A[1:2]]                   # nB = 1: a copy, a complement, all-zeros, all-ones
    got = _bf(gpu_ctx, da, db, 96, 0.7)
    _bf_check(got, da, db, 0.7)
    d0 = got[0][1]
    assert (d0[:, 0] == 0).all() and d0[0, 1] == 0 and d0[1, 1] == 0          # zeros / ones meet their copy and the zeros / ones row
    assert (got[3][1][:, 0] == 0).all()
    np.testing.assert_array_equal(got[4][1], [[0, INT_MAX], [256, INT_MAX]])
    np.testing.assert_array_equal(got[5][1], [[256, INT_MAX], [0, INT_MAX]])
    np.testing.assert_array_equal(got[6][1], [[256, 256], [0, 0]])
    np.testing.assert_array_equal(got[6][0], [[0, 1], [0, 1]])
    np.testing.assert_array_equal(got[7][1], [[0, 0], [256, 256]])
    for p in (4, 5, 8, 9, 10, 11):                                            # nB = 1
        assert (got[p][0][:, 0] == 0).all() and (got[p][0][:, 1] == -1).all()
        assert (got[p][1][:, 1] == INT_MAX).all() and not got[p][2].any()
    assert got[8][1][2, 0] == 0 and got[9][1][2, 0] == 256


def test_bf2nn_pipeline_ties_across_accumulators_and_buffers(gpu_ctx):
    """Identical train rows 32 apart (one in each accumulator of the ping-pong), 64 apart (one in each tile buffer) and both: equal
    distances, the lower index wins the first slot and the next lower the second."""
    rng = np.random.default_rng(78)
    na, nb = 48, 320
    A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    want = np.zeros((na, 2), np.int32)
    used = np.zeros(nb, bool)
    for q in range(na):
        offs = [(0, 32), (0, 64), (0, 32, 64)][q % 3]
        j = next(j for j in range(7 * q % 50, nb - 64) if not any(used[j + o] for o in offs))
        for o in offs:
            B[j + o] = _flip(A[q], [q, 255 - q][:1 + q % 2])
            used[j + o] = True
        want[q] = (j, j + offs[1])
    got = _bf(gpu_ctx, [A, A[:33]], [B, B[:97]], 320, 1.0)
    _bf_check(got, [A, A[:33]], [B, B[:97]], 1.0)
    np.testing.assert_array_equal(got[0][0], want)
    assert (got[0][1][:, 0] == got[0][1][:, 1]).all() and not got[0][2].any()          # equal distances never pass a strict ratio test


def _fisheye_frames(rng):
    """Frames for the sliced instance: lapping offsets in {0, 1, 33} on both sides, right slice lengths from the nB list (each with every
    offset), left slice lengths from the nA list.  A scene seen by the rig, the right rows in another order, a few bits apart."""
    import oracle_bind as ob
    import oracle_match_bind as om
    from test_stereo_fisheye_oracle import RIG
    c1, c2 = (1, RIG["cam1"].astype(np.float64)), (1, RIG["cam2"].astype(np.float64))
    R, t = RIG["Rlr"].astype(np.float64), RIG["tlr"].astype(np.float64)
    frames = []
    for k, sb in enumerate(NB * 3):
        monoR = (0, 1, 33)[(k // len(NB)) % 3]
        monoL = (0, 1, 33)[(k + k // len(NB) + 1) % 3]
        sa = (NA + [64, 97])[k % 9]
        nL, nR = monoL + sa, monoR + sb
        n = max(nL, nR, 1)
        X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(1.5, 3.5, n)], 1)
        uvL, uvR = om.kb8_project_np(c1, X), om.kb8_project_np(c2, (X - t) @ R)
        D = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        DR = D ^ (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8) & 0x11)
        octv = rng.integers(0, 3, n)
        kpL = np.zeros(nL, ob.KP_DTYPE); kpR = np.zeros(nR, ob.KP_DTYPE)
        kpL["x"], kpL["y"], kpL["octave"] = uvL[:nL, 0], uvL[:nL, 1], octv[:nL]
        # the right frame shows the points the left slice shows (as far as it has room), in another order, behind its own offset
        seen = monoL + np.arange(sa)
        if sb > sa:
            seen = np.concatenate([seen, np.setdiff1d(np.arange(n), seen)[:sb - sa]])
        src = np.concatenate([rng.integers(0, n, monoR), rng.permutation(seen)[:sb]]).astype(np.int64)
        kpR["x"], kpR["y"], kpR["octave"] = uvR[src, 0], uvR[src, 1], octv[src]
        dL = D[:nL].copy()
        dL[monoL + 1::4] = rng.integers(0, 256, (len(dL[monoL + 1::4]), 32), dtype=np.uint8)      # unrelated descriptors: the ratio test rejects them
        frames.append((kpL, dL, monoL, kpR, DR[src].copy(), monoR))
    return frames


def test_stereo_fisheye_sliced_instance_offsets_and_slice_lengths(gpu_ctx):
    """k_bf2nn_mfma<true> through compute_stereo_fisheye_matches_device: l2r / r2l (and depth, points, counts) equal the oracle
    composition for every right slice length of the nB list behind every lapping offset."""
    import oracle_bind as ob
    from test_gpu_stereo_fisheye import _dev, _run_device
    from test_stereo_fisheye_oracle import fisheye_oracle, level_sigma2
    rng = np.random.default_rng(79)
    frames = _fisheye_frames(rng)
    Bn, max_n = len(frames), 360
    KL = np.zeros((Bn, max_n), ob.KP_DTYPE); KR = np.zeros((Bn, max_n), ob.KP_DTYPE)
    DL = np.zeros((Bn, max_n, 32), np.uint8); DR = np.zeros((Bn, max_n, 32), np.uint8)
    nL = np.zeros(Bn, np.int32); nR = np.zeros(Bn, np.int32); mL = np.zeros(Bn, np.int32); mR = np.zeros(Bn, np.int32)
    for f, (kpL, dL, monoL, kpR, dR, monoR) in enumerate(frames):
        KL[f, :len(kpL)] = kpL; DL[f, :len(kpL)] = dL; KR[f, :len(kpR)] = kpR; DR[f, :len(kpR)] = dR
        nL[f], nR[f], mL[f], mR[f] = len(kpL), len(kpR), monoL, monoR
    exp = [fisheye_oracle(*fr) for fr in frames]
    assert sum(e[4] for e in exp) > 1000                                      # on the CPU first: real matches that triangulate ...
    for fr, e in zip(frames, exp):
        if len(fr[3]) - fr[5] >= 32 and len(fr[0]) - fr[2] >= 32:
            assert e[4] > 0 and e[5] < len(fr[0]) - fr[2], (len(fr[0]), len(fr[3]))     # ... and rejected queries in every larger frame
    d = [_dev(a) for a in (KL.view(np.uint8), DL, nL, mL, KR.view(np.uint8), DR, nR, mR)]
    l2r, r2l, depth, x3d, nm = _run_device(gpu_ctx, (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max_n),
                                           (d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), max_n), Bn, max_n, level_sigma2())
    for f, (fr, e) in enumerate(zip(frames, exp)):
        el2r, er2l, edp, ex3d, en, _ = e
        a, b = len(fr[0]), len(fr[3])
        assert l2r[f, :a].tobytes() == el2r.tobytes(), (f, a, b, fr[2], fr[5])
        assert r2l[f, :b].tobytes() == er2l.tobytes(), (f, a, b, fr[2], fr[5])
        assert depth[f, :a].tobytes() == edp.tobytes() and x3d[f, :a].tobytes() == ex3d.tobytes(), f
        assert nm[f] == en, (f, nm[f], en)
