"""HIP-vs-oracle parity of the Hamming matching kernels (rows M1, M2), through the C ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf(gpu_ctx, descs_a, descs_b, max_n, ratio=0.7, pad=(0, 0)):
    """descs_*: list of [n,32] uint8 arrays (ragged).  pad: extra bytes (multiples of 16) after each pair's max_n rows of A / B, filled with
    0xA5 (strides larger than 32 * max_n).  Returns per-pair (idx2, dist2, accept); rows beyond nA must be untouched."""
    import torch
    import orbhip
    P = len(descs_a)
    sA, sB = max_n * 32 + pad[0], max_n * 32 + pad[1]
    assert sA % 16 == 0 and sB % 16 == 0                  # the kernels' uint4 loads
    A = np.full((P, sA), 0xA5, np.uint8)
    B = np.full((P, sB), 0xA5, np.uint8)
    A[:, :max_n * 32] = 0
    B[:, :max_n * 32] = 0
    nA = np.array([len(d) for d in descs_a], np.int32)
    nB = np.array([len(d) for d in descs_b], np.int32)
    for p in range(P):
        A[p, :nA[p] * 32] = np.asarray(descs_a[p], np.uint8).reshape(-1)
        B[p, :nB[p] * 32] = np.asarray(descs_b[p], np.uint8).reshape(-1)
    dA, dB, dnA, dnB = _dev(A), _dev(B), _dev(nA), _dev(nB)
    idx = torch.full((P, max_n, 2), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((P, max_n, 2), -7, dtype=torch.int32, device="cuda")
    acc = torch.full((P, max_n), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    orbhip.match_bf2nn_device(gpu_ctx, dA.data_ptr(), dnA.data_ptr(), sA, dB.data_ptr(), dnB.data_ptr(),
                              sB, P, max_n, ratio, idx.data_ptr(), dist.data_ptr(), acc.data_ptr())
    gpu_ctx.synchronize()
    idx, dist, acc = idx.cpu().numpy(), dist.cpu().numpy(), acc.cpu().numpy()
    for p in range(P):
        assert (idx[p, nA[p]:] == -7).all() and (dist[p, nA[p]:] == -7).all() and (acc[p, nA[p]:] == 9).all(), p
    return [(idx[p, :nA[p]], dist[p, :nA[p]], acc[p, :nA[p]]) for p in range(P)]


def test_descriptor_distance_host():
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = rng.integers(0, 256, 32, dtype=np.uint8)
        d = orbhip.descriptor_distance(a, b)
        assert d == om.descriptor_distance(a, b) == int(np.unpackbits(a ^ b).sum())
    z = np.zeros(32, np.uint8)
    assert orbhip.descriptor_distance(z, z) == 0
    assert orbhip.descriptor_distance(z, ~z) == 256


def test_bf2nn_random_ragged(gpu_ctx):
    import oracle_match_bind as om
    rng = np.random.default_rng(1)
    sizes = [(0, 5), (5, 0), (1, 1), (3, 1), (257, 300), (1000, 1037), (256, 256), (700, 2)]
    da = [rng.integers(0, 256, (a, 32), dtype=np.uint8) for a, _ in sizes]
    db = [rng.integers(0, 256, (b, 32), dtype=np.uint8) for _, b in sizes]
    got = _bf(gpu_ctx, da, db, 1100)
    for p, (a, b) in enumerate(sizes):
        oi, od, oa = om.bf2nn(da[p], db[p], 0.7)
        np.testing.assert_array_equal(got[p][0], oi, err_msg="idx pair %d" % p)
        np.testing.assert_array_equal(got[p][1], od, err_msg="dist pair %d" % p)
        np.testing.assert_array_equal(got[p][2], oa, err_msg="accept pair %d" % p)


def test_bf2nn_ties_and_duplicates(gpu_ctx):
    """Collisions: duplicated train rows -> lowest index must win both slots' ordering."""
    import oracle_match_bind as om
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    B = np.concatenate([base, base, base[:10]])          # every row appears 2-3 times
    A = base.copy()
    A[::3, 0] ^= 1
    got = _bf(gpu_ctx, [A], [B], 128)[0]
    oi, od, oa = om.bf2nn(A, B, 0.7)
    np.testing.assert_array_equal(got[0], oi)
    np.testing.assert_array_equal(got[1], od)
    np.testing.assert_array_equal(got[2], oa)
    assert (got[0][:, 0] < 40).all()


def test_bf2nn_on_extracted_frames(gpu_ctx):
    import orbhip
    import oracle_match_bind as om
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    imgs = orbhip.synth_frames(640, 480, 4, seed=31)
    res = ext.extract_host(imgs)
    da = [res[i][1] for i in range(3)]
    db = [res[i + 1][1] for i in range(3)]
    got = _bf(gpu_ctx, da, db, ext.max_keypoints)
    n_acc = 0
    for p in range(3):
        oi, od, oa = om.bf2nn(da[p], db[p], 0.7)
        np.testing.assert_array_equal(got[p][0], oi)
        np.testing.assert_array_equal(got[p][1], od)
        np.testing.assert_array_equal(got[p][2], oa)
        n_acc += int(oa.sum())
    assert n_acc > 100          # consecutive synthetic frames really do match
    ext.close()


def _flip(d, bits):
    """d with the given bit positions (0..255) inverted: a train row at a chosen Hamming distance from a query."""
    u = np.unpackbits(np.asarray(d, np.uint8))
    u[np.asarray(bits, np.int64)] ^= 1
    return np.packbits(u)


def _plant(rng, A, B, queries, rows, dists):
    """Train row rows[k] becomes a copy of query queries[k] at Hamming distance dists[k] (the planted rows of one query are its two
    nearest: unrelated random descriptors sit ~128 bits away)."""
    for q, j, d in zip(queries, rows, dists):
        B[j] = _flip(A[q], rng.choice(256, d, replace=False))


def _bf_check(got, da, db, ratio):
    import oracle_match_bind as om
    for p in range(len(da)):
        oi, od, oa = om.bf2nn(da[p], db[p], ratio)
        np.testing.assert_array_equal(got[p][0], oi, err_msg="idx pair %d" % p)
        np.testing.assert_array_equal(got[p][1], od, err_msg="dist pair %d" % p)
        np.testing.assert_array_equal(got[p][2], oa, err_msg="accept pair %d" % p)


# (best, second) distances with best == ratio * second exactly in double: the strict < of Frame.cc:1153 must reject them
_EXACT = {0.6: [(3, 5), (6, 10), (0, 0)], 0.75: [(3, 4), (6, 8), (9, 12)], 1.0: [(5, 5), (0, 0), (7, 7)]}


@pytest.mark.parametrize("ratio", [0.6, 0.75, 1.0])
@pytest.mark.parametrize("max_n", [1, 2, 31, 63, 64])
def test_bf2nn_small_frames(gpu_ctx, max_n, ratio):
    """max_n < 64 goes to the xor / popcount kernel k_bf2nn (64: the matrix-core one): ragged nA / nB in {0, 1, max_n}, strides above
    32 * max_n, planted neighbours at best == ratio * second, just inside and just outside the ratio."""
    rng = np.random.default_rng(max_n * 10 + int(ratio * 100))
    sizes = sorted({(a, b) for a in (0, 1, max_n) for b in (0, 1, max_n)})
    da, db = [], []
    for a, b in sizes:
        A = rng.integers(0, 256, (a, 32), dtype=np.uint8)
        B = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        if a and b >= 2:
            pairs = _EXACT[ratio] + [(4, 9), (8, 9), (2, 2), (1, 60)]
            for q in range(min(a, b // 2)):
                d1, d2 = pairs[q % len(pairs)]
                j1, j2 = rng.choice(b, 2, replace=False)
                _plant(rng, A, B, [q, q], [j1, j2], [d1, d2])
        da.append(A); db.append(B)
    for pad in ((0, 0), (16, 48), (32 * 7, 16)):
        _bf_check(_bf(gpu_ctx, da, db, max_n, ratio, pad=pad), da, db, ratio)


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("max_n,nb", [(40000, 40000), (65535, 65535)])
def test_bf2nn_high_train_indices(gpu_ctx, monkeypatch, path, max_n, nb):
    """Train indices above 32767 (the 16-bit index field of the 2-NN keys) and the last one, nB - 1: every query's two nearest rows
    are planted high; duplicates 64 and 256 rows apart (one matrix-core / xor tile) where the lower index must win."""
    if path == "valu":
        monkeypatch.setenv("ORBHIP_BF2NN_VALU", "1")                       # read on every call
    else:
        monkeypatch.delenv("ORBHIP_BF2NN_VALU", raising=False)
    rng = np.random.default_rng(nb)
    na = 300
    A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    hi = 32768 + rng.choice(nb - 32768 - 300, na, replace=False)
    for q in range(na):
        k = q % 6
        if k == 0:                                                        # the best at the very last row (B[nb - 1] = A[0], below)
            if q:
                A[q] = _flip(A[0], rng.choice(256, 2, replace=False))
            _plant(rng, A, B, [q], [hi[q]], [3])
        elif k == 1:                                                      # identical copies 64 rows apart: equal distance, lower index first
            B[hi[q]] = B[hi[q] + 64] = _flip(A[q], rng.choice(256, 2, replace=False))
        elif k == 2:                                                      # 256 rows apart
            B[hi[q]] = B[hi[q] + 256] = _flip(A[q], rng.choice(256, 4, replace=False))
        elif k == 3:                                                      # best == 0.75 * second, both high
            _plant(rng, A, B, [q, q], [hi[q], hi[q] + 1], [3, 4])
        elif k == 4:                                                      # best high, second low
            _plant(rng, A, B, [q, q], [hi[q], 5 + q], [2, 3])
        else:                                                             # best just above 32767
            _plant(rng, A, B, [q, q], [32768 + q, hi[q]], [0, 5])
    B[nb - 1] = A[0]
    # (a plant may overwrite an earlier one; the oracle decides what is right)
    for ratio, pad in ((0.75, (0, 0)), (0.6, (16, 32)), (1.0, (0, 16))):
        got = _bf(gpu_ctx, [A, A[:7]], [B, B[:nb // 2]], max_n, ratio, pad=pad)
        _bf_check(got, [A, A[:7]], [B, B[:nb // 2]], ratio)
    bi = got[0][0][:, 0]
    assert (bi > 32767).mean() > 0.8 and (bi == nb - 1).sum() >= na // 6 - 2
    assert (got[0][0][:, 1] - bi == 64).sum() > 30 and (got[0][0][:, 1] - bi == 256).sum() > 30


# ------------------------------------------------------------------ M3 + M4: SearchForInitialization
@pytest.fixture(params=["replay", "sequential", "sequential-small-lds-off", "sequential-small-lds-64"])
def si_form(request, monkeypatch):
    """SearchForInitialization has two forms with identical results: candidate lists for all F1 points at once + a replay of the
    vMatchedDistance rule (k_si_prep / k_si_candidates / k_si_replay, the default; pairs it cannot finish fall back on the device) and
    the sequential one-wave-per-pair loop (k_search_init).  ORBHIP_SI_PARALLEL_MAX_PAIRS=0 keeps the sequential kernel alone.
    The sequential kernel is launched twice (round 4): with LDS for ORBHIP_SI_SMALL_CAP0 (default 512) octave-0 points per frame first,
    then with the full carve for the pairs the first launch flagged; 0 switches the first launch off, 64 sends most pairs of these
    tests through the flag and the second launch."""
    monkeypatch.setenv("ORBHIP_SI_PARALLEL_MAX_PAIRS", "1048576" if request.param == "replay" else "0")
    if request.param == "sequential-small-lds-off":
        monkeypatch.setenv("ORBHIP_SI_SMALL_CAP0", "0")
    elif request.param == "sequential-small-lds-64":
        monkeypatch.setenv("ORBHIP_SI_SMALL_CAP0", "64")
    else:
        monkeypatch.delenv("ORBHIP_SI_SMALL_CAP0", raising=False)
    return request.param


def _search_init(gpu_ctx, frames_a, frames_b, bounds, prevs, max_n, window=100, ratio=0.9, check_ori=True):
    """frames_*: list of (kp structured array, desc [n,32]).  Returns per pair (nmatches, m12, prev)."""
    import torch
    import orbhip
    P = len(frames_a)
    kpA = np.zeros((P, max_n), orbhip.KP_DTYPE); kpB = np.zeros((P, max_n), orbhip.KP_DTYPE)
    dA = np.zeros((P, max_n, 32), np.uint8); dB = np.zeros((P, max_n, 32), np.uint8)
    nA = np.array([len(f[0]) for f in frames_a], np.int32); nB = np.array([len(f[0]) for f in frames_b], np.int32)
    prev = np.zeros((P, max_n, 2), np.float32)
    for p in range(P):
        kpA[p, :nA[p]] = frames_a[p][0]; dA[p, :nA[p]] = frames_a[p][1]
        kpB[p, :nB[p]] = frames_b[p][0]; dB[p, :nB[p]] = frames_b[p][1]
        prev[p, :nA[p]] = prevs[p]
    t = [torch.from_numpy(a.view(np.uint8) if a.dtype == orbhip.KP_DTYPE else a).cuda() for a in (kpA, dA, nA, kpB, dB, nB, prev)]
    m12 = torch.full((P, max_n), -9, dtype=torch.int32, device="cuda")
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_for_initialization_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                            t[4].data_ptr(), t[5].data_ptr(), P, max_n, max_n, bounds, window, ratio,
                                            check_ori, t[6].data_ptr(), m12.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12 = m12.cpu().numpy(); nm = nm.cpu().numpy(); pv = t[6].cpu().numpy()
    return [(int(nm[p]), m12[p, :nA[p]], pv[p, :nA[p]]) for p in range(P)]


@pytest.mark.parametrize("check_ori,window,ratio", [(True, 100, 0.9), (False, 100, 0.9), (True, 30, 0.6), (True, 400, 0.95)])
def test_search_for_initialization_parity(gpu_ctx, check_ori, window, ratio, si_form):
    import orbhip
    import oracle_match_bind as om
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    imgs = orbhip.synth_frames(640, 480, 6, seed=77)
    res = ext.extract_host(imgs, lap=(0, 0))
    fa = [(res[i][0], res[i][1]) for i in (0, 1, 2, 3, 4)]
    fb = [(res[i][0], res[i][1]) for i in (1, 2, 3, 5, 4)]        # incl. a 2-frame jump and a self-match
    bounds = (0.0, 0.0, 640.0, 480.0)
    prevs = [np.stack([f[0]["x"], f[0]["y"]], 1) for f in fa]     # Tracking.cc:1497-1499
    got = _search_init(gpu_ctx, fa, fb, bounds, prevs, ext.max_keypoints, window, ratio, check_ori)
    total = 0
    for p in range(len(fa)):
        n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], bounds, prevs[p], window, ratio, check_ori)
        assert got[p][0] == n, (p, got[p][0], n)
        np.testing.assert_array_equal(got[p][1], m12)
        assert got[p][2].tobytes() == prev.tobytes()
        total += n
    assert total > 50
    ext.close()


def test_search_for_initialization_edge_cases(gpu_ctx, si_form):
    """Empty frames, keypoints outside the grid, duplicated descriptors (ties), prev far off-image."""
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(5)

    def mk(n, spread=1.0):
        kp = np.zeros(n, orbhip.KP_DTYPE)
        kp["x"] = rng.uniform(-20, 660, n).astype(np.float32) * spread
        kp["y"] = rng.uniform(-20, 500, n).astype(np.float32) * spread
        kp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        kp["octave"] = rng.integers(0, 3, n)
        d = rng.integers(0, 256, (max(n // 8, 1), 32), dtype=np.uint8)[rng.integers(0, max(n // 8, 1), n)]   # many duplicates
        d[:, 0] ^= rng.integers(0, 4, n).astype(np.uint8)
        return kp, d
    fa = [mk(0), mk(50), mk(300), mk(200), mk(700)]
    fb = [mk(10), mk(0), mk(300), mk(200), mk(650)]
    fb[2] = (fa[2][0].copy(), fa[2][1].copy())                     # identical frame: every level-0 point has an exact twin
    bounds = (0.0, 0.0, 640.0, 480.0)
    prevs = [np.stack([f[0]["x"], f[0]["y"]], 1) for f in fa]
    prevs[3] = prevs[3] + 5000.0                                    # windows entirely outside the grid
    got = _search_init(gpu_ctx, fa, fb, bounds, prevs, 800, 100, 0.9, True)
    for p in range(len(fa)):
        n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], bounds, prevs[p], 100, 0.9, True)
        assert got[p][0] == n, (p, got[p][0], n)
        np.testing.assert_array_equal(got[p][1], m12)
        assert got[p][2].tobytes() == prev.tobytes()


def test_search_for_initialization_contested_points(gpu_ctx, si_form):
    """Dense clusters with few distinct descriptors: many F1 points want the same F2 point (vMatchedDistance displaces earlier matches,
    later queries skip deep into their lists), windows with more than 64 candidates (truncated lists: the replay form must notice when a
    list runs dry and hand the pair to the sequential kernel), one exact-copy pair (every point has a distance-0 twin)."""
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(91)

    def mk(n, cx, cy, sigma, ndesc, flips):
        kp = np.zeros(n, orbhip.KP_DTYPE)
        kp["x"] = np.clip(rng.normal(cx, sigma, n), 1, 638).astype(np.float32)
        kp["y"] = np.clip(rng.normal(cy, sigma, n), 1, 478).astype(np.float32)
        kp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        kp["octave"] = (rng.uniform(0, 1, n) < 0.1).astype(np.int32)             # 90 % at octave 0
        base = rng.integers(0, 256, (ndesc, 32), dtype=np.uint8)
        d = base[rng.integers(0, ndesc, n)].copy()
        for _ in range(flips):                                                    # a few random bit flips: distances 0 .. 2 * flips
            d[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
        return kp, d
    protos = [mk(1, 0, 0, 1, 6, 0)[1]]
    fa, fb = [], []
    for (n, sig, nd, fl) in [(300, 40, 6, 3), (500, 25, 4, 5), (250, 90, 12, 2), (600, 60, 3, 8), (180, 15, 2, 4)]:
        a = mk(n, 320, 240, sig, nd, fl); b = mk(n + 30, 325, 238, sig, nd, fl)
        b[1][:] = a[1][rng.integers(0, n, n + 30)]                                # F2 descriptors drawn from F1's: small distances everywhere
        b[1][np.arange(n + 30), rng.integers(0, 32, n + 30)] ^= (1 << rng.integers(0, 8, n + 30)).astype(np.uint8)
        fa.append(a); fb.append(b)
    fa.append(fa[0]); fb.append((fa[0][0].copy(), fa[0][1].copy()))
    bounds = (0.0, 0.0, 640.0, 480.0)
    prevs = [np.stack([f[0]["x"], f[0]["y"]], 1) for f in fa]
    for window, ratio in ((100, 0.9), (40, 0.99)):
        got = _search_init(gpu_ctx, fa, fb, bounds, prevs, 800, window, ratio, True)
        tot = 0
        for p in range(len(fa)):
            n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], bounds, prevs[p], window, ratio, True)
            assert got[p][0] == n, (p, window, got[p][0], n)
            np.testing.assert_array_equal(got[p][1], m12)
            assert got[p][2].tobytes() == prev.tobytes()
            tot += n
        assert tot > 100, tot


# ------------------------------------------------------------------ M3 + M4: SearchByProjection (tracking)
@pytest.fixture(params=["replay", "sequential"])
def sbp_form(request, monkeypatch):
    """SearchByProjection has two forms with identical results: candidate lists for all queries at once + a replay of the claim rule (calls
    with few frame pairs: Tracking's one) and the sequential one-wave-per-pair loop (batches).  ORBHIP_SBP_PARALLEL_MAX_PAIRS moves the switch."""
    monkeypatch.setenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS", "64" if request.param == "replay" else "0")
    return request.param


def _sbp(gpu_ctx, cases, max_q, max_n, bounds, th_high=100, check_ori=True, stereo=False, map_ratio=None):
    """cases: list of (q, dq, kp, d, u_right|None, train_match).  Returns per pair (nmatches, train_match)."""
    import torch
    import orbhip
    P = len(cases)
    Q = np.zeros((P, max_q), orbhip.PROJ_QUERY_DTYPE); DQ = np.zeros((P, max_q, 32), np.uint8)
    KP = np.zeros((P, max_n), orbhip.KP_DTYPE); D = np.zeros((P, max_n, 32), np.uint8)
    UR = np.full((P, max_n), -1, np.float32); TM = np.full((P, max_n), -1, np.int32)
    nq = np.array([len(c[0]) for c in cases], np.int32); n = np.array([len(c[2]) for c in cases], np.int32)
    for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
        Q[p, :nq[p]] = q; DQ[p, :nq[p]] = dq; KP[p, :n[p]] = kp; D[p, :n[p]] = d; TM[p, :n[p]] = tm
        if ur is not None:
            UR[p, :n[p]] = ur
    t = [torch.from_numpy(a.view(np.uint8) if a.dtype in (orbhip.KP_DTYPE, orbhip.PROJ_QUERY_DTYPE) else a).cuda()
         for a in (Q, DQ, nq, KP, D, UR, n, TM)]
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if map_ratio is None:
        orbhip.search_by_projection_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), max_q, t[3].data_ptr(),
                                           t[4].data_ptr(), t[5].data_ptr() if stereo else None, t[6].data_ptr(), max_n, max_n, P,
                                           bounds, th_high, check_ori, t[7].data_ptr(), nm.data_ptr())
    else:
        orbhip.search_local_map_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), max_q, t[3].data_ptr(),
                                       t[4].data_ptr(), t[5].data_ptr() if stereo else None, t[6].data_ptr(), max_n, max_n, P,
                                       bounds, th_high, map_ratio, t[7].data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    tm = t[7].cpu().numpy(); nm = nm.cpu().numpy()
    return [(int(nm[p]), tm[p, :n[p]]) for p in range(P)]


@pytest.mark.parametrize("stereo,check_ori", [(False, True), (True, True), (False, False)])
def test_search_by_projection_synthetic_parity(gpu_ctx, stereo, check_ori, sbp_form):
    """Ragged batch incl. empty sides, out-of-grid keypoints, duplicated descriptors (ties), pre-held keypoints,
    re-claims by points without observations, all three level-range modes."""
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case
    rng = np.random.default_rng(21 + stereo)
    bounds = (0.0, 0.0, 640.0, 480.0)
    cases = [make_sbp_case(rng, n, nq, stereo) for n, nq in ((0, 10), (60, 0), (300, 300), (1000, 900), (2048, 2048), (700, 1500))]
    got = _sbp(gpu_ctx, cases, 2048, 2048, bounds, 100, check_ori, stereo)
    tot = 0
    for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
        n_ref, tm_ref = om.search_by_projection(q, dq, kp, d, ur if stereo else None, bounds, tm, 100, check_ori)
        assert got[p][0] == n_ref, (p, got[p][0], n_ref)
        np.testing.assert_array_equal(got[p][1], tm_ref)
        tot += n_ref
    assert tot > 500


def test_search_by_projection_on_extracted_frames(gpu_ctx, sbp_form):
    """TrackWithMotionModel shape: last frame's keypoints projected with the synthetic inter-frame motion."""
    import orbhip
    import oracle_match_bind as om
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    imgs = orbhip.synth_frames(640, 480, 5, seed=99)
    res = ext.extract_host(imgs, lap=(0, 0))
    sf = ext.table(0)
    bounds = (0.0, 0.0, 640.0, 480.0)
    cases = []
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 4)):
        kpa, da = res[a][0], res[a][1]
        q = np.zeros(len(kpa), orbhip.PROJ_QUERY_DTYPE)
        q["u"] = kpa["x"]; q["v"] = kpa["y"]; q["angle"] = kpa["angle"]
        q["radius"] = (np.float32(15.0) * sf[kpa["octave"]]).astype(np.float32)       # th = 15 (Tracking.cc:2685), ORBmatcher.cc:2014
        q["min_level"] = kpa["octave"] - 1; q["max_level"] = kpa["octave"] + 1          # neither forward nor backward
        q["has_obs"] = 1; q["ur"] = -1
        inside = (q["u"] >= 0) & (q["u"] <= 640) & (q["v"] >= 0) & (q["v"] <= 480)   # ORBmatcher.cc:2005-2008
        cases.append((q[inside], da[inside], res[b][0], res[b][1], None, np.full(len(res[b][0]), -1, np.int32)))
    got = _sbp(gpu_ctx, cases, ext.max_keypoints, ext.max_keypoints, bounds)
    for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
        n_ref, tm_ref = om.search_by_projection(q, dq, kp, d, None, bounds, tm, 100, True)
        assert got[p][0] == n_ref
        np.testing.assert_array_equal(got[p][1], tm_ref)
        assert n_ref > 100
    ext.close()


@pytest.mark.parametrize("mode", ["last_frame", "local_map"])
def test_search_by_projection_contested_keypoints(gpu_ctx, sbp_form, mode):
    """Many queries with near-identical descriptors over the same window, all carrying observations: every claim blocks the keypoint for
    the later ones, so query t ends up with the t-th best -- the replay form walks deep into its lists and, where a list cut at its 32 entries
    runs dry, hands the pair to the sequential kernel.  Mixed with queries without observations (claims that do not block) and pre-held keypoints."""
    import oracle_match_bind as om
    import orbhip
    rng = np.random.default_rng(77)
    bounds = (0.0, 0.0, 640.0, 480.0)
    cases = []
    for n, nq, spread in ((400, 150, 25.0), (300, 40, 8.0), (1200, 600, 60.0)):
        kp = np.zeros(n, orbhip.KP_DTYPE)
        kp["x"] = (320 + rng.normal(0, spread, n)).astype(np.float32); kp["y"] = (240 + rng.normal(0, spread, n)).astype(np.float32)
        kp["octave"] = rng.integers(0, 3, n); kp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d = np.tile(base, (n, 1)); flips = rng.integers(0, 32, (n, 3)); d[np.arange(n)[:, None], flips] ^= (1 << rng.integers(0, 8, (n, 3))).astype(np.uint8)
        q = np.zeros(nq, orbhip.PROJ_QUERY_DTYPE)
        q["u"] = (320 + rng.normal(0, 3, nq)).astype(np.float32); q["v"] = (240 + rng.normal(0, 3, nq)).astype(np.float32)
        q["radius"] = np.float32(3 * spread); q["min_level"] = 0; q["max_level"] = 3; q["ur"] = -1; q["angle"] = rng.uniform(0, 360, nq).astype(np.float32)
        q["has_obs"] = (rng.random(nq) < 0.8).astype(np.int32)
        dq = np.tile(base, (nq, 1)); dq[np.arange(nq), rng.integers(0, 32, nq)] ^= (1 << rng.integers(0, 8, nq)).astype(np.uint8)
        tm = np.where(rng.random(n) < 0.1, 5, -1).astype(np.int32)
        cases.append((q, dq, kp, d, None, tm))
    if mode == "last_frame":
        got = _sbp(gpu_ctx, cases, 1024, 2048, bounds, 100, True, False)
    else:
        got = _sbp(gpu_ctx, cases, 1024, 2048, bounds, 100, True, False, map_ratio=0.9)
    for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
        if mode == "last_frame":
            n_ref, tm_ref = om.search_by_projection(q, dq, kp, d, None, bounds, tm, 100, True)
        else:
            n_ref, tm_ref = om.search_by_projection_map(q, dq, kp, d, None, bounds, tm, 100, 0.9)
        assert got[p][0] == n_ref, (p, got[p][0], n_ref)
        np.testing.assert_array_equal(got[p][1], tm_ref)
        assert n_ref >= 10


def test_search_by_projection_big_keyframes_and_capacity(gpu_ctx):
    """Frames / keyframes beyond the replay form's 2048 keypoints (the two first keyframes of a monocular map carry 5 x nFeatures,
    Tracking.cc:210) take the sequential kernel alone (round 4; refused in round 3): 2100 and 5200 keypoints equal the oracle.  What LDS
    cannot hold (17 B per keypoint + 3 B per query + the grid > 160 KB) is refused with ORBHIP_E_CAPACITY, loudly."""
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case
    rng = np.random.default_rng(3)
    bounds = (0.0, 0.0, 640.0, 480.0)
    for n, nq in ((2100, 10), (5200, 900)):
        c = make_sbp_case(rng, n, nq, False)
        got = _sbp(gpu_ctx, [c], max(nq, 16), n, bounds)
        q, dq, kp, d, ur, tm = c
        n_ref, tm_ref = om.search_by_projection(q, dq, kp, d, ur, bounds, tm, 100, True)
        assert got[0][0] == n_ref
        np.testing.assert_array_equal(got[0][1], tm_ref)
    c = make_sbp_case(rng, 9000, 10, False)
    with pytest.raises(orbhip.OrbHipError):
        _sbp(gpu_ctx, [c], 16, 9000, bounds)
    gpu_ctx.check_status()


def test_search_for_initialization_5x_features(gpu_ctx, si_form):
    """The monocular-initialisation extractor runs 5 x nFeatures (Tracking.cc:210): 5000 keypoints, > 1024 at octave 0."""
    import orbhip
    import oracle_match_bind as om
    ext = orbhip.Extractor(gpu_ctx, 5000, 1.2, 8, 20, 7)
    imgs = orbhip.synth_frames(1280, 960, 3, seed=5)
    res = ext.extract_host(imgs, lap=(0, 0))
    assert len(res[0][0]) > 4000 and (res[0][0]["octave"] == 0).sum() > 1024
    fa = [(res[i][0], res[i][1]) for i in (0, 1)]
    fb = [(res[i][0], res[i][1]) for i in (1, 2)]
    bounds = (0.0, 0.0, 1280.0, 960.0)
    prevs = [np.stack([f[0]["x"], f[0]["y"]], 1) for f in fa]
    got = _search_init(gpu_ctx, fa, fb, bounds, prevs, ext.max_keypoints, 100, 0.9, True)
    for p in range(2):
        n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], bounds, prevs[p], 100, 0.9, True)
        assert got[p][0] == n and n > 100
        np.testing.assert_array_equal(got[p][1], m12)
        assert got[p][2].tobytes() == prev.tobytes()
    ext.close()


def test_search_for_initialization_2000_features(gpu_ctx, si_form):
    """BASELINE config #3's extractor (2000 features at 1080p): ~434 keypoints at octave 0, the eight-slot register-resident loop
    (the 1000-feature tests take the four-slot one, the 5000-feature test the general LDS loop)."""
    import orbhip
    import oracle_match_bind as om
    ext = orbhip.Extractor(gpu_ctx, 2000, 1.2, 8, 20, 7)
    imgs = orbhip.synth_frames(1920, 1080, 3, seed=15)
    res = ext.extract_host(imgs, lap=(0, 0))
    n_oct0 = int((res[0][0]["octave"] == 0).sum())
    assert 256 < n_oct0 <= 512, n_oct0
    fa = [(res[i][0], res[i][1]) for i in (0, 1, 2)]
    fb = [(res[i][0], res[i][1]) for i in (1, 2, 2)]
    bounds = (0.0, 0.0, 1920.0, 1080.0)
    prevs = [np.stack([f[0]["x"], f[0]["y"]], 1) for f in fa]
    got = _search_init(gpu_ctx, fa, fb, bounds, prevs, ext.max_keypoints, 100, 0.9, True)
    for p in range(3):
        n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], bounds, prevs[p], 100, 0.9, True)
        assert got[p][0] == n and n > 20, (p, got[p][0], n)
        np.testing.assert_array_equal(got[p][1], m12)
        assert got[p][2].tobytes() == prev.tobytes()
    ext.close()


@pytest.mark.parametrize("stereo,ratio", [(False, 0.8), (True, 0.8), (False, 0.6)])
def test_search_local_map_parity(gpu_ctx, stereo, ratio, sbp_form):
    """TrackLocalMap matcher (ORBmatcher.cc:48-218): best / second best with the same-octave ratio rule, claim rule."""
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case
    rng = np.random.default_rng(41 + stereo)
    bounds = (0.0, 0.0, 640.0, 480.0)
    cases = [make_sbp_case(rng, n, nq, stereo) for n, nq in ((0, 10), (60, 0), (300, 300), (1000, 900), (2048, 2048), (700, 1500))]
    for c in cases:
        c[0]["min_level"] = np.maximum(c[0]["max_level"], 0) - 1; c[0]["max_level"] = c[0]["min_level"] + 1
    got = _sbp(gpu_ctx, cases, 2048, 2048, bounds, 100, False, stereo, map_ratio=ratio)
    tot = 0
    for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
        n_ref, tm_ref = om.search_by_projection_map(q, dq, kp, d, ur if stereo else None, bounds, tm, 100, ratio)
        assert got[p][0] == n_ref, (p, got[p][0], n_ref)
        np.testing.assert_array_equal(got[p][1], tm_ref)
        tot += n_ref
    assert tot > 300


def test_distinctive_descriptors_parity(gpu_ctx):
    """MapPoint::ComputeDistinctiveDescriptors batched: ragged observation counts incl. 0, 1, 2, duplicates, 256."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(17)
    counts = [0, 1, 2, 3, 5, 10, 33, 64, 65, 100, 200, 256] + list(rng.integers(1, 40, 200))
    P, M = len(counts), 256
    desc = np.zeros((P, M, 32), np.uint8)
    for p, n in enumerate(counts):
        if n == 0:
            continue
        base = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        d = np.repeat(base, n, 0) ^ (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8))
        if n > 3:
            d[n - 1] = d[0]
        desc[p, :n] = d
    d_desc = torch.from_numpy(desc).cuda(); d_n = torch.tensor(counts, dtype=torch.int32, device="cuda")
    bi = torch.full((P,), -9, dtype=torch.int32, device="cuda"); bd = torch.zeros((P, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    orbhip.distinctive_descriptors_device(gpu_ctx, d_desc.data_ptr(), d_n.data_ptr(), P, M, bi.data_ptr(), bd.data_ptr())
    gpu_ctx.synchronize()
    bi = bi.cpu().numpy(); bd = bd.cpu().numpy()
    for p, n in enumerate(counts):
        ref = om.distinctive_descriptor(desc[p, :n])
        assert bi[p] == ref, (p, n, bi[p], ref)
        if n > 0:
            assert bd[p].tobytes() == desc[p, ref].tobytes()


def test_bow_transform_parity(gpu_ctx):
    """Per-feature DBoW2 tree descent on synthetic vocabularies (k=10/L=4 regular; ragged tree), ragged frame sizes."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(29)
    for k, L, ragged, levelsup in ((10, 4, False, 2), (5, 5, True, 4), (10, 3, False, 4)):
        voc = om.make_vocabulary(rng, k, L, ragged)
        counts = [0, 1, 300, 777]
        F, M = len(counts), 800
        desc = np.zeros((F, M, 32), np.uint8)
        for f, n in enumerate(counts):
            leaves = rng.integers(1, len(voc["node_desc"]), n)
            desc[f, :n] = voc["node_desc"][leaves] ^ (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8))
        dv = [torch.from_numpy(np.ascontiguousarray(voc[key])).cuda() for key in ("node_desc", "child_start", "child_ids", "node_word", "node_weight")]
        d_desc = torch.from_numpy(desc).cuda(); d_n = torch.tensor(counts, dtype=torch.int32, device="cuda")
        wid = torch.full((F, M), -9, dtype=torch.int32, device="cuda"); w = torch.zeros((F, M), dtype=torch.float64, device="cuda")
        nid = torch.full((F, M), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        orbhip.bow_transform_device(gpu_ctx, d_desc.data_ptr(), d_n.data_ptr(), F, M, M, [t.data_ptr() for t in dv], L, levelsup,
                                    wid.data_ptr(), w.data_ptr(), nid.data_ptr())
        gpu_ctx.synchronize()
        wid, w, nid = wid.cpu().numpy(), w.cpu().numpy(), nid.cpu().numpy()
        for f, n in enumerate(counts):
            for i in range(0, n, 7):
                assert (int(wid[f, i]), float(w[f, i]), int(nid[f, i])) == om.bow_transform(desc[f, i], voc, levelsup)
            assert (wid[f, n:] == -9).all()


@pytest.mark.parametrize("stereo", [False, True])
def test_fuse_search_parity(gpu_ctx, stereo):
    import torch
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case
    rng = np.random.default_rng(51 + stereo)
    bounds = (0.0, 0.0, 640.0, 480.0)
    sig = (np.float32(1.0) / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
    cases = [make_sbp_case(rng, n, nq, stereo) for n, nq in ((0, 10), (60, 0), (300, 500), (1000, 900), (2000, 2048))]
    for c in cases:
        c[0]["min_level"] = np.maximum(c[0]["max_level"], 0) - 1; c[0]["max_level"] = c[0]["min_level"] + 1
        c[0]["radius"] = np.float32(3.0) * np.float32(1.2) ** c[0]["max_level"].astype(np.float32)
    P, MQ, MN = len(cases), 2048, 2048
    Q = np.zeros((P, MQ), orbhip.PROJ_QUERY_DTYPE); DQ = np.zeros((P, MQ, 32), np.uint8)
    KP = np.zeros((P, MN), orbhip.KP_DTYPE); D = np.zeros((P, MN, 32), np.uint8); UR = np.full((P, MN), -1, np.float32)
    nq = np.array([len(c[0]) for c in cases], np.int32); n = np.array([len(c[2]) for c in cases], np.int32)
    for p, (q, dq, kp, d, ur, _) in enumerate(cases):
        Q[p, :nq[p]] = q; DQ[p, :nq[p]] = dq; KP[p, :n[p]] = kp; D[p, :n[p]] = d
        if ur is not None:
            UR[p, :n[p]] = ur
    t = [torch.from_numpy(a.view(np.uint8) if a.dtype in (orbhip.KP_DTYPE, orbhip.PROJ_QUERY_DTYPE) else a).cuda() for a in (Q, DQ, nq, KP, D, UR, n)]
    bi = torch.full((P, MQ), -9, dtype=torch.int32, device="cuda"); bd = torch.full((P, MQ), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.fuse_search_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), MQ, t[3].data_ptr(), t[4].data_ptr(),
                              t[5].data_ptr() if stereo else None, t[6].data_ptr(), MN, MN, P, sig, bounds, bi.data_ptr(), bd.data_ptr())
    gpu_ctx.check_status()
    bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    hits = 0
    for p, (q, dq, kp, d, ur, _) in enumerate(cases):
        ri, rd = om.fuse_search(q, dq, kp, d, ur if stereo else None, sig, bounds)
        np.testing.assert_array_equal(bi[p, :nq[p]], ri); np.testing.assert_array_equal(bd[p, :nq[p]], rd)
        hits += int((ri >= 0).sum())
    assert hits > 200


@pytest.mark.parametrize("ratio,check_ori", [(0.7, True), (0.9, False)])
def test_search_by_bow_parity(gpu_ctx, ratio, check_ori):
    """TrackReferenceKeyFrame / Relocalization matcher (ORBmatcher.cc:273-475) on ragged pairs incl. empty sides."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(61)
    cases = [om.make_bow_case(rng, nk, nf, nn) for nk, nf, nn in ((0, 20, 10), (30, 0, 10), (200, 260, 40), (1000, 950, 100), (2000, 2048, 300), (600, 1500, 900))]
    P, MN, MNODE = len(cases), 2048, 2048
    arr = dict(ki=np.zeros((P, MNODE), np.int32), ks=np.zeros((P, MNODE + 1), np.int32), kf=np.zeros((P, MN), np.int32), kn=np.zeros(P, np.int32),
               fi=np.zeros((P, MNODE), np.int32), fs=np.zeros((P, MNODE + 1), np.int32), ff=np.zeros((P, MN), np.int32), fn=np.zeros(P, np.int32),
               va=np.zeros((P, MN), np.uint8), kpk=np.zeros((P, MN), orbhip.KP_DTYPE), kpf=np.zeros((P, MN), orbhip.KP_DTYPE),
               dk=np.zeros((P, MN, 32), np.uint8), df=np.zeros((P, MN, 32), np.uint8), nF=np.zeros(P, np.int32))
    for p, c in enumerate(cases):
        ki, ks, kf = om.feature_vector_csr(c["nid_k"]); fi, fs, ff = om.feature_vector_csr(c["nid_f"])
        arr["ki"][p, :len(ki)] = ki; arr["ks"][p, :len(ks)] = ks; arr["kf"][p, :len(kf)] = kf; arr["kn"][p] = len(ki)
        arr["fi"][p, :len(fi)] = fi; arr["fs"][p, :len(fs)] = fs; arr["ff"][p, :len(ff)] = ff; arr["fn"][p] = len(fi)
        nk, nf = len(c["kp_k"]), len(c["kp_f"])
        arr["va"][p, :nk] = c["valid"]; arr["kpk"][p, :nk] = c["kp_k"]; arr["kpf"][p, :nf] = c["kp_f"]
        arr["dk"][p, :nk] = c["d_k"]; arr["df"][p, :nf] = c["d_f"]; arr["nF"][p] = nf
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype == orbhip.KP_DTYPE else v).cuda() for k, v in arr.items()}
    mf = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_by_bow_device(gpu_ctx, [t[k].data_ptr() for k in ("ki", "ks", "kf", "kn", "va", "kpk", "dk")],
                                [t[k].data_ptr() for k in ("fi", "fs", "ff", "fn", "kpf", "df")], t["nF"].data_ptr(), P, MNODE, MN, MN,
                                ratio, check_ori, mf.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    mf, nm = mf.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = om.search_by_bow(c, ratio, check_ori)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        np.testing.assert_array_equal(mf[p, :len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 300


@pytest.mark.gpu
@pytest.mark.parametrize("stereo_frac,only_stereo,coarse,mono,check_ori", [(0.0, False, False, True, True), (0.4, False, False, False, True),
                                                                             (0.5, True, False, False, False), (0.0, False, True, True, True)])
def test_search_for_triangulation_parity(gpu_ctx, stereo_frac, only_stereo, coarse, mono, check_ori):
    """CreateNewMapPoints matcher (ORBmatcher.cc:969-1210) on ragged keyframe pairs incl. empty sides, bit-exact vs the oracle."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(83)
    cases = [om.make_tri_case(rng, a, b, nn, stereo_frac, only_stereo, coarse)
             for a, b, nn in ((0, 20, 10), (30, 0, 10), (200, 260, 40), (1000, 950, 100), (2000, 2048, 300), (600, 1500, 900))]
    P, MN, MNODE = len(cases), 2048, 2048
    arr = dict(nid1=np.zeros((P, MN), np.int32), mp1=np.zeros((P, MN), np.uint8), kp1=np.zeros((P, MN), orbhip.KP_DTYPE),
               d1=np.zeros((P, MN, 32), np.uint8), ur1=np.full((P, MN), -1, np.float32), n1=np.zeros(P, np.int32),
               i2=np.zeros((P, MNODE), np.int32), s2=np.zeros((P, MNODE + 1), np.int32), f2=np.zeros((P, MN), np.int32), nn2=np.zeros(P, np.int32),
               mp2=np.zeros((P, MN), np.uint8), kp2=np.zeros((P, MN), orbhip.KP_DTYPE), d2=np.zeros((P, MN, 32), np.uint8),
               ur2=np.full((P, MN), -1, np.float32), n2=np.zeros(P, np.int32), geom=np.zeros(P, orbhip.TRI_PAIR_DTYPE))
    for p, c in enumerate(cases):
        a, b = len(c["kp1"]), len(c["kp2"])
        i2, s2, f2 = om.feature_vector_csr(c["nid2"])
        arr["nid1"][p, :a] = c["nid1"]; arr["mp1"][p, :a] = c["mp1"]; arr["kp1"][p, :a] = c["kp1"]; arr["d1"][p, :a] = c["d1"]
        arr["ur1"][p, :a] = c["ur1"]; arr["n1"][p] = a
        arr["i2"][p, :len(i2)] = i2; arr["s2"][p, :len(s2)] = s2; arr["f2"][p, :len(f2)] = f2; arr["nn2"][p] = len(i2)
        arr["mp2"][p, :b] = c["mp2"]; arr["kp2"][p, :b] = c["kp2"]; arr["d2"][p, :b] = c["d2"]; arr["ur2"][p, :b] = c["ur2"]; arr["n2"][p] = b
        arr["geom"][p] = (c["F12"], c["ep"][0], c["ep"][1], int(only_stereo), int(coarse))
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in arr.items()}
    m12 = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ur1 = 0 if mono else t["ur1"].data_ptr(); ur2 = 0 if mono else t["ur2"].data_ptr()
    orbhip.search_for_triangulation_device(gpu_ctx, [t["nid1"].data_ptr(), t["mp1"].data_ptr(), t["kp1"].data_ptr(), t["d1"].data_ptr(), ur1, t["n1"].data_ptr()],
                                           [t["i2"].data_ptr(), t["s2"].data_ptr(), t["f2"].data_ptr(), t["nn2"].data_ptr(), t["mp2"].data_ptr(),
                                            t["kp2"].data_ptr(), t["d2"].data_ptr(), ur2, t["n2"].data_ptr()],
                                           t["geom"].data_ptr(), P, MNODE, MN, MN, cases[0]["scale"], cases[0]["sigma2"], check_ori,
                                           m12.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = om.search_for_triangulation(c, check_ori, mono)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        np.testing.assert_array_equal(m12[p, :len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 300


@pytest.mark.gpu
@pytest.mark.parametrize("mode,check_ori,big", [("kb8", True, False), ("rig", True, False), ("rig", False, False), ("pinhole", True, False), ("rig", True, True)])
def test_search_for_triangulation_points_parity(gpu_ctx, mode, check_ori, big):
    """The SearchForTriangulation overload that returns the triangulated points (ORBmatcher.cc:1212-1402; KannalaBrandt8::matchAndtriangulate,
    KannalaBrandt8.cpp:240-332): matches AND world points bit-exact vs the oracle on fisheye mono keyframes and fisheye rigs (all four camera
    pairs); a Pinhole first camera matches nothing (Pinhole.h:91-94); has_mp / rotation-histogram gates as the first overload; the points
    sit on the scene (they re-project into both keyframes).  big: keyframes above 4096 keypoints take the global-memory variant."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(1291)
    sizes = ((0, 20, 10), (30, 0, 10), (200, 260, 40), (1000, 950, 100), (2000, 2048, 300), (600, 1500, 900)) if not big else ((5200, 4700, 800), (300, 5000, 100))
    cases = [om.make_tri_general_case(rng, a, b, mode, nn, True, False) for a, b, nn in sizes]       # only_stereo set: must be ignored
    poses = [om.tri_case_poses(c, i) for i, c in enumerate(cases)]
    P, MN, MNODE = len(cases), (5248 if big else 2048), 2048
    arr = dict(nid1=np.zeros((P, MN), np.int32), mp1=np.zeros((P, MN), np.uint8), kp1=np.zeros((P, MN), orbhip.KP_DTYPE),
               d1=np.zeros((P, MN, 32), np.uint8), n1=np.zeros(P, np.int32),
               i2=np.zeros((P, MNODE), np.int32), s2=np.zeros((P, MNODE + 1), np.int32), f2=np.zeros((P, MN), np.int32), nn2=np.zeros(P, np.int32),
               mp2=np.zeros((P, MN), np.uint8), kp2=np.zeros((P, MN), orbhip.KP_DTYPE), d2=np.zeros((P, MN, 32), np.uint8),
               n2=np.zeros(P, np.int32), geom=np.zeros(P, orbhip.TRI_GENERAL_DTYPE), poses=np.zeros(P, orbhip.TRI_POSES_DTYPE))
    assert orbhip.TRI_POSES_DTYPE == om.TRI_POSES_DTYPE
    for p, c in enumerate(cases):
        a, b = len(c["kp1"]), len(c["kp2"])
        i2, s2, f2 = om.feature_vector_csr(c["nid2"])
        arr["nid1"][p, :a] = c["nid1"]; arr["mp1"][p, :a] = c["mp1"]; arr["kp1"][p, :a] = c["kp1"]; arr["d1"][p, :a] = c["d1"]; arr["n1"][p] = a
        arr["i2"][p, :len(i2)] = i2; arr["s2"][p, :len(s2)] = s2; arr["f2"][p, :len(f2)] = f2; arr["nn2"][p] = len(i2)
        arr["mp2"][p, :b] = c["mp2"]; arr["kp2"][p, :b] = c["kp2"]; arr["d2"][p, :b] = c["d2"]; arr["n2"][p] = b
        arr["geom"][p] = c["geom"]; arr["poses"][p] = poses[p]
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in arr.items()}
    m12 = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    pts = torch.full((P, MN, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kf1 = [t["nid1"].data_ptr(), t["mp1"].data_ptr(), t["kp1"].data_ptr(), t["d1"].data_ptr(), t["n1"].data_ptr()]
    kf2 = [t["i2"].data_ptr(), t["s2"].data_ptr(), t["f2"].data_ptr(), t["nn2"].data_ptr(), t["mp2"].data_ptr(), t["kp2"].data_ptr(), t["d2"].data_ptr(),
           t["n2"].data_ptr()]
    orbhip.match_and_triangulate_device(gpu_ctx, kf1, kf2, t["geom"].data_ptr(), t["poses"].data_ptr(), P, MNODE, MN, MN, cases[0]["sigma2_1"],
                                        cases[0]["sigma2"], check_ori, m12.data_ptr(), pts.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12h, nmh, ptsh = m12.cpu().numpy(), nm.cpu().numpy(), pts.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref, p_ref = om.search_for_triangulation_points(c, poses[p], check_ori)
        assert nmh[p] == n_ref, (p, nmh[p], n_ref)
        np.testing.assert_array_equal(m12h[p, :len(m_ref)], m_ref)
        np.testing.assert_array_equal(ptsh[p, :len(m_ref)].view(np.uint32), p_ref.view(np.uint32))
        tot += n_ref
        # the kept points are the scene's: in front of KF2's left camera and re-projecting onto the matched KF1 keypoint
        keep = np.flatnonzero(m_ref >= 0)
        if len(keep):
            T1 = poses[p]["Tcw1"].reshape(2, 3, 4).astype(np.float64)
            right1 = (c["geom"]["nleft1"] != -1) & (keep >= c["geom"]["nleft1"])
            X = p_ref[keep].astype(np.float64)
            Xc = np.einsum("kij,kj->ki", T1[right1.astype(int), :, :3], X) + T1[right1.astype(int), :, 3]
            assert (Xc[:, 2] > 0).all()
            cam = np.where(right1[:, None], c["geom"]["cam1"][1][None], c["geom"]["cam1"][0][None]).astype(np.float64)
            uv = np.stack([om.kb8_project_np((1, cam[i]), Xc[i]) for i in range(len(keep))])
            err2 = ((uv - np.stack([c["kp1"]["x"][keep], c["kp1"]["y"][keep]], 1)) ** 2).sum(1)
            assert (err2 <= 5.991 * c["sigma2_1"][c["kp1"]["octave"][keep]] * 1.001 + 1e-3).all()
    if mode == "pinhole":
        assert tot == 0
    else:
        assert tot > 300
    if mode == "rig" and not big:                             # all four camera pairs produced matches
        c = cases[4]; m = m12h[4, :len(c["kp1"])]; i1 = np.flatnonzero(m >= 0)
        combo = 2 * (i1 >= c["geom"]["nleft1"]) + (m[i1] >= c["geom"]["nleft2"])
        assert set(combo.tolist()) == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("mode,only_stereo,coarse,check_ori", [("pinhole", False, False, True), ("pinhole", True, False, False), ("kb8", False, False, True),
                                                                ("kb8", False, True, True), ("rig", False, False, True), ("rig", False, False, False),
                                                                ("rig", True, False, True)])
def test_search_for_triangulation_general_parity(gpu_ctx, mode, only_stereo, coarse, check_ori):
    """SearchForTriangulation for every camera combination (ORBmatcher.cc:969-1210): Pinhole and KannalaBrandt8 single cameras, two-fisheye
    rigs (NLeft != -1, the four relative poses, KannalaBrandt8::epipolarConstrain by triangulation) -- ragged keyframe pairs incl. empty
    sides, bit-exact vs the oracle; the Pinhole cases also against the fast-path kernel."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(1183)
    cases = [om.make_tri_general_case(rng, a, b, mode, nn, only_stereo, coarse)
             for a, b, nn in ((0, 20, 10), (30, 0, 10), (200, 260, 40), (1000, 950, 100), (2000, 2048, 300), (600, 1500, 900))]
    P, MN, MNODE = len(cases), 2048, 2048
    arr = dict(nid1=np.zeros((P, MN), np.int32), mp1=np.zeros((P, MN), np.uint8), kp1=np.zeros((P, MN), orbhip.KP_DTYPE),
               d1=np.zeros((P, MN, 32), np.uint8), ur1=np.full((P, MN), -1, np.float32), n1=np.zeros(P, np.int32),
               i2=np.zeros((P, MNODE), np.int32), s2=np.zeros((P, MNODE + 1), np.int32), f2=np.zeros((P, MN), np.int32), nn2=np.zeros(P, np.int32),
               mp2=np.zeros((P, MN), np.uint8), kp2=np.zeros((P, MN), orbhip.KP_DTYPE), d2=np.zeros((P, MN, 32), np.uint8),
               ur2=np.full((P, MN), -1, np.float32), n2=np.zeros(P, np.int32), geom=np.zeros(P, orbhip.TRI_GENERAL_DTYPE),
               fast=np.zeros(P, orbhip.TRI_PAIR_DTYPE))
    assert orbhip.TRI_GENERAL_DTYPE == om.TRI_GENERAL_DTYPE
    for p, c in enumerate(cases):
        a, b = len(c["kp1"]), len(c["kp2"])
        i2, s2, f2 = om.feature_vector_csr(c["nid2"])
        arr["nid1"][p, :a] = c["nid1"]; arr["mp1"][p, :a] = c["mp1"]; arr["kp1"][p, :a] = c["kp1"]; arr["d1"][p, :a] = c["d1"]
        arr["ur1"][p, :a] = c["ur1"]; arr["n1"][p] = a
        arr["i2"][p, :len(i2)] = i2; arr["s2"][p, :len(s2)] = s2; arr["f2"][p, :len(f2)] = f2; arr["nn2"][p] = len(i2)
        arr["mp2"][p, :b] = c["mp2"]; arr["kp2"][p, :b] = c["kp2"]; arr["d2"][p, :b] = c["d2"]; arr["ur2"][p, :b] = c["ur2"]; arr["n2"][p] = b
        arr["geom"][p] = c["geom"]
        arr["fast"][p] = (c["geom"]["F12"][0], c["geom"]["ep_x"], c["geom"]["ep_y"], int(only_stereo), int(coarse))
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in arr.items()}
    m12 = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kf1 = [t["nid1"].data_ptr(), t["mp1"].data_ptr(), t["kp1"].data_ptr(), t["d1"].data_ptr(), t["ur1"].data_ptr(), t["n1"].data_ptr()]
    kf2 = [t["i2"].data_ptr(), t["s2"].data_ptr(), t["f2"].data_ptr(), t["nn2"].data_ptr(), t["mp2"].data_ptr(), t["kp2"].data_ptr(), t["d2"].data_ptr(),
           t["ur2"].data_ptr(), t["n2"].data_ptr()]
    orbhip.search_for_triangulation_general_device(gpu_ctx, kf1, kf2, t["geom"].data_ptr(), P, MNODE, MN, MN, cases[0]["sigma2_1"], cases[0]["scale"],
                                                   cases[0]["sigma2"], check_ori, m12.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12h, nmh = m12.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = om.search_for_triangulation_general(c, check_ori)
        assert nmh[p] == n_ref, (p, nmh[p], n_ref)
        np.testing.assert_array_equal(m12h[p, :len(m_ref)], m_ref)
        tot += n_ref
    if mode == "rig" and only_stereo:
        assert tot == 0                                       # rig keyframes have no stereo keypoints (ORBmatcher.cc:1044-1048)
    else:
        assert tot > (100 if only_stereo else 300)
    if mode == "rig" and not only_stereo:                     # all four camera pairs produced matches
        c = cases[4]; m = m12h[4, :len(c["kp1"])]; i1 = np.flatnonzero(m >= 0)
        combo = 2 * (i1 >= c["geom"]["nleft1"]) + (m[i1] >= c["geom"]["nleft2"])
        assert set(combo.tolist()) == {0, 1, 2, 3}
    if mode == "pinhole":
        m12b = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nmb = torch.full((P,), -9, dtype=torch.int32, device="cuda")
        orbhip.search_for_triangulation_device(gpu_ctx, kf1, kf2, t["fast"].data_ptr(), P, MNODE, MN, MN, cases[0]["scale"], cases[0]["sigma2"], check_ori,
                                               m12b.data_ptr(), nmb.data_ptr())
        gpu_ctx.check_status()
        assert torch.equal(nm, nmb)
        for p, c in enumerate(cases):
            assert torch.equal(m12[p, :len(c["kp1"])], m12b[p, :len(c["kp1"])])


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,check_ori", [(0.75, True), (0.9, False)])
def test_search_by_bow_kf_parity(gpu_ctx, ratio, check_ori):
    """LoopClosing's KF-KF matcher (ORBmatcher.cc:827-967) on ragged pairs incl. empty sides, bit-exact vs the oracle."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(67)
    cases = [om.make_bow_case(rng, nk, nf, nn) for nk, nf, nn in ((0, 20, 10), (30, 0, 10), (200, 260, 40), (1000, 950, 100), (2048, 2000, 300), (600, 1500, 900))]
    for c in cases:
        c["valid2"] = (rng.random(len(c["kp_f"])) < 0.8).astype(np.uint8)
    P, MN, MNODE = len(cases), 2048, 2048
    arr = dict(ki=np.zeros((P, MNODE), np.int32), ks=np.zeros((P, MNODE + 1), np.int32), kf=np.zeros((P, MN), np.int32), kn=np.zeros(P, np.int32),
               fi=np.zeros((P, MNODE), np.int32), fs=np.zeros((P, MNODE + 1), np.int32), ff=np.zeros((P, MN), np.int32), fn=np.zeros(P, np.int32),
               va=np.zeros((P, MN), np.uint8), vb=np.zeros((P, MN), np.uint8), kpk=np.zeros((P, MN), orbhip.KP_DTYPE), kpf=np.zeros((P, MN), orbhip.KP_DTYPE),
               dk=np.zeros((P, MN, 32), np.uint8), df=np.zeros((P, MN, 32), np.uint8), n1=np.zeros(P, np.int32), n2=np.zeros(P, np.int32))
    for p, c in enumerate(cases):
        ki, ks, kf = om.feature_vector_csr(c["nid_k"]); fi, fs, ff = om.feature_vector_csr(c["nid_f"])
        arr["ki"][p, :len(ki)] = ki; arr["ks"][p, :len(ks)] = ks; arr["kf"][p, :len(kf)] = kf; arr["kn"][p] = len(ki)
        arr["fi"][p, :len(fi)] = fi; arr["fs"][p, :len(fs)] = fs; arr["ff"][p, :len(ff)] = ff; arr["fn"][p] = len(fi)
        nk, nf = len(c["kp_k"]), len(c["kp_f"])
        arr["va"][p, :nk] = c["valid"]; arr["vb"][p, :nf] = c["valid2"]; arr["kpk"][p, :nk] = c["kp_k"]; arr["kpf"][p, :nf] = c["kp_f"]
        arr["dk"][p, :nk] = c["d_k"]; arr["df"][p, :nf] = c["d_f"]; arr["n1"][p] = nk; arr["n2"][p] = nf
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype == orbhip.KP_DTYPE else v).cuda() for k, v in arr.items()}
    m12 = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_by_bow_kf_device(gpu_ctx, [t[k].data_ptr() for k in ("ki", "ks", "kf", "kn", "va", "kpk", "dk", "n1")],
                                   [t[k].data_ptr() for k in ("fi", "fs", "ff", "fn", "vb", "kpf", "df", "n2")], P, MNODE, MN, MN,
                                   ratio, check_ori, m12.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = om.search_by_bow_kf(c, ratio, check_ori)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        np.testing.assert_array_equal(m12[p, :len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 300


@pytest.mark.gpu
def test_sim3_searches_parity(gpu_ctx, sbp_form):
    """LoopClosing's Sim3 matchers through the existing kernels: SearchByProjection(KF, Scw, ...)
    (ORBmatcher.cc:477-708) = orbhip_search_by_projection_device with has_obs = 1, no uRight, no rotation check,
    th_high = floor(TH_LOW*ratioHamming); the per-point searches of SearchBySim3 (:1813-1851) and Fuse(KF, Scw) (:1687-1720) =
    orbhip_fuse_search_device with an all-zero inverse sigma table.  Bit-exact vs oracles restated from those reference lines."""
    import torch
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import _sim3_case
    rng = np.random.default_rng(71)
    bounds = (0.0, 0.0, 640.0, 480.0)
    cases = [_sim3_case(rng, n, nq) for n, nq in ((0, 10), (60, 0), (300, 500), (1000, 900), (2000, 2048))]
    P, MQ, MN = len(cases), 2048, 2048
    Q = np.zeros((P, MQ), orbhip.PROJ_QUERY_DTYPE); DQ = np.zeros((P, MQ, 32), np.uint8)
    KP = np.zeros((P, MN), orbhip.KP_DTYPE); D = np.zeros((P, MN, 32), np.uint8); TM = np.full((P, MN), -1, np.int32)
    nq = np.array([len(c[0]) for c in cases], np.int32); n = np.array([len(c[2]) for c in cases], np.int32)
    for p, (q, dq, kp, d, tm) in enumerate(cases):
        Q[p, :nq[p]] = q; DQ[p, :nq[p]] = dq; KP[p, :n[p]] = kp; D[p, :n[p]] = d; TM[p, :n[p]] = tm
    t = [torch.from_numpy(a.view(np.uint8) if a.dtype in (orbhip.KP_DTYPE, orbhip.PROJ_QUERY_DTYPE) else a).cuda() for a in (Q, DQ, nq, KP, D, n)]
    tot = 0
    for ratio in (1.0, 0.5):
        tm_d = torch.from_numpy(TM).cuda(); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        orbhip.search_by_projection_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), MQ, t[3].data_ptr(), t[4].data_ptr(), None,
                                           t[5].data_ptr(), MN, MN, P, bounds, int(np.floor(np.float32(50) * np.float32(ratio))), False,
                                           tm_d.data_ptr(), nm.data_ptr())
        gpu_ctx.check_status()
        got, nm = tm_d.cpu().numpy(), nm.cpu().numpy()
        for p, (q, dq, kp, d, tm) in enumerate(cases):
            n_ref, m_ref = om.search_by_projection_sim3(q, dq, kp, d, bounds, tm, ratio)
            assert nm[p] == n_ref
            np.testing.assert_array_equal(got[p, :n[p]], np.where(tm != -1, -2, m_ref))
            tot += n_ref
    assert tot > 300
    bi = torch.full((P, MQ), -9, dtype=torch.int32, device="cuda"); bd = torch.full((P, MQ), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.fuse_search_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), MQ, t[3].data_ptr(), t[4].data_ptr(), None, t[5].data_ptr(),
                              MN, MN, P, np.zeros(8, np.float32), bounds, bi.data_ptr(), bd.data_ptr())
    gpu_ctx.check_status()
    bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    for p, (q, dq, kp, d, tm) in enumerate(cases):
        ri, rd = om.window_best(q, dq, kp, d, bounds)
        np.testing.assert_array_equal(bi[p, :nq[p]], ri); np.testing.assert_array_equal(bd[p, :nq[p]], np.where(ri < 0, 256, rd))


@pytest.mark.gpu
def test_frame_glue_parity(gpu_ctx):
    """Frame::UndistortKeyPoints + Frame::AssignFeaturesToGrid on a ragged batch (incl. an empty frame): bit-exact vs the oracle."""
    import torch
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case, EUROC_K, EUROC_DIST
    rng = np.random.default_rng(91)
    ns = (0, 1, 300, 2500, 4096)
    F, MN = len(ns), 4096
    KP = np.zeros((F, MN), orbhip.KP_DTYPE)
    for f, n in enumerate(ns):
        KP[f, :n] = make_sbp_case(rng, n, 0, False)[2]
    d_kp = torch.from_numpy(KP.view(np.uint8)).cuda(); d_n = torch.tensor(ns, dtype=torch.int32, device="cuda")
    for dist in (EUROC_DIST, EUROC_DIST + (0.01,), (0.0, 0.1, 0.0, 0.0)):
        d_un = torch.zeros_like(d_kp)
        torch.cuda.synchronize()                  # torch's fill runs on torch's stream, the library on its own
        orbhip.undistort_keypoints_device(gpu_ctx, d_kp.data_ptr(), d_n.data_ptr(), F, MN, MN, EUROC_K, dist, d_un.data_ptr())
        gpu_ctx.synchronize()
        un = d_un.cpu().numpy().view(orbhip.KP_DTYPE).reshape(F, MN)
        for f, n in enumerate(ns):
            ref = om.undistort_keypoints(KP[f, :n], EUROC_K, dist)
            assert un[f, :n].tobytes() == ref.tobytes(), (f, dist)
    bounds = (-12.5, -9.0, 760.0, 490.0)
    cs = torch.full((F, 64 * 48 + 1), -9, dtype=torch.int32, device="cuda"); it = torch.full((F, MN), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.assign_features_to_grid_device(gpu_ctx, d_un.data_ptr(), d_n.data_ptr(), F, MN, MN, bounds, cs.data_ptr(), it.data_ptr())
    gpu_ctx.check_status()
    cs, it = cs.cpu().numpy(), it.cpu().numpy()
    for f, n in enumerate(ns):
        rcs, rit = om.assign_features_to_grid(un[f, :n], bounds)
        np.testing.assert_array_equal(cs[f], rcs)
        np.testing.assert_array_equal(it[f, :len(rit)], rit)


@pytest.mark.gpu
def test_windowed_matchers_random_sizes(gpu_ctx, sbp_form):
    """Randomised sizes (odd counts, one-off-capacity, tiny / empty sides) through the claim-rule matcher, the all-pairs matcher and
    the BoW matcher: bit-exact vs the oracle for every pair of 3 x 12 random cases."""
    import oracle_match_bind as om
    from test_oracle_match_ba import make_sbp_case
    rng = np.random.default_rng(2024)
    bounds = (0.0, 0.0, 640.0, 480.0)
    sizes = [0, 1, 2, 7, 63, 64, 65, 127, 511, 1000, 2047, 2048]
    for rep in range(3):
        ns = rng.permutation(sizes); nqs = rng.permutation(sizes)
        stereo = bool(rep & 1)
        cases = [make_sbp_case(rng, int(n), int(nq), stereo) for n, nq in zip(ns, nqs)]
        got = _sbp(gpu_ctx, cases, 2048, 2048, bounds, 100, True, stereo)
        for p, (q, dq, kp, d, ur, tm) in enumerate(cases):
            n_ref, tm_ref = om.search_by_projection(q, dq, kp, d, ur if stereo else None, bounds, tm, 100, True)
            assert got[p][0] == n_ref, (rep, p, ns[p], nqs[p])
            np.testing.assert_array_equal(got[p][1], tm_ref)
        # all-pairs 2-NN on the same descriptor sets
        da = [c[1] for c in cases]; db = [c[3] for c in cases]
        res = _bf(gpu_ctx, da, db, 2048, 0.7)
        for p in range(len(cases)):
            i2, d2, ac = om.bf2nn(da[p], db[p], 0.7)
            np.testing.assert_array_equal(res[p][0], i2); np.testing.assert_array_equal(res[p][1], d2); np.testing.assert_array_equal(res[p][2], ac)


@pytest.mark.gpu
def test_bow_vectors_parity(gpu_ctx):
    """mFeatVec / mBowVec assembly on the device: bit-exact vs the oracle (node / word order, feature order inside a node, f64 sums
    and the L1 normalisation), ragged frames incl. empty and all-stopped ones; the CSR it writes drives SearchByBoW unchanged."""
    import torch
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import _bow_inputs
    rng = np.random.default_rng(17)
    ns = (0, 1, 50, 700, 2048, 4096, 333)
    F, MN, MNODE = len(ns), 4096, 512
    WID = np.zeros((F, MN), np.int32); W = np.zeros((F, MN), np.float64); NID = np.zeros((F, MN), np.int32)
    cases = []
    for f, n in enumerate(ns):
        wid, w, nid = _bow_inputs(rng, n, n_words=900 if n > 1000 else 300, n_nodes=100 if n > 1000 else 40, stop_frac=1.0 if f == 6 else 0.1)
        WID[f, :n] = wid; W[f, :n] = w; NID[f, :n] = nid; cases.append((wid, w, nid))
    t = [torch.from_numpy(a).cuda() for a in (WID, W, NID, np.array(ns, np.int32))]
    ni = torch.full((F, MNODE), -9, dtype=torch.int32, device="cuda"); st = torch.full((F, MNODE + 1), -9, dtype=torch.int32, device="cuda")
    ft = torch.full((F, MN), -9, dtype=torch.int32, device="cuda"); nn = torch.full((F,), -9, dtype=torch.int32, device="cuda")
    bw = torch.full((F, MN), -9, dtype=torch.int32, device="cuda"); bv = torch.zeros((F, MN), dtype=torch.float64, device="cuda")
    nw = torch.full((F,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.bow_vectors_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), F, MN, MNODE, ni.data_ptr(), st.data_ptr(),
                              ft.data_ptr(), nn.data_ptr(), bw.data_ptr(), bv.data_ptr(), nw.data_ptr())
    gpu_ctx.check_status()
    ni, st, ft, nn, bw, bv, nw = (x.cpu().numpy() for x in (ni, st, ft, nn, bw, bv, nw))
    for f, (wid, w, nid) in enumerate(cases):
        r_ni, r_ns, r_ft, r_bw, r_bv = om.bow_vectors(wid, w, nid)
        assert nn[f] == len(r_ni) and nw[f] == len(r_bw), (f, nn[f], len(r_ni), nw[f], len(r_bw))
        np.testing.assert_array_equal(ni[f, :nn[f]], r_ni); np.testing.assert_array_equal(st[f, :nn[f] + 1], r_ns)
        np.testing.assert_array_equal(ft[f, :len(r_ft)], r_ft)
        np.testing.assert_array_equal(bw[f, :nw[f]], r_bw)
        assert bv[f, :nw[f]].tobytes() == r_bv.tobytes(), f
    assert nw[6] == 0 and nn[6] == 0


@pytest.mark.gpu
def test_bow_pipeline_stays_on_device(gpu_ctx):
    """ComputeBoW -> SearchByBoW without a host round trip: descriptors -> orbhip_bow_transform_device -> orbhip_bow_vectors_device ->
    orbhip_search_by_bow_device (the CSR buffers passed straight through); result == the oracle chain on the same inputs."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(31)
    voc = om.make_vocabulary(rng, 10, 4)
    P, MN, MNODE, L, LUP = 5, 1024, 1024, 4, 2
    n = np.array([0, 40, 900, 1024, 333, 777], np.int32)               # frames 0..P: pair p = (keyframe p, frame p+1)
    F = P + 1
    desc = np.zeros((F, MN, 32), np.uint8); kp = np.zeros((F, MN), orbhip.KP_DTYPE)
    base = voc["node_desc"][rng.integers(1, len(voc["node_desc"]), 1024)]
    for f in range(F):
        src = rng.integers(0, 1024, n[f])
        desc[f, :n[f]] = base[src] ^ (rng.integers(0, 256, (n[f], 32), dtype=np.uint8) & rng.integers(0, 256, (n[f], 32), dtype=np.uint8) & rng.integers(0, 256, (n[f], 32), dtype=np.uint8))
        kp[f, :n[f]]["angle"] = rng.uniform(0, 360, n[f]).astype(np.float32)
    valid = (rng.random((F, MN)) < 0.85).astype(np.uint8)
    dv = [torch.from_numpy(np.ascontiguousarray(voc[key])).cuda() for key in ("node_desc", "child_start", "child_ids", "node_word", "node_weight")]
    d_desc = torch.from_numpy(desc).cuda(); d_kp = torch.from_numpy(kp.view(np.uint8)).cuda(); d_n = torch.from_numpy(n).cuda(); d_valid = torch.from_numpy(valid).cuda()
    wid = torch.zeros((F, MN), dtype=torch.int32, device="cuda"); w = torch.zeros((F, MN), dtype=torch.float64, device="cuda"); nid = torch.zeros((F, MN), dtype=torch.int32, device="cuda")
    ni = torch.zeros((F, MNODE), dtype=torch.int32, device="cuda"); st = torch.zeros((F, MNODE + 1), dtype=torch.int32, device="cuda")
    ft = torch.zeros((F, MN), dtype=torch.int32, device="cuda"); nn = torch.zeros((F,), dtype=torch.int32, device="cuda")
    bw = torch.zeros((F, MN), dtype=torch.int32, device="cuda"); bv = torch.zeros((F, MN), dtype=torch.float64, device="cuda"); nw = torch.zeros((F,), dtype=torch.int32, device="cuda")
    mf = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.bow_transform_device(gpu_ctx, d_desc.data_ptr(), d_n.data_ptr(), F, MN, MN, [t.data_ptr() for t in dv], L, LUP, wid.data_ptr(), w.data_ptr(), nid.data_ptr())
    orbhip.bow_vectors_device(gpu_ctx, wid.data_ptr(), w.data_ptr(), nid.data_ptr(), d_n.data_ptr(), F, MN, MNODE, ni.data_ptr(), st.data_ptr(), ft.data_ptr(),
                              nn.data_ptr(), bw.data_ptr(), bv.data_ptr(), nw.data_ptr())
    # pair p: keyframe = frame p, frame = frame p+1 -> the "frame" side pointers start one row later
    orbhip.search_by_bow_device(gpu_ctx, [ni.data_ptr(), st.data_ptr(), ft.data_ptr(), nn.data_ptr(), d_valid.data_ptr(), d_kp.data_ptr(), d_desc.data_ptr()],
                                [ni.data_ptr() + 4 * MNODE, st.data_ptr() + 4 * (MNODE + 1), ft.data_ptr() + 4 * MN, nn.data_ptr() + 4,
                                 d_kp.data_ptr() + 28 * MN, d_desc.data_ptr() + 32 * MN], d_n.data_ptr() + 4, P, MNODE, MN, MN, 0.7, True, mf.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    mf, nm, h_nid = mf.cpu().numpy(), nm.cpu().numpy(), nid.cpu().numpy()
    tot = 0
    for p in range(P):
        nid_k = np.array([om.bow_transform(desc[p, i], voc, LUP)[2] for i in range(n[p])], np.int32)
        nid_f = np.array([om.bow_transform(desc[p + 1, i], voc, LUP)[2] for i in range(n[p + 1])], np.int32)
        np.testing.assert_array_equal(h_nid[p, :n[p]], nid_k)
        c = dict(kp_k=kp[p, :n[p]], d_k=desc[p, :n[p]], nid_k=nid_k, valid=valid[p, :n[p]], kp_f=kp[p + 1, :n[p + 1]], d_f=desc[p + 1, :n[p + 1]], nid_f=nid_f)
        n_ref, m_ref = om.search_by_bow(c, 0.7, True)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        np.testing.assert_array_equal(mf[p, :len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 30


@pytest.mark.gpu
def test_matchers_against_committed_fixture(gpu_ctx):
    """The claim-rule matcher (both modes) and the Fuse search against tests/golden/match_golden.npz -- no oracle involved."""
    import os
    from test_oracle_match_ba import _load_match_golden
    g, bounds = _load_match_golden()
    case = (g["sbp_q"], g["sbp_dq"], g["sbp_kp"], g["sbp_d"], g["sbp_ur"], g["sbp_tm"])
    got = _sbp(gpu_ctx, [case], 256, 256, bounds, 100, True, True)
    assert got[0][0] == int(g["sbp_n"]); np.testing.assert_array_equal(got[0][1], g["sbp_m"])
    got = _sbp(gpu_ctx, [case], 256, 256, bounds, 100, False, True, map_ratio=0.8)
    assert got[0][0] == int(g["map_n"]); np.testing.assert_array_equal(got[0][1], g["map_m"])


# ------------------------------------------------------------------ frames of a two-camera rig (Nleft != -1)
@pytest.mark.parametrize("mode", [0, 1])
def test_rig_search_by_projection_parity(gpu_ctx, mode):
    """SearchByProjection on stereo-fisheye frames (ORBmatcher.cc:2013-2016, 2089-2153 / 113-122, 136-214): left and right camera
    queries in the reference's order over mGrid / mGridRight, cross-camera mirroring of a match (mode 1), bit-exact vs the oracle."""
    import torch
    import orbhip
    import oracle_match_bind as om
    from test_oracle_match_ba import make_rig_case
    rng = np.random.default_rng(900 + mode)
    bounds = (0.0, 0.0, 512.0, 512.0)
    cases = [make_rig_case(rng, nl, nr, npts, mode) for nl, nr, npts in ((0, 30, 20), (50, 0, 40), (300, 280, 250), (1000, 1040, 900), (700, 500, 1100))]
    P, MN, MQ = len(cases), 2048, 2048
    aq = np.zeros((P, MQ), orbhip.PROJ_QUERY_DTYPE); adq = np.zeros((P, MQ, 32), np.uint8); anq = np.zeros(P, np.int32)
    akp = np.zeros((P, MN), orbhip.KP_DTYPE); ad = np.zeros((P, MN, 32), np.uint8); an = np.zeros(P, np.int32); anl = np.zeros(P, np.int32)
    ami = np.full((P, MN), -1, np.int32); atm = np.full((P, MN), -1, np.int32)
    for p, (q, dq, kp, d, mirror, tm) in enumerate(cases):
        aq[p, :len(q)] = q; adq[p, :len(q)] = dq; anq[p] = len(q)
        akp[p, :len(kp)] = kp; ad[p, :len(kp)] = d; an[p] = len(kp); ami[p, :len(kp)] = mirror; atm[p, :len(kp)] = tm
    for p, nl in enumerate((0, 50, 300, 1000, 700)):
        anl[p] = nl
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype in (orbhip.KP_DTYPE, orbhip.PROJ_QUERY_DTYPE) else v).cuda()
         for k, v in dict(q=aq, dq=adq, nq=anq, kp=akp, d=ad, n=an, nl=anl, mi=ami, tm=atm).items()}
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_by_projection_rig_device(gpu_ctx, mode, t["q"].data_ptr(), t["dq"].data_ptr(), t["nq"].data_ptr(), MQ, t["kp"].data_ptr(),
                                           t["d"].data_ptr(), t["n"].data_ptr(), t["nl"].data_ptr(), t["mi"].data_ptr() if mode == 1 else None, MN, MN, P,
                                           bounds, 100, 0.8, True, t["tm"].data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    got_tm, got_nm = t["tm"].cpu().numpy(), nm.cpu().numpy()
    tot = right = 0
    for p, (q, dq, kp, d, mirror, tm) in enumerate(cases):
        n_ref, tm_ref = om.search_by_projection_rig(mode, q, dq, kp, d, int(anl[p]), mirror if mode == 1 else None, bounds, tm, 100, 0.8, True)
        assert got_nm[p] == n_ref, (p, got_nm[p], n_ref)
        np.testing.assert_array_equal(got_tm[p, :len(kp)], tm_ref)
        tot += n_ref; right += int((tm_ref[int(anl[p]):] >= 0).sum())
    assert tot > 500 and right > 150


def test_rig_search_by_bow_parity(gpu_ctx):
    """SearchByBoW(KeyFrame, Frame) with F.Nleft != -1 (ORBmatcher.cc:338-359, 393-425), bit-exact vs the oracle."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(161)
    cases = [om.make_bow_case(rng, nk, nf, nn) for nk, nf, nn in ((30, 0, 10), (200, 260, 40), (1000, 950, 100), (2000, 2048, 300), (600, 1500, 900))]
    nlefts = [0, 130, 500, 1024, 1500]                          # the last frame has no right-camera features at all
    P, MN, MNODE = len(cases), 2048, 2048
    arr = dict(ki=np.zeros((P, MNODE), np.int32), ks=np.zeros((P, MNODE + 1), np.int32), kf=np.zeros((P, MN), np.int32), kn=np.zeros(P, np.int32),
               fi=np.zeros((P, MNODE), np.int32), fs=np.zeros((P, MNODE + 1), np.int32), ff=np.zeros((P, MN), np.int32), fn=np.zeros(P, np.int32),
               va=np.zeros((P, MN), np.uint8), kpk=np.zeros((P, MN), orbhip.KP_DTYPE), kpf=np.zeros((P, MN), orbhip.KP_DTYPE),
               dk=np.zeros((P, MN, 32), np.uint8), df=np.zeros((P, MN, 32), np.uint8), nF=np.zeros(P, np.int32), nl=np.array(nlefts, np.int32))
    for p, c in enumerate(cases):
        ki, ks, kf = om.feature_vector_csr(c["nid_k"]); fi, fs, ff = om.feature_vector_csr(c["nid_f"])
        arr["ki"][p, :len(ki)] = ki; arr["ks"][p, :len(ks)] = ks; arr["kf"][p, :len(kf)] = kf; arr["kn"][p] = len(ki)
        arr["fi"][p, :len(fi)] = fi; arr["fs"][p, :len(fs)] = fs; arr["ff"][p, :len(ff)] = ff; arr["fn"][p] = len(fi)
        nk, nf = len(c["kp_k"]), len(c["kp_f"])
        arr["va"][p, :nk] = c["valid"]; arr["kpk"][p, :nk] = c["kp_k"]; arr["kpf"][p, :nf] = c["kp_f"]
        arr["dk"][p, :nk] = c["d_k"]; arr["df"][p, :nf] = c["d_f"]; arr["nF"][p] = nf
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype == orbhip.KP_DTYPE else v).cuda() for k, v in arr.items()}
    mf = torch.full((P, MN), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_by_bow_rig_device(gpu_ctx, [t[k].data_ptr() for k in ("ki", "ks", "kf", "kn", "va", "kpk", "dk")],
                                    [t[k].data_ptr() for k in ("fi", "fs", "ff", "fn", "kpf", "df")], t["nF"].data_ptr(), t["nl"].data_ptr(), P, MNODE,
                                    MN, MN, 0.7, True, mf.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    mf, nm = mf.cpu().numpy(), nm.cpu().numpy()
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = om.search_by_bow_rig(c, nlefts[p], 0.7, True)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        np.testing.assert_array_equal(mf[p, :len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 300


def test_rig_assign_features_to_grid(gpu_ctx):
    """Frame::AssignFeaturesToGrid with Nleft != -1: mGrid from the left keypoints, mGridRight from the right ones with indices i - Nleft
    (Frame.cc:395-405) == the single-camera oracle on each half."""
    import torch
    import orbhip
    import oracle_match_bind as om
    rng = np.random.default_rng(5)
    bounds = (0.0, 0.0, 512.0, 512.0)
    F, MN = 3, 1500
    kps, ns, nls = np.zeros((F, MN), orbhip.KP_DTYPE), np.array([1500, 700, 40], np.int32), np.array([800, 700, 0], np.int32)
    for f in range(F):
        kps["x"][f, :ns[f]] = rng.uniform(-10, 530, ns[f]); kps["y"][f, :ns[f]] = rng.uniform(-10, 530, ns[f])
    d_kp = torch.from_numpy(kps.view(np.uint8)).cuda(); d_n = torch.from_numpy(ns).cuda(); d_nl = torch.from_numpy(nls).cuda()
    cs = torch.zeros((F, 2 * 3072 + 1), dtype=torch.int32, device="cuda"); it = torch.full((F, MN), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.assign_features_to_grid_rig_device(gpu_ctx, d_kp.data_ptr(), d_n.data_ptr(), d_nl.data_ptr(), F, MN, MN, bounds, cs.data_ptr(), it.data_ptr())
    gpu_ctx.check_status()
    cs, it = cs.cpu().numpy(), it.cpu().numpy()
    for f in range(F):
        csl, itl = om.assign_features_to_grid(kps[f, :nls[f]], bounds)
        csr, itr = om.assign_features_to_grid(kps[f, nls[f]:ns[f]], bounds)
        np.testing.assert_array_equal(cs[f, :3073], csl)
        np.testing.assert_array_equal(cs[f, 3072:], csr + csl[-1])
        np.testing.assert_array_equal(it[f, :csl[-1]], itl[:csl[-1]])
        np.testing.assert_array_equal(it[f, csl[-1]:csl[-1] + csr[-1]], itr[:csr[-1]])


@pytest.mark.gpu
def test_ctx_wait_for_orders_two_contexts(gpu_ctx):
    """orbhip_ctx_wait_for: stream order across two contexts without a host synchronisation.  The extraction runs on one context, the
    windowed matcher on another that waits for it, and the first context waits for the matcher before it extracts OTHER images into the
    same result arrays: the matcher must have seen the first extraction (same matches as the one-context run), many times over."""
    import torch
    import orbhip
    B, W, H = 16, 640, 480
    imgs = orbhip.synth_frames(W, H, 2 * B, seed=991, first=0)
    d = torch.from_numpy(imgs).cuda()
    ctx2 = orbhip.Context(0)
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7); ext.reserve(W, H, B)
    mk = ext.max_keypoints
    kp, desc, cnt, _ = ext.results_device(); ds = mk * 32
    prev = torch.zeros((B, mk, 2), dtype=torch.float32, device="cuda")
    m12 = torch.full((B, mk), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros((B,), dtype=torch.int32, device="cuda")

    def match(c):
        orbhip.prev_matched_init_device(c, kp, mk, B - 1, mk, prev.data_ptr())
        orbhip.search_for_initialization_device(c, kp, desc, cnt, kp + mk * 28, desc + ds, cnt + 4, B - 1, mk, mk, (0.0, 0.0, float(W), float(H)), 100, 0.9, True,
                                                prev.data_ptr(), m12.data_ptr(), nm.data_ptr())
    ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0)); match(gpu_ctx); gpu_ctx.synchronize()
    ref = m12.clone(); ref_n = nm.clone()
    assert int(ref_n.sum()) > 500
    for it in range(6):
        m12.fill_(-7); torch.cuda.synchronize()
        ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
        ctx2.wait_for(gpu_ctx)
        match(ctx2)
        gpu_ctx.wait_for(ctx2)
        ext.extract_device(d.data_ptr() + B * W * H, W, H, W, W * H, B, (0, 0))      # overwrites the arrays the matcher read
        gpu_ctx.synchronize()                                                        # (covers ctx2's work: this context waited for it)
        assert torch.equal(m12, ref) and torch.equal(nm, ref_n), it
    ext.close(); ctx2.close()


@pytest.mark.gpu
def test_two_matchers_side_by_side_equal_the_serial_step(gpu_ctx, monkeypatch):
    """bench.py's step since round 4: the 2-NN matcher on the extraction's context, SearchForInitialization (sequential form: small-LDS launch +
    flagged second launch) on a second context beside it, ordered by orbhip_ctx_wait_for both ways.  Every output of both matchers must equal
    the one-context step's, step after step."""
    import torch
    import orbhip
    monkeypatch.setenv("ORBHIP_SI_PARALLEL_MAX_PAIRS", "0")
    B, W, H = 48, 640, 480
    imgs = orbhip.synth_frames(W, H, B, seed=1234, first=0)
    d = torch.from_numpy(imgs).cuda()
    ctx2 = orbhip.Context(0)
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7); ext.reserve(W, H, B)
    mk = ext.max_keypoints
    kp, desc, cnt, _ = ext.results_device(); ds = mk * 32
    prev = torch.zeros((B, mk, 2), dtype=torch.float32, device="cuda")
    m12 = torch.full((B, mk), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
    idx2 = torch.full((B, mk, 2), -9, dtype=torch.int32, device="cuda"); dist2 = torch.full((B, mk, 2), -9, dtype=torch.int32, device="cuda")
    acc = torch.zeros((B, mk), dtype=torch.uint8, device="cuda")

    def windowed(c):
        orbhip.prev_matched_init_device(c, kp, mk, B - 1, mk, prev.data_ptr())
        orbhip.search_for_initialization_device(c, kp, desc, cnt, kp + mk * 28, desc + ds, cnt + 4, B - 1, mk, mk, (0.0, 0.0, float(W), float(H)), 100, 0.9, True,
                                                prev.data_ptr(), m12.data_ptr(), nm.data_ptr())

    def bf(c):
        orbhip.match_bf2nn_device(c, desc, cnt, ds, desc + ds, cnt + 4, ds, B - 1, mk, 0.7, idx2.data_ptr(), dist2.data_ptr(), acc.data_ptr())

    ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0)); bf(gpu_ctx); windowed(gpu_ctx); gpu_ctx.synchronize()
    gpu_ctx.check_status()
    ref = [t.clone() for t in (m12, nm, idx2, dist2, acc)]
    assert int(ref[1].sum()) > 1000 and int(ref[4].sum()) > 1000
    for it in range(4):
        for t, v in ((m12, -7), (idx2, -9), (dist2, -9)):
            t.fill_(v)
        nm.zero_(); acc.zero_(); torch.cuda.synchronize()
        for _ in range(3):                                       # three steps back to back, as the bench times them
            gpu_ctx.wait_for(ctx2)
            ext.extract_device(d.data_ptr(), W, H, W, W * H, B, (0, 0))
            ctx2.wait_for(gpu_ctx)
            windowed(ctx2)
            bf(gpu_ctx)
        gpu_ctx.synchronize(); ctx2.synchronize()
        gpu_ctx.check_status(); ctx2.check_status()
        for got, want in zip((m12, nm, idx2, dist2, acc), ref):
            assert torch.equal(got[:B - 1], want[:B - 1]), it
    ext.close(); ctx2.close()
