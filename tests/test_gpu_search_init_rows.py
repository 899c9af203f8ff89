"""SearchForInitialization, rows form (k_si_rows + k_si_chain) against the register loops of k_search_init and the CPU oracle.

Every case runs three times -- ORBHIP_SI_ROWS=1, ORBHIP_SI_ROWS=0 (both with ORBHIP_SI_PARALLEL_MAX_PAIRS=0: the sequential path)
and oracle_match_bind.search_for_initialization -- and demands equal nmatches, equal m12 and byte-equal prev among all three.
The inputs are crafted keypoint / descriptor arrays: octave-0 points are the only ones that take part, the others are mixed in so
that an index inside the octave-0 subset is never the index inside the frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _flip(d, rng, k):
    """d with k distinct bits inverted: a descriptor at Hamming distance k."""
    u = np.unpackbits(np.asarray(d, np.uint8))
    u[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(u)


def _frame(rng, xy0, desc0, n_other):
    """A frame whose octave-0 keypoints are xy0 / desc0 in this order, with n_other keypoints of octaves 1..7 at random places
    between them (at least one in front when there are any: subset index != frame index)."""
    import orbhip
    n0 = len(xy0)
    n = n0 + n_other
    kp = np.zeros(n, orbhip.KP_DTYPE)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    is0 = np.zeros(n, bool)
    if n0:
        lo = 1 if n_other else 0
        is0[lo + np.sort(rng.choice(n - lo, n0, replace=False))] = True
    kp["x"] = rng.uniform(0, 640, n).astype(np.float32)
    kp["y"] = rng.uniform(0, 480, n).astype(np.float32)
    kp["octave"] = rng.integers(1, 8, n)
    kp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    if n0:
        kp["x"][is0] = np.asarray(xy0, np.float32)[:, 0]
        kp["y"][is0] = np.asarray(xy0, np.float32)[:, 1]
        kp["octave"][is0] = 0
        kp["angle"][is0] = rng.uniform(0, 20, n0).astype(np.float32)     # rotations in four histogram bins: the check drops some, not most
        desc[is0] = desc0
    return kp, desc, np.flatnonzero(is0)


def _device_run(gpu_ctx, fa, fb, prevs, max_n, window, ratio, check_ori):
    import torch
    import orbhip
    P = len(fa)
    kpA = np.zeros((P, max_n), orbhip.KP_DTYPE); kpB = np.zeros((P, max_n), orbhip.KP_DTYPE)
    dA = np.zeros((P, max_n, 32), np.uint8); dB = np.zeros((P, max_n, 32), np.uint8)
    nA = np.array([len(f[0]) for f in fa], np.int32); nB = np.array([len(f[0]) for f in fb], np.int32)
    prev = np.zeros((P, max_n, 2), np.float32)
    for p in range(P):
        kpA[p, :nA[p]] = fa[p][0]; dA[p, :nA[p]] = fa[p][1]
        kpB[p, :nB[p]] = fb[p][0]; dB[p, :nB[p]] = fb[p][1]
        prev[p, :nA[p]] = prevs[p]
    t = [torch.from_numpy(a.view(np.uint8) if a.dtype == orbhip.KP_DTYPE else a).cuda() for a in (kpA, dA, nA, kpB, dB, nB, prev)]
    m12 = torch.full((P, max_n), -9, dtype=torch.int32, device="cuda")
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.search_for_initialization_device(gpu_ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                            t[4].data_ptr(), t[5].data_ptr(), P, max_n, max_n, BOUNDS, window, ratio,
                                            check_ori, t[6].data_ptr(), m12.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    m12 = m12.cpu().numpy(); nm = nm.cpu().numpy(); pv = t[6].cpu().numpy()
    return [(int(nm[p]), m12[p, :nA[p]], pv[p, :nA[p]]) for p in range(P)]


def _three_way(gpu_ctx, monkeypatch, fa, fb, prevs, max_n, window=100, ratio=0.9, check_ori=True):
    """Rows form, register loops and oracle on the same pairs; returns the oracle's (nmatches, m12, prev) per pair."""
    import oracle_match_bind as om
    monkeypatch.setenv("ORBHIP_SI_PARALLEL_MAX_PAIRS", "0")
    monkeypatch.delenv("ORBHIP_SI_SMALL_CAP0", raising=False)
    got = {}
    for rows in ("1", "0"):
        monkeypatch.setenv("ORBHIP_SI_ROWS", rows)
        got[rows] = _device_run(gpu_ctx, fa, fb, prevs, max_n, window, ratio, check_ori)
    out = []
    for p in range(len(fa)):
        n, m12, prev = om.search_for_initialization(fa[p][0], fa[p][1], fb[p][0], fb[p][1], BOUNDS, prevs[p], window, ratio, check_ori)
        for rows in ("1", "0"):
            g = got[rows][p]
            assert g[0] == n, ("nmatches", "ORBHIP_SI_ROWS=" + rows, p, g[0], n)
            np.testing.assert_array_equal(g[1], m12, err_msg="m12, ORBHIP_SI_ROWS=%s, pair %d" % (rows, p))
            assert g[2].tobytes() == np.asarray(prev, np.float32).tobytes(), ("prev", "ORBHIP_SI_ROWS=" + rows, p)
        out.append((n, m12, prev))
    return out


def _related_pair(rng, na0, nb0, other_a, other_b):
    """F2's octave-0 points are moved, bit-flipped copies of random F1 octave-0 points (several per F1 point: contested), so
    matches, displacements and skips all happen; the windows are centred on the F1 keypoints."""
    xa = np.stack([rng.uniform(5, 635, na0), rng.uniform(5, 475, na0)], 1).astype(np.float32)
    da = rng.integers(0, 256, (na0, 32), dtype=np.uint8)
    if na0 and nb0:
        src = rng.integers(0, na0, nb0)
        xb = (xa[src] + rng.normal(0, 12, (nb0, 2))).astype(np.float32)
        db = np.stack([_flip(da[s], rng, int(k)) for s, k in zip(src, rng.integers(0, 60, nb0))])
    else:
        xb = np.stack([rng.uniform(5, 635, nb0), rng.uniform(5, 475, nb0)], 1).astype(np.float32)
        db = rng.integers(0, 256, (nb0, 32), dtype=np.uint8)
    a = _frame(rng, xa, da, other_a)
    b = _frame(rng, xb, db, other_b)
    return a[:2], b[:2], np.stack([a[0]["x"], a[0]["y"]], 1)


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]       # every boundary of the 64-lane x 4- / 8-slot layout; 513 falls back


@pytest.mark.parametrize("side", ["f1", "f2", "both"])
def test_rows_subset_sizes(gpu_ctx, monkeypatch, side):
    rng = np.random.default_rng({"f1": 11, "f2": 12, "both": 13}[side])
    fa, fb, prevs = [], [], []
    for c in SIZES:
        na0, nb0 = {"f1": (c, 300), "f2": (300, c), "both": (c, c)}[side]
        a, b, pv = _related_pair(rng, na0, nb0, 40 + int(rng.integers(0, 50)), 40 + int(rng.integers(0, 50)))
        fa.append(a); fb.append(b); prevs.append(pv)
    res = _three_way(gpu_ctx, monkeypatch, fa, fb, prevs, 640)
    assert sum(r[0] for r in res) > 50                          # the cases really match


@pytest.mark.parametrize("ratio", [0.9, 1.5])
def test_rows_visiting_order(gpu_ctx, monkeypatch, ratio):
    """Identical descriptors on several F2 points of one window: every distance ties, and the first point in GetFeaturesInArea's
    order (cell column, cell row, index inside the cell) is the best.  With nn_ratio <= 1 a tie of best and second best is rejected
    whatever the order; nn_ratio = 1.5 accepts it, and m12 then names the point that was visited first."""
    rng = np.random.default_rng(int(ratio * 10))
    r = 100.0
    xa, da, xb, db = [], [], [], []
    # (dx, dy) sets around the window centre; cells are 10 x 10 pixels
    patterns = [
        [(-35, 22), (41, -17), (3, 58), (-62, -49), (77, 9)],                       # different cells of one window
        [(12.0, 12.0), (13.5, 14.0), (11.0, 15.5), (14.5, 11.5)],                  # one cell: index order decides
        [(-99.5, 0), (99.5, 0), (0, -99.5), (0, 99.5)],                            # first / last cell column and row of the window
        [(-99.5, -99.5), (99.5, 99.5), (-99.5, 99.5), (99.5, -99.5), (0, 0)],      # its four corner cells and the centre
        [(-45, 30), (-45, 31), (-45, -52), (-44, -52), (60, 31)],                  # same column, rows apart; same cell twice
    ]
    centres = [(120 + 200 * (i % 3), 120 + 240 * (i // 3)) for i in range(6)]      # windows 200 apart in x: planted points do not mix
    for q, (cx, cy) in enumerate(centres):
        pat = patterns[q % len(patterns)]
        qd = rng.integers(0, 256, 32, dtype=np.uint8)
        xa.append((cx, cy)); da.append(qd)
        twin = _flip(qd, rng, 3 + q)
        order = rng.permutation(len(pat))                                           # frame order unrelated to the cell order
        for k in order:
            xb.append((cx + pat[k][0], cy + pat[k][1])); db.append(twin)
    for q in (6, 7):                                                                # windows clamped at the image border: c0 / r0 = 0, c1 / r1 = last
        cx, cy = (30.0, 40.0) if q == 6 else (615.0, 450.0)
        qd = rng.integers(0, 256, 32, dtype=np.uint8)
        xa.append((cx, cy)); da.append(qd)
        twin = _flip(qd, rng, 5)
        for dx, dy in rng.permutation([(-25, -35), (20, 25), (-28, 27), (22, -38), (5, 5), (6, 6)]):
            xb.append((cx + dx, cy + dy)); db.append(twin)
    a = _frame(rng, np.array(xa), np.array(da), 30)
    b = _frame(rng, np.array(xb), np.array(db), 45)
    pv = np.stack([a[0]["x"], a[0]["y"]], 1)
    res = _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 256, window=int(r), ratio=ratio, check_ori=False)
    assert res[0][0] == (len(xa) if ratio > 1 else 0)


def test_rows_contested_points(gpu_ctx, monkeypatch):
    """Many F1 points want one F2 point: with decreasing distances every one displaces the last (m12[old] = -1), with equal and
    increasing distances the later ones are skipped (vMatchedDistance <= dist) and fall to their second candidate or to nothing."""
    rng = np.random.default_rng(7)
    xa, da, xb, db = [], [], [], []
    for g, dists in enumerate([[40, 33, 27, 20, 12, 5, 0], [18] * 6, [2, 9, 17, 26, 38, 50], [30, 10, 30, 10, 5, 5, 45, 1]]):
        cx, cy = 100 + 140 * g, 200.0
        target = rng.integers(0, 256, 32, dtype=np.uint8)
        xb.append((cx, cy)); db.append(target)
        xb.append((cx + 8, cy - 6)); db.append(_flip(target, rng, 90))             # a poor second candidate in every window
        for k, d in enumerate(dists):
            xa.append((cx + rng.uniform(-15, 15), cy + rng.uniform(-15, 15))); da.append(_flip(target, rng, d))
    a = _frame(rng, np.array(xa), np.array(da), 25)
    b = _frame(rng, np.array(xb), np.array(db), 25)
    pv = np.stack([a[0]["x"], a[0]["y"]], 1)
    for ratio in (0.9, 0.6):
        _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 128, window=40, ratio=ratio, check_ori=True)
        res = _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 128, window=40, ratio=ratio, check_ori=False)
        assert 1 <= res[0][0] <= 8                                                  # at most one per target and one per poor second


@pytest.mark.parametrize("window", [1, 100, 400])
def test_rows_windows(gpu_ctx, monkeypatch, window):
    """Window centres within r of each border (clamped cell ranges), far off-image (empty rows), F2 points at exactly |dx| == r
    and |dy| == r (strict <), and one step inside."""
    rng = np.random.default_rng(100 + window)
    r = float(window)
    xa, da, xb, db, centres = [], [], [], [], []

    def query(kx, ky, px, py, pts):
        """An F1 keypoint at (kx, ky) whose window centre (prev) is (px, py), and F2 points at the given places with near-copies."""
        qd = rng.integers(0, 256, 32, dtype=np.uint8)
        xa.append((kx, ky)); da.append(qd); centres.append((px, py))
        for k, (x, y) in enumerate(pts):
            xb.append((x, y)); db.append(_flip(qd, rng, 4 + 30 * k))

    h = np.float32(0.5) if window > 1 else np.float32(0.25)
    for (px, py) in [(2.0, 2.0), (638.0, 3.0), (1.5, 477.0), (637.0, 478.5), (320.0, 1.0), (0.5, 240.0), (639.0, 240.0), (320.0, 479.0)]:
        query(px, py, px, py, [(min(max(px + h, 0.5), 639.0), min(max(py - h, 0.5), 479.0)), (min(px + r - h, 639.0), min(py + r - h, 479.0))])
    for (px, py) in [(-5000.0, 240.0), (320.0, 9000.0), (1e7, -1e7), (640.0 + r + 40, 240.0), (320.0, -r - 40.0), (-r - 11.0, -r - 11.0)]:
        query(300.0, 200.0, px, py, [(300.0, 200.0)])                               # windows that touch no cell, or no point
    for s in (-1.0, 1.0):                                                           # exactly on the window's edge, and just inside
        query(200.0, 100.0 + 40 * s, 200.0, 100.0 + 40 * s, [(200.0 + s * r, 100.0 + 40 * s), (200.0, 100.0 + 40 * s)])
        query(420.0, 300.0 + 40 * s, 420.0, 300.0 + 40 * s, [(420.0, 300.0 + 40 * s + s * r), (420.0 + s * (r - h), 300.0 + 40 * s)])
        query(300.0 + 40 * s, 400.0, 300.0 + 40 * s, 400.0, [(300.0 + 40 * s + s * (r - h), 400.0 - s * (r - h))])
    a = _frame(rng, np.array(xa), np.array(da), 20)
    b = _frame(rng, np.array(xb), np.array(db), 60)
    pv = np.zeros((len(a[0]), 2), np.float32)
    pv[:] = rng.uniform(0, 640, pv.shape)
    pv[a[2]] = np.asarray(centres, np.float32)
    _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 192, window=window, ratio=0.9, check_ori=True)
    res = _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 192, window=window, ratio=0.9, check_ori=False)
    assert res[0][0] >= 4


@pytest.mark.parametrize("ratio", [0.1, 0.6, 0.9])
def test_rows_distances(gpu_ctx, monkeypatch, ratio):
    """Exact copies (0), complements (256), best at 50 / 51 around TH_LOW, and a second best just either side of best / ratio --
    also where that lies above 255, which a byte per distance could not tell from 255."""
    rng = np.random.default_rng(int(ratio * 100))
    xa, da, xb, db = [], [], [], []
    cases = [(0, 256), (0, 0), (0, 1), (50, 256), (51, 256), (50, 140), (51, 140), (256, 256), (1, 256), (49, 50)]
    for best in (1, 5, 20, 25, 26, 30, 45, 50):
        edge = int(np.ceil(best / ratio))
        for d2 in (edge - 1, edge, edge + 1, edge + 2):
            if best <= d2 <= 256:
                cases.append((best, d2))
    for q, (d1, d2) in enumerate(cases):
        cx, cy = 25.0 + 45 * (q % 14), 25.0 + 45 * (q // 14)                        # windows of 12 around centres 45 apart: two candidates each
        qd = rng.integers(0, 256, 32, dtype=np.uint8)
        xa.append((cx, cy)); da.append(qd)
        pts = [((cx + 4, cy - 3), _flip(qd, rng, d1)), ((cx - 5, cy + 2), _flip(qd, rng, d2))]
        for k in rng.permutation(2):
            xb.append(pts[k][0]); db.append(pts[k][1])
    assert 25.0 + 45 * ((len(cases) - 1) // 14) < 470
    a = _frame(rng, np.array(xa), np.array(da), 33)
    b = _frame(rng, np.array(xb), np.array(db), 33)
    pv = np.stack([a[0]["x"], a[0]["y"]], 1)
    _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 256, window=12, ratio=ratio, check_ori=True)
    res = _three_way(gpu_ctx, monkeypatch, [a[:2]], [b[:2]], [pv], 256, window=12, ratio=ratio, check_ori=False)
    assert 2 <= res[0][0] < len(cases)


@pytest.mark.parametrize("check_ori", [True, False])
def test_rows_mixed_pairs_in_one_call(gpu_ctx, monkeypatch, check_ori):
    """Pairs of every tier side by side: the 4-slot and 8-slot chains, pairs that fall back to k_search_init (more than 512
    octave-0 points in F1, in F2, in both) and empty ones."""
    rng = np.random.default_rng(40 + int(check_ori))
    fa, fb, prevs = [], [], []
    for na0, nb0 in [(200, 220), (530, 100), (300, 300), (100, 600), (0, 50), (256, 257), (700, 700), (64, 512), (50, 0), (512, 64)]:
        a, b, pv = _related_pair(rng, na0, nb0, 20 + int(rng.integers(0, 60)), 20 + int(rng.integers(0, 60)))
        fa.append(a); fb.append(b); prevs.append(pv)
    res = _three_way(gpu_ctx, monkeypatch, fa, fb, prevs, 800, check_ori=check_ori)
    assert sum(r[0] for r in res) > 50
    res = _three_way(gpu_ctx, monkeypatch, fa[:3], fb[:3], prevs[:3], 800, window=30, ratio=0.6, check_ori=check_ori)
    assert sum(r[0] for r in res) > 0
