"""The candidate lists and images that the octree stage is run on, on the device (tests/test_gpu_octree_table.py, tests/test_gpu_octree_pipeline.py), with
what the oracle and the closed form say about each; tests/test_octree_table_model.py checks the premises (how many lists are legal, how many the
tables give up on, which levels of which image) on the CPU.  Everything is computed once per process."""
import functools

import numpy as np

import octree_table_model as M


def n_ini_of(W, H):
    return int(np.floor(np.float32(W) / np.float32(H) + 0.5))


def cell_order(c):
    """(the list order the kernels see: candidates sorted into the level's FAST cells, row-major, stable; the largest number of candidates in
    one cell; cell_cap = what non-maximum suppression can leave in a cell at most; number of cells)."""
    import oracle_bind
    ncols, nrows, wcell, hcell = oracle_bind.cell_grid(c["W"] + 32, c["H"] + 32)
    cell = np.minimum(c["ys"] // hcell, nrows - 1) * ncols + np.minimum(c["xs"] // wcell, ncols - 1)
    most = int(np.bincount(cell).max()) if len(cell) else 0
    return np.argsort(cell, kind="stable"), most, ((wcell + 1) // 2) * ((hcell + 1) // 2), ncols * nrows


def prepare(c, dmax, name=None):
    """The case in cell order with the oracle's kept keys (`want`, rows x, y, score) and whether tables down to `dmax` give up on it (`deep`);
    None for a list no FAST stage can produce (more candidates in a cell than cell_cap)."""
    import oracle_bind
    o, most, cap, _ = cell_order(c)
    if most > cap:
        return None
    W, H, N = c["W"], c["H"], c["N"]
    xs, ys, ss = c["xs"][o], c["ys"][o], c["ss"][o]
    keep = oracle_bind.octree(xs, ys, ss, 16, 16 + W, 16, 16 + H, N)
    deep = 1 if len(xs) and M.octree_table(xs, ys, ss, 16, 16 + W, 16, 16 + H, N, dmax=dmax) is None else 0
    return dict(W=W, H=H, N=N, xs=xs, ys=ys, ss=ss, name=name, deep=deep,
                want=np.stack([xs[keep], ys[keep], ss[keep]], 1).astype(np.int32).reshape(-1, 3))


# ------------------------------------------------------------------ the random lists of the CPU test, grouped by extractor
@functools.lru_cache(None)
def random_groups():
    """{(W, H, N): [prepared case, ...]} over the 240 random_case lists, and the number of lists left out as illegal."""
    groups, skipped = {}, 0
    for kind in range(3):
        for seed in range(80):
            c = M.random_case(kind, seed)
            p = prepare(c, M.table_depth(n_ini_of(c["W"], c["H"]), [c["N"]]), name="kind%d_seed%d" % (kind, seed))
            if p is None:
                skipped += 1
            else:
                groups.setdefault((c["W"], c["H"], c["N"]), []).append(p)
    return groups, skipped


def check_random_balance():
    """Both kernels are honestly exercised: few lists are left out, the tables give up on many and complete many more."""
    groups, skipped = random_groups()
    cases = [p for v in groups.values() for p in v]
    flagged = sum(p["deep"] for p in cases)
    assert len(groups) == 40 and len(cases) + skipped == 240 and all(1 <= len(v) <= 9 for v in groups.values())
    assert skipped <= 12, skipped
    assert flagged >= 30 and len(cases) - flagged >= 150, (flagged, len(cases))
    return len(cases), skipped, flagged


@functools.lru_cache(None)
def split_cases():
    """Lists around the 2048 keys a workgroup keeps in registers (OCT_KR * 256), at 608 x 448 with quota 400: exactly K distinct uniform keys, and one
    of 2049 whose last key in cell order -- the only one on the global-memory path -- is alone in its root quadrant."""
    W, H, N = 608, 448, 400
    dmax = M.table_depth(1, [N])
    out = []
    for K in (2047, 2048, 2049, 2305):
        rng = np.random.RandomState(4000 + K)
        pix = rng.permutation(W * H)[:K]
        c = dict(W=W, H=H, N=N, xs=(pix % W).astype(np.int32), ys=(pix // W).astype(np.int32), ss=rng.randint(7, 256, K).astype(np.int32))
        out.append(prepare(c, dmax, name="uniform_%d" % K))
    rng = np.random.RandomState(4999)
    pix = rng.permutation(W * H)
    x, y = pix % W, pix // W
    first = np.flatnonzero((x < W // 2) | (y < H // 2))[:2048]                   # nothing in the lower right quadrant of the one root ...
    c = dict(W=W, H=H, N=N, xs=np.append(x[first], 600).astype(np.int32), ys=np.append(y[first], 440).astype(np.int32),   # ... but one key, in the last cell
             ss=np.append(rng.randint(7, 256, 2048), 9).astype(np.int32))
    out.append(prepare(c, dmax, name="lone_key_2049"))
    assert all(p is not None for p in out)
    return out


def check_split_cases():
    cases = split_cases()
    assert [len(p["xs"]) for p in cases] == [2047, 2048, 2049, 2305, 2049]
    for p in cases:
        assert len(np.unique(p["ys"] * 4096 + p["xs"])) == len(p["xs"]) and (p["W"], p["H"], p["N"]) == (608, 448, 400)
    p = cases[-1]
    lone = (p["xs"] >= 304) & (p["ys"] >= 224)                                  # DivideNode: the root splits at ceil(608 / 2), ceil(448 / 2)
    assert lone.sum() == 1 and lone[2048]                                       # key 2048 is the first one past the registers
    assert (p["want"] == [p["xs"][2048], p["ys"][2048], p["ss"][2048]]).all(1).sum() == 1


# ------------------------------------------------------------------ an 8-level extractor, 40 frames, flagged lists in chosen places
REDO_LEVELS = (0, 3, 7)
REDO_FRAMES = 40
# frames of the flagged lists: adjacent ones and distant ones, and 7 | 8 is where level 3 (lists 120 .. 159 of 8 * 40) crosses a multiple of 64: the
# boundary between the second and the third workgroup of k_octree_redo
REDO_FLAGGED_AT = (0, 1, 6, 7, 8, 9, 19, 30, 38, 39)


def pyramid_dims(w, h, nlevels=8, nfeatures=1000, scale=1.2):
    """[(width, height)] of the levels and the per-level quotas, from the oracle's tables (ORBextractor.cc:1152-1160: cvRound of size * inverse scale)."""
    import oracle_bind
    t = oracle_bind.OracleExtractor(nfeatures, scale, nlevels, 20, 7).tables()
    dims = [(int(np.rint(np.float32(w) * s)), int(np.rint(np.float32(h) * s))) for s in t["inv_scale"]]
    return dims, [int(q) for q in t["per_level"]]


@functools.lru_cache(None)
def redo_lists(level):
    """40 prepared lists for `level` of the 640 x 480, 1000-feature, 8-level extractor: all three kinds, the flagged ones at REDO_FLAGGED_AT and nowhere else."""
    dims, quotas = pyramid_dims(640, 480)
    W, H = dims[level][0] - 32, dims[level][1] - 32
    dmax = M.table_depth(max(n_ini_of(w - 32, h - 32) for w, h in dims), quotas)
    pools = {0: [], 1: []}
    need = {1: len(REDO_FLAGGED_AT), 0: REDO_FRAMES - len(REDO_FLAGGED_AT)}
    kinds = {0: set(), 1: set()}
    for seed in range(400):                                   # redraw until both pools are full (illegal lists are passed over)
        if all(len(pools[k]) >= need[k] for k in (0, 1)):
            break
        kind = seed % 3
        p = prepare(M.random_case(kind, 100 + seed, geometry=(W, H), quota=quotas[level]), dmax, name="L%d_kind%d_seed%d" % (level, kind, 100 + seed))
        if p is not None and len(pools[p["deep"]]) < need[p["deep"]]:
            pools[p["deep"]].append(p)
            kinds[p["deep"]].add(kind)
    assert all(len(pools[k]) == need[k] for k in (0, 1)), (level, len(pools[0]), len(pools[1]))
    assert len(kinds[0] | kinds[1]) == 3
    it = {k: iter(pools[k]) for k in (0, 1)}
    return [next(it[1 if f in REDO_FLAGGED_AT else 0]) for f in range(REDO_FRAMES)], dmax


def check_redo_lists(level):
    cases, dmax = redo_lists(level)
    flagged = [f for f, p in enumerate(cases) if p["deep"]]
    assert len(cases) == REDO_FRAMES and flagged == list(REDO_FLAGGED_AT)
    assert len(flagged) >= 8 and REDO_FRAMES - len(flagged) >= 8
    gaps = np.diff(flagged)
    assert (gaps == 1).any() and (gaps >= 8).any()                              # adjacent frames and distant ones
    w = [level * REDO_FRAMES + f for f in flagged]                              # list numbers as k_octree_redo counts them
    assert max(np.bincount(np.asarray(w) // 64)) >= 2                           # several in one workgroup, one after the other
    if level == 3:
        assert {v // 64 for v in w} == {1, 2} and 127 in w and 128 in w
    assert all(max(p["xs"], default=0) < p["W"] and max(p["ys"], default=0) < p["H"] for p in cases)
    return flagged


# the second path of oct_gather (per-cell copy loops): more cells than 16 * NC LDS words hold offsets for -- a small quota on a large image
GATHER_SHAPE = dict(nfeatures=50, nlevels=2, w=1200, h=900)


@functools.lru_cache(None)
def gather_lists(level):
    """Uniform and tight-block lists for a level of the GATHER_SHAPE extractor, with the premise of the second gather path."""
    g = GATHER_SHAPE
    dims, quotas = pyramid_dims(g["w"], g["h"], g["nlevels"], g["nfeatures"])
    W, H = dims[level][0] - 32, dims[level][1] - 32
    n_ini = max(n_ini_of(w - 32, h - 32) for w, h in dims)
    dmax = M.table_depth(n_ini, quotas)
    nc = max(max(q + 16, 4 * n_ini + 4) for q in quotas)
    out = []
    for kind, seed in ((0, 3), (0, 4), (0, 7), (2, 2), (2, 5), (2, 6), (2, 10), (0, 12)):
        p = prepare(M.random_case(kind, seed, geometry=(W, H), quota=quotas[level]), dmax, name="gather_kind%d_seed%d" % (kind, seed))
        if p is not None:
            out.append(p)
    # a tight block among a few scattered keys: every pass splits off little, the tree outgrows the tables before it reaches the small quota
    for seed in range(200):
        rng = np.random.RandomState(7000 + 10 * level + seed)
        pick = np.sort(rng.permutation(400)[:200])
        bx, by = rng.randint(0, W - 20), rng.randint(0, H - 20)
        x = np.concatenate([rng.randint(0, W, 5), bx + pick % 20]); y = np.concatenate([rng.randint(0, H, 5), by + pick // 20])
        _, first = np.unique(y * 4096 + x, return_index=True); first.sort()
        c = dict(W=W, H=H, N=quotas[level], xs=x[first].astype(np.int32), ys=y[first].astype(np.int32), ss=rng.randint(7, 256, len(first)).astype(np.int32))
        p = prepare(c, dmax, name="gather_block_deep_seed%d" % seed)
        if p is not None and p["deep"]:
            out.insert(3, p)
            if sum(q["deep"] for q in out) == 2:
                break
    ncells = cell_order(out[0])[3]
    return out, dmax, ncells, nc


def check_gather_lists(level):
    cases, dmax, ncells, nc = gather_lists(level)
    assert ncells + 1 > 16 * nc, (ncells, nc)
    assert sum(p["deep"] for p in cases) == 2 and sum(1 - p["deep"] for p in cases) >= 4
    assert max(len(p["xs"]) for p in cases) > 2048
    assert sum(p["name"].startswith("gather_kind0") for p in cases) >= 3 and sum(p["name"].startswith("gather_kind2") for p in cases) >= 3


# ------------------------------------------------------------------ images whose levels the tables give up on
PIPE_FRAMES = 24
PIPE_CONSTRUCTED = {                                      # frame -> blocks of M.block_image
    0: (11, [(100, 140, 100, 140, 4), (300, 420, 400, 560, 4)]),
    7: (12, [(0, 480, 0, 640, 4)]),
    8: (13, [(0, 480, 0, 640, 8), (200, 240, 300, 340, 2)]),
    23: (14, [(60, 100, 500, 540, 4), (250, 400, 80, 260, 4)]),
}
PIPE_ORDINARY = (3, 16)


def pipeline_images(synth_frames):
    """24 VGA frames: synthetic scenes with the constructed images at frames 0, 7, 8 and 23."""
    imgs = synth_frames(640, 480, PIPE_FRAMES, seed=2718).copy()
    for f, (seed, blocks) in PIPE_CONSTRUCTED.items():
        imgs[f] = M.block_image(640, 480, seed, blocks)
    return imgs


def flagged_levels(img, nfeatures=1000, nlevels=8):
    """Levels of `img` whose candidate list (the oracle's) the tables of the extractor's depth give up on; the closed form at full depth must equal
    the oracle on every level.  Returns (set of levels, n_ini per level)."""
    import oracle_bind
    ora = oracle_bind.OracleExtractor(nfeatures, 1.2, nlevels, 20, 7)
    ora.extract(img)
    dims, quotas = pyramid_dims(img.shape[1], img.shape[0], nlevels, nfeatures)
    n_inis = [n_ini_of(w - 32, h - 32) for w, h in dims]
    dmax = M.table_depth(max(n_inis), quotas)
    deep = set()
    for l, (w, h) in enumerate(dims):
        xs, ys, ss = ora.fast_candidates(l)
        full = M.octree_table(xs, ys, ss, 16, w - 16, 16, h - 16, quotas[l])
        assert np.array_equal(full, oracle_bind.octree(xs, ys, ss, 16, w - 16, 16, h - 16, quotas[l])), l
        if len(xs) and M.octree_table(xs, ys, ss, 16, w - 16, 16, h - 16, quotas[l], dmax=dmax) is None:
            deep.add(l)
    return deep, n_inis


def wide_pair(synth_frames):
    """Two 700 x 480 frames, a synthetic scene and a constructed one: nIni is 1 on the large levels and 2 on the small ones."""
    imgs = synth_frames(700, 480, 2, seed=3141).copy()
    imgs[1] = M.block_image(700, 480, 15, [(120, 160, 90, 130, 4), (260, 400, 380, 600, 4)])
    return imgs
