"""GPU: the table form of the octree (k_octree_tab, with k_octree_redo behind it) against the oracle and against the iterative form, through
the octree-only test entry: kept keys and their order, bit for bit.  Cases: tests/octree_table_model.py (checked against the oracle on the CPU
by tests/test_octree_table_model.py) and tests/octree_device_cases.py (the random lists of the CPU test, lists around the register / global-memory
split, an 8-level extractor with 40 frames and the flagged lists in chosen places, the second path of oct_gather)."""
import numpy as np
import pytest

import octree_device_cases as D
import octree_table_model as M

pytestmark = pytest.mark.gpu

# (W, H, quota, cases of one launch): one level geometry and 2 to 4 frames per batch
BATCHES = [
    (300, 300, 20, ["empty", "one_key", "two_keys_last_table", "quirk_one_quadrant"]),
    (300, 300, 20, ["two_keys_deep", "one_key"]),
    (300, 300, 4, ["equal_scores", "one_key"]),
    (500, 250, 40, ["empty_root_nini2", "one_key"]),
    (600, 200, 60, ["empty_root_nini3", "one_key"]),
    (640, 160, 60, ["empty_root_nini4", "one_key", "empty"]),
    (300, 300, 16, ["quota_exact_full_pass", "empty"]),
    (300, 300, 40, ["quota_mid_final", "one_key"]),
    (300, 300, 30, ["final_tie", "one_key"]),
    (300, 300, 12, ["final_two_iterations", "one_key"]),
    (608, 448, 400, ["tight_block_deep", "many_keys", "uniform_900"]),
]


@pytest.fixture(scope="module")
def cases():
    c = M.hand_cases()
    rng = np.random.RandomState(3)
    x, y = rng.randint(0, 608, 900), rng.randint(0, 448, 900)
    _, first = np.unique(y * 4096 + x, return_index=True); first.sort()
    c["uniform_900"] = dict(W=608, H=448, N=400, xs=x[first].astype(np.int32), ys=y[first].astype(np.int32),
                            ss=rng.randint(7, 256, len(first)).astype(np.int32))
    return c


def _cell_order(c, W, H):
    """The list order the kernels see: candidates sorted into the level's FAST cells, row-major, stable."""
    import ctypes as C
    import oracle_bind
    g = [C.c_int() for _ in range(4)]
    oracle_bind.lib.orc_cell_grid(W + 32, H + 32, *[C.byref(v) for v in g])
    ncols, nrows, wcell, hcell = (v.value for v in g)
    cell = np.minimum(c["ys"] // hcell, nrows - 1) * ncols + np.minimum(c["xs"] // wcell, ncols - 1)
    return np.argsort(cell, kind="stable")


@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: "%dx%d_q%d_%s" % (b[0], b[1], b[2], b[3][0]))
def test_table_form_matches_oracle_and_iterative_form(gpu_ctx, cases, batch):
    import oracle_bind
    import orbhip
    W, H, N, names = batch
    ext = orbhip.Extractor(gpu_ctx, N, 1.2, 1, 20, 7)
    ext.reserve(W + 32, H + 32, 4)
    lists, want, deep = [], [], []
    n_ini = int(np.floor(np.float32(W) / np.float32(H) + 0.5))
    dmax = M.table_depth(n_ini, [N])
    assert dmax >= 2
    for name in names:
        c = cases[name]
        assert c["W"] == W and c["H"] == H or name in ("empty", "one_key")
        o = _cell_order(c, W, H)
        xs, ys, ss = c["xs"][o], c["ys"][o], c["ss"][o]
        lists.append((xs, ys, ss))
        keep = oracle_bind.octree(xs, ys, ss, 16, 16 + W, 16, 16 + H, N)
        want.append(np.stack([xs[keep], ys[keep], ss[keep]], 1).astype(np.int32).reshape(-1, 3))
        deep.append(1 if len(xs) and M.octree_table(xs, ys, ss, 16, 16 + W, 16, 16 + H, N, dmax=dmax) is None else 0)
    tab, redo = ext.debug_octree(0, lists, "table")
    tab2, redo2 = ext.debug_octree(0, lists, "table")
    it, _ = ext.debug_octree(0, lists, "iterative")
    for f, name in enumerate(names):
        assert np.array_equal(tab[f], want[f]), (name, "table form vs oracle")
        assert np.array_equal(it[f], want[f]), (name, "iterative form vs oracle")
        assert tab2[f].tobytes() == tab[f].tobytes(), (name, "second run differs")
    assert redo == deep and redo2 == deep, (names, redo, deep)            # the iterative form ran exactly where the tables do not reach
    if "tight_block_deep" in names:
        assert deep == [1, 0, 0] and len(lists[1][0]) > 2048             # both paths in one launch; the global-memory key path
    ext.close()


def _three_runs(ext, level, cases, tag):
    """Table form, table form again, iterative form: both equal the oracle, the repeat is identical, and the iterative form ran behind the table
    form exactly where the closed form with tables of the extractor's depth gives up.  Returns the flags."""
    lists = [(p["xs"], p["ys"], p["ss"]) for p in cases]
    tab, redo = ext.debug_octree(level, lists, "table")
    tab2, redo2 = ext.debug_octree(level, lists, "table")
    it, _ = ext.debug_octree(level, lists, "iterative")
    for f, p in enumerate(cases):
        assert np.array_equal(tab[f], p["want"]), (tag, f, p["name"], "table form vs oracle")
        assert np.array_equal(it[f], p["want"]), (tag, f, p["name"], "iterative form vs oracle")
        assert tab2[f].tobytes() == tab[f].tobytes(), (tag, f, p["name"], "second run differs")
    deep = [p["deep"] for p in cases]
    assert redo == deep and redo2 == deep, (tag, [p["name"] for p in cases], redo, redo2, deep)
    return redo


@pytest.mark.parametrize("geometry", M.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_random_lists_on_the_device(gpu_ctx, geometry):
    """The 240 seeded lists of the CPU test (uniform, clustered, tight blocks), less those no FAST stage can produce, one launch per (W, H, quota):
    up to 9 lists of mixed depth side by side."""
    import orbhip
    groups, skipped = D.random_groups()
    D.check_random_balance()
    ran = 0
    for (W, H, N), cases in sorted(groups.items()):
        if (W, H) != geometry:
            continue
        assert M.table_depth(D.n_ini_of(W, H), [N]) >= 2
        ext = orbhip.Extractor(gpu_ctx, N, 1.2, 1, 20, 7)
        ext.reserve(W + 32, H + 32, len(cases))
        assert ext.level_dims(0) == (W + 32, H + 32) and ext.features_per_level()[0] == N
        _three_runs(ext, 0, cases, (W, H, N))
        ext.close()
        ran += len(cases)
    assert ran >= 30                                                      # every geometry has its share of the 229


def test_register_global_split(gpu_ctx):
    """2047, 2048, 2049 and 2305 keys: a workgroup keeps OCT_KR * 256 = 2048 in registers and the rest in global memory; in the last list the one key
    on the global path is alone in its root quadrant, so it makes a node of its own and must come out."""
    import orbhip
    cases = D.split_cases()
    D.check_split_cases()
    ext = orbhip.Extractor(gpu_ctx, 400, 1.2, 1, 20, 7)
    ext.reserve(608 + 32, 448 + 32, len(cases))
    _three_runs(ext, 0, cases, "split")
    ext.close()


@pytest.mark.parametrize("level", D.REDO_LEVELS)
def test_redo_in_every_position(gpu_ctx, level):
    """k_octree_redo beyond workgroup 0 and level 0: 8 levels x 40 frames = 320 lists, 64 per workgroup, the lists of `level` filled and ten of
    them deeper than the tables -- adjacent and distant frames, several per workgroup one after the other in the same LDS, and at level 3 (lists
    120 .. 159) on both sides of list 128, where the second workgroup ends."""
    import orbhip
    cases, dmax = D.redo_lists(level)
    D.check_redo_lists(level)
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    ext.reserve(640, 480, D.REDO_FRAMES)
    w, h = ext.level_dims(level)
    assert (w - 32, h - 32) == (cases[0]["W"], cases[0]["H"]) and ext.features_per_level()[level] == cases[0]["N"]
    n_ini = max(D.n_ini_of(ext.level_dims(l)[0] - 32, ext.level_dims(l)[1] - 32) for l in range(8))
    assert M.table_depth(n_ini, ext.features_per_level().tolist()) == dmax
    redo = _three_runs(ext, level, cases, "level %d" % level)
    assert [f for f in range(D.REDO_FRAMES) if redo[f]] == list(D.REDO_FLAGGED_AT)
    ext.close()


def test_second_gather_path(gpu_ctx):
    """oct_gather copies cell by cell where the cell offsets do not fit the LDS (ncells + 1 > 16 * NC): a quota of 50 on 1200 x 900.  Uniform lists
    (one of more than 2048 keys), tight blocks, and blocks deeper than the tables, so that both forms and the second launch gather that way."""
    import orbhip
    g = D.GATHER_SHAPE
    ext = orbhip.Extractor(gpu_ctx, g["nfeatures"], 1.2, g["nlevels"], 20, 7)
    for level in range(g["nlevels"]):
        cases, dmax, ncells, nc = D.gather_lists(level)
        D.check_gather_lists(level)
        ext.reserve(g["w"], g["h"], len(cases))
        quotas = ext.features_per_level().tolist()
        assert nc == max(max(q + 16, 8) for q in quotas) and ncells + 1 > 16 * nc          # the premise, from the extractor's own quotas
        w, h = ext.level_dims(level)
        assert (w - 32, h - 32) == (cases[0]["W"], cases[0]["H"]) and quotas[level] == cases[0]["N"]
        redo = _three_runs(ext, level, cases, "gather level %d" % level)
        assert sum(redo) >= 2
    ext.close()
