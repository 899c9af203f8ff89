"""GPU: the table form of the octree (k_octree_tab, with k_octree_redo behind it) against the oracle and against the iterative form, through
the octree-only test entry: kept keys and their order, bit for bit.  Cases: tests/octree_table_model.py (checked against the oracle on the CPU
by tests/test_octree_table_model.py)."""
import numpy as np
import pytest

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
