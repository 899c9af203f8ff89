"""k_fast_cells walks a frame's cells by a table built at reserve (tests/test_fast_cell_table.py checks the table itself).  Here the
per-cell candidate lists of every level, on synthetic frames, are compared byte for byte with the C oracle's for geometries at the
table's edges: the smallest 8-level size and an odd one in batches of 3 (chunks cross level and frame boundaries), a skipped column,
the large-cell instance, level-range launches, and chunks of 1 and 5 cells in a process of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_table_child as child
from test_fast_cell_table import reference_cells, level_sizes

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle_lists(case):
    """the oracle's lists of the case's frames, computed once"""
    if case not in _oracle:
        import oracle_bind as ob
        w, h, nlevels, n = child.CASES[case]
        imgs = child.frames(case)
        out = {}
        for f in range(n):
            ora = ob.OracleExtractor(1000, 1.2, nlevels, 20, 7)
            ora.extract(np.ascontiguousarray(imgs[f]))
            for l in range(nlevels):
                out["f%d_l%d" % (f, l)] = np.stack(ora.fast_candidates(l))
        _oracle[case] = out
    return _oracle[case]


def facts_of(case):
    w, h, nlevels, _ = child.CASES[case]
    ws, hs = level_sizes(w, h, nlevels)
    want, facts = reference_cells(ws, hs)
    assert want is not None
    return facts


def assert_equal_lists(got, want, what):
    assert sorted(k for k in got if k != "kernel") == sorted(want)
    for key in want:
        assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize("case,instance", [("min8", 0), ("odd", 1), ("skip", 0), ("large", 0)])
def test_lists_equal_oracle(gpu_ctx, case, instance, monkeypatch):
    monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)
    monkeypatch.delenv("ORBHIP_TUNE_L0_EARLY", raising=False)
    facts = facts_of(case)
    if case == "odd":
        assert facts["clipped"] > 0
    if case == "skip":
        assert facts["skipped"] > 0
    got = child.lists(gpu_ctx, case)
    assert int(got["kernel"]) in (0, 1) and (instance is None or int(got["kernel"]) == instance)
    want = oracle_lists(case)
    assert_equal_lists(got, want, case)
    counts = [want[k].shape[1] for k in sorted(want)]
    assert sum(counts) > 100 and sum(1 for c in counts if c > 0) > len(counts) // 2, counts       # (the frames do have corners)


def test_level_range_launches(gpu_ctx, monkeypatch):
    """a batch of 16 with level 0 launched ahead of the pyramid and levels 1 .. 7 after it (ORBHIP_TUNE_L0_EARLY=1): two launches over
    sub-ranges of the table.  Lists equal to the one-launch path's and the oracle's."""
    monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)
    monkeypatch.delenv("ORBHIP_TUNE_L0_EARLY", raising=False)
    plain = child.lists(gpu_ctx, "batch16")
    monkeypatch.setenv("ORBHIP_TUNE_L0_EARLY", "1")
    early = child.lists(gpu_ctx, "batch16")
    want = oracle_lists("batch16")
    assert_equal_lists(plain, want, "one launch")
    assert_equal_lists(early, want, "level-range launches")


@pytest.mark.parametrize("chunk,case,instance", [(1, "min8", 0), (5, "min8", 0), (5, "odd", 1)])
def test_chunks(gpu_ctx, chunk, case, instance, tmp_path, monkeypatch):
    """ORBHIP_TUNE_FAST_CHUNK = 1 and 5 on the 8-level cases (either instance): with 5, chunks run over level and frame boundaries and the
    last one is short (3 x 93 and 3 x 356 cells)"""
    monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)
    assert "ORBHIP_TUNE_FAST_CHUNK" not in os.environ
    out = tmp_path / "chunk.npz"
    env = dict(os.environ, ORBHIP_TUNE_FAST_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, child.__file__, str(out), case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    there = dict(np.load(out))
    assert int(there["kernel"]) == instance
    assert_equal_lists(there, oracle_lists(case), "chunk %d" % chunk)
