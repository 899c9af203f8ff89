"""The per-cell FAST stage on the device (k_fast_cells for large and small cells, k_fast_runs<4> and <6>) on the crafted frames of
fast_cases.py: every candidate list equal to the C oracle's and the plain model's in count, order, x, y and score (test_fast_cases.py
holds both to the declarations), the instance that ran asserted, the paths the frames take through each instance counted from the
model's per-cell facts, and chunks of several cells in a process of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_cases as fc
import fast_model as fm

pytestmark = pytest.mark.gpu
KERNELS = ("cells", "runs")
INSTANCE = ("k_fast_cells<5,32,5>", "k_fast_cells<3,24,2>", "k_fast_runs<4>", "k_fast_runs<6>")


def _set_kernel(monkeypatch, kernel):
    """(the variable is read when the extractor reserves: set before the extractor is made)"""
    if kernel == "runs":
        monkeypatch.setenv("ORBHIP_FAST_KERNEL", "runs")
    else:
        monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)


def _assert_lists(got, geom, fr):
    mx, my, ms, _ = fc.model_results(geom)[fr.name]
    ox, oy, os_ = fc.oracle_results(geom)[fr.name]
    gx, gy, gs = got
    assert len(gx) == len(ox) == len(mx), (geom, fr.name, len(gx), len(ox), len(mx))
    for g, o, m, what in ((gx, ox, mx, "x"), (gy, oy, my, "y"), (gs, os_, ms, "score")):
        np.testing.assert_array_equal(g, o, err_msg="%s %s %s against the oracle" % (geom, fr.name, what))
        np.testing.assert_array_equal(g, m, err_msg="%s %s %s against the model" % (geom, fr.name, what))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("geom", list(fc.GEOMS))
def test_device_lists_equal_oracle_and_model(gpu_ctx, geom, kernel, monkeypatch):
    """every frame of the geometry through the host entry, one-level extractors, batches of at most 16 frames; no capacity error"""
    import orbhip
    _set_kernel(monkeypatch, kernel)
    g = fc.GEOMS[geom]
    bad = []
    for (ini, mn), batch in fc.batches(geom):
        ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 1, ini, mn)
        ext.extract_host(np.stack([fr.img for fr in batch]))
        assert ext.fast_kernel() == (g["inst"] if kernel == "cells" else g["runs"]), (geom, INSTANCE[ext.fast_kernel()])
        for f, fr in enumerate(batch):
            try:
                _assert_lists(ext.fast_candidates(f, 0), geom, fr)
            except AssertionError as e:
                bad.append((fr.name, str(e).strip().splitlines()[-1] if len(bad) else str(e)))
        ext.close()
    assert not bad, (geom, INSTANCE[g["inst"] if kernel == "cells" else g["runs"]], [b[0] for b in bad], bad[0][1])


@pytest.mark.parametrize("kernel", KERNELS)
def test_device_entry(gpu_ctx, kernel, monkeypatch):
    """the same lists through the device entry (images resident on the device, a padded row stride)"""
    import torch
    import orbhip
    _set_kernel(monkeypatch, kernel)
    geom = "g123"
    (ini, mn), batch = fc.batches(geom)[0]
    imgs = np.stack([fr.img for fr in batch])
    B, H, W = imgs.shape
    buf = np.full((B, H, W + 5), 77, np.uint8)
    buf[:, :, :W] = imgs
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 1, ini, mn)
    ext.reserve(W, H, B)
    ext.extract_device(d.data_ptr(), W, H, W + 5, (W + 5) * H, B)
    gpu_ctx.synchronize()
    assert ext.fast_kernel() == (fc.GEOMS[geom]["inst"] if kernel == "cells" else fc.GEOMS[geom]["runs"])
    for f, fr in enumerate(batch):
        _assert_lists(ext.fast_candidates(f, 0), geom, fr)
    ext.close()


def _cell_facts(instance):
    """(geometry dict, frame, facts of one live or skipped cell) of every frame the test above runs under that instance"""
    for geom, g in fc.GEOMS.items():
        if instance in (g["inst"], g["runs"]):
            for fr in fc.frames(geom):
                for f in fc.model_results(geom)[fr.name][3]:
                    yield g, fr, f


@pytest.mark.parametrize("instance", (0, 1, 2, 3))
def test_path_ledger(instance):
    """The paths through one instance that the frames of its geometries take, from the model's per-cell facts (no device work here: the
    lists of these very frames are compared above).  Every entry at least once."""
    hit = set()
    for g, fr, f in _cell_facts(instance):
        ncols, nrows, wcell, hcell = g["grid"]
        if f["skipped"]:
            hit.add("skipped cell")
            continue
        hit |= {w for w, on in (("second pass", f["second_pass"]), ("clipped cell", f["dw"] < wcell or f["dh"] < hcell), ("odd dw", f["dw"] % 2 == 1),
                                ("odd dw, clipped", f["dw"] % 2 == 1 and f["dw"] < wcell), ("empty after both passes", f["second_pass"] and f["n"] == 0),
                                ("second pass finds corners", f["second_pass"] and f["n"] > 0)) if on}
        if instance < 2:
            # k_fast_cells: rpt rows per trip of the necessary test (from the level's nominal cell width), a queue of dh * npb entries scored 64 at a time
            rpt = 64 // ((((wcell + 1) >> 1) + 1) >> 1)
            hit |= {w for w, on in (("several trips", f["dh"] > rpt), ("more than 64 queue entries", max(f["nq"]) > 64),
                                    ("full queue", f["nq"][0] == f["dh"] * f["npb"]), ("second pass, more than 64 queue entries", len(f["nq"]) > 1 and f["nq"][1] > 64)) if on}
    if instance >= 2:
        # k_fast_runs: runs of rpc cells of a cell row; queue entries of a run counted over the band of the whole run
        for geom, g in fc.GEOMS.items():
            if g["runs"] != instance:
                continue
            ncols, nrows, wcell, hcell = g["grid"]
            for fr in fc.frames(geom):
                facts = {(f["ci"], f["cj"]): f for f in fc.model_results(geom)[fr.name][3]}
                M = fm.compass_map(fr.img)
                for ci in range(nrows):
                    for cj in range(0, ncols, g["rpc"]):
                        run = [facts[(ci, c)] for c in range(cj, min(cj + g["rpc"], ncols))]
                        if run[0]["skipped"]:
                            continue
                        dw, dh = sum(f["dw"] for f in run), run[0]["dh"]
                        nq = fm.compass_pairs(M, 16 + cj * wcell + 3, 16 + ci * hcell + 3, dw, dh, fr.ini)
                        hit |= {w for w, on in (("several trips", (dh + 1) // 2 > 7), ("more than 64 queue entries", nq > 64), ("full queue", nq == dh * ((dw + 1) // 2)),
                                                ("odd band height", dh % 2 == 1)) if on}
                        if len(run) == 1:
                            hit.add("one-cell run")
                            if g["rpc"] == 2:
                                hit.add("one-cell run after two-cell runs")
                        elif run[1]["skipped"]:
                            hit.add("two-cell run, right cell skipped")
                        else:
                            hit.add("two-cell run: %s" % {(False, False): "neither empty at ini", (True, False): "left empty", (False, True): "right empty",
                                                          (True, True): "both empty"}[(run[0]["second_pass"], run[1]["second_pass"])])
                            if run[0]["dw"] % 2:
                                hit.add("two-cell run, a pixel pair across the cells")
    want = {"second pass", "skipped cell", "clipped cell", "odd dw", "odd dw, clipped", "several trips", "more than 64 queue entries", "full queue",
            "empty after both passes", "second pass finds corners"}
    if instance < 2:
        want |= {"second pass, more than 64 queue entries"}
    else:
        want |= {"two-cell run: neither empty at ini", "two-cell run: left empty", "two-cell run: right empty", "two-cell run: both empty",
                 "two-cell run, right cell skipped", "two-cell run, a pixel pair across the cells", "odd band height"}
        if instance == 2:
            want |= {"one-cell run", "one-cell run after two-cell runs"}
    assert hit >= want, (INSTANCE[instance], sorted(want - hit))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk", (3, 7))
def test_chunks_of_several_cells(gpu_ctx, chunk, kernel, monkeypatch, tmp_path):
    """A wave walks from cell to cell (column, row, level, frame) only inside a chunk of several cells, which the default sizing gives only
    to batches of hundreds of frames.  ORBHIP_TUNE_FAST_CHUNK = 3 and 7 in a child process (the variable is read once per process): 3 frames,
    2 levels, 30 x 3 cells with a skipped column at level 0.  Equal to this process's lists (chunks of one cell), the oracle's and the model's
    (level 1 of the model from the oracle's pyramid)."""
    import oracle_bind as ob
    import fast_chunk_child as child
    _set_kernel(monkeypatch, kernel)
    assert "ORBHIP_TUNE_FAST_CHUNK" not in os.environ
    here = child.lists(gpu_ctx)
    out = tmp_path / "chunk.npz"
    env = dict(os.environ, ORBHIP_TUNE_FAST_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, child.__file__, str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    there = np.load(out)
    g = fc.GEOMS["g933c"]
    assert int(there["kernel"]) == int(here["kernel"]) == (g["inst"] if kernel == "cells" else g["runs"])
    imgs = fc.chunk_batch()
    counts = []
    for f in range(len(imgs)):
        ora = ob.OracleExtractor(1000, 1.2, 2, 20, 7)
        ora.extract(np.ascontiguousarray(imgs[f]))
        for l in range(2):
            key = "f%d_l%d" % (f, l)
            level = ora.pyramid_level(l)
            if l == 0:
                np.testing.assert_array_equal(level, imgs[f])
            mx, my, ms, facts = fm.cells(level, 20, 7)
            want = np.stack(ora.fast_candidates(l))
            np.testing.assert_array_equal(want, np.stack([mx, my, ms]), err_msg=key + " oracle against the model")
            np.testing.assert_array_equal(there[key], want, err_msg="%s chunk %d against the oracle" % (key, chunk))
            np.testing.assert_array_equal(there[key], here[key], err_msg="%s chunk %d against chunks of one cell" % (key, chunk))
            assert l == 1 or any(c["skipped"] for c in facts)
            counts.append(len(mx))
    assert min(counts[2:]) > 200 and counts[0] > 0, counts            # (the first frame has corners outside the bands only: level 1 stays empty)
