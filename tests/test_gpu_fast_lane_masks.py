"""k_fast_cells (both instances) on frames crafted for the way a wave walks a cell: the necessary test runs in trips of rpt band rows,
lane = (row of the trip, two adjacent pixel pairs), its survivors go to a queue that is scored and suppressed 64 entries at a time, and the
kept pixels leave in cv::FAST's raster order.  Every candidate list equal to the C oracle's and the plain model's in count, order, x, y and
score; the instance that ran asserted; a ledger derives from the model's per-cell facts and the lane layout (restated here) that every
situation occurred:

  the first and the last trip of one lane flagged, in a cell with the most trips the instance reaches (6: 40 x 36 cells; 13: the 58 x 58 cell)
  every pair of a cell flagged (a full queue, every flag of every lane)
  queues of exactly 64 and 65 entries; more than 64 kept corners in one cell (emission over several queue iterations)
  kept corners of one row found by different lanes; kept corners of a later trip found by a lower lane (raster order is not lane order)
  a clipped cell with an odd band whose last pair reaches past the band and whose last lane's second pair lies wholly past it, both on corners
  a cell empty at iniThFAST with more than 64 entries in the second pass
  a skipped cell between live ones inside a chunk of four cells (child process: ORBHIP_TUNE_FAST_CHUNK is read once per process)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_cases as fc
import fast_model as fm

pytestmark = pytest.mark.gpu
INSTANCE = ("k_fast_cells<5,32,5>", "k_fast_cells<3,24,2>")
INI, MN, BG = 20, 7, 100
# image size, the instance k_fast_cells must select, the most trips a cell of the geometry takes
GEOMS = {
    "m111": dict(w=111, h=104, inst=1, grid=(2, 2, 40, 36), trips=6),     # the small instance's largest cells; last column clipped to dw 33 (17 pairs)
    "g90": dict(w=90, h=90, inst=0, grid=(1, 1, 58, 58), trips=13),       # one 58 x 58 cell, band 52 x 52: rpt 4, the most trips of any geometry
    "g118": dict(w=118, h=100, inst=0, grid=(2, 2, 43, 34), trips=7),     # last column clipped to dw 37 (19 pairs) under the large instance
}
CHUNK = 4
CHUNK_GEOMS = {"g933": 0, "g933s": 1}          # fast_cases.py: 30 columns, the last one skipped; the instance each selects


def layout(geom):
    """(tpr, rpt) of the necessary test from the nominal cell width: two-pair tasks per row, rows per trip"""
    wcell = GEOMS[geom]["grid"][2]
    tpr = (((wcell + 1) >> 1) + 1) >> 1
    return tpr, 64 // tpr


def lane_bit(geom, bx, by):
    """(lane, flag bit 2 trip + pair) that evaluates band pixel (bx, by)"""
    tpr, rpt = layout(geom)
    bp = bx >> 1
    return (by % rpt) * tpr + (bp >> 1), 2 * (by // rpt) + (bp & 1)


def _blank(geom):
    g = GEOMS[geom]
    return np.full((g["h"], g["w"]), BG, np.uint8)


def _dot(img, geom, ci, cj, bx, by):
    g = GEOMS[geom]
    ini_x, ini_y, dw, dh = fm.cell_band(g["w"], g["h"], ci, cj)
    img[ini_y + 3 + by, ini_x + 3 + bx] = 255


def _lattice_slots(geom, ci, cj):
    g = GEOMS[geom]
    _, _, dw, dh = fm.cell_band(g["w"], g["h"], ci, cj)
    return [(bx, by) for by in range(1, dh, 4) for bx in range(1, dw, 4)]


@functools.lru_cache(maxsize=None)
def frames(geom):
    """{name: image}.  An isolated bright dot is a corner of score 154 that survives the NMS, and it flags exactly its own pixel pair in the
    necessary test (its compass neighbours see one bright end of one diametral pair only); dots 4 apart do not meet on a ring."""
    g = GEOMS[geom]
    tpr, rpt = layout(geom)
    yy, xx = np.mgrid[0:g["h"], 0:g["w"]]
    out = {}
    if geom != "g118":
        img = _blank(geom)                                 # one lane (row 1 of a trip, pairs 4 and 5), first and last trip, both pairs
        for by in (1, (g["trips"] - 1) * rpt + 1):
            _dot(img, geom, 0, 0, 9, by)
        _dot(img, geom, 0, 0, 11, (g["trips"] - 1) * rpt + 1)
        out["hibit"] = img
        for n in (64, 65):
            img = _blank(geom)
            for bx, by in _lattice_slots(geom, 0, 0)[:n]:
                _dot(img, geom, 0, 0, bx, by)
            out["q%d" % n] = img
        img = _blank(geom)
        for ci in range(g["grid"][1]):
            for cj in range(g["grid"][0]):
                for bx, by in _lattice_slots(geom, ci, cj):
                    _dot(img, geom, ci, cj, bx, by)
        out["lattice"] = img
        out["weakramp"] = (BG + np.abs((7 * xx + 3 * yy) % 40 - 20)).astype(np.uint8)
    out["ramp"] = np.abs((43 * xx + 24 * yy) % 510 - 255).astype(np.uint8)
    if geom != "g90":
        cj = g["grid"][0] - 1
        _, _, dw, dh = fm.cell_band(g["w"], g["h"], 0, cj)
        assert dw % 2 == 1 and ((dw + 1) // 2) % 2 == 1 and dw < g["grid"][2]
        img = _blank(geom)
        for bx, by in ((dw, 5), (dw + 1, 12), (dw + 2, 20), (dw - 1, 27), (2, 5), (dw - 1, 12)):
            _dot(img, geom, 0, cj, bx, by)
        out["odd"] = img
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(geom):
    """{name: (model xs, ys, scores, facts, oracle xs, ys, scores)}, computed once"""
    import oracle_bind as ob
    out = {}
    for name, img in frames(geom).items():
        assert fm.grid(GEOMS[geom]["w"], GEOMS[geom]["h"]) == GEOMS[geom]["grid"]
        ora = ob.OracleExtractor(1000, 1.2, 1, INI, MN)
        ora.extract(np.ascontiguousarray(img))
        out[name] = fm.cells(img, INI, MN) + tuple(ora.fast_candidates(0))
    return out


def _assert_equal(got, want_model, want_oracle, what):
    assert len(got[0]) == len(want_model[0]) == len(want_oracle[0]), (what, len(got[0]), len(want_model[0]), len(want_oracle[0]))
    for k, n in enumerate(("x", "y", "score")):
        np.testing.assert_array_equal(got[k], want_oracle[k], err_msg="%s %s against the oracle" % (what, n))
        np.testing.assert_array_equal(got[k], want_model[k], err_msg="%s %s against the model" % (what, n))


@pytest.mark.parametrize("geom", list(GEOMS))
def test_lists_equal_oracle_and_model(gpu_ctx, geom, monkeypatch):
    import orbhip
    monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)
    names = list(frames(geom))
    assert len(names) <= 8
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 1, INI, MN)
    ext.extract_host(np.stack([frames(geom)[n] for n in names]))
    assert ext.fast_kernel() == GEOMS[geom]["inst"], (geom, ext.fast_kernel())
    bad = []
    for f, n in enumerate(names):
        e = expected(geom)[n]
        try:
            _assert_equal(ext.fast_candidates(f, 0), e[:3], e[4:], "%s %s" % (geom, n))
        except AssertionError as err:
            bad.append((n, str(err).strip().splitlines()[-1]))
    ext.close()
    assert not bad, (geom, INSTANCE[GEOMS[geom]["inst"]], bad)


def _cells(geom, name):
    """per live cell of a frame: facts, flagged pairs per pass [(by, bp)], kept pixels [(bx, by)] in list order"""
    g = GEOMS[geom]
    img = frames(geom)[name]
    mx, my, ms, facts = expected(geom)[name][:4]
    M = fm.compass_map(img)
    at = 0
    for f in facts:
        if f["skipped"]:
            continue
        ini_x, ini_y, dw, dh = fm.cell_band(g["w"], g["h"], f["ci"], f["cj"])
        flagged = []
        for th in ([INI, MN] if f["second_pass"] else [INI]):
            flagged.append([(by, bp) for by in range(dh) for bp in range(f["npb"])
                            if max(M[ini_y + 3 + by, ini_x + 3 + 2 * bp], M[ini_y + 3 + by, ini_x + 3 + 2 * bp + 1]) > th])
        assert [len(q) for q in flagged] == f["nq"]
        kept = [(int(mx[i]) - 3 - f["cj"] * g["grid"][2], int(my[i]) - 3 - f["ci"] * g["grid"][3]) for i in range(at, at + f["n"])]
        at += f["n"]
        yield f, flagged, kept, M, (ini_x, ini_y, dw, dh)


@pytest.mark.parametrize("instance", (0, 1))
def test_ledger(instance):
    """every situation of the module's list occurs in the frames that run under the instance (no device work: the lists of these very
    frames are compared above, those of the chunk geometries in the test below)"""
    hit = set()
    for geom, g in GEOMS.items():
        if g["inst"] != instance:
            continue
        tpr, rpt = layout(geom)
        wcell, hcell = g["grid"][2:]
        for name in frames(geom):
            for f, flagged, kept, M, (ini_x, ini_y, dw, dh) in _cells(geom, name):
                trips = -(-dh // rpt)
                assert 2 * trips <= 32
                masks = {}
                for by, bp in flagged[0]:
                    lane, bit = lane_bit(geom, 2 * bp, by)
                    masks[lane] = masks.get(lane, 0) | 1 << bit
                most = max(gg["trips"] for gg in GEOMS.values() if gg["inst"] == instance)
                if trips == most and any(m & 3 and m >> (2 * trips - 2) for m in masks.values()):
                    hit.add("first and last trip of one lane, most trips")
                if f["nq"][0] == dh * f["npb"] and trips == most and all(masks.get(lane_bit(geom, 2 * bp, by)[0], 0) == (1 << 2 * trips) - 1
                                                                         for by in range(min(rpt, dh - (trips - 1) * rpt)) for bp in range(0, f["npb"] - 1, 2)):
                    hit.add("every pair flagged")
                hit |= {"queue of %d" % n for n in f["nq"] if n in (64, 65)}
                if f["n"] > 64:
                    hit.add("more than 64 kept corners")
                lanes = [lane_bit(geom, bx, by) for bx, by in kept]
                assert kept == sorted(kept, key=lambda p: (p[1], p[0]))
                if any(a[1] == b[1] and la[0] != lb[0] for a, la in zip(kept, lanes) for b, lb in zip(kept, lanes)):
                    hit.add("one row, different lanes")
                if any(lb[1] >> 1 > la[1] >> 1 and lb[0] < la[0] for i, la in enumerate(lanes) for lb in lanes[i + 1:]):
                    hit.add("later trip, lower lane")
                if dw % 2 == 1 and dw < wcell and f["npb"] % 2 == 1:
                    col = lambda bx: M[ini_y + 3:ini_y + 3 + dh, ini_x + 3 + bx]
                    if (col(dw) > INI).any() and (np.maximum(col(dw + 1), col(dw + 2)) > INI).any() and (dw - 1) in [bx for bx, _ in kept]:
                        hit.add("clipped odd band: corners past the band in the last pair and in the last lane's second pair")
                if f["second_pass"] and f["nq"][1] > 64:
                    hit.add("second pass, more than 64 entries")
    for geom, inst in CHUNK_GEOMS.items():
        if inst != instance:
            continue
        import fast_lane_mask_child as child
        assert fc.GEOMS[geom]["inst"] == instance
        walk = [f["skipped"] for fr in child.batch(geom) for f in fc.model_results(geom)[fr.name][3]]
        if any(s and i % CHUNK in (1, 2) and not walk[i - 1] and not walk[i + 1] for i, s in enumerate(walk[:-1])):
            hit.add("skipped cell between live ones inside a chunk")
    want = {"first and last trip of one lane, most trips", "every pair flagged", "queue of 64", "queue of 65", "more than 64 kept corners",
            "one row, different lanes", "later trip, lower lane", "clipped odd band: corners past the band in the last pair and in the last lane's second pair",
            "second pass, more than 64 entries", "skipped cell between live ones inside a chunk"}
    assert hit >= want, (INSTANCE[instance], sorted(want - hit))


@pytest.mark.parametrize("geom", list(CHUNK_GEOMS))
def test_skipped_cell_inside_a_chunk(gpu_ctx, geom, monkeypatch, tmp_path):
    """three frames of 30 cell columns, the last one skipped, in chunks of four cells: equal to this process's lists (chunks of one
    cell), the oracle's and the model's"""
    import fast_lane_mask_child as child
    monkeypatch.delenv("ORBHIP_FAST_KERNEL", raising=False)
    assert "ORBHIP_TUNE_FAST_CHUNK" not in os.environ
    here = child.lists(gpu_ctx, geom)
    out = tmp_path / "chunk.npz"
    env = dict(os.environ, ORBHIP_TUNE_FAST_CHUNK=str(CHUNK))
    r = subprocess.run([sys.executable, child.__file__, str(out), geom], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    there = np.load(out)
    assert int(there["kernel"]) == int(here["kernel"]) == CHUNK_GEOMS[geom]
    for f, fr in enumerate(child.batch(geom)):
        key = "f%d" % f
        _assert_equal(tuple(there[key]), fc.model_results(geom)[fr.name][:3], fc.oracle_results(geom)[fr.name], "%s %s chunk %d" % (geom, fr.name, CHUNK))
        np.testing.assert_array_equal(there[key], here[key], err_msg="%s %s against chunks of one cell" % (geom, fr.name))
