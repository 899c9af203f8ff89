"""The crafted FAST frames of fast_cases.py on the CPU: the plain model (fast_model.py) and the C oracle both meet every declaration and
agree on every whole list, and the ledgers say that every outcome, every weakest ring position, every NMS direction and every seam
occurs at every geometry it applies to.  test_gpu_fast_cases.py then holds the device to these lists."""
import numpy as np
import pytest

import fast_cases as fc
import fast_model as fm
import oracle_bind as ob


def test_geometries_are_what_the_case_file_says():
    assert fc.RING == list(zip(fm.DX, fm.DY))
    for name, g in fc.GEOMS.items():
        assert g["w"] >= 75 and g["h"] >= 75
        assert fm.grid(g["w"], g["h"]) == g["grid"] == ob.cell_grid(g["w"], g["h"]), name
        ncols, nrows, wcell, hcell = g["grid"]
        assert g["inst"] == (1 if wcell <= 40 and hcell <= 36 else 0) and g["runs"] == (2 if hcell <= 45 else 3), name
        assert g["rpc"] == (2 if 2 * wcell <= 64 else 1) and wcell <= 64 and hcell <= 64, name
        for ci in range(nrows):
            for cj in range(ncols):
                ix, iy, dw, dh = fm.cell_band(g["w"], g["h"], ci, cj)
                assert fc.band(g, ci, cj) == (ix - 16 + 3, iy - 16 + 3, dw, dh), (name, ci, cj)
    b = lambda geom, ci, cj: fc.band(fc.GEOMS[geom], ci, cj)[2:]
    assert b("g123", 0, 2) == (23, 33) and b("g933", 0, 29) == (0, 0) and b("g933", 0, 28) == (27, 37) and b("g90", 0, 0) == (52, 52)
    assert b("g903", 28, 0) == (0, 0) and b("g903", 27, 0) == (30, 28)
    # 903 is the smallest height whose last cell row is skipped (ini_y >= max_by - 3), whatever the width
    first = next(h for h in range(75, 1101) if 16 + (fm.grid(512, h)[1] - 1) * fm.grid(512, h)[3] >= h - 16 - 3)
    assert first == 903 == fc.GEOMS["g903"]["h"]


def test_stored_nms_patches_still_are_what_they_declare():
    """A and B of every stored patch, on a flat canvas, by the plain arc score: the declared scores, A above (or level with) B, and
    everybody else in their 3 x 3 below them"""
    for (base, rel), ((dx, dy), a, b, raw) in fc.NMS_PATCHES.items():
        img = np.full((25, 25), fc.BG, np.uint8)
        img[8:17, 8:17] = np.frombuffer(raw, np.uint8).reshape(9, 9)
        S = lambda x, y: fm.arc_score(img, 12 + x, 12 + y) - 1
        assert (S(0, 0), S(dx, dy)) == (a, b) and (a > b if rel == "gt" else a == b) and b > 20
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                if (i, j) not in ((0, 0), (dx, dy)):
                    assert S(i, j) < a
                if (i + dx, j + dy) not in ((0, 0), (dx, dy)):
                    assert S(i + dx, j + dy) < b


def _check_declarations(fr, xs, ys, ss, facts, S, who):
    """every declared pixel of a frame against one candidate list; S(x, y) = arc score at a candidate coordinate"""
    g = fr.g
    got = {(int(x), int(y)): int(s) for x, y, s in zip(xs, ys, ss)}
    assert len(got) == len(xs)
    fact = {(f["ci"], f["cj"]): f for f in facts}
    lo = min(fr.ini, fr.mn)
    for x, y, outcome, score, meta in fr.decl:
        at, tag = got.get((x, y)), (who, fr.geom, fr.name, x, y, outcome, meta)
        cell = fc.cell_of(g, x, y)
        s = S(x, y)
        if outcome == "KEPT":
            assert at == score and s == score + 1 and score >= fr.ini and cell is not None, tag
        elif outcome == "WEAK_KEPT":
            assert at == score and s == score + 1 and fr.mn <= score < fr.ini and fact[cell]["second_pass"], tag
        elif outcome == "NMS_LOST":
            assert at is None and s > fr.ini and cell is not None, tag
            near = [got.get((x + i, y + j), 0) for j in (-1, 0, 1) for i in (-1, 0, 1) if (i or j) and fc.cell_of(g, x + i, y + j) == cell]
            assert meta["rel"] == "eq" or max(near) > s - 1, tag        # (equal scores: neither is in the list)
        elif outcome == "ARC_SHORT":
            assert at is None and s <= 0 and meta["L"] == 8 and cell is not None, tag
        elif outcome == "AT_THRESHOLD":
            assert at is None and s == meta["th"] and meta["th"] in (fr.ini, fr.mn) and cell is not None, tag
            assert meta["th"] == fr.ini or (meta["th"] == lo and fact[cell]["second_pass"]), tag
        elif outcome == "OUT_OF_BAND":
            assert at is None and s > fr.ini and cell is None, tag
        elif outcome == "WEAK_DROPPED":
            assert at is None and fr.mn < s <= fr.ini and fact[cell]["n"] > 0 and not fact[cell]["second_pass"], tag
        else:
            raise AssertionError(tag)


@pytest.mark.parametrize("geom", list(fc.GEOMS))
def test_model_and_oracle_meet_every_declaration_and_agree(geom):
    model, oracle = fc.model_results(geom), fc.oracle_results(geom)
    for fr in fc.frames(geom):
        mx, my, ms, facts = model[fr.name]
        ox, oy, os_ = oracle[fr.name]
        for a, b, what in ((mx, ox, "x"), (my, oy, "y"), (ms, os_, "score")):
            np.testing.assert_array_equal(a, b, err_msg="%s %s %s" % (geom, fr.name, what))
        _check_declarations(fr, mx, my, ms, facts, lambda x, y: fm.arc_score(fr.img, x + 16, y + 16), "model")
        _check_declarations(fr, ox, oy, os_, facts, lambda x, y: ob.fast_arc_score(fr.img, x + 16, y + 16), "oracle")


@pytest.mark.parametrize("geom", list(fc.GEOMS))
def test_outcome_ledger(geom):
    """what the rows of a geometry must bring about, counted from the declarations (which the test above holds true)"""
    g, rows = fc.GEOMS[geom], fc.GEOMS[geom]["rows"]
    decl = [(fr, d) for fr in fc.frames(geom) for d in fr.decl]
    seen = {d[2] for _, d in decl}
    want = {"OUT_OF_BAND"} | ({"KEPT"} if "seams" in rows else set())
    if "arcs" in rows:
        want |= {"KEPT", "ARC_SHORT"}
        arcs = [d for fr, d in decl if fr.row == "arcs"]
        for pol in (1, -1):
            kept = [d for d in arcs if d[4]["pol"] == pol and d[2] == "KEPT"]
            assert {d[4]["weakest"] for d in kept} == set(range(16)), (geom, pol)
            assert {d[4]["weakest"] for d in kept if d[4]["L"] == 9} == set(range(16)), (geom, pol)
            for L in (8, 9, 10, 15, 16):
                assert {d[4]["start"] for d in arcs if d[4]["pol"] == pol and d[4]["L"] == L and (d[2] == "ARC_SHORT") == (L == 8)} == set(range(16))
            assert any(d[4]["start"] + d[4]["L"] > 16 for d in kept)              # arcs that wrap past ring index 15
    if "thresholds" in rows:
        want |= {"AT_THRESHOLD", "WEAK_KEPT"}
        for ini, mn in fc.PARAMS:
            th = [d for fr, d in decl if fr.row == "thresholds" and (fr.ini, fr.mn) == (ini, mn)]
            assert any(d[2] == "AT_THRESHOLD" and d[4]["th"] == ini for d in th) and any(d[2] == "KEPT" and d[3] == ini for d in th)
            assert sum(d[2] == "KEPT" and d[3] == 254 for d in th) >= 2
            if mn < ini:
                assert any(d[2] == "AT_THRESHOLD" and d[4]["th"] == mn for d in th) and any(d[2] == "WEAK_KEPT" and d[3] == mn for d in th)
    if "nms" in rows:
        want |= {"NMS_LOST"}
        prs = [(fr, d) for fr, d in decl if fr.row == "nms"]
        dirs = {(i, j) for j in (-1, 0, 1) for i in (-1, 0, 1) if i or j}
        assert {d[4]["dir"] for _, d in prs if d[2] == "KEPT"} == dirs                                  # the neighbour in that direction is lower
        assert {d[4]["dir"] for _, d in prs if d[2] == "NMS_LOST" and d[4]["rel"] == "gt"} == dirs    # ... higher (seen from B: the opposite one)
        assert {d[4]["dir"] for _, d in prs if d[2] == "NMS_LOST" and d[4]["rel"] == "eq"} == dirs    # ... equal
        # horizontal neighbours: the two pixels of one pixel pair, and the two across a pair boundary
        same = set()
        for fr, (x, y, outcome, score, meta) in prs:
            if meta["who"] == "A" and meta["dir"][1] == 0:
                ci, cj = fc.cell_of(g, x, y)
                same.add((meta["rel"], (x + min(0, meta["dir"][0]) - fc.band(g, ci, cj)[0]) % 2 == 0))
        assert same >= {("gt", True), ("gt", False), ("eq", True), ("eq", False)}, (geom, same)
    if "retry" in rows:
        want |= {"WEAK_KEPT", "WEAK_DROPPED"}
    if "seams" in rows:
        ncols, nrows = g["grid"][:2]
        lives = fc.live_cells(g)
        first_last = set()
        for fr, (x, y, outcome, score, meta) in decl:
            if fr.name == "edges":
                x0, y0, dw, dh = fc.band(g, *fc.cell_of(g, x, y))
                first_last |= {w for w, hit in (("col0", x == x0), ("colN", x == x0 + dw - 1), ("row0", y == y0), ("rowN", y == y0 + dh - 1)) if hit}
                assert outcome == "KEPT"
        assert first_last == {"col0", "colN", "row0", "rowN"}
        across = {(d[4]["rel"], d[4]["dir"]) for fr, d in decl if fr.name.startswith(("seam_", "corner_"))}
        need = set()
        if any((ci, cj + 1) in lives for ci, cj in lives):
            need |= {(1, 0), (-1, 0)}
        if any((ci + 1, cj) in lives for ci, cj in lives):
            need |= {(0, 1), (0, -1)}
        if len(need) == 4:
            need |= {(1, 1), (1, -1), (-1, 1), (-1, -1)}
        assert across == {(rel, d) for rel in ("gt", "eq") for d in need}, (geom, across)
    if any(fc.band(g, ci, cj)[2] % 2 for ci, cj in fc.live_cells(g)) and ("seams" in rows or "outside" in rows):
        # the last column of an odd band (kept) and the pixel just past it (never reported)
        odd = [(ci, cj) for ci, cj in fc.live_cells(g) if fc.band(g, ci, cj)[2] % 2 and (ci, cj + 1) not in fc.live_cells(g)]
        ends = {fc.band(g, ci, cj)[0] + fc.band(g, ci, cj)[2] for ci, cj in odd}
        assert any(d[2] == "OUT_OF_BAND" and d[0] in ends for _, d in decl) and any(d[2] == "KEPT" and d[0] + 1 in ends for _, d in decl)
    assert seen >= want, (geom, want - seen)
    if rows == fc.ALL_ROWS:
        assert seen == set(fc.OUTCOMES), geom
    # a strong corner in the band every skipped cell would have had
    for ci in range(g["grid"][1]):
        for cj in range(g["grid"][0]):
            if (ci, cj) not in fc.live_cells(g) and (cj % 2 == 0 or cj == g["grid"][0] - 1):
                x0, y0 = cj * g["grid"][2] + 3, ci * g["grid"][3] + 3
                assert any(d[2] == "OUT_OF_BAND" and x0 <= d[0] < x0 + 20 and y0 <= d[1] < y0 + 20 for _, d in decl), (geom, ci, cj)


def test_load_frames_fill_the_queue_and_the_lists():
    """What the load row does, by the model: the ramp fills the necessary-test queue of every cell to its capacity dh * npb (salt and pepper
    does not: about half); the densest lattice is the dots of period 4, one candidate per 4 x 4 pixels."""
    for geom, g in fc.GEOMS.items():
        if "load" not in g["rows"]:
            continue
        res = fc.model_results(geom)
        live = lambda name: [f for f in res[name][3] if not f["skipped"]]
        assert all(f["nq"][0] == f["dh"] * f["npb"] for f in live("ramp")), geom
        assert all(f["nq"][0] < f["dh"] * f["npb"] for f in live("salt")), geom
        assert max(f["nq"][0] for f in live("salt")) > 64
        dens = {fr.name: len(res[fr.name][0]) for fr in fc.frames(geom) if fr.row == "load" and fr.name != "ramp" and fr.name != "salt"}
        assert max(dens, key=dens.get) == "dots44" and dens["dots44"] > 0, (geom, dens)
