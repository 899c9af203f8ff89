"""The blurred pyramid in tiles of 16 x 8 pixels (the matrix-core blur writes them, k_orient_desc_tiled reads them) against the
row-major layout of the same build (ORBHIP_BLUR_TILED=0) and against the oracle, bit for bit.  Batch 16 with ORBHIP_BLUR_MFMA=1 is the
smallest batch that reaches the matrix-core blur.

Geometries: VGA; a level 0 whose width is 1 (mod 16) and whose height is 1 (mod 8), so that the last tile column / row of level 0 hold one
pixel column / row; and the small end of test_extract_random_geometries (tests/test_gpu_orb.py).  Its draw rule allows 75 x 61 at one
level, which the extractor rejects (61 rows are one short of a FAST cell: (h - 16) - 16 < 30), so the smallest size it can draw AND extract
is 75 x 62; the smallest its seed does draw, 169 x 143 at two levels of 1.17, is taken as well.

The oracle runs once per geometry (module fixture) and is shared by the tests."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 16
GEOMETRIES = {
    #            w    h   nfeat scale nlev ini min  seed
    "vga":      (640, 480, 1000, 1.2, 8, 20, 7, 11),
    "mod1":     (369, 281, 600, 1.2, 8, 20, 7, 5),
    "rule_min": (75, 62, 100, 1.2, 1, 20, 7, 3),
    "drawn_min": (169, 143, 1375, 1.17, 2, 19, 6, 9),
}
LAP = (100, 300)


class _Env:
    """environment for the extractors made inside (the switches are read when an extractor reserves)"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle(name):
    """oracle results of a geometry's 16 frames: final output per frame, level keypoints (level coordinates) of all frames, blur of frame 0"""
    import orbhip
    import oracle_bind as ob
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    imgs = orbhip.synth_frames(w, h, B, seed=seed)
    ora = ob.OracleExtractor(nfeat, scale, nlev, ini, mn)
    out, lvl_xy, blur0 = [], [[] for _ in range(nlev)], None
    for f in range(B - 1, -1, -1):                     # frame 0 last: its blurred levels stay in the oracle
        out.append(ora.extract(imgs[f], LAP))
        for l in range(nlev):
            k = ora.level_keypoints(l)
            lvl_xy[l].append(np.stack([np.rint(k["x"]).astype(np.int64), np.rint(k["y"]).astype(np.int64)], 1))
    blur0 = [ora.blurred_level(l) for l in range(nlev)]
    return dict(imgs=imgs, out=out[::-1], lvl_xy=[np.concatenate(v) for v in lvl_xy], blur0=blur0)


def _run(gpu_ctx, name, imgs, tiled):
    """one batch-16 call with the matrix-core blur, tiled or row-major: final output and the blurred levels of frames 0 and 15"""
    import orbhip
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    with _Env(ORBHIP_BLUR_MFMA="1", ORBHIP_BLUR_TILED=None if tiled else "0", ORBHIP_ROWS_MIN_BATCH=None):
        ext = orbhip.Extractor(gpu_ctx, nfeat, scale, nlev, ini, mn)
        got = ext.extract_host(imgs, LAP)
        assert ext.blur_kernel(B) == "k_blur_mfma" and ext.blur_tiled(B) == tiled and not ext.blur_tiled(1)
        blur = {f: [ext.blurred_level(f, l) for l in range(nlev)] for f in (0, B - 1)}
        dims = [ext.level_dims(l) for l in range(nlev)]
        ext.close()
    return dict(got=got, blur=blur, dims=dims)


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            o = _oracle(name)
            cache[name] = dict(ora=o, tiled=_run(gpu_ctx, name, o["imgs"], True), rows=_run(gpu_ctx, name, o["imgs"], False))
        return cache[name]
    return get


def _same(a, b):
    return a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def coverage(per_geometry):
    """per_geometry: [(level dims [(w, h)], level keypoints [(n, 2) x y])].  What of the tiled staging the keypoints exercise."""
    rx, ry, ncols, edges = set(), set(), set(), set()
    for dims, lvl_xy in per_geometry:
        for (w, h), xy in zip(dims, lvl_xy):
            if not len(xy):
                continue
            x, y = xy[:, 0], xy[:, 1]
            tiles_x, tiles_y = (w + 15) // 16, (h + 7) // 8
            rx |= set(((x - 18) % 16).tolist()); ry |= set(((y - 18) % 8).tolist())
            ncols |= set((((x + 18) >> 4) - ((x - 18) >> 4) + 1).tolist())
            if (((x - 18) >> 4) == 0).any(): edges.add("first tile column")
            if (((x + 18) >> 4) == tiles_x - 1).any(): edges.add("last tile column")
            if (((y - 18) >> 3) == 0).any(): edges.add("first tile row")
            if (((y + 18) >> 3) == tiles_y - 1).any(): edges.add("last tile row")
    return rx, ry, ncols, edges


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_blurred_levels_are_the_same_bytes(runs, name):
    """(a) get_blurred_level, frames 0 and 15, every level: tiled == row-major; frame 0 == the oracle's blur"""
    r = runs(name)
    for f in (0, B - 1):
        for l, (t, q) in enumerate(zip(r["tiled"]["blur"][f], r["rows"]["blur"][f])):
            assert t.shape == q.shape and t.tobytes() == q.tobytes(), "frame %d level %d: tiled vs row-major" % (f, l)
    checked = 0
    for l, ob_ in enumerate(r["ora"]["blur0"]):
        if ob_ is not None:                                # the oracle blurs the levels that have keypoints
            np.testing.assert_array_equal(r["tiled"]["blur"][0][l], ob_, err_msg="blur L%d vs oracle" % l)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_keypoints_angles_descriptors_are_bit_equal(runs, name):
    """(b) final keypoints (angles inside), descriptors and the return value: tiled == oracle == row-major, all 16 frames; and the inputs
    of the four geometries together exercise every alignment of the tiled staging (seeds chosen on the CPU with the oracle)"""
    r = runs(name)
    n = 0
    for f in range(B):
        assert _same(r["tiled"]["got"][f], r["ora"]["out"][f]), "frame %d: tiled vs oracle" % f
        assert _same(r["tiled"]["got"][f], r["rows"]["got"][f]), "frame %d: tiled vs row-major" % f
        n += len(r["ora"]["out"][f][0])
    assert n > 0
    rx, ry, ncols, edges = coverage([(runs(g)["tiled"]["dims"], runs(g)["ora"]["lvl_xy"]) for g in GEOMETRIES])
    print("keypoints %d; x residues %d, y residues %d, tile columns %s, %s" % (n, len(rx), len(ry), sorted(ncols), sorted(edges)))
    assert rx == set(range(16)) and ry == set(range(8))
    assert ncols == {3, 4}
    assert edges == {"first tile column", "last tile column", "first tile row", "last tile row"}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_one_extractor_switches_layout_with_the_batch(gpu_ctx, runs, name):
    """(c) one extractor: 16 frames (tiles), 1 frame (row-major, the LDS tile blur), 16 again -- every call equals the oracle"""
    import orbhip
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    o = runs(name)["ora"]
    with _Env(ORBHIP_BLUR_MFMA="1", ORBHIP_BLUR_TILED=None, ORBHIP_ROWS_MIN_BATCH=None):
        ext = orbhip.Extractor(gpu_ctx, nfeat, scale, nlev, ini, mn)
        for batch in (B, 1, B):
            got = ext.extract_host(o["imgs"][:batch], LAP)
            assert ext.blur_tiled(batch) == (batch == B)
            for f in range(batch):
                assert _same(got[f], o["out"][f]), "batch %d frame %d" % (batch, f)
            for l, ob_ in enumerate(o["blur0"]):
                if ob_ is not None:
                    np.testing.assert_array_equal(ext.blurred_level(0, l), ob_, err_msg="batch %d blur L%d" % (batch, l))
        ext.close()
