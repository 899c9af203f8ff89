"""The descriptor kernels' trip head (count, key and position fetched side by side, the keys in work order written by the octree, the head
of a wave's next trip fetched during the current one) against the oracle, bit for bit: keypoints with angles, descriptors, return value.

Forms: batch 16 with ORBHIP_BLUR_MFMA=1 is the tiled reader, ORBHIP_BLUR_TILED=0 the row-major one; batch 15 has no permutation (the slot
order, no work-order keys); 9 and 17 give the XCDs unequal frame counts; batch 1.  ORBHIP_TUNE_DESC_BLOCKS=1 / 3 caps the grid at 2 / 6 waves
per XCD, so that a wave makes many trips and the carried head is what every trip but the first runs on.

Geometries: the small ones of tests/test_gpu_blur_tiles.py.  The 17 frames of a geometry are synth_frames of its seed with the contrast of
frame f lowered around mid-grey by CONTRAST[f]: the textured frames fill their levels, the flat ones leave levels with a handful of
keypoints or none.  The factors were chosen on the CPU with the oracle (per-level counts of every frame, fed to trip_coverage below with the
slices and wave counts the extractor reports) until `mod1` alone held, at every capped grid, a group beyond its level's count followed by a
valid group in the same wave, a wave that ends on a skipped group, levels of count 0 and of count 1, 2 and 3 (mod 4); the test asserts it.

The oracle runs once per geometry (module fixture) and is shared by the tests."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF = 17
GEOMETRIES = {
    #            w    h   nfeat scale nlev ini min  seed
    "mod1":     (369, 281, 600, 1.2, 8, 20, 7, 5),
    "rule_min": (75, 62, 100, 1.2, 1, 20, 7, 3),
    "drawn_min": (169, 143, 1375, 1.17, 2, 19, 6, 9),
}
CONTRAST = (1.0, 1.0, 0.5, 0.3, 1.0, 0.05, 0.15, 1.0, 0.12, 1.0, 0.04, 0.25, 1.0, 0.03, 0.4, 1.0, 0.02)
LAP = (100, 300)
BATCHES = (16, 15, 9, 17, 1)


def frames_of(name):
    import orbhip
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    imgs = orbhip.synth_frames(w, h, NF, seed=seed).astype(np.float32)
    c = np.asarray(CONTRAST, np.float32)[:, None, None]
    return np.clip(np.rint(128.0 + (imgs - 128.0) * c), 0, 255).astype(np.uint8)


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


def oracle_of(name, imgs):
    """final output and per-level counts of every frame"""
    import oracle_bind as ob
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    ora = ob.OracleExtractor(nfeat, scale, nlev, ini, mn)
    out, counts = [], np.zeros((len(imgs), nlev), np.int64)
    for f in range(len(imgs)):
        out.append(ora.extract(imgs[f], LAP))
        for l in range(nlev):
            counts[f, l] = len(ora.level_keypoints(l))
    return out, counts


def trip_coverage(counts, kp_base, kp_cap, waves, batch):
    """What the trips of a call exercise.  counts[f][l] per-level keypoint counts, kp_base / kp_cap the level slices of a frame's staging slots,
    waves = waves per XCD.  Frame f belongs to XCD f % 8; wave w of an XCD takes groups w, w + waves, ... of (its frames) x (slots / 4); a group
    whose first slot lies at or beyond its level's count is skipped."""
    gpf = int(kp_base[-1] + kp_cap[-1]) // 4
    lvl_of = np.searchsorted(np.asarray(kp_base), 4 * np.arange(gpf), side="right") - 1
    got = set()
    for x in range(8):
        frames = list(range(x, batch, 8))
        for w in range(waves):
            skipped = []
            for q in range(w, len(frames) * gpf, waves):
                fk, g = divmod(q, gpf)
                l = lvl_of[g]
                skipped.append(4 * g - kp_base[l] >= counts[frames[fk]][l])
            if not skipped:
                continue
            if len(skipped) > 1:
                got.add("many trips")
            if any(a and not b for a, b in zip(skipped, skipped[1:])):
                got.add("skipped then valid")
            if any(a and not b for i, a in enumerate(skipped) for b in skipped[i + 1:]):
                got.add("skipped, later valid")
            if skipped[-1] and not all(skipped):
                got.add("ends on a skipped group")
    c = np.asarray(counts)[:batch]
    got |= {"count %d mod 4" % r for r in (1, 2, 3) if ((c % 4) == r).any()}
    if (c == 0).any():
        got.add("count 0")
    return got


WANT = {"many trips", "skipped then valid", "ends on a skipped group", "count 0", "count 1 mod 4", "count 2 mod 4", "count 3 mod 4"}


def _extract(gpu_ctx, name, imgs, tiled=True, cap=None, octree=None):
    """one call per batch size with a fresh extractor: {batch: (results, waves per XCD)}, and the level slices"""
    import orbhip
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    res = {}
    with _Env(ORBHIP_BLUR_MFMA="1", ORBHIP_BLUR_TILED=None if tiled else "0", ORBHIP_ROWS_MIN_BATCH=None, ORBHIP_TUNE_DESC_BLOCKS=cap,
              ORBHIP_OCTREE=octree):
        for batch in BATCHES:
            ext = orbhip.Extractor(gpu_ctx, nfeat, scale, nlev, ini, mn)
            got = ext.extract_host(imgs[:batch], LAP)
            assert ext.blur_tiled(batch) == (tiled and batch >= 16)
            base, capv, waves = ext.desc_plan(batch)
            res[batch] = (got, waves)
            ext.close()
    return res, base, capv


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            imgs = frames_of(name)
            out, counts = oracle_of(name, imgs)
            cache[name] = dict(imgs=imgs, out=out, counts=counts)
        return cache[name]
    return get


def _same(a, b):
    return a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _check(res, out, tag):
    n = 0
    for batch, (got, _) in res.items():
        assert len(got) == batch
        for f in range(batch):
            assert _same(got[f], out[f]), "%s: batch %d frame %d differs from the oracle" % (tag, batch, f)
            n += len(out[f][0])
    assert n > 0
    return n


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "rowmajor"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_forms(gpu_ctx, runs, name, tiled):
    """(1) both readers at batches 16, 15, 9, 17 and 1, the launcher's own grid"""
    r = runs(name)
    res, _, _ = _extract(gpu_ctx, name, r["imgs"], tiled=tiled)
    _check(res, r["out"], "%s %s" % (name, "tiled" if tiled else "row-major"))


@pytest.mark.parametrize("cap", ["1", "3"])
@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "rowmajor"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_many_trips(gpu_ctx, runs, name, tiled, cap):
    """(2) the same batches on 2 and 6 waves per XCD: equal to the oracle (and so to the uncapped run of test_forms); for `mod1` the inputs hold
    every case of the carried head (module docstring), at batch 16 and 17 each"""
    r = runs(name)
    res, base, capv = _extract(gpu_ctx, name, r["imgs"], tiled=tiled, cap=cap)
    _check(res, r["out"], "%s cap %s" % (name, cap))
    for batch, (_, waves) in res.items():
        assert waves <= 2 * int(cap)
        cov = trip_coverage(r["counts"], base, capv, waves, batch)
        print(name, "batch", batch, "waves", waves, sorted(cov))
        if name == "mod1" and batch >= 16:
            assert cov >= WANT, (batch, sorted(WANT - cov))


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "rowmajor"])
def test_stale_work_order_entries(gpu_ctx, runs, tiled):
    """(3) one extractor, one context: textured frames, then frames with far fewer keypoints per level (some levels empty), then the first
    again -- a work-order key or position left by an earlier call must not be used"""
    import orbhip
    name = "mod1"
    w, h, nfeat, scale, nlev, ini, mn, seed = GEOMETRIES[name]
    r = runs(name)
    c = np.asarray(CONTRAST)
    textured = [f for f in range(NF) if c[f] == 1.0]
    flat = [f for f in range(NF) if c[f] <= 0.05]
    order_a = (textured * 3)[:16]
    order_b = (flat * 4)[:16]
    assert r["counts"][order_b].sum() < r["counts"][order_a].sum() // 4 and (r["counts"][order_b] == 0).any()
    assert (r["counts"][order_b].max(0) < r["counts"][order_a].min(0)).all()          # every level shrinks: stale entries lie beyond the count
    with _Env(ORBHIP_BLUR_MFMA="1", ORBHIP_BLUR_TILED=None if tiled else "0", ORBHIP_ROWS_MIN_BATCH=None, ORBHIP_TUNE_DESC_BLOCKS="3",
              ORBHIP_OCTREE=None):
        ext = orbhip.Extractor(gpu_ctx, nfeat, scale, nlev, ini, mn)
        for call, order in enumerate((order_a, order_b, order_a, order_b[:15], order_a)):
            got = ext.extract_host(r["imgs"][order], LAP)
            for i, f in enumerate(order):
                assert _same(got[i], r["out"][f]), "call %d frame %d (input %d)" % (call, i, f)
        ext.close()


def test_iterative_octree_writes_the_work_order_keys(gpu_ctx, runs):
    """(4a) ORBHIP_OCTREE=iterative: k_octree writes the keys in work order too"""
    r = runs("mod1")
    res, _, _ = _extract(gpu_ctx, "mod1", r["imgs"], tiled=True, cap="3", octree="iterative")
    _check(res, r["out"], "iterative octree")


def test_redo_octree_writes_the_work_order_keys(gpu_ctx):
    """(4b) k_octree_redo inside the pipeline (the constructed frames of tests/octree_device_cases.py, 24 VGA frames): every frame equals the
    oracle, tiled reader on 6 waves per XCD"""
    import orbhip
    import oracle_bind as ob
    import octree_device_cases as D
    imgs = D.pipeline_images(orbhip.synth_frames)
    ora = ob.OracleExtractor(1000, 1.2, 8, 20, 7)
    with _Env(ORBHIP_BLUR_MFMA="1", ORBHIP_BLUR_TILED=None, ORBHIP_ROWS_MIN_BATCH=None, ORBHIP_TUNE_DESC_BLOCKS="3", ORBHIP_OCTREE=None):
        ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
        got = ext.extract_host(imgs, (0, 1000))
        assert ext.blur_tiled(len(imgs))
        ext.close()
    for f in range(len(imgs)):
        assert _same(got[f], ora.extract(imgs[f], (0, 1000))), "frame %d" % f
