"""The row-streaming pyramid kernel walks SOURCE rows (one horizontal pass per source row, the previous row kept in registers) in bands
of `resize_band_rows` output rows and a fixed number of steps; the matrix-core blur keeps its accumulators' start values in registers.
Every pyramid level and every blurred level must equal the oracle's byte for byte on geometries that hit the schedule's corners.  The
descriptor kernel is unchanged; its test pins down what it does with groups of 4 slots that a level's keypoint count fills only partly."""
import numpy as np
import pytest

gpu = pytest.mark.gpu             # per test: the geometry picks are checked without a GPU

RS_STEPS = 24            # ORB_RS_STEPS (csrc/orb_internal.h)


# ---- a mirror of the host tables, used only to PICK geometries; the test asserts it against the library (level_dims, resize_band_rows)
def _level_sizes(n, scale, nlevels):
    s, out = np.float32(1.0), []
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(scale))
        out.append(int(np.rint(np.float32(n) * (np.float32(1.0) / s))))
    return out


def _rows(sn, dn):
    """(row0, row1) per output row: cv::resize INTER_LINEAR, clamped as the kernel's table clamps them"""
    sc = 1.0 / (float(dn) / sn)
    out = []
    for d in range(dn):
        s = int(np.floor(np.float32((d + 0.5) * sc - 0.5)))
        out.append((min(max(s, 0), sn - 1), min(max(s + 1, 0), sn - 1)))
    return out


def _steps(rows, y0, y1):
    n, prev = 0, -1
    for r0, r1 in rows[y0:y1]:
        if n == 0 or prev != r0:
            n += 1
        n += 1
        prev = r1
    return n


def _band_rows(sn, dn):
    rows = _rows(sn, dn)
    for rsr in range(RS_STEPS - 1, 1, -1):
        if all(_steps(rows, y0, min(y0 + rsr, dn)) <= RS_STEPS for y0 in range(0, dn, rsr)):
            return rsr
    return 1


def _level1(h, scale=1.2):
    dn = _level_sizes(h, scale, 2)[1]
    return dn, _band_rows(h, dn), _rows(h, dn)


def _find_height(pred, lo=240, hi=420):
    for h in range(lo, hi):
        dn, rsr, rows = _level1(h)
        if pred(dn, rsr, rows):
            return h
    raise AssertionError("no height with the wanted property")


def _boundary_after_jump(dn, rsr, rows):
    """a band starts on an output row whose first source row advanced by 2 (nothing shared with the row before)"""
    return any(rows[y][0] - rows[y - 1][0] == 2 for y in range(rsr, dn, rsr))


H_JUMP = _find_height(_boundary_after_jump)
H_LAST1 = _find_height(lambda dn, rsr, rows: dn % rsr == 1)
H_LASTM1 = _find_height(lambda dn, rsr, rows: dn % rsr == rsr - 1)


def _mk(gpu_ctx, nfeat, scale, nlev):
    import orbhip
    import oracle_bind as ob
    return orbhip.Extractor(gpu_ctx, nfeat, scale, nlev, 20, 7), ob.OracleExtractor(nfeat, scale, nlev, 20, 7)


def _check_mirror(ext, w, h, scale, nlev):
    ws, hs = _level_sizes(w, scale, nlev), _level_sizes(h, scale, nlev)
    for l in range(nlev):
        assert ext.level_dims(l) == (ws[l], hs[l]), "level %d size" % l
    for l in range(1, nlev):
        got = ext.resize_band_rows(l)
        assert got > 0, "level %d does not take the row-streaming kernel" % l
        assert got == _band_rows(hs[l - 1], hs[l]), "level %d band rows" % l


def _compare_levels(ext, ora, imgs, frames, padded_levels=()):
    for f in frames:
        ora.extract(imgs[f])
        for l in range(ext.nlevels):
            np.testing.assert_array_equal(ext.pyramid_level(f, l), ora.pyramid_level(l), err_msg="pyramid frame %d L%d" % (f, l))
        for l in padded_levels:
            np.testing.assert_array_equal(ext.pyramid_level(f, l, padded=True), ora.pyramid_level(l, padded=True), err_msg="padded frame %d L%d" % (f, l))
        nb = 0
        for l in range(ext.nlevels):
            ob_ = ora.blurred_level(l)
            if ob_ is not None:
                np.testing.assert_array_equal(ext.blurred_level(f, l), ob_, err_msg="blur frame %d L%d" % (f, l))
                nb += 1
        assert nb > 0


GEOMETRIES = [
    # w, h, scale, levels, batch, blur ("rows" / "mfma")
    (640, H_JUMP, 1.2, 8, 2, "rows"),            # a band boundary on a row that shares nothing with the row before
    (641, H_LAST1, 1.2, 8, 2, "mfma"),           # last band of level 1: one row;           w % 4 == 1
    (642, H_LASTM1, 1.2, 8, 2, "rows"),          # last band of level 1: band rows - 1;      w % 4 == 2
    (643, 481, 1.2, 8, 2, "mfma"),               # w % 4 == 3
    (752, 480, 1.2, 8, 2, "mfma"),
    (752, 480, 1.2, 12, 2, "rows"),
    (752, 480, 1.1, 8, 2, "rows"),
    (752, 480, 1.1, 12, 2, "mfma"),
    (752, 480, 1.44, 5, 2, "rows"),              # (8 levels at 1.44 leave a VGA-sized top level smaller than one FAST cell)
    (512, 512, 1.2, 8, 2, "mfma"),
    (1920, 1080, 1.2, 8, 2, "rows"),
    (1920, 1080, 1.44, 8, 1, "mfma"),
    (3840, 2160, 1.2, 8, 1, "rows"),
    (3840, 2160, 1.44, 8, 1, "rows"),
    (3600, 3600, 1.44, 12, 1, "rows"),           # 12 levels at 1.44 shrink 55 times: only an image this tall keeps a FAST cell at the top
]


@gpu
@pytest.mark.parametrize("w,h,scale,nlev,batch,blur", GEOMETRIES)
def test_pyramid_and_blur_levels_match_oracle(gpu_ctx, w, h, scale, nlev, batch, blur, monkeypatch):
    import orbhip
    monkeypatch.setenv("ORBHIP_ROWS_MIN_BATCH", "1")                 # the row-streaming kernels at any batch
    monkeypatch.setenv("ORBHIP_BLUR_MFMA", "1" if blur == "mfma" else "0")
    ext, ora = _mk(gpu_ctx, 1000, scale, nlev)
    imgs = orbhip.synth_frames(w, h, batch, seed=7000 + w + h + nlev)
    ext.extract_host(imgs)
    assert ext.blur_kernel(batch) == ("k_blur_mfma" if blur == "mfma" else "k_blur_rows")
    _check_mirror(ext, w, h, scale, nlev)
    _compare_levels(ext, ora, imgs, range(batch), padded_levels=(0, 1, nlev - 1))
    gpu_ctx.check_status()
    ext.close()


def test_corner_geometries_are_corners():
    """the heights picked above have the properties they were picked for (level 1, scale 1.2)"""
    dn, rsr, rows = _level1(H_JUMP)
    assert _boundary_after_jump(dn, rsr, rows)
    assert _level1(H_LAST1)[0] % _level1(H_LAST1)[1] == 1
    assert _level1(H_LASTM1)[0] % _level1(H_LASTM1)[1] == _level1(H_LASTM1)[1] - 1
    assert {g[0] % 4 for g in GEOMETRIES} == {0, 1, 2, 3}
    # at most one output row completes per source-row step, and a band never needs more steps than the kernel walks
    for sn, dn in ((480, 400), (H_JUMP, _level1(H_JUMP)[0]), (1080, 750), (2160, 1500)):
        rows, rsr = _rows(sn, dn), _band_rows(sn, dn)
        assert max(_steps(rows, y0, min(y0 + rsr, dn)) for y0 in range(0, dn, rsr)) <= RS_STEPS


@gpu
@pytest.mark.parametrize("batch", [16, 128])
def test_default_kernels_at_their_batch_thresholds(gpu_ctx, batch):
    """defaults: 16 frames is where the row-streaming kernels start, 128 where the matrix-core blur does (VGA)"""
    import orbhip
    ext, ora = _mk(gpu_ctx, 1000, 1.2, 8)
    imgs = orbhip.synth_frames(640, 480, batch, seed=90 + batch)
    ext.extract_host(imgs)
    assert ext.blur_kernel(batch) == ("k_blur_mfma" if batch >= 128 else "k_blur_rows")
    _check_mirror(ext, 640, 480, 1.2, 8)
    frames = range(batch) if batch <= 16 else [0, 1, 7, 8, 63, 64, 100, 126, 127]      # the oracle runs on the CPU: a spread of a large batch
    _compare_levels(ext, ora, imgs, frames, padded_levels=(1,))
    gpu_ctx.check_status()
    ext.close()


@gpu
@pytest.mark.parametrize("w,h,stride", [(640, 480, 704), (333, 277, 336), (322, H_LAST1, 328)])
def test_level0_in_the_callers_buffer(gpu_ctx, w, h, stride):
    """extract_device with a row stride wider than the width: level 0 IS the caller's buffer (stride % 4 == 0, nothing staged), level 1
    is resized straight from it; the same frames through the extractor's own level-0 buffer give the same bytes"""
    import torch
    import orbhip
    B = 16
    ext, ora = _mk(gpu_ctx, 600, 1.2, 8)
    imgs = orbhip.synth_frames(w, h, B, seed=3 + w)
    ext.extract_host(imgs)                                              # level 0 in the extractor's own buffer
    own = [[ext.pyramid_level(f, l).copy() for l in range(8)] + [ext.blurred_level(f, l).copy() for l in range(8)] for f in (0, B - 1)]
    _compare_levels(ext, ora, imgs, (0, 5, B - 1))
    buf = np.full((B, h, stride), 0xA5, np.uint8)                       # the bytes between the rows are not image
    buf[:, :, :w] = imgs
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    ext.extract_device(d.data_ptr(), w, h, stride, stride * h, B, (0, 1000))
    gpu_ctx.synchronize()
    _check_mirror(ext, w, h, 1.2, 8)
    _compare_levels(ext, ora, imgs, (0, 5, B - 1), padded_levels=(0, 1))
    for i, f in enumerate((0, B - 1)):
        lv = [ext.pyramid_level(f, l) for l in range(8)] + [ext.blurred_level(f, l) for l in range(8)]
        for a, b in zip(own[i], lv):
            np.testing.assert_array_equal(a, b)
    gpu_ctx.check_status()
    del d
    ext.close()


@gpu
@pytest.mark.parametrize("w,h,nfeat,batch", [(640, 480, 997, 3), (640, 480, 1203, 16), (333, 277, 301, 16), (752, 480, 1501, 5)])
def test_descriptors_and_angles_with_partly_filled_slot_groups(gpu_ctx, w, h, nfeat, batch):
    """k_orient_desc works on groups of 4 slots; the slots past a level's count do no staging and store nothing.  Frames whose per-level
    counts are no multiples of 4: angles, descriptors and the final arrays equal the oracle's (a regression test of that kernel)."""
    import orbhip
    ext, ora = _mk(gpu_ctx, nfeat, 1.2, 8)
    imgs = orbhip.synth_frames(w, h, batch, seed=500 + nfeat)
    got = ext.extract_host(imgs, (0, 1000))
    ragged = 0
    for f in range(batch):
        kp, desc, mono = ora.extract(imgs[f], (0, 1000))
        for l in range(8):
            gk, ok = ext.level_keypoints(f, l), ora.level_keypoints(l)
            assert len(gk) == len(ok), "count frame %d L%d" % (f, l)
            ragged += len(ok) % 4 != 0
            assert gk["angle"].tobytes() == ok["angle"].tobytes(), "angle bits frame %d L%d" % (f, l)
            assert gk.tobytes() == ok.tobytes(), "level keypoints frame %d L%d" % (f, l)
        gk, gd, gm = got[f]
        assert gm == mono and len(gk) == len(kp)
        assert gk.tobytes() == kp.tobytes(), "final keypoints frame %d" % f
        assert gd.tobytes() == desc.tobytes(), "final descriptors frame %d" % f
    assert ragged >= batch, "the frames do not stress partly filled slot groups (%d ragged levels)" % ragged
    gpu_ctx.check_status()
    ext.close()
