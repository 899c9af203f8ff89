"""Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1128-1168) on the device: through the host class (host_smoke stereofe, the
stereo-fisheye constructor's sequence), through the batched device form on extractor results, and on crafted arrays -- all bit-exact
against the oracle composition of tests/test_stereo_fisheye_oracle.py."""
import numpy as np
import pytest

from test_gpu_host_kf import run_smoke
from test_stereo_fisheye_oracle import RIG, F32, crafted_case, fisheye_oracle, level_sigma2

pytestmark = pytest.mark.gpu


def _kb8_unproject_vec(cam, u, v):
    """KannalaBrandt8::unproject in double, vectorised (for building the warped views only)"""
    p = cam.astype(np.float64)
    pwx, pwy = (u - p[2]) / p[0], (v - p[3]) / p[1]
    td = np.clip(np.hypot(pwx, pwy), 0, np.pi / 2)
    th = td.copy()
    for _ in range(10):
        t2 = th * th
        th = th - (th * (1 + p[4] * t2 + p[5] * t2 ** 2 + p[6] * t2 ** 3 + p[7] * t2 ** 4) - td) / (1 + 3 * p[4] * t2 + 5 * p[5] * t2 ** 2 + 7 * p[6] * t2 ** 3 + 9 * p[7] * t2 ** 4)
    sc = np.where(td > 1e-8, np.tan(th) / np.maximum(td, 1e-12), 1.0)
    return np.stack([pwx * sc, pwy * sc, np.ones_like(pwx)], -1)


def warp_right(left, plane_z):
    """The right view of the rig looking at the left image painted on the plane Z = plane_z of the left camera (bilinear)."""
    import oracle_match_bind as om
    H, W = left.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = _kb8_unproject_vec(RIG["cam2"], u, v) @ RIG["Rlr"].astype(np.float64).T           # right ray in the left frame
    t = RIG["tlr"].astype(np.float64)
    s = (plane_z - t[2]) / np.where(np.abs(ray[..., 2]) > 1e-9, ray[..., 2], 1e-9)
    X = s[..., None] * ray + t
    uv = om.kb8_project_np((1, RIG["cam1"].astype(np.float64)), X)
    x, y = uv[..., 0], uv[..., 1]
    ok = (s > 0) & (x >= 0) & (y >= 0) & (x < W - 1) & (y < H - 1) & (np.abs(ray[..., 2]) > 0.2)
    x0, y0 = np.clip(np.floor(x).astype(int), 0, W - 2), np.clip(np.floor(y).astype(int), 0, H - 2)
    fx, fy = np.clip(x - x0, 0, 1), np.clip(y - y0, 0, 1)
    L = left.astype(np.float64)
    val = (L[y0, x0] * (1 - fx) * (1 - fy) + L[y0, x0 + 1] * fx * (1 - fy) + L[y0 + 1, x0] * (1 - fx) * fy + L[y0 + 1, x0 + 1] * fx * fy)
    return np.ascontiguousarray(np.where(ok, np.clip(np.rint(val), 0, 255), 128).astype(np.uint8))


def _rig_arrays():
    return dict(types=np.array(RIG["types"], np.int32), cams=np.concatenate([RIG["cam1"], RIG["cam2"]]).astype(F32),
                Tlr=np.ascontiguousarray(RIG["Tlr"], F32).reshape(-1))


# left lapping, right lapping, right image kind, floor of kept matches (CPU oracle rehearsal of the same inputs)
CASES = [((0, 511), (0, 511), "warp", 150), ((100, 400), (120, 420), "warp", 120), ((0, 511), (0, 511), "unrelated", 0), ((0, 511), (0, 511), "flat", 0)]


@pytest.mark.parametrize("lapL,lapR,kind,floor", CASES)
def test_frame_compute_stereo_fisheye_matches_drop_in(tmp_path, lapL, lapR, kind, floor):
    """Frame::ComputeStereoFishEyeMatches() through the class in the constructor's sequence (:1049-1097): mvKeys as the oracle extracts
    them, mvLeftToRightMatch / mvRightToLeftMatch / mvDepth bytes and mvStereo3Dpoints (3 x 1 float exactly where l2r >= 0) equal to
    the oracle composition, mvuRight all -1, a second call repeats it, a frame whose extractor moved on is refused loudly."""
    import oracle_bind as ob
    import orbhip
    W = H = 512
    nfeat = 1000
    left = orbhip.synth_frames(W, H, 1, seed=5120)[0]
    if kind == "warp":
        right = warp_right(left, 2.7)
    elif kind == "unrelated":
        right = orbhip.synth_frames(W, H, 1, seed=777)[0]
    else:
        right = np.full((H, W), 128, np.uint8)
    out = run_smoke("stereofe", tmp_path, dict(dims=np.array([W, H, nfeat], np.int32), left=left.reshape(-1), right=right.reshape(-1),
                                               lap=np.array(list(lapL) + list(lapR), np.int32), **_rig_arrays()), "HOST_STEREOFE_OK")
    eL = ob.OracleExtractor(nfeat, 1.2, 8, 20, 7); eR = ob.OracleExtractor(nfeat, 1.2, 8, 20, 7)
    kpL, dL, mL = eL.extract(left, lapL); kpR, dR, mR = eR.extract(right, lapR)
    assert out["n"][0] == len(kpL) and out["nr"][0] == len(kpR)
    assert list(out["mono"]) == [mL, mR]
    assert out["kpx"].tobytes() == kpL["x"].tobytes() and out["kpy"].tobytes() == kpL["y"].tobytes()
    np.testing.assert_array_equal(out["kpo"], kpL["octave"])
    l2r, r2l, depth, x3d, n, desc = fisheye_oracle(kpL, dL, mL, kpR, dR, mR, RIG, level_sigma2())
    assert out["l2r"].tobytes() == l2r.tobytes()
    assert out["r2l"].tobytes() == r2l.tobytes()
    assert out["depth"].tobytes() == depth.tobytes()
    np.testing.assert_array_equal(out["has3d"], (l2r >= 0).astype(np.int32))
    assert out["x3d"].tobytes() == x3d.reshape(-1).tobytes()
    assert (out["uright"] == -1).all() and len(out["uright"]) == len(kpL)
    assert out["close"][0] == 0
    assert out["same"][0] == 1
    assert out["stale"][0] == 1, out["_log"][-800:]
    assert "not the latest extractions" in out["_log"]
    if kind == "warp":
        assert n > floor and desc > n, (n, desc)                      # real matches triangulate; the triangulation rejects some
        if lapL[0] > 0:
            assert mL > 0 and mR > 0
    else:
        assert n == 0, n
        if kind == "unrelated":
            assert desc > 0                                           # descriptor matches exist and the triangulation rejects them all


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_device(gpu_ctx, left, right, batch, max_n, sigma2):
    """left / right = (d_kp, d_desc, d_n, d_mono, stride).  Returns host (l2r, r2l, depth, x3d, n)."""
    import torch
    import orbhip
    l2r = torch.full((batch, max_n), -7, dtype=torch.int32, device="cuda"); r2l = torch.full((batch, max_n), -7, dtype=torch.int32, device="cuda")
    depth = torch.full((batch, max_n), -7.0, dtype=torch.float32, device="cuda"); x3d = torch.full((batch, max_n, 3), -7.0, dtype=torch.float32, device="cuda")
    nm = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.compute_stereo_fisheye_matches_device(gpu_ctx, left, right, batch, max_n, RIG, sigma2, l2r.data_ptr(), r2l.data_ptr(), depth.data_ptr(),
                                                 x3d.data_ptr(), nm.data_ptr())
    gpu_ctx.synchronize()
    gpu_ctx.check_status()                                            # raises on a capacity flag
    return l2r.cpu().numpy(), r2l.cpu().numpy(), depth.cpu().numpy(), x3d.cpu().numpy(), nm.cpu().numpy()


def test_stereo_fisheye_device_batch_of_extractions(gpu_ctx):
    """The batched device form on 32 frame pairs extracted by orbhip_extract_batch_device on two extractors (lapping {0, 511} left,
    {40, 470} right): frame by frame equal to the oracle composition on the oracle's extraction of the same images."""
    import oracle_bind as ob
    import orbhip
    W = H = 512
    B = 32
    lefts = orbhip.synth_frames(W, H, B, seed=9000)
    rights = np.stack([warp_right(lefts[f], 2.0 + 2.0 * f / (B - 1)) if f % 8 != 7 else orbhip.synth_frames(W, H, 1, seed=100 + f)[0] for f in range(B)])
    eL, eR = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7), orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    dl, dr = _dev(lefts), _dev(rights)
    eL.extract_device(dl.data_ptr(), W, H, W, W * H, B, (0, 511))
    eR.extract_device(dr.data_ptr(), W, H, W, W * H, B, (40, 470))
    gpu_ctx.synchronize()
    mk = orbhip.lib.orbhip_extractor_max_keypoints(eL.h)
    assert orbhip.lib.orbhip_extractor_max_keypoints(eR.h) == mk
    kL, dL_, nL, mL = eL.results_device(); kR, dR_, nR, mR = eR.results_device()
    l2r, r2l, depth, x3d, nm = _run_device(gpu_ctx, (kL, dL_, nL, mL, mk), (kR, dR_, nR, mR, mk), B, mk, level_sigma2())
    oL, oR = ob.OracleExtractor(1000, 1.2, 8, 20, 7), ob.OracleExtractor(1000, 1.2, 8, 20, 7)
    total = 0
    for f in range(B):
        kpL, dsL, moL = oL.extract(lefts[f], (0, 511)); kpR, dsR, moR = oR.extract(rights[f], (40, 470))
        el2r, er2l, edp, ex3d, en, _ = fisheye_oracle(kpL, dsL, moL, kpR, dsR, moR)
        nl, nr = len(kpL), len(kpR)
        assert l2r[f, :nl].tobytes() == el2r.tobytes(), f
        assert r2l[f, :nr].tobytes() == er2l.tobytes(), f
        assert depth[f, :nl].tobytes() == edp.tobytes(), f
        assert x3d[f, :nl].tobytes() == ex3d.tobytes(), f
        assert nm[f] == en, (f, nm[f], en)
        assert (l2r[f, nl:] == -1).all() and (r2l[f, nr:] == -1).all() and (depth[f, nl:] == -1).all()
        total += en
    assert total > 16 * 100
    eL.close(); eR.close()


def test_stereo_fisheye_device_crafted_arrays(gpu_ctx):
    """Hand-made keypoints / descriptors: ties, many-to-one picks (r2l takes the HIGHEST left index), right slices of 0, 1 and 2 rows,
    mono offsets on both sides, one frame whose slice is empty on the left; under the matrix-core size (max_n < 64: xor / popcount
    kernel) and above it."""
    import oracle_bind as ob
    for max_n in (48, 96):
        rng = np.random.default_rng(max_n)
        frames = []
        for f in range(8):
            kpL, dL, kpR, dR = crafted_case(rng, n_pts=40)
            monoL, monoR = [(0, 0), (3, 5), (0, 38), (2, 39), (0, 40), (40, 0), (7, 0), (1, 30)][f]
            frames.append((kpL, dL, monoL, kpR, dR, monoR))
        B = len(frames)
        KL = np.zeros((B, max_n), ob.KP_DTYPE); KR = np.zeros((B, max_n), ob.KP_DTYPE)
        DL = np.zeros((B, max_n, 32), np.uint8); DR = np.zeros((B, max_n, 32), np.uint8)
        nL = np.zeros(B, np.int32); nR = np.zeros(B, np.int32); mL = np.zeros(B, np.int32); mR = np.zeros(B, np.int32)
        for f, (kpL, dL, monoL, kpR, dR, monoR) in enumerate(frames):
            KL[f, :len(kpL)] = kpL; DL[f, :len(kpL)] = dL; KR[f, :len(kpR)] = kpR; DR[f, :len(kpR)] = dR
            nL[f], nR[f], mL[f], mR[f] = len(kpL), len(kpR), monoL, monoR
        d = [_dev(a) for a in (KL.view(np.uint8), DL, nL, mL, KR.view(np.uint8), DR, nR, mR)]
        l2r, r2l, depth, x3d, nm = _run_device(gpu_ctx, (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max_n),
                                               (d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), max_n), B, max_n, level_sigma2())
        many = 0
        for f, (kpL, dL, monoL, kpR, dR, monoR) in enumerate(frames):
            el2r, er2l, edp, ex3d, en, _ = fisheye_oracle(kpL, dL, monoL, kpR, dR, monoR)
            assert l2r[f, :40].tobytes() == el2r.tobytes(), (max_n, f)
            assert r2l[f, :40].tobytes() == er2l.tobytes(), (max_n, f)
            assert depth[f, :40].tobytes() == edp.tobytes() and x3d[f, :40].tobytes() == ex3d.tobytes(), (max_n, f)
            assert nm[f] == en, (max_n, f)
            if 40 - monoR < 2 or monoL >= 40:
                assert en == 0
            hits = np.bincount(el2r[el2r >= 0], minlength=40)
            for j in np.flatnonzero(hits > 1):
                many += 1
                assert er2l[j] == np.flatnonzero(el2r == j).max()
        assert many > 0
