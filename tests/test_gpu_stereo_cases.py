"""Frame::ComputeStereoMatches on the device (k_stereo_match, k_stereo_median) on the crafted lists of stereo_cases.py: real pyramids,
keypoints / descriptors / counts overwritten in the extractors' device result buffers, mvuRight / mvDepth bit-equal to the C oracle
(which test_stereo_cases.py holds to the plain-Python model on the same frames).  And the dynamic-LDS bound of k_stereo_median."""
import numpy as np
import pytest

import stereo_cases as sc

pytestmark = pytest.mark.gpu
SENT = 7.0


def _pair(ctxL, ctxR, geom, nfeat=sc.NFEAT, scale=1.2):
    import orbhip
    nlev = sc.GEOMS[geom][2]
    return orbhip.Extractor(ctxL, nfeat, scale, nlev, 20, 7), orbhip.Extractor(ctxR, nfeat, scale, nlev, 20, 7)


def _extract(extL, extR, batch, geom):
    """the real extraction underneath (host entry: synchronous), the same on both sides as the oracle's"""
    resL = extL.extract_host(np.stack([fr["left"] for fr in batch]), lap=(0, 0))
    resR = extR.extract_host(np.stack([fr["right"] for fr in batch]), lap=(0, 0))
    for f, fr in enumerate(batch):
        o = sc.oracle_results(geom)[fr["name"]]
        assert resL[f][0].tobytes() == o["realL"][0].tobytes() and resR[f][1].tobytes() == o["realR"][1].tobytes(), fr["name"]
    return resL, resR


def _craft(ctxL, ctxR, extL, extR, batch):
    ctxL.synchronize(); ctxR.synchronize()
    sc.upload_lists(extL, "L", batch); sc.upload_lists(extR, "R", batch)


def _outputs(B, M):
    import torch
    ur = torch.full((B, M), SENT, dtype=torch.float32, device="cuda"); dp = torch.full((B, M), SENT, dtype=torch.float32, device="cuda")
    nk = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return ur, dp, nk


def _stereo(extL, extR, out):
    import orbhip
    orbhip.compute_stereo_matches_device(extL, extR, sc.MB, sc.MBF, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())


def _check(batch, geom, out):
    ur, dp, nk = (t.cpu().numpy() for t in out)
    for f, fr in enumerate(batch):
        o = sc.oracle_results(geom)[fr["name"]]; n = len(fr["kpL"])
        assert nk[f] == o["kept"], (fr["name"], nk[f], o["kept"])
        assert ur[f, :n].tobytes() == o["ur"].tobytes(), fr["name"]
        assert dp[f, :n].tobytes() == o["dp"].tobytes(), fr["name"]
        assert (ur[f, n:] == SENT).all() and (dp[f, n:] == SENT).all(), fr["name"]       # nothing written beyond nL


@pytest.mark.parametrize("geom", list(sc.GEOMS))
def test_crafted_batches_match_the_oracle(gpu_ctx, geom):
    """every crafted frame, in batches in which frames of differing counts (a zero-left and a zero-right one among them) sit side by side"""
    extL, extR = _pair(gpu_ctx, gpu_ctx, geom)
    for batch in sc.batches(geom):
        _extract(extL, extR, batch, geom)
        _craft(gpu_ctx, gpu_ctx, extL, extR, batch)
        out = _outputs(len(batch), extL.max_keypoints)
        _stereo(extL, extR, out)
        gpu_ctx.synchronize()
        _check(batch, geom, out)
    extL.close(); extR.close()


def test_crafted_batch_with_the_right_extractor_on_a_second_context(gpu_ctx):
    import orbhip
    ctxR = orbhip.Context(0)
    extL, extR = _pair(gpu_ctx, ctxR, "qvga8")
    batch = sc.batches("qvga8")[0]
    _extract(extL, extR, batch, "qvga8")
    _craft(gpu_ctx, ctxR, extL, extR, batch)
    out = _outputs(len(batch), extL.max_keypoints)
    _stereo(extL, extR, out)
    gpu_ctx.synchronize(); ctxR.synchronize()
    _check(batch, "qvga8", out)
    extL.close(); extR.close(); ctxR.close()


def test_crafted_two_steps_back_to_back_on_two_contexts(gpu_ctx):
    """Step 0's stereo kernels (left stream) read the crafted right lists and the right pyramid; step 1's extractions are queued right behind
    them with no wait in between, the right one on its own stream: it must wait for those kernels before it overwrites what they read.
    (Step 1's lists can only be crafted once its extraction has finished; both steps are checked.)"""
    import torch
    import orbhip
    ctxR = orbhip.Context(0)
    extL, extR = _pair(gpu_ctx, ctxR, "qvga8")
    b0, b1 = sc.batches("qvga8")
    W, H, _ = sc.GEOMS["qvga8"]; B = len(b0)
    dL = torch.from_numpy(np.stack([fr["left"] for fr in b1])).cuda(); dR = torch.from_numpy(np.stack([fr["right"] for fr in b1])).cuda()
    _extract(extL, extR, b0, "qvga8")
    _craft(gpu_ctx, ctxR, extL, extR, b0)
    out0, out1 = _outputs(B, extL.max_keypoints), _outputs(B, extL.max_keypoints)
    _stereo(extL, extR, out0)                                       # asynchronous ...
    extL.extract_device(dL.data_ptr(), W, H, W, W * H, B, (0, 0))   # ... and the next step's extractions right behind it
    extR.extract_device(dR.data_ptr(), W, H, W, W * H, B, (0, 0))
    _craft(gpu_ctx, ctxR, extL, extR, b1)
    _stereo(extL, extR, out1)
    gpu_ctx.synchronize(); ctxR.synchronize()
    _check(b0, "qvga8", out0); _check(b1, "qvga8", out1)
    extL.close(); extR.close(); ctxR.close()


def test_crafted_lists_after_a_larger_extraction(gpu_ctx):
    """The real extraction finds more keypoints per frame than the crafted lists hold, and a stereo call on it fills the SAD scratch beyond
    the crafted counts: neither the stale keypoints nor the stale SADs may leak into n_kept or the outputs of the crafted call."""
    import oracle_bind as ob
    geom = "qvga8"
    extL, extR = _pair(gpu_ctx, gpu_ctx, geom)
    batch = sc.batches(geom)[0]
    resL, resR = _extract(extL, extR, batch, geom)
    out = _outputs(len(batch), extL.max_keypoints)
    _stereo(extL, extR, out)
    gpu_ctx.synchronize()
    ur, dp, nk = (t.cpu().numpy() for t in out)
    stale = 0
    for f, fr in enumerate(batch):
        o = sc.oracle_results(geom)[fr["name"]]
        kept, ur_ref, dp_ref, _ = ob.compute_stereo_matches(o["eL"], o["eR"], o["realL"][0], o["realL"][1], o["realR"][0], o["realR"][1], sc.MB, sc.MBF)
        n = len(resL[f][0])
        assert n > len(fr["kpL"]) and len(resR[f][0]) > len(fr["kpR"]), fr["name"]             # the previous extraction is the larger one
        assert nk[f] == kept and ur[f, :n].tobytes() == ur_ref.tobytes() and dp[f, :n].tobytes() == dp_ref.tobytes(), fr["name"]
        stale += int((ur_ref[len(fr["kpL"]):] >= 0).sum())
    assert stale > 50                                               # accepted matches (SAD >= 0 in the scratch) beyond the crafted counts
    _craft(gpu_ctx, gpu_ctx, extL, extR, batch)
    out = _outputs(len(batch), extL.max_keypoints)
    _stereo(extL, extR, out)
    gpu_ctx.synchronize()
    _check(batch, geom, out)
    extL.close(); extR.close()


def test_max_keypoints_over_the_lds_bound_is_a_bad_argument(gpu_ctx):
    """k_stereo_median holds one 4-byte key per keypoint slot in LDS: 160 KB minus its static 16 bytes bound max_keypoints to 40956.  The
    extractor's own octree bound (2383 features per level, 16 levels) keeps every extractor it reserves below 38500 today, so the pair
    here is one whose reservation it refused: the stereo entry point names its own bound first, and launches nothing."""
    import torch
    import orbhip
    a, b = _pair(gpu_ctx, gpu_ctx, "qvga8", nfeat=48000)
    for e in (a, b):
        with pytest.raises(orbhip.OrbHipError):
            e.reserve(320, 240, 1)
        assert e.max_keypoints > 40956
    t = torch.zeros(8, dtype=torch.float32, device="cuda")
    with pytest.raises(orbhip.OrbHipError) as ei:
        orbhip.compute_stereo_matches_device(a, b, sc.MB, sc.MBF, t.data_ptr(), t.data_ptr())
    assert ei.value.code == orbhip.E_BADARG and "max_keypoints" in str(ei.value) and "40956" in str(ei.value), str(ei.value)
    a.close(); b.close()


def test_feature_budget_over_64_kb_of_median_keys(gpu_ctx):
    """max_keypoints a little above 16384: k_stereo_median's dynamic LDS passes 64 KB, which the launch has to be opted in to.  At scale
    factor 1.2 the extractor's octree bound stops the budget near 11000 features, so the pyramid here has scale factor 1.02 (8 nearly
    equal levels of the 320 x 240 pair), where 17600 features are accepted."""
    import oracle_bind as ob
    import orbhip
    nfeat, scale = 17600, 1.02
    left, right = sc.shifted_pair(320, 240, 4, 301)
    extL = orbhip.Extractor(gpu_ctx, nfeat, scale, 8, 20, 7); extR = orbhip.Extractor(gpu_ctx, nfeat, scale, 8, 20, 7)
    resL = extL.extract_host(left[None], lap=(0, 0)); resR = extR.extract_host(right[None], lap=(0, 0))
    M = extL.max_keypoints
    assert 16384 < M <= 40956, M
    eL = ob.OracleExtractor(nfeat, scale, 8, 20, 7); eR = ob.OracleExtractor(nfeat, scale, 8, 20, 7)
    kpL, dL, _ = eL.extract(left, (0, 0)); kpR, dR, _ = eR.extract(right, (0, 0))
    assert kpL.tobytes() == resL[0][0].tobytes() and dR.tobytes() == resR[0][1].tobytes()          # same inputs on both sides
    kept, ur_ref, dp_ref, _ = ob.compute_stereo_matches(eL, eR, kpL, dL, kpR, dR, sc.MB, sc.MBF)
    out = _outputs(1, M)
    _stereo(extL, extR, out)
    gpu_ctx.synchronize()
    ur, dp, nk = (t.cpu().numpy() for t in out)
    n = len(kpL)
    print("max_keypoints", M, "left", n, "right", len(kpR), "kept", kept)
    assert kept > 300 and nk[0] == kept
    assert ur[0, :n].tobytes() == ur_ref.tobytes() and dp[0, :n].tobytes() == dp_ref.tobytes()
    assert (ur[0, n:] == SENT).all() and (dp[0, n:] == SENT).all()
    extL.close(); extR.close()
