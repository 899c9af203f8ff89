"""Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1128-1168) composed from the oracle's pieces (bf2nn = cv::BFMatcher knnMatch k=2,
kb8_triangulate_matches = KannalaBrandt8::TriangulateMatches), checked against an independent numpy model; the new C ABI symbols; the
stereo-fisheye constructor's call lines linked against host/Frame.cc.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam3-mac_amd")
F32 = np.float32

# the TUM-VI 512 x 512 rig (KannalaBrandt8 x 2, right -> left transform): BASELINE config #5's calibration
RIG = dict(types=(1, 1),
           cam1=np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                          0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], F32),
           cam2=np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                          0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039], F32),
           Tlr=np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224, 0.101063427414194],
                         [-0.000823363992158, 0.998899461915674, 0.046895490788700, 0.001946204678584],
                         [-0.000656143613644, -0.046896036240590, 0.998899560146304, 0.001015350132563]], F32))
RIG["Rlr"] = np.ascontiguousarray(RIG["Tlr"][:, :3]); RIG["tlr"] = np.ascontiguousarray(RIG["Tlr"][:, 3])


def level_sigma2(scale=1.2, nlevels=8):
    """ORBextractor.cc:413-421 in float"""
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(s[-1] * F32(scale)))
    return np.array([F32(v * v) for v in s], F32)


def fisheye_oracle(kpL, dL, monoL, kpR, dR, monoR, rig=RIG, sigma2=None):
    """Frame.cc:1128-1168 with the oracle's matcher and triangulation: (l2r, r2l, depth, x3d [nL][3] (0 where none), n, descMatches)."""
    import oracle_match_bind as om
    sigma2 = level_sigma2() if sigma2 is None else sigma2
    nL, nR = len(kpL), len(kpR)
    l2r = np.full(nL, -1, np.int32); r2l = np.full(nR, -1, np.int32)
    depth = np.full(nL, -1, F32); x3d = np.zeros((nL, 3), F32)
    n = desc = 0
    if nL - monoL <= 0:
        return l2r, r2l, depth, x3d, n, desc
    idx, dist, acc = om.bf2nn(dL[monoL:], dR[monoR:], 0.7)
    for q in range(nL - monoL):
        if idx[q, 1] < 0 or not acc[q]:                               # size() >= 2 && d0 < d1 * 0.7
            continue
        desc += 1
        i, j = q + monoL, int(idx[q, 0]) + monoR
        z, x = om.kb8_triangulate_matches(rig["types"][0], rig["cam1"], rig["types"][1], rig["cam2"], (kpL["x"][i], kpL["y"][i]),
                                          (kpR["x"][j], kpR["y"][j]), rig["Rlr"], rig["tlr"], sigma2[kpL["octave"][i]], sigma2[kpR["octave"][j]])
        if F32(z) > F32(0.0001):
            l2r[i] = j; r2l[j] = i; depth[i] = F32(z); x3d[i] = x; n += 1
    return l2r, r2l, depth, x3d, n, desc


def bf2nn_np(A, B, ratio=0.7):
    """cv::BFMatcher knnMatch(k=2) by numpy popcount: (idx [n][2], dist [n][2], accept); the lower train index wins equal distances"""
    na, nb = len(A), len(B)
    idx = np.full((na, 2), -1, np.int32); dist = np.full((na, 2), np.iinfo(np.int32).max, np.int32); acc = np.zeros(na, np.uint8)
    if na == 0 or nb == 0:
        return idx, dist, acc
    D = np.unpackbits(A[:, None, :] ^ B[None, :, :], axis=2).sum(2)
    order = np.argsort(D * 65536 + np.arange(nb)[None, :], axis=1, kind="stable")
    k = min(2, nb)
    idx[:, :k] = order[:, :k]; dist[:, :k] = np.take_along_axis(D, order[:, :k], 1)
    if nb >= 2:
        acc[:] = (dist[:, 0].astype(F32).astype(np.float64) < dist[:, 1].astype(F32).astype(np.float64) * ratio)
    return idx, dist, acc


def crafted_case(rng, n_pts=40, rig=RIG):
    """Keypoints / descriptors of a scene seen by the rig: good matches, a many-to-one pair, a tie, a far (no parallax) point, a right
    keypoint off by 12 px (reprojection), unrelated descriptors.  Returns kpL, dL, kpR, dR (KP_DTYPE, uint8)."""
    import oracle_bind as ob
    import oracle_match_bind as om
    c1, c2 = (1, rig["cam1"].astype(np.float64)), (1, rig["cam2"].astype(np.float64))
    R, t = rig["Rlr"].astype(np.float64), rig["tlr"].astype(np.float64)
    X = np.stack([rng.uniform(-2, 2, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(1.5, 3.5, n_pts)], 1)
    X[3] = [0.5, 0.2, 900.0]                                          # parallax below the cos 0.9998 limit
    Xr = (X - t) @ R                                                  # right camera: R^T (X - t)
    uvL, uvR = om.kb8_project_np(c1, X), om.kb8_project_np(c2, Xr)
    uvR[5] += [12.0, -9.0]                                            # reprojection error in the right camera
    uvL[7] = uvL[8] + [0.4, -0.3]                                     # left 7 is a near-duplicate of left 8 (same point, same pick)
    oct_ = rng.integers(0, 3, n_pts)
    oct_[7] = oct_[8]
    dL = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    dR = dL.copy()
    flips = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8) & rng.integers(0, 256, (n_pts, 32), dtype=np.uint8) & 0x11
    dR ^= flips                                                       # a few bits differ per pair
    dL[7] = dL[8] ^ 1                                                 # left 7 and 8 both pick right 8 (many-to-one) ...
    dR[7] = rng.integers(0, 256, 32, dtype=np.uint8)
    dR[10] = dR[11]                                                   # right 10 == right 11: a tie (ratio test fails for 10 and 11)
    dL[12:14] = rng.integers(0, 256, (2, 32), dtype=np.uint8)         # unrelated descriptors
    kpL = np.zeros(n_pts, ob.KP_DTYPE); kpR = np.zeros(n_pts, ob.KP_DTYPE)
    kpL["x"], kpL["y"], kpL["octave"] = uvL[:, 0], uvL[:, 1], oct_
    kpR["x"], kpR["y"], kpR["octave"] = uvR[:, 0], uvR[:, 1], oct_
    perm = rng.permutation(n_pts)                                     # right order unrelated to the left one
    return kpL, dL, kpR[perm], dR[perm]


def test_bf2nn_oracle_against_numpy_popcount():
    """The oracle's knnMatch(k=2) + ratio flag equals a numpy popcount model: ties (lower index first, ratio fails), one train row (no
    second neighbour: rejected), none."""
    import oracle_match_bind as om
    rng = np.random.default_rng(5)
    for na, nb in [(50, 60), (20, 1), (7, 2), (9, 0), (64, 64)]:
        A = rng.integers(0, 256, (na, 32), dtype=np.uint8)
        B = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        if nb >= 4:
            B[3] = B[1]; A[0] = B[1] ^ 3                              # a tie between train rows 1 and 3
        i, d, a = om.bf2nn(A, B, 0.7)
        ri, rd, ra = bf2nn_np(A, B)
        np.testing.assert_array_equal(i, ri); np.testing.assert_array_equal(d[:, :min(nb, 2)], rd[:, :min(nb, 2)])
        np.testing.assert_array_equal(a, ra)
        if nb < 2:
            assert not a.any()


@pytest.mark.parametrize("seed,monoL,monoR", [(1, 0, 0), (2, 6, 4), (3, 0, 39), (4, 5, 40)])
def test_fisheye_composition_against_numpy_model(seed, monoL, monoR):
    """The Python composition of Frame.cc:1128-1168 against a numpy model (popcount 2-NN + TriangulateMatches in double with numpy's
    SVD): same l2r / r2l wherever no triangulation test sits within 1e-3 of its threshold, depth and point within 2e-3; many-to-one
    keeps the highest left index in r2l; parallax and reprojection rejections drop descriptor matches; slices of 1 and 0 right rows."""
    from test_oracle_match_ba import _triangulate_matches_np
    rng = np.random.default_rng(seed)
    kpL, dL, kpR, dR = crafted_case(rng)
    l2r, r2l, depth, x3d, n, desc = fisheye_oracle(kpL, dL, monoL, kpR, dR, monoR)
    idx, _, acc = bf2nn_np(dL[monoL:], dR[monoR:])
    s2 = level_sigma2().astype(np.float64)
    el2r = np.full(len(kpL), -1); er2l = np.full(len(kpR), -1)
    for q in range(len(kpL) - monoL):
        if idx[q, 1] < 0 or not acc[q]:
            continue
        i, j = q + monoL, idx[q, 0] + monoR
        z, X, margin = _triangulate_matches_np(RIG["cam1"].astype(np.float64), RIG["cam2"].astype(np.float64),
                                               (float(kpL["x"][i]), float(kpL["y"][i])), (float(kpR["x"][j]), float(kpR["y"][j])),
                                               RIG["Rlr"].astype(np.float64), RIG["tlr"].astype(np.float64), s2[kpL["octave"][i]], s2[kpR["octave"][j]])
        if margin < 1e-3:                                             # undecided by the double model: take the oracle's decision
            el2r[i] = l2r[i]
            if l2r[i] >= 0:
                er2l[j] = i
            continue
        if z > 1e-4:
            el2r[i] = j; er2l[j] = i
            assert abs(depth[i] - z) <= 2e-3 * z and np.allclose(x3d[i], X, rtol=2e-3, atol=2e-3), (i, depth[i], z)
    np.testing.assert_array_equal(l2r, el2r)
    np.testing.assert_array_equal(r2l, er2l)
    assert n == (l2r >= 0).sum() and ((depth > 0) == (l2r >= 0)).all() and (x3d[l2r < 0] == 0).all()
    if len(kpR) - monoR >= 2 and monoL <= 3:
        assert n > 20 and desc > n                                    # triangulation rejects some descriptor matches
        i3 = 3
        assert l2r[i3] == -1                                          # the far point: parallax
    if monoR == 0 and monoL < 7:
        j8 = int(np.flatnonzero(np.all(dR == dR[np.argmin(np.unpackbits(dR ^ dL[8], axis=1).sum(1))], 1))[0])
        if l2r[7] == j8 and l2r[8] == j8:
            assert r2l[j8] == 8                                       # many-to-one: the highest left index
    if len(kpR) - monoR < 2:
        assert n == 0 and desc == 0                                   # fewer than 2 right rows: knnMatch returns < 2 neighbours


def test_fisheye_symbols_exported():
    """Both forms of the new entry point are exported by liborbhip.so (C linkage)."""
    so = os.path.join(PKG, "lib", "liborbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("orbhip_compute_stereo_fisheye_matches_device", "orbhip_compute_stereo_fisheye_matches_host"):
        assert s in names, s


def test_fisheye_constructor_call_lines_link_against_frame(tmp_path):
    """host/compile_callers.cc's stereo-fisheye constructor lines call Frame::ComputeStereoFishEyeMatches, and linking them with
    host/Frame.cc (+ what it needs: frame_cache, ORBextractor, the context, liborbhip.so) resolves it: no undefined Frame member left."""
    obj = str(tmp_path / "callers.o")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-Wall", "-Werror", "-c", "-o", obj, os.path.join(PKG, "host", "compile_callers.cc")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    und = subprocess.run(["nm", "-C", "-u", obj], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "ORB_SLAM3::Frame::ComputeStereoFishEyeMatches()" in und
    out = str(tmp_path / "libcallers.so")
    srcs = [os.path.join(PKG, "host", s) for s in ("Frame.cc", "frame_cache.cc", "ORBextractor.cc", "hip_context.cc")]
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-o", out, obj] + srcs + ["-L" + os.path.join(PKG, "lib"), "-lorbhip", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    defined = subprocess.run(["nm", "-C", "--defined-only", out], stdout=subprocess.PIPE, text=True, check=True).stdout
    undefined = subprocess.run(["nm", "-C", "-u", out], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "ORB_SLAM3::Frame::ComputeStereoFishEyeMatches()" in defined and "frame_fisheye_constructor_calls" in defined
    assert "Frame::ComputeStereoFishEyeMatches" not in undefined                # (the orbhip_* C entry points come from liborbhip.so)
