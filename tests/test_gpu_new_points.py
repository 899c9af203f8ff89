"""LocalMapping::CreateNewMapPoints on the device (csrc/newpoints_kernels.hip) against the model of tests/new_points_model.py: outcome
codes and world points bit for bit on ragged batches of the three camera set-ups, the flag update, the search -> create chain without a
host visit, the host form, limits and errors, and the class drop-in."""
import os
import subprocess

import numpy as np
import pytest

import new_points_model as npm
import synth_new_points as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MN = 608            # row capacity of the batches below (no multiple of the 256-keypoint tile)


def _upload(pairs, max_n=MN, flags=False):
    """the batched device arrays of orbhip_create_new_map_points_device for a list of synth_new_points pairs"""
    import torch
    import orbhip
    P = len(pairs)
    a = dict(kp1=np.zeros((P, max_n), orbhip.KP_DTYPE), raw1=np.zeros((P, max_n), orbhip.KP_DTYPE), ur1=np.full((P, max_n), -1, np.float32),
             dp1=np.full((P, max_n), -1, np.float32), n1=np.zeros(P, np.int32), kp2=np.zeros((P, max_n), orbhip.KP_DTYPE),
             raw2=np.zeros((P, max_n), orbhip.KP_DTYPE), ur2=np.full((P, max_n), -1, np.float32), dp2=np.full((P, max_n), -1, np.float32),
             n2=np.zeros(P, np.int32), m12=np.full((P, max_n), -1, np.int32), mp1=np.zeros((P, max_n), np.uint8), mp2=np.zeros((P, max_n), np.uint8))
    for p, pr in enumerate(pairs):
        n1, n2 = len(pr["kp1"]), len(pr["kp2"])
        a["kp1"][p, :n1] = pr["kp1"]; a["raw1"][p, :n1] = pr["kp1_raw"]; a["ur1"][p, :n1] = pr["ur1"]; a["dp1"][p, :n1] = pr["depth1"]; a["n1"][p] = n1
        a["kp2"][p, :n2] = pr["kp2"]; a["raw2"][p, :n2] = pr["kp2_raw"]; a["ur2"][p, :n2] = pr["ur2"]; a["dp2"][p, :n2] = pr["depth2"]; a["n2"][p] = n2
        a["m12"][p, :n1] = pr["matches12"]
        if flags:
            a["mp1"][p, :n1] = pr.get("mp1", 0); a["mp2"][p, :n2] = pr.get("mp2", 0)
    t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in a.items()}
    t["x3D"] = torch.full((P, max_n, 3), 7.0, dtype=torch.float32, device="cuda")
    t["out"] = torch.full((P, max_n), 99, dtype=torch.uint8, device="cuda")
    t["nc"] = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def _create(ctx, t, pairs, max_n=MN, raw=True, stereo=True, flags=False):
    import orbhip
    kf1 = [t["kp1"].data_ptr(), t["raw1"].data_ptr() if raw else 0, t["ur1"].data_ptr() if stereo else 0, t["dp1"].data_ptr() if stereo else 0, t["n1"].data_ptr()]
    kf2 = [t["kp2"].data_ptr(), t["raw2"].data_ptr() if raw else 0, t["ur2"].data_ptr() if stereo else 0, t["dp2"].data_ptr() if stereo else 0, t["n2"].data_ptr()]
    rec = np.array([pr["P"] for pr in pairs], orbhip.NEWPOINTS_PAIR_DTYPE)
    orbhip.create_new_map_points_device(ctx, kf1, kf2, t["m12"].data_ptr(), rec, max_n, max_n, sy.SIGMA2, sy.SCALE, sy.SIGMA2, sy.SCALE,
                                        t["x3D"].data_ptr(), t["out"].data_ptr(), t["nc"].data_ptr(),
                                        t["mp1"].data_ptr() if flags else None, t["mp2"].data_ptr() if flags else None)


def _compare(kind, pairs, out, x3D, nc):
    """codes and points bit for bit; the one licence: a stereo match whose model outcome flips with one float ulp of its stereo cosine"""
    assert npm.PAIR_DTYPE == __import__("orbhip").NEWPOINTS_PAIR_DTYPE
    counts = np.zeros(14, int)
    stereo_matches = left_out = 0
    for p, pr in enumerate(pairs):
        n1 = len(pr["kp1"])
        ref = npm.run_pair(pr)
        counts += np.bincount(ref["outcome"], minlength=14)
        diff = np.flatnonzero((out[p, :n1] != ref["outcome"]) | np.any(x3D[p, :n1].view(np.uint32) != ref["x3D"].view(np.uint32), axis=1))
        for i in np.flatnonzero(pr["matches12"] >= 0):
            stereo_matches += bool(pr["P"]["nleft1"] == -1 and (pr["ur1"][i] >= 0 or pr["ur2"][pr["matches12"][i]] >= 0))
        for i in diff:
            licensed = pr["matches12"][i] >= 0 and int(i) not in pr["crafted"] and npm.libm_sensitive(pr, int(i))
            assert licensed, (kind, p, int(i), int(out[p, i]), int(ref["outcome"][i]), x3D[p, i], ref["x3D"][i])
            left_out += 1
        if len(diff) == 0:
            assert nc[p] == ref["n_created"], (p, nc[p], ref["n_created"])
        assert np.all(out[p, n1:] == 99) and np.all(x3D[p, n1:] == 7.0)       # nothing past the pair's keypoints
    print("%s: outcome counts %s, %d of %d stereo matches left out" % (kind, counts.tolist(), left_out, stereo_matches))
    assert left_out <= 0.01 * stereo_matches
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo", "rig"])
def test_device_form_matches_the_model(gpu_ctx, kind):
    """One ragged batch per camera set-up: pairs with 0, 1, 63, 64, 65, 255, 256 and 257 matches (the compaction and workgroup boundaries)
    and the degenerate pair (w == 0, a zero distance), crafted matches for every outcome the set-up can reach."""
    pairs = sy.scene(kind)
    assert [int(np.sum(pr["matches12"] >= 0)) for pr in pairs[:8]] == list(sy.COUNTS)
    t = _upload(pairs)
    _create(gpu_ctx, t, pairs, raw=kind == "stereo", stereo=kind == "stereo")
    gpu_ctx.synchronize(); gpu_ctx.check_status()
    counts = _compare(kind, pairs, t["out"].cpu().numpy(), t["x3D"].cpu().numpy(), t["nc"].cpu().numpy())
    want = {1, 4, 5, 7, 8, 9, 10, 11, 12, 13} | ({2, 3, 6} if kind == "stereo" else set())
    assert want <= set(np.flatnonzero(counts).tolist())


@pytest.mark.gpu
def test_flag_rows(gpu_ctx):
    """writable has_mp rows end as the model's (earlier flags kept, idx1 / idx2 of every created point set); NULL rows: nothing is written"""
    rng = np.random.default_rng(5)
    pairs = [dict(pr, mp1=(rng.random(len(pr["kp1"])) < 0.2).astype(np.uint8), mp2=(rng.random(len(pr["kp2"])) < 0.2).astype(np.uint8))
             for pr in sy.scene("stereo")[4:7]]
    t = _upload(pairs, flags=True)
    before1, before2 = t["mp1"].cpu().numpy().copy(), t["mp2"].cpu().numpy().copy()
    _create(gpu_ctx, t, pairs, flags=False)
    gpu_ctx.synchronize(); gpu_ctx.check_status()
    assert np.array_equal(t["mp1"].cpu().numpy(), before1) and np.array_equal(t["mp2"].cpu().numpy(), before2)
    _create(gpu_ctx, t, pairs, flags=True)
    gpu_ctx.synchronize(); gpu_ctx.check_status()
    mp1, mp2 = t["mp1"].cpu().numpy(), t["mp2"].cpu().numpy()
    for p, pr in enumerate(pairs):
        ref = npm.run_pair(pr)
        assert ref["n_created"] > 10
        n1, n2 = len(pr["kp1"]), len(pr["kp2"])
        assert np.array_equal(mp1[p, :n1], ref["has_mp1"]) and np.array_equal(mp2[p, :n2], ref["has_mp2"])
        assert not mp1[p, n1:].any() and not mp2[p, n2:].any()


def _chain_device(ctx, pairs):
    """search (general) -> create -> search -> create ... on the context's stream, one synchronisation at the end"""
    import torch
    import orbhip
    import oracle_match_bind as om
    N = 320
    n1 = len(pairs[0]["kp1"])
    keep = []
    mp1 = torch.zeros((1, N), dtype=torch.uint8, device="cuda")
    res = []
    for pr in pairs:
        n2 = len(pr["kp2"])
        i2, s2, f2 = om.feature_vector_csr(pr["nid2"])
        a = dict(nid1=np.zeros((1, N), np.int32), kp1=np.zeros((1, N), orbhip.KP_DTYPE), d1=np.zeros((1, N, 32), np.uint8), ur1=np.full((1, N), -1, np.float32),
                 dp1=np.full((1, N), -1, np.float32), raw1=np.zeros((1, N), orbhip.KP_DTYPE), n1=np.array([n1], np.int32),
                 i2=np.zeros((1, N), np.int32), s2=np.zeros((1, N + 1), np.int32), f2=np.zeros((1, N), np.int32), nn2=np.array([len(i2)], np.int32),
                 kp2=np.zeros((1, N), orbhip.KP_DTYPE), d2=np.zeros((1, N, 32), np.uint8), ur2=np.full((1, N), -1, np.float32),
                 dp2=np.full((1, N), -1, np.float32), raw2=np.zeros((1, N), orbhip.KP_DTYPE), n2=np.array([n2], np.int32),
                 geom=np.array([sy.chain_case(pr, None, None)["geom"]], orbhip.TRI_GENERAL_DTYPE))
        a["nid1"][0, :n1] = pr["nid1"]; a["kp1"][0, :n1] = pr["kp1"]; a["d1"][0, :n1] = pr["d1"]; a["ur1"][0, :n1] = pr["ur1"]; a["dp1"][0, :n1] = pr["depth1"]
        a["raw1"][0, :n1] = pr["kp1_raw"]; a["i2"][0, :len(i2)] = i2; a["s2"][0, :len(s2)] = s2; a["f2"][0, :len(f2)] = f2
        a["kp2"][0, :n2] = pr["kp2"]; a["d2"][0, :n2] = pr["d2"]; a["ur2"][0, :n2] = pr["ur2"]; a["dp2"][0, :n2] = pr["depth2"]; a["raw2"][0, :n2] = pr["kp2_raw"]
        t = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in a.items()}
        t["mp2"] = torch.zeros((1, N), dtype=torch.uint8, device="cuda")
        t["m12"] = torch.full((1, N), -9, dtype=torch.int32, device="cuda"); t["nm"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        t["x3D"] = torch.zeros((1, N, 3), dtype=torch.float32, device="cuda"); t["out"] = torch.zeros((1, N), dtype=torch.uint8, device="cuda")
        t["nc"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        keep.append(t)
    torch.cuda.synchronize()
    for pr, t in zip(pairs, keep):
        kf1 = [t["nid1"].data_ptr(), mp1.data_ptr(), t["kp1"].data_ptr(), t["d1"].data_ptr(), t["ur1"].data_ptr(), t["n1"].data_ptr()]
        kf2 = [t["i2"].data_ptr(), t["s2"].data_ptr(), t["f2"].data_ptr(), t["nn2"].data_ptr(), t["mp2"].data_ptr(), t["kp2"].data_ptr(), t["d2"].data_ptr(),
               t["ur2"].data_ptr(), t["n2"].data_ptr()]
        orbhip.search_for_triangulation_general_device(ctx, kf1, kf2, t["geom"].data_ptr(), 1, N, N, N, sy.SIGMA2, sy.SCALE, sy.SIGMA2, True,
                                                       t["m12"].data_ptr(), t["nm"].data_ptr())
        orbhip.create_new_map_points_device(ctx, [t["kp1"].data_ptr(), t["raw1"].data_ptr(), t["ur1"].data_ptr(), t["dp1"].data_ptr(), t["n1"].data_ptr()],
                                            [t["kp2"].data_ptr(), t["raw2"].data_ptr(), t["ur2"].data_ptr(), t["dp2"].data_ptr(), t["n2"].data_ptr()],
                                            t["m12"].data_ptr(), np.array([pr["P"]], orbhip.NEWPOINTS_PAIR_DTYPE), N, N, sy.SIGMA2, sy.SCALE, sy.SIGMA2,
                                            sy.SCALE, t["x3D"].data_ptr(), t["out"].data_ptr(), t["nc"].data_ptr(), mp1.data_ptr(), t["mp2"].data_ptr())
    ctx.synchronize(); ctx.check_status()
    for t in keep:
        res.append(dict(matches12=t["m12"].cpu().numpy()[0, :n1], outcome=t["out"].cpu().numpy()[0, :n1], x3D=t["x3D"].cpu().numpy()[0, :n1],
                        n_created=int(t["nc"].cpu().numpy()[0])))
    return res, mp1.cpu().numpy()[0, :n1]


def _assert_chain_equal(got, ref):
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g["matches12"], r["matches12"]), k
        assert np.array_equal(g["outcome"], r["outcome"]), k
        assert g["x3D"].tobytes() == r["x3D"].tobytes(), k
        assert g["n_created"] == r["n_created"], k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo", "rig"])
def test_chain_without_a_host_visit(gpu_ctx, kind):
    """One current keyframe, 3 neighbours: the device chain equals the CPU's alternation of the oracle's SearchForTriangulation and the
    model, and neighbour 2's match list is not what one search of all neighbours against the initial flags gives."""
    pairs = sy.chain_world(kind)
    ref, ref_mp1 = sy.chain_reference(kind)
    at_once, _ = sy.chain_reference(kind, carry=False)
    assert not np.array_equal(ref[1]["matches12"], at_once[1]["matches12"])
    assert sum(r["n_created"] for r in ref) > 30
    for k, pr in enumerate(pairs):                                            # (the licence of the batch test is not needed here: assert it)
        q = dict(pr, matches12=ref[k]["matches12"])
        assert not any(npm.libm_sensitive(q, int(i)) for i in np.flatnonzero(q["matches12"] >= 0))
    got, mp1 = _chain_device(gpu_ctx, pairs)
    _assert_chain_equal(got, ref)
    assert np.array_equal(mp1, ref_mp1)


def _host_keyframes(pairs):
    import oracle_match_bind as om
    p0 = pairs[0]
    stereo = p0["kind"] == "stereo"
    cur = dict(kp=p0["kp1"], kp_raw=p0["kp1_raw"] if stereo else None, desc=p0["d1"], u_right=p0["ur1"] if stereo else None,
               depth=p0["depth1"] if stereo else None, has_mp=np.zeros(len(p0["kp1"]), np.uint8), nid=p0["nid1"], level_sigma2=sy.SIGMA2,
               scale_factors=sy.SCALE)
    neigh = []
    for pr in pairs:
        i2, s2, f2 = om.feature_vector_csr(pr["nid2"])
        neigh.append(dict(kp=pr["kp2"], kp_raw=pr["kp2_raw"] if stereo else None, desc=pr["d2"], u_right=pr["ur2"] if stereo else None,
                          depth=pr["depth2"] if stereo else None, has_mp=np.zeros(len(pr["kp2"]), np.uint8), node_ids=i2, node_start=s2, feat=f2,
                          level_sigma2=sy.SIGMA2, scale_factors=sy.SCALE))
    geom = np.array([sy.chain_case(pr, None, None)["geom"] for pr in pairs])
    return cur, neigh, geom


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo", "rig"])
def test_host_form_equals_the_device_chain(gpu_ctx, kind):
    """orbhip_create_new_map_points_host (one blob each way, the whole chain on the device) against the device chain and the model chain"""
    import orbhip
    pairs = sy.chain_world(kind)
    cur, neigh, geom = _host_keyframes(pairs)
    rec = np.array([pr["P"] for pr in pairs], orbhip.NEWPOINTS_PAIR_DTYPE)
    m, x, o, nc, mp1 = orbhip.create_new_map_points_host(gpu_ctx, cur, neigh, geom, rec, True)
    host = [dict(matches12=m[k], outcome=o[k], x3D=x[k], n_created=int(nc[k])) for k in range(len(pairs))]
    dev, dev_mp1 = _chain_device(gpu_ctx, pairs)
    _assert_chain_equal(host, dev)
    assert np.array_equal(mp1, dev_mp1)
    ref, ref_mp1 = sy.chain_reference(kind)
    _assert_chain_equal(host, ref)
    assert np.array_equal(mp1, ref_mp1)
    # no neighbours, and a neighbour without keypoints: reset rows, nothing launched
    m, x, o, nc, mp1 = orbhip.create_new_map_points_host(gpu_ctx, cur, [], geom[:0], rec[:0], True)
    assert m.shape[0] == 0 and not mp1.any()
    empty = dict(neigh[0], kp=neigh[0]["kp"][:0], kp_raw=None if neigh[0]["kp_raw"] is None else neigh[0]["kp_raw"][:0], desc=neigh[0]["desc"][:0],
                 u_right=None if neigh[0]["u_right"] is None else neigh[0]["u_right"][:0], depth=None if neigh[0]["depth"] is None else neigh[0]["depth"][:0],
                 has_mp=neigh[0]["has_mp"][:0], node_ids=neigh[0]["node_ids"][:0], node_start=np.zeros(1, np.int32), feat=neigh[0]["feat"][:0])
    m, x, o, nc, mp1 = orbhip.create_new_map_points_host(gpu_ctx, cur, [empty, neigh[0]], geom[[0, 0]], rec[[0, 0]], True)
    assert np.all(m[0] == -1) and not o[0].any() and not x[0].any() and nc[0] == 0
    assert np.array_equal(m[1], ref[0]["matches12"]) and np.array_equal(o[1], ref[0]["outcome"]) and x[1].tobytes() == ref[0]["x3D"].tobytes()


@pytest.mark.gpu
def test_limits_and_errors(gpu_ctx):
    import orbhip
    pairs = sy.scene("rig")[2:4]
    t = _upload(pairs)
    with pytest.raises(orbhip.OrbHipError) as e:
        _create(gpu_ctx, t, pairs, max_n=16385)
    assert e.value.code == orbhip.E_CAPACITY and "max_n" in str(e.value)
    mixed = [dict(pairs[0], P=pairs[0]["P"].copy()), pairs[1]]
    mixed[0]["P"]["nleft2"] = -1
    with pytest.raises(orbhip.OrbHipError) as e:
        _create(gpu_ctx, t, mixed)
    assert e.value.code == orbhip.E_BADARG and "nleft" in str(e.value)
    kf = [t["kp1"].data_ptr(), 0, 0, 0, t["n1"].data_ptr()]
    rec = np.array([pr["P"] for pr in pairs], orbhip.NEWPOINTS_PAIR_DTYPE)
    with pytest.raises(orbhip.OrbHipError) as e:
        orbhip.create_new_map_points_device(gpu_ctx, kf, kf, t["m12"].data_ptr(), rec, MN, MN, np.ones(17), np.ones(17), np.ones(17), np.ones(17),
                                            t["x3D"].data_ptr(), t["out"].data_ptr(), t["nc"].data_ptr())
    assert e.value.code == orbhip.E_BADARG and "nlevels" in str(e.value)
    # a pair whose count exceeds max_n: status word, rows untouched; the other pair is served
    import torch
    t["n2"][0] = MN + 1
    torch.cuda.synchronize()
    _create(gpu_ctx, t, pairs, flags=True)
    gpu_ctx.synchronize()
    with pytest.raises(orbhip.OrbHipError) as e:
        gpu_ctx.check_status()
    assert e.value.code == orbhip.E_CAPACITY
    gpu_ctx.check_status()                                                    # (reading the word clears it)
    out, x3D = t["out"].cpu().numpy(), t["x3D"].cpu().numpy()
    assert np.all(out[0] == 99) and np.all(x3D[0] == 7.0) and not t["mp1"][0].any().item() and not t["mp2"][0].any().item()
    ref = npm.run_pair(pairs[1])
    n1 = len(pairs[1]["kp1"])
    assert np.array_equal(out[1, :n1], ref["outcome"]) and x3D[1, :n1].tobytes() == ref["x3D"].tobytes()


EXE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_newpoints_smoke")


def _run_class(tmp_path, kind, check_true_at):
    from synth_sim3 import read_flat, write_flat
    arrays, used, kf_of = sy.class_case(kind, check_true_at)
    fin, fout = str(tmp_path / "np.in"), str(tmp_path / "np.out")
    write_flat(fin, arrays)
    r = subprocess.run([EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "map points created" in r.stdout, r.stdout[-2000:]
    return arrays, used, kf_of, read_flat(fout)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,check_true_at", [("mono", -1), ("stereo", -1), ("rig", -1), ("stereo", 3)])
def test_class_drop_in(tmp_path, kind, check_true_at):
    """LocalMapping::CreateNewMapPoints (host/LocalMapping_CreateNewMapPoints.cc) through lib/host_newpoints_smoke against the model chain:
    the created points, their two observations, the order of mlpRecentAddedMapPoints (= the Atlas's), mvpMapPoints of every keyframe,
    the neighbour the baseline tests skip (no point, its mvpMapPoints unchanged) and CheckNewKeyFrames turning true at its third call.
    The class derives poses, centres and F12 from Tcw in float (the reference's cv::Mat arithmetic), the scene hands the model the
    same quantities rounded from double: positions are compared to 1e-4 relative, everything else exactly."""
    arrays, used, kf_of, out = _run_class(tmp_path, kind, check_true_at)
    ref, mp1 = sy.run_chain(used, carry=True, check_ori=False)
    n1 = len(used[0]["kp1"])
    exp_pos, exp_obs = [], []
    kfmp = {k: np.where(arrays["mp%d" % k] != 0, -2, -1) for k in range(int(arrays["nkf"][0]))}
    for k, r in zip(kf_of, ref):
        for i in np.flatnonzero((r["outcome"] >= 1) & (r["outcome"] <= 3)):
            j = int(r["matches12"][i])
            kfmp[0][i] = len(exp_obs); kfmp[k][j] = len(exp_obs)              # a later point at the same KF2 keypoint replaces the earlier one
            exp_pos.append(r["x3D"][i]); exp_obs.append((int(i), k, j))
    assert len(exp_obs) > 30
    assert out["n_created"][0] == len(exp_obs)
    assert np.array_equal(out["obs"].reshape(-1, 3), np.array(exp_obs))
    assert np.allclose(out["pos"].reshape(-1, 3), np.array(exp_pos), rtol=1e-4, atol=1e-5)
    assert out["atlas_same_order"][0] == 1
    for k in kfmp:
        assert np.array_equal(out["kfmp%d" % k], kfmp[k]), k
    assert np.all(out["kfmp2"] < 0)                                           # the skipped neighbour
    assert out["desc_updates"][0] == len(exp_obs) and out["normal_updates"][0] == len(exp_obs)
    assert out["check_calls"][0] == 3
    if check_true_at == 3:
        assert kf_of == [1, 3] and np.all(out["kfmp4"] < 0)
