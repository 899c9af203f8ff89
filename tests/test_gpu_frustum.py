"""Frame::isInFrustum and the query builder of the local-map matcher on the device (csrc/frustum_kernels.hip) against the model of
tests/frustum_model.py, bit for bit: track records, outcome codes, queries, gathered descriptors, owner map, nq and nToMatch on ragged
batches of the three camera set-ups; the crafted boundary rows; th and the far-point filter; the frustum -> matcher chain against the
oracle's matchers; both sides of the matcher's 2048-query threshold; the host form, limits and errors; the class drop-in."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frustum_model as fm
import oracle_match_bind as omb
import synth_frustum as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xAB


def _thresholds(fr):
    import orbhip
    return orbhip.predict_scale_thresholds(fr["log_scale_factor"], int(fr["nlevels"]))


def _take(pts, idx):
    return {k: v[idx].copy() for k, v in pts.items()}


@functools.lru_cache(maxsize=None)
def _model(kind, n, seed, th=1.0, far=False, th_far=0.0):
    """one scene and what the model makes of it (computed once, shared, not modified)"""
    fr, pts = sf.make_scene(kind, n, seed, th=th, far_points=far, th_far_points=th_far)
    rec, ntm, und = fm.frustum(fr, pts)
    assert not und.any()
    return fr, pts, rec, ntm


def _upload(frames, max_points, max_q):
    """the batched device arrays of orbhip_frustum_queries_device for a list of (fr, pts); outputs pre-filled with FILL bytes"""
    import torch
    import orbhip
    F = len(frames)
    a = dict(Xw=np.zeros((F, max_points, 3), np.float32), normal=np.zeros((F, max_points, 3), np.float32), min_dist=np.zeros((F, max_points), np.float32),
             max_dist=np.zeros((F, max_points), np.float32), flags=np.zeros((F, max_points), np.uint8), desc=np.zeros((F, max_points, 32), np.uint8),
             track_depth=np.zeros((F, max_points), np.float32))
    recs = np.zeros(F, orbhip.FRUSTUM_FRAME_DTYPE)
    for f, (fr, pts) in enumerate(frames):
        n = len(pts["flags"])
        for k in a:
            a[k][f, :n] = pts[k]
        recs[f] = sf.frame_record(fr, n, _thresholds(fr), orbhip.FRUSTUM_FRAME_DTYPE)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    for k, nbytes in (("track", F * max_points * orbhip.TRACK_RECORD_DTYPE.itemsize), ("ntm", F * 4), ("q", F * max_q * 32), ("dq", F * max_q * 32),
                      ("owner", F * max_q * 4), ("nq", F * 4)):
        t[k] = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t, recs


def _frustum(ctx, frames, max_points, max_q):
    import orbhip
    t, recs = _upload(frames, max_points, max_q)
    orbhip.frustum_queries_device(ctx, recs, max_points, t["Xw"].data_ptr(), t["normal"].data_ptr(), t["min_dist"].data_ptr(), t["max_dist"].data_ptr(),
                                  t["flags"].data_ptr(), t["desc"].data_ptr(), t["track_depth"].data_ptr(), frames[0][0]["bounds"],
                                  max_q, t["track"].data_ptr(), t["ntm"].data_ptr(), t["q"].data_ptr(), t["dq"].data_ptr(), t["owner"].data_ptr(), t["nq"].data_ptr())
    ctx.synchronize()
    return _download(t, len(frames), max_points, max_q)


def _download(t, F, max_points, max_q):
    import orbhip
    return dict(track=t["track"].cpu().numpy().view(orbhip.TRACK_RECORD_DTYPE).reshape(F, max_points), ntm=t["ntm"].cpu().numpy().view(np.int32),
                q=t["q"].cpu().numpy().view(orbhip.PROJ_QUERY_DTYPE).reshape(F, max_q), dq=t["dq"].cpu().numpy().reshape(F, max_q, 32),
                owner=t["owner"].cpu().numpy().view(np.int32).reshape(F, max_q), nq=t["nq"].cpu().numpy().view(np.int32))


def _compare(frames, out, models=None):
    """every row of every frame against the model, bit for bit (`ur` of a rig frame's queries excepted: the rig matcher does not read it;
    the kernel stores the record's proj_xr there, i.e. the right camera's u or 0); nothing is written past a frame's points / queries"""
    import orbhip
    assert fm.TRACK_RECORD_DTYPE == orbhip.TRACK_RECORD_DTYPE
    fill_rec = np.frombuffer(bytes([FILL]) * orbhip.TRACK_RECORD_DTYPE.itemsize, orbhip.TRACK_RECORD_DTYPE)[0]
    for f, (fr, pts) in enumerate(frames):
        n = len(pts["flags"])
        rec, ntm, und = models[f] if models else fm.frustum(fr, pts)
        assert not und.any()
        q, dq, owner = fm.queries(fr, pts, rec)
        got = out["track"][f]
        bad = [i for i in range(n) if got[i].tobytes() != rec[i].tobytes()]
        assert not bad, (fr["kind"], f, bad[:5], got[bad[0]], rec[bad[0]])
        assert all(got[i].tobytes() == fill_rec.tobytes() for i in range(n, len(got))), (f, "records past n_points were written")
        assert out["ntm"][f] == ntm and out["nq"][f] == len(q), (f, out["ntm"][f], ntm, out["nq"][f], len(q))
        gq = out["q"][f][:len(q)]
        for name in omb.PROJ_QUERY_DTYPE.names:
            if name == "ur" and fr["rig"]:
                continue
            assert np.array_equal(gq[name].view(np.uint32), q[name].view(np.uint32)), (fr["kind"], f, name)
        assert np.array_equal(out["dq"][f][:len(q)], dq) and np.array_equal(out["owner"][f][:len(q)], owner), (f, "descriptors / owner map")
        assert np.all(out["q"][f][len(q):].view(np.uint8) == FILL) and np.all(out["dq"][f][len(q):] == FILL) and \
            np.all(out["owner"][f][len(q):].view(np.uint8) == FILL), (f, "queries past nq were written")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sf.KINDS)
def test_device_form_matches_the_model(gpu_ctx, kind):
    """One launch per camera set-up: frames of 0, 1, 63, 64, 65, C-1, C, C+1 and 2C+1 points (C = the kernel's chunk: the wave and chunk
    boundaries of the ordered compaction), one frame whose points are all accepted, one with none accepted, one whose last point alone is.
    The 2C+1 frame's scene covers every outcome at least 8 times per camera and every level."""
    import orbhip
    C = orbhip.FRUSTUM_CHUNK
    assert C == 256
    fr, pts, rec, _ = _model(kind, 2 * C + 1, 11)
    print(kind, sf.assert_covers(fr, rec))
    frames = []
    for k, n in enumerate((0, 1, 63, 64, 65, C - 1, C, C + 1)):
        f2, p2, _, _ = _model(kind, 2 * C + 1, 20 + k)
        frames.append((f2, _take(p2, np.arange(n))))
    frames.append((fr, pts))
    big_fr, big_pts, big_rec, _ = _model(kind, 1000, 3)
    ok = np.flatnonzero((big_rec["code"] == 0) & ((big_rec["code_r"] == 0) | (not big_fr["rig"])))
    no = np.flatnonzero((big_rec["code"] > 1) & ((big_rec["code_r"] > 1) | (not big_fr["rig"])))
    assert len(ok) >= 100 and len(no) >= 100
    frames += [(big_fr, _take(big_pts, ok[:100])), (big_fr, _take(big_pts, no[:100])), (big_fr, _take(big_pts, np.concatenate([no[:99], ok[:1]])))]
    max_points = 2 * C + 1
    max_q = 2 * max_points if kind == "rig" else max_points
    out = _frustum(gpu_ctx, frames, max_points, max_q)
    gpu_ctx.check_status()
    _compare(frames, out)
    per_point = 2 if kind == "rig" else 1
    assert out["nq"][9] == 100 * per_point and out["ntm"][9] == 100 and out["nq"][10] == 0 and out["ntm"][10] == 0 and out["nq"][11] == per_point
    assert out["owner"][11][0] == 99


@pytest.mark.gpu
def test_boundary_rows(gpu_ctx):
    """the crafted rows of synth_frustum.boundary_rows: the codes written by hand there, the number of queries per row, both radii"""
    for fr, pts, names, codes, nq_row, radius in sf.boundary_rows():
        n = len(names)
        out = _frustum(gpu_ctx, [(fr, pts)], n, 2 * n)
        gpu_ctx.check_status()
        got = out["track"][0]
        assert np.array_equal(got["code"], codes[:, 0]) and np.array_equal(got["code_r"], codes[:, 1]), (names, got["code"], got["code_r"])
        owner = out["owner"][0][:out["nq"][0]]
        assert np.array_equal(np.bincount(owner, minlength=n), nq_row), (names, owner)
        for name, r in radius.items():
            k = int(np.flatnonzero(owner == names.index(name))[0])
            assert out["q"][0][k]["radius"] == r, (name, out["q"][0][k]["radius"], r)
        _compare([(fr, pts)], out)


@pytest.mark.gpu
@pytest.mark.parametrize("th", [1.0, 3.0])
@pytest.mark.parametrize("far", [False, True])
def test_th_and_far_points(gpu_ctx, th, far):
    """the radius factor (applied when th != 1, to the left / only camera's query) and the far-point filter, which reads the depth the left
    camera stored or, for a rig point only the right camera sees, the stale one"""
    for kind in ("mono", "rig"):
        fr0, pts, rec, _ = _model(kind, 400, 31)
        th_far = float(np.median(rec["depth"][rec["code"] == 0]))
        fr, pts, rec, ntm = _model(kind, 400, 31, th, far, th_far)
        q, _, owner = fm.queries(fr, pts, rec)
        if far:
            q0, _, owner0 = fm.queries(dict(fr, far_points=0), pts, rec)
            assert len(set(owner0) - set(owner)) >= 8                       # the filter removes at least 8 accepted points
            if kind == "rig":
                stale = [i for i in set(owner0) - set(owner) if not rec["in_view"][i]]
                assert stale                                                # ... some of them by their stale depth alone
        out = _frustum(gpu_ctx, [(fr, pts)], 400, 800)
        gpu_ctx.check_status()
        _compare([(fr, pts)], out, [(rec, ntm, np.zeros(len(rec), bool))])
        if kind == "mono" and th == 3.0:
            q1 = fm.queries(dict(fr, th=np.float32(1.0)), pts, rec)[0]
            assert len(q1) == len(q) and np.all(q["radius"] > 2.99 * q1["radius"])


# ---------------------------------------------------------------- the chain: frustum -> matcher without a host visit
@functools.lru_cache(maxsize=None)
def _chain_case(kind, n, seed):
    fr, pts = sf.make_scene(kind, n, seed)
    pts = {k: v.copy() for k, v in pts.items()}
    rec0, _, _ = fm.frustum(fr, pts)
    rivals = sf.add_rivals(pts, rec0)
    rec, ntm, und = fm.frustum(fr, pts)
    assert not und.any()
    tr = sf.make_train_frame(fr, pts, rec, seed, first=rivals)
    q, dq, owner = fm.queries(fr, pts, rec)
    return fr, pts, rec, ntm, tr, q, dq, owner


def _oracle(fr, tr, q, dq, nn_ratio=0.8):
    b = tuple(fr["bounds"])
    if fr["rig"]:
        return omb.search_by_projection_rig(1, q, dq, tr["kp"], tr["desc"], tr["nleft"], tr["mirror"], b, tr["train_match"], nn_ratio=nn_ratio)
    return omb.search_by_projection_map(q, dq, tr["kp"], tr["desc"], tr["u_right"], b, tr["train_match"], nn_ratio=nn_ratio)


def _chain(ctx, cases, max_points, max_q, max_n):
    """orbhip_search_local_points_device on a list of _chain_case results -> (outputs, train_match [F][max_n], nmatches [F])"""
    import torch
    import orbhip
    frames = [(c[0], c[1]) for c in cases]
    F = len(frames)
    rig = bool(frames[0][0]["rig"])
    t, recs = _upload(frames, max_points, max_q)
    kp = np.zeros((F, max_n), orbhip.KP_DTYPE); desc = np.zeros((F, max_n, 32), np.uint8); ur = np.full((F, max_n), -1, np.float32)
    nn = np.zeros(F, np.int32); nl = np.zeros(F, np.int32); mi = np.full((F, max_n), -1, np.int32); tm = np.full((F, max_n), -1, np.int32)
    for f, c in enumerate(cases):
        tr = c[4]; n = len(tr["kp"])
        kp[f, :n] = tr["kp"]; desc[f, :n] = tr["desc"]; nn[f] = n; nl[f] = max(tr["nleft"], 0); tm[f, :n] = tr["train_match"]
        if tr["u_right"] is not None:
            ur[f, :n] = tr["u_right"]
        if tr["mirror"] is not None:
            mi[f, :n] = tr["mirror"]
    d = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).cuda() for k, v in dict(kp=kp, desc=desc, ur=ur, n=nn, nl=nl, mi=mi, tm=tm).items()}
    d["nm"] = torch.full((F,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stereo = frames[0][0]["kind"] == "stereo"
    orbhip.search_local_points_device(ctx, recs, max_points, t["Xw"].data_ptr(), t["normal"].data_ptr(), t["min_dist"].data_ptr(), t["max_dist"].data_ptr(),
                                      t["flags"].data_ptr(), t["desc"].data_ptr(), t["track_depth"].data_ptr(), max_q, d["kp"].data_ptr(), d["desc"].data_ptr(),
                                      d["ur"].data_ptr() if stereo else None, d["n"].data_ptr(), d["nl"].data_ptr() if rig else None,
                                      d["mi"].data_ptr() if rig else None, max_n, max_n, frames[0][0]["bounds"], 100, 0.8, t["track"].data_ptr(),
                                      t["ntm"].data_ptr(), t["q"].data_ptr(), t["dq"].data_ptr(), t["owner"].data_ptr(), t["nq"].data_ptr(),
                                      d["tm"].data_ptr(), d["nm"].data_ptr())
    ctx.synchronize()
    return _download(t, F, max_points, max_q), d["tm"].cpu().numpy(), d["nm"].cpu().numpy()


def _same_claims(got_tm, want_tm):
    """train_match: >= 0 = the owning query; a keypoint that was claimed before the search comes back as -2 on the device"""
    return np.array_equal(np.where(got_tm >= 0, got_tm, -1), np.where(want_tm >= 0, want_tm, -1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sf.KINDS)
def test_chain_equals_model_queries_through_the_oracle(gpu_ctx, kind):
    """orbhip_search_local_points_device == the model's queries fed to the oracle's matcher (search_by_projection_map, with u_right for
    stereo; search_by_projection_rig mode 1): train_match and nmatches identical on two frames.  Per frame at least 8 matches are rejected
    by the ratio rule (found with nn_ratio 1) and at least 8 keypoints are decided by the order of claims (found by reversing the list)."""
    cases = [_chain_case(kind, 600, 5), _chain_case(kind, 500, 6)]
    max_n = max(len(c[4]["kp"]) for c in cases) + 3
    out, tm, nm = _chain(gpu_ctx, cases, 600, 1200 if kind == "rig" else 600, max_n)
    gpu_ctx.check_status()
    for f, (fr, pts, rec, ntm, tr, q, dq, owner) in enumerate(cases):
        n = len(tr["kp"])
        assert 250 <= n <= 400
        want_nm, want_tm = _oracle(fr, tr, q, dq)
        loose_nm, loose_tm = _oracle(fr, tr, q, dq, nn_ratio=1.0)
        rev_nm, rev_tm = _oracle(fr, tr, q[::-1], dq[::-1])
        own = np.where(want_tm >= 0, owner[np.maximum(want_tm, 0)], -1); own_rev = np.where(rev_tm >= 0, owner[::-1][np.maximum(rev_tm, 0)], -1)
        assert np.sum((loose_tm >= 0) & (want_tm < 0)) >= 8 and np.sum(own != own_rev) >= 8 and want_nm >= 50
        assert out["ntm"][f] == ntm and out["nq"][f] == len(q)
        assert nm[f] == want_nm and _same_claims(tm[f, :n], want_tm), (kind, f, nm[f], want_nm)
        assert np.array_equal(out["owner"][f][:len(q)], owner)
    _compare([(c[0], c[1]) for c in cases], out, [(c[2], c[3], np.zeros(len(c[2]), bool)) for c in cases])


@pytest.mark.gpu
def test_either_side_of_2048_queries(gpu_ctx):
    """2600 points of which fewer than 2048 are in view: max_q = 2048 (the matcher's replay form) and max_q = 2600 (its large form) give
    the same result, the oracle's; max_q below the number of queries is refused with ORBHIP_E_CAPACITY and nq = 0, not a fault"""
    import orbhip
    case = _chain_case("mono", 2600, 9)
    fr, pts, rec, ntm, tr, q, dq, owner = case
    assert 512 < len(q) < 2048
    want_nm, want_tm = _oracle(fr, tr, q, dq)
    n = len(tr["kp"])
    results = []
    for max_q in (2048, 2600):
        out, tm, nm = _chain(gpu_ctx, [case], 2600, max_q, n)
        gpu_ctx.check_status()
        assert out["nq"][0] == len(q) and nm[0] == want_nm and _same_claims(tm[0, :n], want_tm), max_q
        results.append((tm.copy(), nm.copy(), out["track"].tobytes()))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1] and results[0][2] == results[1][2]
    out = _frustum(gpu_ctx, [(fr, pts)], 2600, 512)
    with pytest.raises(orbhip.OrbHipError) as ei:
        gpu_ctx.check_status()
    assert ei.value.code == orbhip.E_CAPACITY and out["nq"][0] == 0 and out["ntm"][0] == ntm
    gpu_ctx.check_status()                                                  # the word is cleared


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sf.KINDS)
def test_host_form_equals_the_device_chain(gpu_ctx, kind):
    import orbhip
    fr, pts, rec, ntm, tr, q, dq, owner = _chain_case(kind, 600, 5)
    want_nm, want_tm = _oracle(fr, tr, q, dq)
    frame = sf.frame_record(fr, len(rec), _thresholds(fr), orbhip.FRUSTUM_FRAME_DTYPE)
    track, got_ntm, got_owner, tm, nm = orbhip.search_local_points_host(gpu_ctx, frame, pts, tr["kp"], tr["desc"], tr["u_right"], fr["bounds"], tr["train_match"],
                                                                       nleft=tr["nleft"], mirror=tr["mirror"])
    assert track.tobytes() == rec.tobytes() and got_ntm == ntm and np.array_equal(got_owner, owner)
    assert nm == want_nm and _same_claims(tm, want_tm)
    if kind != "rig":                                                       # the resident form: the train side is on the device already
        import torch
        dkp = torch.from_numpy(np.ascontiguousarray(tr["kp"]).view(np.uint8)).cuda(); dd = torch.from_numpy(tr["desc"]).cuda()
        torch.cuda.synchronize()
        r = orbhip.search_local_points_host(gpu_ctx, frame, pts, tr["kp"], None, tr["u_right"], fr["bounds"], tr["train_match"], d_kp=dkp.data_ptr(),
                                            d_desc=dd.data_ptr())
        assert r[0].tobytes() == rec.tobytes() and r[1] == ntm and np.array_equal(r[2], owner) and r[4] == want_nm and _same_claims(r[3], want_tm)
    # no points: nothing runs; no keypoints: the frustum half alone
    empty = _take(pts, np.arange(0))
    r = orbhip.search_local_points_host(gpu_ctx, sf.frame_record(fr, 0, _thresholds(fr), orbhip.FRUSTUM_FRAME_DTYPE), empty, tr["kp"], tr["desc"], tr["u_right"],
                                        fr["bounds"], tr["train_match"], nleft=tr["nleft"], mirror=tr["mirror"])
    assert len(r[0]) == 0 and r[1] == 0 and len(r[2]) == 0 and r[4] == 0
    r = orbhip.search_local_points_host(gpu_ctx, frame, pts, tr["kp"][:0], tr["desc"][:0], None, fr["bounds"], tr["train_match"][:0],
                                        nleft=0 if kind == "rig" else -1)
    assert r[0].tobytes() == rec.tobytes() and r[1] == ntm and np.array_equal(r[2], owner) and r[4] == 0


@pytest.mark.gpu
def test_limits_and_errors_are_refused_on_the_host(gpu_ctx):
    """every limit the host can know is refused there, before anything is launched, with the field named"""
    import orbhip
    fr, pts, rec, ntm, tr, q, dq, owner = _chain_case("mono", 600, 5)
    n = len(rec)
    good = sf.frame_record(fr, n, _thresholds(fr), orbhip.FRUSTUM_FRAME_DTYPE)
    t, _ = _upload([(fr, pts)], n, n)

    def device(frame, max_points=n, max_q=n, **null):
        p = {k: (None if k in null else t[k].data_ptr()) for k in ("Xw", "normal", "min_dist", "max_dist", "flags", "desc", "track", "ntm", "q", "dq", "owner", "nq")}
        orbhip.frustum_queries_device(gpu_ctx, frame, max_points, p["Xw"], p["normal"], p["min_dist"], p["max_dist"], p["flags"], p["desc"], None, fr["bounds"],
                                      max_q, p["track"], p["ntm"], p["q"], p["dq"], p["owner"], p["nq"])

    def refused(word, call, *a, **kw):
        with pytest.raises(orbhip.OrbHipError) as ei:
            call(*a, **kw)
        assert ei.value.code == orbhip.E_BADARG and word in str(ei.value), str(ei.value)
    refused("NULL", device, good, Xw=1)
    refused("NULL", device, good, owner=1)
    bad = good.copy(); bad["nlevels"] = 33
    refused("nlevels", device, bad)
    bad = good.copy(); bad["rig"] = 1                                          # cam_type[1] is -1: no second camera
    refused("cam_type[1]", device, bad)
    bad = good.copy(); bad["n_points"] = n + 1
    refused("n_points", device, bad)
    refused("max_q", device, good, max_q=0)
    refused("frames", device, np.zeros(0, orbhip.FRUSTUM_FRAME_DTYPE))
    # the host form: mismatched counts, NULL arrays, a rig record against a single-camera train side
    host = functools.partial(orbhip.search_local_points_host, gpu_ctx)
    refused("n_points", host, sf.frame_record(fr, n - 1, _thresholds(fr), orbhip.FRUSTUM_FRAME_DTYPE), pts, tr["kp"], tr["desc"], None, fr["bounds"], tr["train_match"])
    refused("NULL", host, good, dict(pts, normal=None), tr["kp"], tr["desc"], None, fr["bounds"], tr["train_match"])
    fr_rig, pts_rig = _model("rig", 600, 5)[:2]
    refused("rig", host, sf.frame_record(fr_rig, len(pts_rig["flags"]), _thresholds(fr_rig), orbhip.FRUSTUM_FRAME_DTYPE), pts_rig, tr["kp"], tr["desc"], None,
            fr["bounds"], tr["train_match"])
    gpu_ctx.check_status()


# ---------------------------------------------------------------- the class drop-in: Tracking::SearchLocalPoints through lib/host_frustum_smoke
SMOKE = os.path.join(ROOT, "orb-slam3-mac_amd", "lib", "host_frustum_smoke")


def _drop_in_case(kind, seed, jitter=1.0, row=(0, 0, 0, 10, 0, 2), n_points=600, n_target=300):
    """a frame with keypoints, a local map with state an earlier frame left, and the Python replay of Tracking.cc:2358-2430 on it.
    row = (sensor, imu initialised, BA2, frame id, last reloc frame id, tracking state)"""
    fr, pts = sf.make_scene(kind, n_points, seed, far_points=True, th_far_points=12.0 if kind != "rig" else 40.0)
    pts = {k: v.copy() for k, v in pts.items()}
    rivals = sf.add_rivals(pts, fm.frustum(fr, pts)[0])
    rec = fm.frustum(fr, pts)[0]
    tr = sf.make_train_frame(fr, pts, rec, seed, n_target=n_target, first=rivals, jitter=jitter)
    n, N = len(rec), len(tr["kp"])
    rng = np.random.default_rng(5000 + seed)
    frame_id = row[3]
    trk_f, trk_i = sf.initial_state(n, seed)
    pts["track_depth"] = trk_f[:, 4].copy()                                 # mTrackDepth as the earlier frame left it
    bad = (rng.random(n) < 0.03).astype(np.int32)
    last_seen = np.where((pts["flags"] & 2) != 0, frame_id, rng.integers(0, frame_id, n)).astype(np.int32)
    fmp = np.full(N, -1, np.int32)                                          # keypoints that hold a local point already: some good, some bad
    held = np.flatnonzero(tr["train_match"] == -2)
    fmp[held] = tr["src"][held]
    fmp[held[::4]] = np.flatnonzero(bad)[:len(held[::4])] if bad.sum() >= len(held[::4]) else fmp[held[::4]]
    th = fm.choose_th(*row)
    fr = dict(fr, th=np.float32(th))
    mps = sf.points_from_state(pts, trk_f, trk_i, bad, last_seen)
    frame_mp = [mps[k] if k >= 0 else None for k in fmp]

    def matcher(q, dq):
        tm0 = np.array([-2 if (p is not None and p.nobs > 0) else -1 for p in frame_mp], np.int32)
        return _oracle(fr, dict(tr, train_match=tm0), q, dq)
    ret, project = fm.search_local_points(fr, pts, mps, frame_mp, frame_id, matcher)
    inp = sf.smoke_input(fr, pts, trk_f, trk_i, tr, bad, last_seen, fmp, sensor=row[0], imu_init=row[1], ba2=row[2], frame_id=row[3], last_reloc=row[4], state=row[5])
    want = dict(ret=-1 if ret is None else ret, fmp=np.array([p.idx if p is not None else -1 for p in frame_mp], np.int32), project=project)
    want["trk_f"], want["trk_i"], want["visible"], want["last_seen"] = sf.state_arrays(mps)
    return inp, want


def _run_smoke(tmp_path, mode, inp):
    a, b = str(tmp_path / ("in_%s.bin" % mode)), str(tmp_path / ("out_%s.bin" % mode))
    sf.write_flat(a, inp)
    r = subprocess.run([SMOKE, mode, a, b], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    return sf.read_flat(b)


def _check_drop_in(got, want, what):
    assert got["ret"][0] == want["ret"], (what, got["ret"], want["ret"])
    assert np.array_equal(got["fmp"], want["fmp"]), (what, np.flatnonzero(got["fmp"] != want["fmp"])[:10])
    assert np.array_equal(got["trk_i"].reshape(-1, 4), want["trk_i"]), what
    assert np.array_equal(got["trk_f"].view(np.uint32).reshape(-1, 8), want["trk_f"].view(np.uint32)), what
    assert np.array_equal(got["visible"], want["visible"]) and np.array_equal(got["last_seen_out"], want["last_seen"]), what
    ids = sorted(want["project"])
    assert list(got["proj_id"]) == ids, what
    xy = np.array([want["project"][k] for k in ids], np.float32).reshape(-1, 2)
    assert np.array_equal(got["proj_xy"].reshape(-1, 2).view(np.uint32), xy.view(np.uint32)), what


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sf.KINDS)
def test_class_drop_in(gpu_ctx, tmp_path, kind):
    """Tracking::SearchLocalPoints (host/Tracking_SearchLocalPoints.cc, one device call) leaves what the Python replay of Tracking.cc:2358-2430
    leaves: mvpMapPoints, every point's mTrack* fields (the ones the reference writes AND the ones it leaves untouched), visible counts,
    mnLastFrameSeen, mmProjectPoints and SearchByProjection's return value.  The path a caller had before -- the host member isInFrustum in a
    loop, then ORBmatcher::SearchByProjection(F, vpMapPoints, ...) -- gives the same."""
    inp, want = _drop_in_case(kind, 7)
    assert want["ret"] >= 50 and (want["fmp"] >= 0).sum() > 50 and np.sum(inp["bad"]) >= 8
    _check_drop_in(_run_smoke(tmp_path, "track", inp), want, kind + " track")
    _check_drop_in(_run_smoke(tmp_path, "today", inp), want, kind + " today")


@pytest.mark.gpu
def test_class_drop_in_th_table(gpu_ctx, tmp_path):
    """the th choice of Tracking.cc:2406-2426 through its effect: keypoints up to 25 pixels from their projections, so that the search radius
    decides what is found; rows of (sensor, IMU initialised, BA2, frame id, last relocalisation, state)"""
    rows = [((0, 0, 0, 10, 0, 2), 1), ((2, 0, 0, 10, 0, 2), 3), ((3, 0, 0, 10, 0, 2), 10), ((4, 1, 1, 10, 0, 2), 2), ((0, 0, 0, 10, 9, 2), 5), ((0, 0, 0, 10, 0, 3), 15)]
    found = []
    for row, th in rows:
        assert fm.choose_th(*row) == th
        inp, want = _drop_in_case("mono", 8, jitter=25.0, row=row)
        _check_drop_in(_run_smoke(tmp_path, "track", inp), want, row)
        found.append(want["ret"])
    assert len(set(found)) >= 5 and found[0] == min(found), found            # the rows are told apart by what they find
