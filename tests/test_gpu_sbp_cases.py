"""The projection-window matchers on the device against the C oracle, bit for bit, on the crafted cases of sbp_cases.py (which
test_sbp_cases.py holds to the model and to their names): k_search_by_projection<DESC_LDS> with its register and LDS loops, the replay form
(k_sbp_prep / k_sbp_candidates / k_sbp_replay), the rig halves and the mirror rule, k_fuse_search<BIG>.  Every case runs in every form that
accepts it; nothing is written beyond n / nq; check_status() stays clean; and the pairs the replay form hands back to the sequential kernel
(orbhip.debug_sbp_handed_back) are the ones the model predicts."""
import functools
import numpy as np
import pytest

import sbp_cases as sc

pytestmark = pytest.mark.gpu
SENT = -7                      # train_match beyond n (the call treats anything but -1 as held, and must leave it alone)
WIDE_SBP, WIDE_FUSE = 2056, 2904          # rows beyond 2048 take the sequential kernel alone; rows beyond 2900 take k_fuse_search<true>


@functools.lru_cache(maxsize=None)
def _oracle(name, stereo):
    return sc.run_oracle(sc.by_name(name), stereo)


@functools.lru_cache(maxsize=None)
def _handback(name, stereo):
    return sc.run_model(sc.by_name(name), stereo=stereo)["handback"]


def _groups(kinds):
    """cases that can share one launch (same entry point, bounds and thresholds); pairs that hand back and pairs that stay alternate, an
    empty pair sits between two full ones"""
    g = {}
    for c in sc.all_cases():
        if c["kind"] in kinds:
            g.setdefault((c["kind"], c["geom"], c["th_high"], c["ratio"], c["check_ori"]), []).append(c)
    out = {}
    for key, cs in g.items():
        hb = [c for c in cs if c["handback"]]; st = [c for c in cs if not c["handback"] and len(c["kp"]) and len(c["q"])]
        em = [c for c in cs if not (len(c["kp"]) and len(c["q"]))]
        order = []
        while hb or st or em:
            for lst in (st, hb, st, em):
                if lst:
                    order.append(lst.pop(0))
        out["-".join(str(k) for k in key)] = order
    return out


SBP_GROUPS, RIG_GROUPS, FUSE_GROUPS = _groups(("frame", "map")), _groups(("rig0", "rig1")), _groups(("fuse",))


def _upload(cases, max_n, max_q, stereo):
    import torch
    import orbhip
    P = len(cases)
    Q = np.zeros((P, max_q), orbhip.PROJ_QUERY_DTYPE); DQ = np.zeros((P, max_q, 32), np.uint8)
    KP = np.zeros((P, max_n), orbhip.KP_DTYPE); D = np.zeros((P, max_n, 32), np.uint8)
    UR = np.full((P, max_n), -1, np.float32); TM = np.full((P, max_n), SENT, np.int32); MI = np.full((P, max_n), -1, np.int32)
    nq = np.array([len(c["q"]) for c in cases], np.int32); n = np.array([len(c["kp"]) for c in cases], np.int32)
    nl = np.array([c["nleft"] if c["nleft"] is not None else 0 for c in cases], np.int32)
    for p, c in enumerate(cases):
        Q[p, :nq[p]] = c["q"]; DQ[p, :nq[p]] = c["dq"]; KP[p, :n[p]] = c["kp"]; D[p, :n[p]] = c["d"]; TM[p, :n[p]] = c["tm"]
        if stereo and c["ur"] is not None:
            UR[p, :n[p]] = c["ur"]
        if c["mirror"] is not None:
            MI[p, :n[p]] = c["mirror"]
    dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype in (orbhip.KP_DTYPE, orbhip.PROJ_QUERY_DTYPE) else a).cuda()
    t = dict(q=dev(Q), dq=dev(DQ), nq=dev(nq), kp=dev(KP), d=dev(D), ur=dev(UR), n=dev(n), tm=dev(TM), nl=dev(nl), mi=dev(MI))
    return t, n, nq


def _run_sbp(gpu_ctx, cases, max_n, max_q, stereo):
    """one launch over `cases` (all of one group); returns (nmatches [P], train_match [P][max_n], n)"""
    import torch
    import orbhip
    c0 = cases[0]
    t, n, nq = _upload(cases, max_n, max_q, stereo)
    P = len(cases)
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda k: t[k].data_ptr()
    if c0["kind"] == "frame":
        orbhip.search_by_projection_device(gpu_ctx, p("q"), p("dq"), p("nq"), max_q, p("kp"), p("d"), p("ur") if stereo else None, p("n"), max_n, max_n, P,
                                           c0["bounds"], c0["th_high"], c0["check_ori"], p("tm"), nm.data_ptr())
    elif c0["kind"] == "map":
        orbhip.search_local_map_device(gpu_ctx, p("q"), p("dq"), p("nq"), max_q, p("kp"), p("d"), p("ur") if stereo else None, p("n"), max_n, max_n, P,
                                       c0["bounds"], c0["th_high"], c0["ratio"], p("tm"), nm.data_ptr())
    else:
        orbhip.search_by_projection_rig_device(gpu_ctx, c0["mode"], p("q"), p("dq"), p("nq"), max_q, p("kp"), p("d"), p("n"), p("nl"),
                                               p("mi") if c0["mode"] == 1 else None, max_n, max_n, P, c0["bounds"], c0["th_high"], c0["ratio"],
                                               c0["check_ori"], p("tm"), nm.data_ptr())
    flags = orbhip.debug_sbp_handed_back(gpu_ctx)            # (waits for the stream; read before any other call on the context)
    gpu_ctx.check_status()
    return nm.cpu().numpy(), t["tm"].cpu().numpy(), n, flags


def _check_sbp(cases, stereo, nm, tm, n):
    for p, c in enumerate(cases):
        n_ref, tm_ref = _oracle(c["name"], stereo and c["ur"] is not None)
        assert nm[p] == n_ref, (c["name"], p, int(nm[p]), n_ref)
        bad = np.flatnonzero(tm[p, :n[p]] != tm_ref)
        assert bad.size == 0, (c["name"], p, bad[:8], tm[p, bad[:8]], tm_ref[bad[:8]])
        assert (tm[p, n[p]:] == SENT).all(), c["name"]        # nothing written beyond n


def _row(cases):
    return max(8, max(len(c["kp"]) for c in cases)), max(8, max(len(c["q"]) for c in cases))


@pytest.mark.parametrize("stereo", [True, False], ids=["uright", "no-uright"])
@pytest.mark.parametrize("form", ["replay", "sequential", "sequential-wide-row"])
@pytest.mark.parametrize("group", list(SBP_GROUPS))
def test_search_by_projection_crafted(gpu_ctx, monkeypatch, group, form, stereo):
    """every single-camera case, batched with the others of its mode / geometry: replay form (with the observed hand-back flags equal to the
    model's prediction for every pair, "32 blocked: stays" and "33 blocked: handed back" among them), sequential form, and a row of 2056
    (sequential kernel alone), each with and without the uRight array"""
    monkeypatch.setenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS", "64" if form == "replay" else "0")
    cases = SBP_GROUPS[group]
    max_n, max_q = _row(cases)
    if form == "sequential-wide-row":
        max_n = WIDE_SBP
    nm, tm, n, flags = _run_sbp(gpu_ctx, cases, max_n, max_q, stereo)
    _check_sbp(cases, stereo, nm, tm, n)
    if form == "replay":
        want = [int(_handback(c["name"], stereo)) for c in cases]
        assert flags.tolist() == want, [(c["name"], int(f), w) for c, f, w in zip(cases, flags, want) if f != w]
        for p in np.flatnonzero(flags):                        # a handed-back pair sits next to one that stayed with the replay result
            assert not all(want[k] for k in (p - 1, p + 1) if 0 <= k < len(want)), group
    else:
        assert flags.size == 0                                 # the sequential kernel ran alone


@pytest.mark.parametrize("wide", [False, True], ids=["narrow-row", "wide-row"])
@pytest.mark.parametrize("group", list(RIG_GROUPS))
def test_rig_search_by_projection_crafted(gpu_ctx, group, wide):
    cases = RIG_GROUPS[group]
    max_n, max_q = _row(cases)
    nm, tm, n, flags = _run_sbp(gpu_ctx, cases, WIDE_SBP if wide else max_n, max_q, False)
    _check_sbp(cases, False, nm, tm, n)
    assert flags.size == 0


@pytest.mark.parametrize("kind", ["frame", "map"])
def test_small_rows_without_descriptors_in_lds(gpu_ctx, monkeypatch, kind):
    """k_search_by_projection<false> on small frames: the launcher keeps the descriptors out of LDS once pairs * (LDS bytes with descriptors)
    exceeds CUs * 150 KB.  The crafted cases of at most 64 keypoints and queries are tiled to the smallest such pair count, computed from
    the device's CU count with the launcher's own formula (sbp_lds_bytes / sbp_launch in match_kernels.hip)."""
    import torch
    monkeypatch.setenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS", "0")
    base = [c for c in SBP_GROUPS["%s-vga-100-0.8-%s" % (kind, kind == "frame")] if len(c["kp"]) <= 64 and len(c["q"]) <= 64]
    assert len(base) >= 6 and any(len(c["kp"]) == 0 for c in base)
    cap = 64
    ncells = 64 * 48
    lds = 4 * (ncells + 1) + cap * (4 + 4 + 2 + 2 + 2 + 2 + 1) + cap * 2 + cap * (2 + 1) + 16         # sbp_lds_bytes(cap_n, cap_q, ncells)
    with_desc = lds + cap * 32
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = cus * 150 * 1024 // with_desc + 1                                                      # the first count with pairs * with_desc > cus * 150 KB
    assert with_desc <= 150 * 1024 and (pairs - 1) * with_desc <= cus * 150 * 1024 < pairs * with_desc and pairs < 20000
    cases = [base[p % len(base)] for p in range(pairs)]
    nm, tm, n, flags = _run_sbp(gpu_ctx, cases, cap, cap, True)
    ref = {c["name"]: _oracle(c["name"], True) for c in base}
    for p, c in enumerate(cases):                                                                   # every tile
        assert nm[p] == ref[c["name"]][0] and np.array_equal(tm[p, :n[p]], ref[c["name"]][1]) and (tm[p, n[p]:] == SENT).all(), (p, c["name"])


@pytest.mark.parametrize("stereo", [True, False], ids=["uright", "no-uright"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow-row", "wide-row"])
@pytest.mark.parametrize("group", list(FUSE_GROUPS))
def test_fuse_search_crafted(gpu_ctx, group, wide, stereo):
    """k_fuse_search<false> and, by a row capacity of 2904, <true>: the chi-square thresholds on both sides, the rows one fused multiply-add
    would flip, uRight == 0 (stereo branch) and -1 (mono branch), [min_level, max_level] with both ends"""
    import torch
    import orbhip
    cases = FUSE_GROUPS[group]
    max_n, max_q = _row(cases)
    if wide:
        max_n = WIDE_FUSE
    t, n, nq = _upload(cases, max_n, max_q, stereo)
    P = len(cases)
    bi = torch.full((P, max_q), -9, dtype=torch.int32, device="cuda"); bd = torch.full((P, max_q), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    orbhip.fuse_search_device(gpu_ctx, t["q"].data_ptr(), t["dq"].data_ptr(), t["nq"].data_ptr(), max_q, t["kp"].data_ptr(), t["d"].data_ptr(),
                              t["ur"].data_ptr() if stereo else None, t["n"].data_ptr(), max_n, max_n, P, cases[0]["sig"], cases[0]["bounds"],
                              bi.data_ptr(), bd.data_ptr())
    gpu_ctx.check_status()
    bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    for p, c in enumerate(cases):
        ri, rd = _oracle(c["name"], stereo)
        assert np.array_equal(bi[p, :nq[p]], ri) and np.array_equal(bd[p, :nq[p]], rd), (c["name"], bi[p, :nq[p]], ri, bd[p, :nq[p]], rd)
        assert (bi[p, nq[p]:] == -9).all() and (bd[p, nq[p]:] == -9).all(), c["name"]              # nothing written beyond nq
