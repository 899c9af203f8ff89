"""The rotation-consistency check of every kernel that owns a histogram, on the cases of rotation_cases.py (both 0.1 * max1 cut-offs,
more than three filled bins with ties, the all-zero histogram; test_rotation_cases.py asserts that the cases are that).  All
(profile, seed) cases of one matcher are the pairs of one launch; match arrays and counts equal the oracle's bit for bit."""
import numpy as np
import pytest
import rotation_cases as rc

pytestmark = pytest.mark.gpu

N = rc.N


def _cases(matcher):
    return [rc.make_case(matcher, prof, seed)[0] for prof in rc.PROFILES for seed in rc.SEEDS[matcher]]


def _check(matcher, cases, nm, match):
    tot = 0
    for p, c in enumerate(cases):
        n_ref, m_ref = rc.oracle(matcher, c, True)
        assert nm[p] == n_ref, (matcher, p, nm[p], n_ref)
        np.testing.assert_array_equal(match[p][:len(m_ref)], m_ref)
        tot += n_ref
    assert tot > 250


def _pack(cases, fields):
    """fields: name -> (per-case array getter, dtype, trailing shape, fill): one [pairs][N]... device tensor each."""
    import torch
    out = {}
    for name, (get, dtype, tail, fill) in fields.items():
        a = np.full((len(cases), N) + tail, fill, dtype) if fill else np.zeros((len(cases), N) + tail, dtype)
        for p, c in enumerate(cases):
            v = get(c)
            a[p, :len(v)] = v
        out[name] = torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()
    return out


def _feature_vectors(cases, key):
    """The cases' FeatureVectors as the device reads them: ids [pairs][N], start [pairs][N + 1], feat [pairs][N], counts [pairs]."""
    import torch
    import oracle_match_bind as om
    P = len(cases)
    ids = np.zeros((P, N), np.int32); st = np.zeros((P, N + 1), np.int32); fe = np.zeros((P, N), np.int32); nn = np.zeros(P, np.int32)
    for p, c in enumerate(cases):
        i, s, f = om.feature_vector_csr(c[key])
        ids[p, :len(i)] = i; st[p, :len(s)] = s; fe[p, :len(f)] = f; nn[p] = len(i)
    return [torch.from_numpy(a).cuda() for a in (ids, st, fe, nn)]


def _out(P):
    import torch
    return torch.full((P, N), -9, dtype=torch.int32, device="cuda"), torch.full((P,), -9, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("form", ["sequential", "replay"])
def test_search_for_initialization_rotation(gpu_ctx, monkeypatch, form):
    """k_search_init (sequential) and k_si_replay (replay): si_tail."""
    from test_gpu_match import _search_init
    monkeypatch.setenv("ORBHIP_SI_PARALLEL_MAX_PAIRS", "1048576" if form == "replay" else "0")
    monkeypatch.delenv("ORBHIP_SI_SMALL_CAP0", raising=False)
    cases = _cases("si")
    got = _search_init(gpu_ctx, [(c["kpA"], c["dA"]) for c in cases], [(c["kpB"], c["dB"]) for c in cases], rc.BOUNDS,
                       [c["prev"] for c in cases], N, 100, 0.9, True)
    _check("si", cases, [g[0] for g in got], [g[1] for g in got])


@pytest.mark.parametrize("form", ["sequential", "replay"])
def test_search_by_projection_rotation(gpu_ctx, monkeypatch, form):
    """k_search_by_projection (sequential) and k_sbp_replay (replay), frame mode."""
    from test_gpu_match import _sbp
    monkeypatch.setenv("ORBHIP_SBP_PARALLEL_MAX_PAIRS", "64" if form == "replay" else "0")
    cases = _cases("sbp")
    got = _sbp(gpu_ctx, cases, N, N, rc.BOUNDS, 100, True, False)
    _check("sbp", cases, [g[0] for g in got], [g[1] for g in got])


@pytest.mark.parametrize("kf", [False, True])
def test_search_by_bow_rotation(gpu_ctx, kf):
    """k_search_by_bow, frame form and keyframe form."""
    import torch
    import orbhip
    matcher = "bow_kf" if kf else "bow"
    cases = _cases(matcher)
    P = len(cases)
    K, F = _feature_vectors(cases, "nid_k"), _feature_vectors(cases, "nid_f")
    t = _pack(cases, dict(va=(lambda c: c["valid"], np.uint8, (), 0), vb=(lambda c: c["valid2"], np.uint8, (), 0),
                          kpk=(lambda c: c["kp_k"], orbhip.KP_DTYPE, (), 0), kpf=(lambda c: c["kp_f"], orbhip.KP_DTYPE, (), 0),
                          dk=(lambda c: c["d_k"], np.uint8, (32,), 0), df=(lambda c: c["d_f"], np.uint8, (32,), 0)))
    n = torch.full((P,), N, dtype=torch.int32, device="cuda")
    match, nm = _out(P)
    torch.cuda.synchronize()
    k = [x.data_ptr() for x in K]; f = [x.data_ptr() for x in F]
    if kf:
        orbhip.search_by_bow_kf_device(gpu_ctx, k + [t["va"].data_ptr(), t["kpk"].data_ptr(), t["dk"].data_ptr(), n.data_ptr()],
                                       f + [t["vb"].data_ptr(), t["kpf"].data_ptr(), t["df"].data_ptr(), n.data_ptr()], P, N, N, N,
                                       0.75, True, match.data_ptr(), nm.data_ptr())
    else:
        orbhip.search_by_bow_device(gpu_ctx, k + [t["va"].data_ptr(), t["kpk"].data_ptr(), t["dk"].data_ptr()],
                                    f + [t["kpf"].data_ptr(), t["df"].data_ptr()], n.data_ptr(), P, N, N, N, 0.7, True,
                                    match.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    _check(matcher, cases, nm.cpu().numpy(), match.cpu().numpy())


@pytest.mark.parametrize("general", [False, True])
def test_search_for_triangulation_rotation(gpu_ctx, general):
    """k_search_triangulation (Pinhole, mono) and k_search_triangulation_general<false, false> (fisheye)."""
    import torch
    import orbhip
    matcher = "tri_general" if general else "tri"
    cases = _cases(matcher)
    P = len(cases)
    S2 = _feature_vectors(cases, "nid2")
    t = _pack(cases, dict(nid1=(lambda c: c["nid1"], np.int32, (), 0), mp1=(lambda c: c["mp1"], np.uint8, (), 0),
                          kp1=(lambda c: c["kp1"], orbhip.KP_DTYPE, (), 0), d1=(lambda c: c["d1"], np.uint8, (32,), 0),
                          ur1=(lambda c: c["ur1"], np.float32, (), -1), mp2=(lambda c: c["mp2"], np.uint8, (), 0),
                          kp2=(lambda c: c["kp2"], orbhip.KP_DTYPE, (), 0), d2=(lambda c: c["d2"], np.uint8, (32,), 0),
                          ur2=(lambda c: c["ur2"], np.float32, (), -1)))
    n = torch.full((P,), N, dtype=torch.int32, device="cuda")
    match, nm = _out(P)
    c0 = cases[0]
    if general:
        geom = np.array([c["geom"] for c in cases], orbhip.TRI_GENERAL_DTYPE)
    else:
        geom = np.zeros(P, orbhip.TRI_PAIR_DTYPE)
        for p, c in enumerate(cases):
            geom[p] = (c["F12"], c["ep"][0], c["ep"][1], 0, 0)
    g = torch.from_numpy(np.ascontiguousarray(geom).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    ur1, ur2 = (t["ur1"].data_ptr(), t["ur2"].data_ptr()) if general else (0, 0)
    kf1 = [t["nid1"].data_ptr(), t["mp1"].data_ptr(), t["kp1"].data_ptr(), t["d1"].data_ptr(), ur1, n.data_ptr()]
    kf2 = [x.data_ptr() for x in S2] + [t["mp2"].data_ptr(), t["kp2"].data_ptr(), t["d2"].data_ptr(), ur2, n.data_ptr()]
    if general:
        orbhip.search_for_triangulation_general_device(gpu_ctx, kf1, kf2, g.data_ptr(), P, N, N, N, c0["sigma2_1"], c0["scale"], c0["sigma2"],
                                                       True, match.data_ptr(), nm.data_ptr())
    else:
        orbhip.search_for_triangulation_device(gpu_ctx, kf1, kf2, g.data_ptr(), P, N, N, N, c0["scale"], c0["sigma2"], True,
                                               match.data_ptr(), nm.data_ptr())
    gpu_ctx.check_status()
    _check(matcher, cases, nm.cpu().numpy(), match.cpu().numpy())
