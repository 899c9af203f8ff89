"""The FeatureVector matchers on the device against the C oracle, bit for bit, on the crafted cases of bow_cases.py (which test_bow_cases.py
holds to the model and to their names): k_search_by_bow<KF_MODE, BIG> with its lane path and its whole-wave path (registers, tail loop, the
two-ahead prefetch, the claim chain), the rig form, k_search_triangulation and k_search_triangulation_general<BIG, false> with one Pinhole
camera.  All cases of one form and ratio are the pairs of one launch; rows are prefilled with -9 and nothing is written beyond n."""
import functools
import numpy as np
import pytest

import bow_cases as bc
import oracle_match_bind as om

pytestmark = pytest.mark.gpu
FILLV = -9
WIDE = 4104                    # rows beyond 4096 dispatch the BIG templates (descriptors read from global memory); the fast triangulation
                               # kernel caps its LDS rows at 4096 and the cases stay below


def _groups():
    g = {}
    for c in bc.bow_cases():
        g.setdefault("%s-%s" % (c["form"], c["ratio"]), []).append(c)
    return g


BOW_GROUPS = _groups()


@functools.lru_cache(maxsize=None)
def _bow_oracle(name, ori):
    return bc.run_bow_oracle(bc.by_name(name), ori)


@functools.lru_cache(maxsize=None)
def _tri_oracle(name, ori, mono):
    return om.search_for_triangulation(bc.by_name(name), ori, mono)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def _bow_upload(cases, MN, MNODE):
    import orbhip
    P = len(cases)
    arr = dict(ki=np.zeros((P, MNODE), np.int32), ks=np.zeros((P, MNODE + 1), np.int32), kf=np.zeros((P, MN), np.int32), kn=np.zeros(P, np.int32),
               fi=np.zeros((P, MNODE), np.int32), fs=np.zeros((P, MNODE + 1), np.int32), ff=np.zeros((P, MN), np.int32), fn=np.zeros(P, np.int32),
               va=np.zeros((P, MN), np.uint8), vb=np.zeros((P, MN), np.uint8), kpk=np.zeros((P, MN), orbhip.KP_DTYPE), kpf=np.zeros((P, MN), orbhip.KP_DTYPE),
               dk=np.zeros((P, MN, 32), np.uint8), df=np.zeros((P, MN, 32), np.uint8), n1=np.zeros(P, np.int32), n2=np.zeros(P, np.int32),
               nl=np.full(P, -1, np.int32))
    for p, c in enumerate(cases):
        ki, ks, kf = om.feature_vector_csr(c["nid_k"]); fi, fs, ff = om.feature_vector_csr(c["nid_f"])
        arr["ki"][p, :len(ki)] = ki; arr["ks"][p, :len(ks)] = ks; arr["kf"][p, :len(kf)] = kf; arr["kn"][p] = len(ki)
        arr["fi"][p, :len(fi)] = fi; arr["fs"][p, :len(fs)] = fs; arr["ff"][p, :len(ff)] = ff; arr["fn"][p] = len(fi)
        nk, nf = len(c["kp_k"]), len(c["kp_f"])
        arr["va"][p, :nk] = c["valid"]; arr["kpk"][p, :nk] = c["kp_k"]; arr["kpf"][p, :nf] = c["kp_f"]
        arr["dk"][p, :nk] = c["d_k"]; arr["df"][p, :nf] = c["d_f"]; arr["n1"][p] = nk; arr["n2"][p] = nf
        if c["form"] == "kf":
            arr["vb"][p, :nf] = c["valid2"]
        if c["form"] == "rig":
            arr["nl"][p] = c["nleft"]
    return {k: _dev(v) for k, v in arr.items()}


def _bow_dims(cases, wide):
    MN = WIDE if wide else max(8, max(max(len(c["kp_k"]), len(c["kp_f"])) for c in cases))
    MNODE = 8 + max(max(len(set(c["nid_k"].tolist())), len(set(c["nid_f"].tolist()))) for c in cases)
    return MN, MNODE


def _bow_launch(gpu_ctx, entry, t, P, MNODE, MN, ratio, ori):
    """entry: "frame" | "kf" | "rig"; returns (matches [P][MN], nmatches [P]) without reading the status word"""
    import torch
    import orbhip
    out = torch.full((P, MN), FILLV, dtype=torch.int32, device="cuda"); nm = torch.full((P,), FILLV, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda *ks: [t[k].data_ptr() for k in ks]
    if entry == "kf":
        orbhip.search_by_bow_kf_device(gpu_ctx, p("ki", "ks", "kf", "kn", "va", "kpk", "dk", "n1"), p("fi", "fs", "ff", "fn", "vb", "kpf", "df", "n2"),
                                       P, MNODE, MN, MN, ratio, ori, out.data_ptr(), nm.data_ptr())
    elif entry == "rig":
        orbhip.search_by_bow_rig_device(gpu_ctx, p("ki", "ks", "kf", "kn", "va", "kpk", "dk"), p("fi", "fs", "ff", "fn", "kpf", "df"), t["n2"].data_ptr(),
                                        t["nl"].data_ptr(), P, MNODE, MN, MN, ratio, ori, out.data_ptr(), nm.data_ptr())
    else:
        orbhip.search_by_bow_device(gpu_ctx, p("ki", "ks", "kf", "kn", "va", "kpk", "dk"), p("fi", "fs", "ff", "fn", "kpf", "df"), t["n2"].data_ptr(),
                                    P, MNODE, MN, MN, ratio, ori, out.data_ptr(), nm.data_ptr())
    return out, nm


def _bow_check(cases, ori, out, nm):
    out, nm = out.cpu().numpy(), nm.cpu().numpy()
    for p, c in enumerate(cases):
        n_ref, m_ref = _bow_oracle(c["name"], ori)
        n = len(m_ref)
        assert nm[p] == n_ref, (c["name"], int(nm[p]), n_ref)
        bad = np.flatnonzero(out[p, :n] != m_ref)
        assert bad.size == 0, (c["name"], bad[:8], out[p, bad[:8]], m_ref[bad[:8]])
        assert (out[p, n:] == FILLV).all(), c["name"]             # nothing written beyond n


@pytest.mark.parametrize("ori", [True, False], ids=["ori", "no-ori"])
@pytest.mark.parametrize("wide", [False, True], ids=["lds-row", "row-4104"])
@pytest.mark.parametrize("group", list(BOW_GROUPS))
def test_search_by_bow_crafted(gpu_ctx, group, wide, ori):
    """every case of one form and ratio in one launch: k_search_by_bow<KF_MODE, false> at a row that fits, <KF_MODE, true> at a row of 4104; the
    frame form's cases also through the rig entry with nleft = -1 for every pair, which must be the frame form exactly, wave path included"""
    cases = BOW_GROUPS[group]
    form, ratio = cases[0]["form"], cases[0]["ratio"]
    MN, MNODE = _bow_dims(cases, wide)
    t = _bow_upload(cases, MN, MNODE)
    out, nm = _bow_launch(gpu_ctx, form, t, len(cases), MNODE, MN, ratio, ori)
    gpu_ctx.check_status()
    _bow_check(cases, ori, out, nm)
    if form == "frame":
        out2, nm2 = _bow_launch(gpu_ctx, "rig", t, len(cases), MNODE, MN, ratio, ori)
        gpu_ctx.check_status()
        _bow_check(cases, ori, out2, nm2)


# ------------------------------------------------------------------ SearchForTriangulation
def _tri_upload(cases, MN, MNODE):
    import orbhip
    P = len(cases)
    arr = dict(nid1=np.zeros((P, MN), np.int32), mp1=np.zeros((P, MN), np.uint8), kp1=np.zeros((P, MN), orbhip.KP_DTYPE),
               d1=np.zeros((P, MN, 32), np.uint8), ur1=np.full((P, MN), -1, np.float32), n1=np.zeros(P, np.int32),
               i2=np.zeros((P, MNODE), np.int32), s2=np.zeros((P, MNODE + 1), np.int32), f2=np.zeros((P, MN), np.int32), nn2=np.zeros(P, np.int32),
               mp2=np.zeros((P, MN), np.uint8), kp2=np.zeros((P, MN), orbhip.KP_DTYPE), d2=np.zeros((P, MN, 32), np.uint8),
               ur2=np.full((P, MN), -1, np.float32), n2=np.zeros(P, np.int32), geom=np.zeros(P, orbhip.TRI_GENERAL_DTYPE),
               fast=np.zeros(P, orbhip.TRI_PAIR_DTYPE))
    assert orbhip.TRI_GENERAL_DTYPE == om.TRI_GENERAL_DTYPE
    for p, c in enumerate(cases):
        a, b = len(c["kp1"]), len(c["kp2"])
        i2, s2, f2 = om.feature_vector_csr(c["nid2"])
        arr["nid1"][p, :a] = c["nid1"]; arr["mp1"][p, :a] = c["mp1"]; arr["kp1"][p, :a] = c["kp1"]; arr["d1"][p, :a] = c["d1"]
        arr["ur1"][p, :a] = c["ur1"]; arr["n1"][p] = a
        arr["i2"][p, :len(i2)] = i2; arr["s2"][p, :len(s2)] = s2; arr["f2"][p, :len(f2)] = f2; arr["nn2"][p] = len(i2)
        arr["mp2"][p, :b] = c["mp2"]; arr["kp2"][p, :b] = c["kp2"]; arr["d2"][p, :b] = c["d2"]; arr["ur2"][p, :b] = c["ur2"]; arr["n2"][p] = b
        arr["geom"][p] = c["geom"]
        arr["fast"][p] = (c["F12"], c["ep"][0], c["ep"][1], int(c["only_stereo"]), int(c["coarse"]))
    return {k: _dev(v) for k, v in arr.items()}


def _tri_dims(cases, wide):
    MN = WIDE if wide else max(16, max(max(len(c["kp1"]), len(c["kp2"])) for c in cases))
    return MN, 8 + max(len(set(c["nid2"].tolist())) for c in cases)


def _tri_launch(gpu_ctx, kernel, t, c0, P, MNODE, MN, ori, mono):
    import torch
    import orbhip
    m12 = torch.full((P, MN), FILLV, dtype=torch.int32, device="cuda"); nm = torch.full((P,), FILLV, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda k: t[k].data_ptr()
    kf1 = [p("nid1"), p("mp1"), p("kp1"), p("d1"), 0 if mono else p("ur1"), p("n1")]
    kf2 = [p("i2"), p("s2"), p("f2"), p("nn2"), p("mp2"), p("kp2"), p("d2"), 0 if mono else p("ur2"), p("n2")]
    if kernel == "fast":
        orbhip.search_for_triangulation_device(gpu_ctx, kf1, kf2, p("fast"), P, MNODE, MN, MN, c0["scale"], c0["sigma2"], ori, m12.data_ptr(),
                                               nm.data_ptr())
    else:
        orbhip.search_for_triangulation_general_device(gpu_ctx, kf1, kf2, p("geom"), P, MNODE, MN, MN, c0["sigma2_1"], c0["scale"], c0["sigma2"], ori,
                                                       m12.data_ptr(), nm.data_ptr())
    return m12, nm


@pytest.mark.parametrize("ori", [True, False], ids=["ori", "no-ori"])
@pytest.mark.parametrize("form", ["fast-no-uright", "fast-uright", "fast-row-4104", "general", "general-row-4104"])
def test_search_for_triangulation_crafted(gpu_ctx, form, ori):
    """k_search_triangulation with null uRight pointers on the cases without stereo keypoints, with the arrays on all of them, at a row of
    4104 (LDS rows capped at 4096); k_search_triangulation_general<false, false> and <true, false> with one Pinhole camera on the same cases:
    the oracle's result, which is the fast kernel's -- the boundary rows of the unfused float expressions included"""
    mono = form == "fast-no-uright"
    cases = [c for c in bc.tri_cases() if not (mono and c["stereo"])]
    MN, MNODE = _tri_dims(cases, form.endswith("4104"))
    t = _tri_upload(cases, MN, MNODE)
    m12, nm = _tri_launch(gpu_ctx, "fast" if form.startswith("fast") else "general", t, cases[0], len(cases), MNODE, MN, ori, mono)
    gpu_ctx.check_status()
    m12, nm = m12.cpu().numpy(), nm.cpu().numpy()
    for p, c in enumerate(cases):
        n_ref, m_ref = _tri_oracle(c["name"], ori, mono)
        n = len(m_ref)
        assert nm[p] == n_ref, (c["name"], int(nm[p]), n_ref)
        bad = np.flatnonzero(m12[p, :n] != m_ref)
        assert bad.size == 0, (c["name"], [c["labels"][i] for i in bad[:8]], m12[p, bad[:8]], m_ref[bad[:8]])
        assert (m12[p, n:] == FILLV).all(), c["name"]


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("entry", ["frame", "kf", "rig", "tri-fast", "tri-general"])
def test_a_pair_beyond_the_row_is_refused(gpu_ctx, entry):
    """one launch of one pair whose feature count exceeds max_n: ORBHIP_E_CAPACITY through the status call, nmatches = 0, the rows untouched"""
    import orbhip
    if entry.startswith("tri"):
        c = bc.by_name("tri-n129")
        MN, MNODE = _tri_dims([c], False)
        t = _tri_upload([c], MN, MNODE)
        out, nm = _tri_launch(gpu_ctx, entry[4:], t, c, 1, MNODE, 128, True, False)
    else:
        c = bc.by_name("%s-%s-chain-distinct-40-40" % (entry, bc.FORM_RATIO[entry]))
        MN, MNODE = _bow_dims([c], False)
        t = _bow_upload([c], MN, MNODE)
        out, nm = _bow_launch(gpu_ctx, entry, t, 1, MNODE, 32, c["ratio"], True)
    with pytest.raises(orbhip.OrbHipError) as e:
        gpu_ctx.check_status()
    assert e.value.code == orbhip.E_CAPACITY
    gpu_ctx.check_status()                                           # reported once, then clear
    assert nm.cpu().numpy().tolist() == [0] and (out.cpu().numpy() == FILLV).all()
