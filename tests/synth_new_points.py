"""Scenes for LocalMapping::CreateNewMapPoints (tests/new_points_model.py): one current keyframe and its neighbours seeing the same
synthetic points, in the reference's three camera set-ups:
  'mono'    single Pinhole cameras, no stereo keypoints;
  'stereo'  rectified-stereo Pinhole keyframes (mvuRight, mvDepth, mb; mvKeys differs from mvKeysUn by a small smooth distortion);
  'rig'     two-camera KannalaBrandt8 rigs (NLeft != -1, keypoints left | right): all four camera combinations.
A pair (current keyframe, neighbour) carries what the device entry point reads, a match list, and CRAFTED matches: keypoints overwritten
so that the match ends in a chosen outcome code with every decision quantity at least 1 % away from its threshold (found by seeded random
proposals -- a good point, a far one, one behind both cameras, one between the cameras, one near the line of motion, keypoints pushed
off their rays, octaves that disagree with the distances, stereo depths <= 0 -- kept when new_point_f64 gives the wanted code with that margin).  Two outcomes need a
construction: w == 0 (two cameras with Rcw = I looking past each other: the smallest singular vector is exactly a direction) and a zero
distance (the centre the pair hands in IS the triangulated point): degenerate_pair()."""
import numpy as np

import new_points_model as npm
import oracle_match_bind as om

KP = om.KP_DTYPE
PIN = np.array([458.0, 457.0, 367.0, 248.0, 0, 0, 0, 0], np.float32)
KBL = np.array([190.9, 190.8, 254.9, 256.8, 0.0034, 0.0007, -0.0020, 0.0002], np.float32)
KBR = np.array([190.4, 190.6, 252.7, 255.0, 0.0031, 0.0009, -0.0019, 0.0003], np.float32)
RRL = om._rot([0.1, 1.0, 0.05], 0.02); TRL = np.array([-0.101, 0.0007, 0.0012])      # X_right = RRL X_left + TRL
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
LV = (SIGMA2, SCALE, SIGMA2, SCALE)
MB = np.float32(0.11)
REL = [(([0.0, 1.0, 0.1], 0.06), (0.35, 0.02, 0.15)), (([1.0, 0.2, 0.0], -0.04), (-0.30, 0.05, 0.40)),
       (([0.2, 0.1, 1.0], 0.08), (0.10, -0.25, -0.50)), (([0.3, 1.0, 0.3], -0.07), (0.50, 0.10, 0.05))]   # X1 = R X2 + t per neighbour
MARGIN = 0.01


def _cams(kind):
    if kind == "rig":
        return 1, KBL, KBR
    return 0, PIN, PIN


def _poses(kind, R, t):
    """[left, right] (R, t) world -> camera"""
    return [(R, t), (RRL @ R, RRL @ t + TRL)] if kind == "rig" else [(R, t)]


def _proj(ctype, cam, Xc):
    return om.kb8_project_np((ctype, cam.astype(np.float64)), Xc)


def _keyframe(kind, rng, R, t, mb):
    return dict(kind=kind, poses=_poses(kind, R, t), mb=np.float32(mb))


def _fill_pair_record(kf1, kf2, far):
    kind = kf1["kind"]; ctype, camL, camR = _cams(kind)
    P = np.zeros(1, npm.PAIR_DTYPE)[0]
    P["cam1"][0] = camL; P["cam1"][1] = camR; P["cam2"][0] = camL; P["cam2"][1] = camR
    P["cam1_type"][:] = ctype; P["cam2_type"][:] = ctype
    for name, kf in (("1", kf1), ("2", kf2)):
        for c, (R, t) in enumerate(kf["poses"]):
            P["Tcw" + name][c] = np.concatenate([R, t[:, None]], 1).astype(np.float32).reshape(12)
            P["Ow" + name][c] = (-R.T @ t).astype(np.float32)
        R, t = kf["poses"][0]
        P["Twc" + name] = np.concatenate([R.T, (-R.T @ t)[:, None]], 1).astype(np.float32).reshape(12)
    P["mb1"], P["mb2"] = kf1["mb"], kf2["mb"]
    P["mbf"] = np.float32(kf1["mb"] * camL[0])
    P["ratio_factor"] = np.float32(1.5) * np.float32(1.2)
    P["far_points"], P["th_far_points"] = int(far), np.float32(6.5)
    return P


def _observe(kind, rng, kf, Xw, right, noise, stereo_frac):
    """keypoints of world points in a keyframe: (kp, kp_raw, ur, depth)"""
    ctype, camL, camR = _cams(kind)
    n = len(Xw)
    kp = np.zeros(n, KP); ur = np.full(n, -1, np.float32); depth = np.full(n, -1, np.float32)
    for i in range(n):
        R, t = kf["poses"][1 if right[i] else 0]
        Xc = R @ Xw[i] + t
        uv = _proj(ctype, camR if right[i] else camL, Xc if Xc[2] > 0 or ctype == 1 else -Xc) + rng.normal(0, 1.0, 2) * noise[i]
        kp["x"][i], kp["y"][i] = uv
        if kind == "stereo" and Xc[2] > 0.5 and rng.random() < stereo_frac:
            ur[i] = np.float32(kp["x"][i] - kf["mb"] * camL[0] / Xc[2] + rng.normal(0, 0.2))
            depth[i] = np.float32(kf["mb"] * camL[0]) / (kp["x"][i] - ur[i])
            if rng.random() < 0.05:
                depth[i] = rng.choice([0.0, -1.0])                          # a stereo keypoint whose UnprojectStereo is empty
    raw = kp.copy()
    if kind == "stereo":
        raw["x"] = kp["x"] + np.float32(1.5) * np.sin(kp["x"] / np.float32(90)); raw["y"] = kp["y"] + np.float32(1.5) * np.cos(kp["y"] / np.float32(70))
    return kp, raw, ur, depth


def make_world(kind, seed, n1=600, n2s=(600, 560, 600, 520)):
    """One current keyframe and len(n2s) neighbours.  Returns a dict with the keyframes' arrays and one pair dict per neighbour (no matches
    yet: craft / fill_matches or the chain's search fill them)."""
    rng = np.random.default_rng(seed)
    rig = kind == "rig"
    R1 = om._rot(rng.normal(size=3), rng.uniform(0.1, 0.4)); t1 = rng.uniform(-1, 1, 3)
    kf1 = _keyframe(kind, rng, R1, t1, MB)
    Xc = np.stack([rng.uniform(-3, 3, n1), rng.uniform(-2, 2, n1), rng.uniform(2, 10, n1)], 1)
    far = rng.random(n1) < 0.12
    Xc[far] *= (rng.uniform(8, 30, far.sum()))[:, None]
    Xw = (Xc - t1) @ R1                                                      # R1^T (Xc - t1)
    nl1 = int(n1 * 0.55) if rig else -1
    right1 = (np.arange(n1) >= nl1) if rig else np.zeros(n1, bool)
    kp1, raw1, ur1, depth1 = _observe(kind, rng, kf1, Xw, right1, np.full(n1, 0.3), 0.6)
    kp1["octave"] = rng.integers(0, 8, n1); kp1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    nid1 = (rng.integers(0, 60, n1) * 3 + 100).astype(np.int32)
    pairs = []
    for k, n2 in enumerate(n2s):
        (ax, ang), trel = REL[k % 4]
        Rrel = om._rot(ax, ang); trel = np.array(trel)
        R2 = Rrel.T @ R1; t2 = Rrel.T @ (t1 - trel)
        kf2 = _keyframe(kind, rng, R2, t2, MB * (np.float32(1.15) if k == 1 else np.float32(1.0)))
        src = np.concatenate([rng.permutation(n1)[:min(n1, n2)], rng.integers(0, n1, max(0, n2 - n1))])
        nl2 = int(n2 * 0.5) if rig else -1
        right2 = (np.arange(n2) >= nl2) if rig else np.zeros(n2, bool)
        kp2, raw2, ur2, depth2 = _observe(kind, rng, kf2, Xw[src], right2, rng.choice([0.2, 0.2, 1.0, 5.0], n2), 0.6)
        wild = rng.random(n2) < 0.1
        kp2["octave"] = np.where(wild, rng.integers(0, 8, n2), np.clip(kp1["octave"][src] + rng.integers(-1, 2, n2), 0, 7))
        kp2["angle"] = (kp1["angle"][src] + rng.normal(0, 4, n2)).astype(np.float32) % np.float32(360)
        noise = rng.integers(0, 256, (n2, 32), dtype=np.uint8) & rng.integers(0, 256, (n2, 32), dtype=np.uint8) & rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        noise[rng.random(n2) < 0.3] = 0
        d2 = d1[src] ^ noise
        nid2 = np.where(rng.random(n2) < 0.9, nid1[src], rng.integers(0, 70, n2) * 3 + 101).astype(np.int32)
        P = _fill_pair_record(kf1, kf2, far=k % 2 == 1)
        P["nleft1"], P["nleft2"] = nl1, nl2
        pr = dict(kind=kind, P=P, lv=LV, kp1=kp1.copy(), kp1_raw=raw1.copy(), ur1=ur1.copy(), depth1=depth1.copy(), kp2=kp2, kp2_raw=raw2, ur2=ur2,
                  depth2=depth2, src=src, d1=d1, d2=d2, nid1=nid1, nid2=nid2, kf1=kf1, kf2=kf2, mbf2=np.float32(kf2["mb"] * _cams(kind)[1][0]),
                  matches12=np.full(n1, -1, np.int32), crafted=[], Xw=Xw)
        pairs.append(pr)
    return dict(kind=kind, pairs=pairs, Xw=Xw)


# ------------------------------------------------------------------ crafted matches
def _propose(pr, rng, i, j):
    """overwrite KF1 keypoint i and KF2 keypoint j with one random proposal"""
    kind = pr["kind"]; ctype, camL, camR = _cams(kind); P = pr["P"]
    c1 = 1 if kind == "rig" and i >= P["nleft1"] else 0
    c2 = 1 if kind == "rig" and j >= P["nleft2"] else 0
    (Ra, ta), (Rb, tb) = pr["kf1"]["poses"][c1], pr["kf2"]["poses"][c2]
    mode = rng.choice(["good", "good", "far", "behind", "between", "near", "axis"])
    Ca, Cb = -Ra.T @ ta, -Rb.T @ tb
    if mode == "between":
        X = Ca + rng.uniform(0.2, 0.9) * (Cb - Ca) + rng.normal(0, 0.05, 3)
    elif mode == "axis":                                                      # near the line of motion: less ray parallax than stereo parallax
        D = rng.uniform(3, 12)
        X = Ca + rng.choice([-1.0, 1.0]) * D * (Cb - Ca) / np.linalg.norm(Cb - Ca) + rng.normal(0, 0.04 * D, 3)
    else:
        z = {"good": rng.uniform(2, 8), "near": rng.uniform(0.6, 2), "far": rng.uniform(60, 300), "behind": -rng.uniform(2, 8)}[mode]
        X = Ra.T @ (np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.25, 0.25) * z, z]) - ta)
    o1 = int(rng.integers(0, 8))
    o2 = int(np.clip(o1 + rng.integers(-1, 2), 0, 7)) if rng.random() < 0.7 else int(rng.integers(0, 8))
    push = rng.choice([0, 0, 1, 2])
    for which, (R, t, cam, kp, raw, ur, depth, idx, o, mb) in enumerate(((Ra, ta, camR if c1 else camL, pr["kp1"], pr["kp1_raw"], pr["ur1"], pr["depth1"], i, o1, pr["kf1"]["mb"]),
                                                                         (Rb, tb, camR if c2 else camL, pr["kp2"], pr["kp2_raw"], pr["ur2"], pr["depth2"], j, o2, pr["kf2"]["mb"]))):
        Xc = R @ X + t
        uv = _proj(ctype, cam, Xc if Xc[2] > 0 else -Xc)
        if push == which + 1:
            a = rng.uniform(0, 2 * np.pi)
            uv = uv + rng.uniform(2.5, 8) * float(SCALE[o]) * np.array([np.cos(a), np.sin(a)])
        kp["x"][idx], kp["y"][idx], kp["octave"][idx] = uv[0], uv[1], o
        ur[idx], depth[idx] = -1, -1
        if kind == "stereo" and rng.random() < 0.5:
            if Xc[2] > 0.3 and rng.random() < 0.85:
                ur[idx] = np.float32(kp["x"][idx] - P["mbf"] / Xc[2]); depth[idx] = np.float32(Xc[2])
            else:
                ur[idx] = np.float32(kp["x"][idx] - 3); depth[idx] = rng.choice([0.0, -1.0])
        raw["x"][idx] = kp["x"][idx]; raw["y"][idx] = kp["y"][idx]
        if kind == "stereo":
            raw["x"][idx] += np.float32(1.5) * np.sin(kp["x"][idx] / np.float32(90)); raw["y"][idx] += np.float32(1.5) * np.cos(kp["y"][idx] / np.float32(70))


def craft(pr, seed, per_code=2, tries=1500):
    """crafted matches of one pair: up to per_code per outcome code, on keypoint slots that carry no match yet"""
    rng = np.random.default_rng(seed)
    n1, n2 = len(pr["kp1"]), len(pr["kp2"])
    free1 = [int(i) for i in rng.permutation(n1) if pr["matches12"][i] < 0]
    used2 = set(int(j) for j in pr["matches12"] if j >= 0)
    free2 = [int(j) for j in rng.permutation(n2) if int(j) not in used2]
    have = {}
    for _ in range(tries):
        if not free1 or not free2:
            break
        i, j = free1[-1], free2[-1]
        keep = [a[idx].copy() for a, idx in ((pr["kp1"], i), (pr["kp1_raw"], i), (pr["ur1"], i), (pr["depth1"], i), (pr["kp2"], j), (pr["kp2_raw"], j),
                                             (pr["ur2"], j), (pr["depth2"], j))]
        _propose(pr, rng, i, j)
        pr["matches12"][i] = j
        a = npm.match_args(pr, i)
        code, _, margin = npm.new_point_f64(*a)
        ok = margin >= MARGIN and have.get(code, 0) < per_code and npm.new_point(*a)[0] == code
        if ok:
            have[code] = have.get(code, 0) + 1
            pr["crafted"].append(i); free1.pop(); free2.pop()
        else:
            pr["matches12"][i] = -1
            for (arr, idx), v in zip(((pr["kp1"], i), (pr["kp1_raw"], i), (pr["ur1"], i), (pr["depth1"], i), (pr["kp2"], j), (pr["kp2_raw"], j),
                                      (pr["ur2"], j), (pr["depth2"], j)), keep):
                arr[idx] = v
    return have


def fill_matches(pr, seed, count):
    """bring the pair's match list to `count` matches (crafted ones included): true correspondences, one in seven of them a wrong partner"""
    rng = np.random.default_rng(seed)
    first = {}
    for j, s in enumerate(pr["src"]):
        first.setdefault(int(s), j)
    used2 = set(int(j) for j in pr["matches12"] if j >= 0)
    have = int(np.sum(pr["matches12"] >= 0))
    assert have <= count
    for i in rng.permutation(len(pr["kp1"])):
        if have == count:
            break
        if pr["matches12"][i] >= 0:
            continue
        j = first.get(int(i), int(rng.integers(0, len(pr["kp2"]))))
        if rng.random() < 1 / 7:
            j = int(rng.integers(0, len(pr["kp2"])))
        if j in used2 and j in [int(pr["matches12"][c]) for c in pr["crafted"]]:
            continue                                                          # a crafted KF2 keypoint keeps its one partner
        pr["matches12"][i] = j; used2.add(j); have += 1
    assert have == count, (have, count)
    return pr


def degenerate_pair(kind):
    """Two exact constructions.  (a) w == 0: Rcw = I in both keyframes, tcw = (0, -+1, 0), keypoint 0 of KF1 at the principal point and its
    partner on the row of KF2's principal point: the columns of A are (-1,0,-1,0), (0,-1,0,-1), (0,0,x2,0), (0,1,0,-1): only columns 0
    and 2 are not orthogonal, the Jacobi rotations touch nothing else, and the smallest singular value (about x2 / sqrt 2 < sqrt 2)
    belongs to a vector in their plane -- its fourth component is an exact zero (the rays are skew: no point, a direction).
    (b) a zero distance: keypoint 1 is a good match, and the centre Ow2 the pair hands in is its triangulated point, bit for bit."""
    ctype, camL, camR = _cams(kind)
    I = np.eye(3)
    kf1 = dict(kind=kind, poses=_poses(kind, I, np.array([0.0, -1.0, 0.0])), mb=MB)
    kf2 = dict(kind=kind, poses=_poses(kind, I, np.array([0.0, 1.0, 0.0])), mb=MB)
    P = _fill_pair_record(kf1, kf2, far=False)
    n = 4
    P["nleft1"], P["nleft2"] = (n, n) if kind == "rig" else (-1, -1)        # every keypoint in the left cameras
    kp1 = np.zeros(n, KP); kp2 = np.zeros(n, KP)
    kp1["x"][0], kp1["y"][0] = camL[2], camL[3]
    kp2["x"][0], kp2["y"][0] = camL[2] + np.float32(0.3) * camL[0], camL[3]
    X = np.array([0.2, 0.1, 3.0])
    for kp, kf in ((kp1, kf1), (kp2, kf2)):
        R, t = kf["poses"][0]
        kp["x"][1], kp["y"][1] = _proj(ctype, camL, R @ X + t)
        kp["x"][2:], kp["y"][2:] = camL[2] + 10, camL[3] - 20
    m = np.array([0, 1, -1, -1], np.int32)
    neg = np.full(n, -1, np.float32)
    pr = dict(kind=kind, P=P, lv=LV, kp1=kp1, kp1_raw=kp1.copy(), ur1=neg.copy(), depth1=neg.copy(), kp2=kp2, kp2_raw=kp2.copy(), ur2=neg.copy(),
              depth2=neg.copy(), matches12=m, crafted=[0, 1], kf1=kf1, kf2=kf2, mbf2=P["mbf"], src=np.arange(n))
    code, x = npm.new_point(*npm.match_args(pr, 1))
    assert code == 1
    P["Ow2"][0] = x
    return pr


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)      # matches per pair of the ragged batch: the compaction and workgroup boundaries

_cache = {}


def scene(kind):
    """the ragged batch of one camera set-up: 8 pairs (two current keyframes with four neighbours each) with COUNTS matches and crafted
    matches in the larger ones, plus the degenerate pair.  Built once per process and shared (do not modify)."""
    if kind not in _cache:
        seed = {"mono": 11, "stereo": 12, "rig": 13}[kind]
        pairs = make_world(kind, seed)["pairs"] + make_world(kind, seed + 100, n1=520, n2s=(500, 600, 480, 600))["pairs"]
        # more matches -> later in the batch; the crafted ones go where there is room for them
        for p, (pr, cnt) in enumerate(zip(pairs, COUNTS)):
            if cnt >= 63:
                craft(pr, 1000 * seed + p)
            fill_matches(pr, 2000 * seed + p, cnt)
        pairs.append(degenerate_pair(kind))
        _cache[kind] = pairs
    return _cache[kind]


def chain_case(pr, mp1, mp2):
    """the dict oracle_match_bind.search_for_triangulation_general reads, for one pair of a world and the current flags"""
    kind = pr["kind"]; ctype, camL, camR = _cams(kind); P = pr["P"]
    g = np.zeros(1, om.TRI_GENERAL_DTYPE)[0]
    rig = kind == "rig"
    for c in range(4 if rig else 1):
        (Ra, ta), (Rb, tb) = pr["kf1"]["poses"][c >> 1], pr["kf2"]["poses"][c & 1]
        R12 = Ra @ Rb.T; t12 = ta - R12 @ tb
        g["R12"][c] = R12.astype(np.float32).reshape(9); g["t12"][c] = t12.astype(np.float32)
    g["cam1"][0] = camL; g["cam2"][0] = camL; g["cam1"][1] = camR; g["cam2"][1] = camR
    g["cam1_type"][:] = ctype; g["cam2_type"][:] = ctype
    if not rig:
        K = np.array([[PIN[0], 0, PIN[2]], [0, PIN[1], PIN[3]], [0, 0, 1]], np.float32)
        Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
        g["F12"][0] = (Kinv.T @ om.skew(g["t12"][0]) @ g["R12"][0].reshape(3, 3) @ Kinv).astype(np.float32).reshape(9)
    (Ra, ta), (Rb, tb) = pr["kf1"]["poses"][0], pr["kf2"]["poses"][0]
    ep = _proj(ctype, camL, Rb @ (-Ra.T @ ta) + tb)
    g["ep_x"], g["ep_y"] = np.float32(ep[0]), np.float32(ep[1])
    g["nleft1"], g["nleft2"] = P["nleft1"], P["nleft2"]
    return dict(kp1=pr["kp1"], d1=pr["d1"], nid1=pr["nid1"], mp1=mp1, ur1=pr["ur1"], kp2=pr["kp2"], d2=pr["d2"], nid2=pr["nid2"], mp2=mp2,
                ur2=pr["ur2"], geom=g, scale=SCALE, sigma2=SIGMA2, sigma2_1=SIGMA2)


def run_chain(pairs, carry=True, check_ori=True):
    """The reference's neighbour loop on the CPU: SearchForTriangulation (the oracle) then the model, per neighbour in order; with
    carry the flags a neighbour's points set are seen by the next search (:715 before ORBmatcher.cc:1039).  Returns per neighbour
    dict(matches12, outcome, x3D, n_created) and the final has_mp1."""
    n1 = len(pairs[0]["kp1"])
    mp1 = np.array(pairs[0].get("mp1_init", np.zeros(n1, np.uint8)), np.uint8)
    out = []
    for pr in pairs:
        mp2 = np.array(pr.get("mp2_init", np.zeros(len(pr["kp2"]), np.uint8)), np.uint8)
        _, m = om.search_for_triangulation_general(chain_case(pr, mp1.copy(), mp2), check_ori)
        q = dict(pr, matches12=m.copy(), mp1=mp1.copy(), mp2=mp2)
        r = npm.run_pair(q)
        if carry:
            mp1 = r["has_mp1"]
        out.append(dict(matches12=m.copy(), outcome=r["outcome"], x3D=r["x3D"], n_created=r["n_created"], has_mp2=r["has_mp2"]))
    return out, mp1


def chain_world(kind):
    """one current keyframe and 3 neighbours of 300 keypoints for the chain tests (shared; do not modify)"""
    key = ("chain", kind)
    if key not in _cache:
        _cache[key] = make_world(kind, {"mono": 31, "stereo": 32, "rig": 33}[kind], n1=300, n2s=(300, 280, 300))["pairs"]
    return _cache[key]


def chain_reference(kind, carry=True):
    """run_chain of chain_world(kind), computed once per process (shared; do not modify)"""
    key = ("chain_ref", kind, carry)
    if key not in _cache:
        _cache[key] = run_chain(chain_world(kind), carry)
    return _cache[key]


def class_case(kind, check_true_at=-1):
    """The class drop-in's scene: the chain world's current keyframe and 3 neighbours, every keyframe with some map points already, plus a
    neighbour the host-side tests skip (second in the covisibility order): its centre 0.02 from the current keyframe's -- below mb
    (:443), and below 0.01 of its median scene depth when monocular (:451).  Returns (the flat arrays of lib/host_newpoints_smoke, the
    pairs the model chain runs on, the keyframe number of each of those pairs).  check_true_at = 3: CheckNewKeyFrames turns true at its
    third call, i.e. before the last neighbour."""
    key = ("class", kind, check_true_at)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(77)
    base = chain_world(kind)
    ctype, camL, camR = _cams(kind)
    n1 = len(base[0]["kp1"])
    mp1_init = (rng.random(n1) < 0.1).astype(np.uint8)
    pairs = [dict(pr, mp1_init=mp1_init, mp2_init=(rng.random(len(pr["kp2"])) < 0.1).astype(np.uint8)) for pr in base]
    T44 = lambda r: np.concatenate([np.asarray(r, np.float32).reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)])
    a = dict(cam_type=np.array([ctype]), cam=camL, cam2=camR, monocular=np.array([int(kind == "mono")]), inertial=np.array([0]),
             far_points=np.array([1]), th_far=np.array([6.5], np.float32), scale=SCALE, sigma2=SIGMA2, check_true_at=np.array([check_true_at]))
    Tlr = np.eye(4); Tlr[:3, :3] = RRL.T; Tlr[:3, 3] = -RRL.T @ TRL
    a["tlr"] = Tlr.astype(np.float32)

    def put(k, Tcw, mb, kp, raw, ur, dp, desc, nid, mp, mpx):
        a["Tcw%d" % k] = Tcw; a["mb%d" % k] = np.array([mb], np.float32)
        a["kp%d" % k] = np.stack([kp["x"], kp["y"]], 1); a["raw%d" % k] = np.stack([raw["x"], raw["y"]], 1); a["oct%d" % k] = kp["octave"]
        a["ur%d" % k] = ur; a["dp%d" % k] = dp; a["desc%d" % k] = desc; a["nid%d" % k] = nid; a["mp%d" % k] = mp.astype(np.int32)
        a["mpx%d" % k] = mpx.astype(np.float32)
    p0 = pairs[0]
    put(0, T44(p0["P"]["Tcw1"][0]), p0["P"]["mb1"], p0["kp1"], p0["kp1_raw"], p0["ur1"], p0["depth1"], p0["d1"], p0["nid1"], mp1_init, p0["Xw"])
    order = [0, None, 1, 2]                                                  # None: the neighbour that is skipped
    nleft = [p0["P"]["nleft1"]]
    used, kf_of = [], []
    for k, which in enumerate(order, start=1):
        pr = pairs[0] if which is None else pairs[which]
        Tcw = T44(pr["P"]["Tcw2"][0])
        if which is None:
            Tcw = T44(p0["P"]["Tcw1"][0]).copy(); Tcw[0, 3] += np.float32(0.02)
        put(k, Tcw, pr["P"]["mb2"], pr["kp2"], pr["kp2_raw"], pr["ur2"], pr["depth2"], pr["d2"], pr["nid2"], pr["mp2_init"], pr["Xw"][pr["src"]])
        nleft.append(pr["P"]["nleft2"])
        if which is not None and not (check_true_at > 0 and k - 1 >= check_true_at):
            used.append(dict(pr, P=pr["P"].copy())); kf_of.append(k)
    a["nkf"] = np.array([len(order) + 1]); a["nleft"] = np.array(nleft)
    for pr in used:                                                          # the drop-in hands in mbFarPoints / mThFarPoints of the LocalMapping object
        pr["P"]["far_points"], pr["P"]["th_far_points"] = 1, np.float32(6.5)
    _cache[key] = (a, used, kf_of)
    return _cache[key]
