"""Seeded scenes for Frame::isInFrustum / Tracking::SearchLocalPoints: one camera (or a two-camera fisheye rig) with a small pose offset,
points in a box that reaches behind the camera and beyond the image, per-point reference distances spread over every octave and past both
ends of the scale-invariance range, normals scattered around the viewing ray.  A scene must produce every outcome at least 8 times per
camera and every predicted level: histogram() counts them and the tests assert it."""
import numpy as np
import frustum_model as fm

f32 = np.float32
KINDS = ("mono", "stereo", "rig")


def _rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


def make_frame(kind, seed=0, nlevels=8, scale_factor=1.2, th=1.0, far_points=False, th_far_points=0.0, limit=0.5):
    """the per-frame record as a dict (frustum_model's `fr`), built with the roundings of host/cvmath.h"""
    rng = np.random.default_rng(1000 + seed)
    R = _rot(0, rng.uniform(-0.05, 0.05)) @ _rot(1, rng.uniform(-0.05, 0.05)) @ _rot(2, rng.uniform(-0.05, 0.05))
    Tcw = np.eye(4, dtype=f32)
    Tcw[:3, :3] = R.astype(f32); Tcw[:3, 3] = rng.uniform(-0.3, 0.3, 3).astype(f32)
    fr = dict(kind=kind, Tcw=Tcw, rig=int(kind == "rig"), nlevels=nlevels, th=f32(th), far_points=int(far_points), th_far_points=f32(th_far_points),
              viewing_cos_limit=f32(limit), mbf=f32(40.0 if kind == "stereo" else 0.0))
    if kind == "rig":                                              # two KannalaBrandt8 cameras, 512 x 512 (TUM-VI like)
        fr["cam"] = np.array([[190.98, 190.97, 254.93, 256.9, 0.0034, 0.0007, -0.002, 0.0002],
                              [190.44, 190.43, 252.6, 254.9, 0.0034, 0.0003, -0.0016, 0.0001]], f32)
        fr["cam_type"] = np.array([1, 1], np.int32)
        fr["bounds"] = (f32(0), f32(0), f32(512), f32(512))
        Rlr = _rot(1, 0.02) @ _rot(0, -0.01)
        Tlr = np.zeros((3, 4), f32); Tlr[:, :3] = Rlr.astype(f32); Tlr[:, 3] = np.array([0.101, 0.002, -0.001], f32)
        Trl = np.zeros((3, 4), f32); Trl[:, :3] = Rlr.T.astype(f32); Trl[:, 3] = (-Rlr.T @ Tlr[:, 3].astype(np.float64)).astype(f32)
        fr["Tlr"], fr["Trl"] = Tlr, Trl
        fr.update(fm.pose_matrices(Tcw, Trl, Tlr))
    else:                                                          # a 752 x 480 pinhole (EuRoC like)
        fr["cam"] = np.array([[458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0], [0] * 8], f32)
        fr["cam_type"] = np.array([0, -1], np.int32)
        fr["bounds"] = (f32(0), f32(0), f32(752), f32(480))
        fr.update(fm.pose_matrices(Tcw))
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))                 # ORBextractor.cc:418-424
    fr["scale_factors"] = np.array(sf, f32)
    fr["log_scale_factor"] = fm.logf(f32(scale_factor))            # Frame.cc:95: mfLogScaleFactor = log(mfScaleFactor)
    return fr


def make_points(fr, n, seed=0):
    """n local map points as the dict frustum_model takes (Xw, normal, min_dist, max_dist, flags, desc, track_depth)"""
    rng = np.random.default_rng(2000 + seed)
    Tcw = fr["Tcw"].astype(np.float64)
    Rwc, Ow = Tcw[:3, :3].T, -Tcw[:3, :3].T @ Tcw[:3, 3]
    z = rng.uniform(-2.0, 12.0, n)
    z[np.abs(z) < 0.05] = 0.05
    half = 1.9 if fr["rig"] else 1.15                               # x / z, y / z reach beyond the image
    xc = rng.uniform(-half, half, n) * np.maximum(np.abs(z), 0.5) * (5.0 if fr["rig"] else 1.0)
    yc = rng.uniform(-half, half, n) * np.maximum(np.abs(z), 0.5) * (5.0 if fr["rig"] else 1.0) * (1.0 if fr["rig"] else 0.7)
    keep = rng.random(n) < (0.45 if fr["rig"] else 0.35)            # a share of the points well inside the image
    xc[keep] *= 0.3; yc[keep] *= 0.3
    Pc = np.stack([xc, yc, z], 1)
    Xw = (Pc @ Rwc.T + Ow).astype(f32)
    PO = Xw.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    nl = int(fr["nlevels"]); sfac = float(fr["scale_factors"][1]) if nl > 1 else 1.2
    e = rng.uniform(-2.0, nl + 1.0, n)                              # octave the point was created at, and some way past both ends
    max_dist = (dist * sfac ** e).astype(f32)                       # MapPoint.cc:455-460: mfMaxDistance = dist * levelScaleFactor
    min_dist = (max_dist / f32(sfac ** (nl - 1))).astype(f32)       #                      mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1]
    ray = PO / dist[:, None]
    ang = np.abs(rng.normal(0.0, np.radians(25.0), n))
    near = rng.random(n) < 0.3
    ang[near] = rng.uniform(0.0, np.radians(3.0), near.sum())       # viewCos above 0.998: the small radius
    wide = rng.random(n) < 0.15
    ang[wide] = rng.uniform(np.radians(50.0), np.radians(90.0), wide.sum())
    t = np.cross(ray, rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=1)[:, None]
    normal = (ray * np.cos(ang)[:, None] + t * np.sin(ang)[:, None]).astype(f32)
    flags = (rng.random(n) < 0.85).astype(np.uint8) | ((rng.random(n) < 0.03).astype(np.uint8) << 1)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    track_depth = (dist * rng.uniform(0.5, 1.5, n)).astype(f32)      # what an earlier frame left in mTrackDepth
    return dict(Xw=Xw, normal=normal, min_dist=min_dist, max_dist=max_dist, flags=flags, desc=desc, track_depth=track_depth)


def make_scene(kind, n=1000, seed=0, **kw):
    fr = make_frame(kind, seed, **kw)
    return fr, make_points(fr, n, seed)


def histogram(fr, rec):
    """outcome counts per camera and the accepted points' level counts"""
    h = dict(left=np.bincount(rec["code"], minlength=8)[:8], levels=np.bincount(rec["level"][rec["code"] == 0], minlength=int(fr["nlevels"])))
    if fr["rig"]:
        h["right"] = np.bincount(rec["code_r"], minlength=8)[:8]
        h["levels_r"] = np.bincount(rec["level_r"][rec["code_r"] == 0], minlength=int(fr["nlevels"]))
    return h


def assert_covers(fr, rec, least=8):
    """every outcome at least `least` times per camera, every level predicted"""
    h = histogram(fr, rec)
    assert h["left"].min() >= least, h
    assert h["levels"].min() >= 1, h
    if fr["rig"]:
        assert h["right"].min() >= least and h["levels_r"].min() >= 1, h
    return h


def frame_record(fr, n_points, thresholds, dtype):
    """one orbhip_frustum_frame (dtype = orbhip.FRUSTUM_FRAME_DTYPE) from the dict"""
    r = np.zeros(1, dtype)[0]
    for k in ("Rcw", "tcw", "Ow", "Rrw", "trw", "Orw", "cam", "cam_type", "rig", "mbf", "nlevels", "th", "far_points", "th_far_points", "viewing_cos_limit"):
        r[k] = fr[k]
    nl = int(fr["nlevels"])
    r["scale_factors"][:nl] = fr["scale_factors"]
    r["level_thresholds"][:nl - 1] = thresholds
    r["n_points"] = n_points
    return r


# ---------------------------------------------------------------- boundary rows: crafted points whose outcome is written by hand
def boundary_rows():
    """[(fr, pts, names, codes [n][2], queries_expected [n] (number of queries the row emits), radius {row name: radius})]: one
    single-camera frame and one rig frame.  Identity rotation, a pinhole with fx = fy = cx = cy = 256 and bounds 0..512, so that every
    quantity of a row is exact in float and its expected code follows from the reference text alone:
      u_min / u_max / v_min / v_max   the projection lies ON the bound: `uv.x<mnMinX || uv.x>mnMaxX` is false, accepted
      near / far                      dist == 0.8f*min, dist == 1.2f*max: `dist<minDistance || dist>maxDistance` is false, accepted
      cos_limit                       viewCos == viewingCosLimit: `viewCos<viewingCosLimit` is false, accepted
      cos_hi / cos_lo                 viewCos = the floats either side of 0.998 (as doubles): radius 2.5 and 4.0 (RadiusByViewingCos)
      neg_zero                        PcZ == -0.0f is not < 0: the projection divides by it, u = +inf, "u outside" (3), not "negative depth"
      nan_u                           PcZ == 0 and x == 0: u is NaN and passes both u tests, v = +inf: "v outside" (4), not "u outside"
      skipped                         flag bit 1
    The rig frame (right camera one unit to the right): right_only_far / right_only_near are outside the left image and inside the right
    one, with a stale mTrackDepth above / below thFarPoints: the first emits no query, the second its right query."""
    one = f32(1.0)
    Tcw = np.eye(4, dtype=f32)
    Tcw[:3, 3] = f32(-0.0)                                         # tcw = -0: the only way Pc.z can come out as -0 (cvmath.h: (double)sum + (double)t)
    cam = np.array([[256, 256, 256, 256, 0, 0, 0, 0], [256, 256, 256, 256, 0, 0, 0, 0]], f32)
    base = dict(Tcw=Tcw, nlevels=8, th=one, far_points=0, th_far_points=f32(0), viewing_cos_limit=f32(0.5), mbf=f32(0), cam=cam,
                bounds=(f32(0), f32(0), f32(512), f32(512)))
    sfs = [one]
    for _ in range(7):
        sfs.append(f32(sfs[-1] * f32(1.2)))
    base["scale_factors"] = np.array(sfs, f32); base["log_scale_factor"] = fm.logf(f32(1.2))
    near_d, far_d = f32(0.8) * f32(2.5), f32(1.2) * f32(2.5)
    hi = f32(0.998); lo = np.nextafter(hi, f32(0))
    assert np.float64(hi) > 0.998 and not np.float64(lo) > 0.998
    rows = [  # name, X, normal, min, max, flag, code
        ("u_min", (-1, 0, 1), (0, 0, 1), 0.5, 4, 1, 0), ("u_max", (1, 0, 1), (0, 0, 1), 0.5, 4, 1, 0),
        ("v_min", (0, -1, 1), (0, 0, 1), 0.5, 4, 1, 0), ("v_max", (0, 1, 1), (0, 0, 1), 0.5, 4, 1, 0),
        ("near", (0, 0, near_d), (0, 0, 1), 2.5, 40, 1, 0), ("far", (0, 0, far_d), (0, 0, 1), 0.1, 2.5, 1, 0),
        ("cos_limit", (0, 0, 2), (0, 0, 0.5), 0.5, 4, 1, 0), ("cos_hi", (0, 0, 1), (0, 0, hi), 0.5, 4, 1, 0), ("cos_lo", (0, 0, 1), (0, 0, lo), 0.5, 4, 0, 0),
        ("neg_zero", (-1, -1, -0.0), (0, 0, 1), 0.5, 4, 1, 3), ("nan_u", (-0.0, -1, -0.0), (0, 0, 1), 0.5, 4, 1, 4),
        ("skipped", (0, 0, 1), (0, 0, 1), 0.5, 4, 3, 1), ("inside", (0.25, 0.25, 1), (0, 0, 1), 0.5, 4, 1, 0), ("behind", (0, 0, -1), (0, 0, 1), 0.5, 4, 1, 2)]

    def pts_of(rows, depth):
        n = len(rows)
        rng = np.random.default_rng(77)
        return dict(Xw=np.array([r[1] for r in rows], f32), normal=np.array([r[2] for r in rows], f32), min_dist=np.array([r[3] for r in rows], f32),
                    max_dist=np.array([r[4] for r in rows], f32), flags=np.array([r[5] for r in rows], np.uint8),
                    desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), track_depth=np.array(depth, f32))
    fr1 = dict(base, kind="mono", rig=0, cam_type=np.array([0, -1], np.int32), **fm.pose_matrices(Tcw))
    codes1 = np.array([[r[6], 255] for r in rows], np.uint8)
    nq1 = np.array([1 if r[6] == 0 else 0 for r in rows])
    radius1 = {"cos_hi": f32(f32(2.5) * sfs[7]), "cos_lo": f32(f32(4.0) * sfs[7])}       # ratio 4: past the last level threshold (1.2^6 = 2.99)
    out = [(fr1, pts_of(rows, [0] * len(rows)), [r[0] for r in rows], codes1, nq1, radius1)]
    Trl = np.zeros((3, 4), f32); Trl[:, :3] = np.eye(3); Trl[0, 3] = -1
    Tlr = np.zeros((3, 4), f32); Tlr[:, :3] = np.eye(3); Tlr[0, 3] = 1
    T2 = np.eye(4, dtype=f32)
    fr2 = dict(base, kind="rig", Tcw=T2, rig=1, cam_type=np.array([0, 0], np.int32), far_points=1, th_far_points=f32(5), Trl=Trl, Tlr=Tlr,
               **fm.pose_matrices(T2, Trl, Tlr))
    rows2 = [("right_only_far", (1.5, 0, 1), (0, 0, 1), 0.5, 4, 1, 3, 0), ("right_only_near", (1.5, 0, 1), (0, 0, 1), 0.5, 4, 1, 3, 0),
             ("both", (0.5, 0, 1), (0, 0, 1), 0.5, 4, 1, 0, 0), ("left_only", (-0.5, 0, 1), (0, 0, 1), 0.5, 4, 1, 0, 3), ("skipped", (0.5, 0, 1), (0, 0, 1), 0.5, 4, 2, 1, 1)]
    codes2 = np.array([[r[6], r[7]] for r in rows2], np.uint8)
    out.append((fr2, pts_of(rows2, [9, 2, 9, 9, 0]), [r[0] for r in rows2], codes2, np.array([0, 1, 2, 1, 0]), {}))
    return out


# ---------------------------------------------------------------- a train frame for the matcher behind the frustum kernel
def make_train_frame(fr, pts, rec, seed=0, n_target=300, first=(), jitter=1.0):
    """Keypoints for the frame `fr` built FROM the projections of the accepted points (rec: the model's records): about n_target keypoints
    near them at the predicted octave, descriptors = the point's with a few flipped bits; twins one pixel away with one more flipped bit
    (the ratio rule rejects the pair), some keypoints claimed before the search.  Rival points (add_rivals) share one keypoint: the
    order of claims decides between them; `first` lists points that must get a keypoint; jitter: how far (pixels) a left keypoint
    may lie from its point's projection (beyond the smallest search radius, th decides what is found).
    Returns dict(kp, desc, u_right or None, nleft, mirror or None, train_match)."""
    import oracle_match_bind as omb
    rng = np.random.default_rng(3000 + seed)
    rig = bool(fr["rig"])
    kps, descs, side, src = [], [], [], []

    def flip(d, nbits):
        d = d.copy()
        for b in rng.choice(256, nbits, replace=False):
            d[b >> 3] ^= 1 << (b & 7)
        return d

    def add(x, y, octave, d, right, point):
        kps.append((x, y, 31.0, 0.0, 1.0, int(octave), -1)); descs.append(d); side.append(right); src.append(point)
    acc = np.flatnonzero(rec["code"] == 0)
    first = [int(i) for i in first]                                # (rivals: their shared keypoint must exist)
    pick = (first + [int(i) for i in rng.permutation(acc) if int(i) not in set(first)])[:n_target * 3 // 4]
    for k, i in enumerate(pick):
        r = rec[i]
        lv = int(r["level"]) - (1 if (k % 3 == 0 and r["level"] > 0) else 0)
        add(f32(r["proj_x"] + rng.uniform(-jitter, jitter)), f32(r["proj_y"] + rng.uniform(-jitter, jitter)), lv, flip(pts["desc"][i], 5), False, int(i))
        if k % 6 == 1:                                             # a twin at the same octave, one bit further: best > 0.8 * second
            add(f32(kps[-1][0] + 1), kps[-1][1], lv, flip(pts["desc"][i], 6), False, int(i))
    if rig:
        accr = np.flatnonzero(rec["code_r"] == 0)
        for k, i in enumerate(rng.permutation(accr)[:n_target // 3]):
            r = rec[i]
            add(f32(r["proj_xr"] + rng.uniform(-1, 1)), f32(r["proj_yr"] + rng.uniform(-1, 1)), int(r["level_r"]), flip(pts["desc"][i], 4), True, int(i))
    order = np.argsort(side, kind="stable")                        # left keypoints first, then the right camera's
    kp = np.array([kps[j] for j in order], omb.KP_DTYPE); desc = np.array([descs[j] for j in order], np.uint8).reshape(-1, 32)
    src = np.array(src)[order]
    nleft = int(np.sum(~np.array(side, bool)))
    out = dict(kp=kp, desc=desc, nleft=nleft if rig else -1, src=src)
    out["u_right"] = None
    if fr["kind"] == "stereo":
        ur = np.full(len(kp), -1, f32)
        for j in range(len(kp)):
            if j % 2 == 0:
                ur[j] = f32(rec["proj_xr"][src[j]] + rng.uniform(-1, 1))
        out["u_right"] = ur
    out["mirror"] = None
    if rig:
        mirror = np.full(len(kp), -1, np.int32)
        first = {}
        for j in range(len(kp)):
            first.setdefault((int(src[j]), j >= nleft), j)
        for (p, right), j in first.items():
            if not right and (p, True) in first and p % 2 == 0:
                mirror[j] = first[(p, True)]; mirror[first[(p, True)]] = j
        out["mirror"] = mirror
    tm = np.full(len(kp), -1, np.int32)
    tm[rng.random(len(kp)) < 0.08] = -2                            # keypoints that hold a map point with observations already
    out["train_match"] = tm
    return out


def add_rivals(pts, rec, count=40):
    """For `count` accepted points i (rec: the model's records of pts) point i + 1 becomes a rival of point i: the same position, normal
    and distances, the descriptor one bit away.  Done BEFORE the model runs for the test: a rival is an ordinary point of the list."""
    n = len(rec)
    rivals = [int(i) for i in np.flatnonzero(rec["code"] == 0) if i % 2 == 0 and i + 1 < n][:count]
    for i in rivals:
        for k in ("Xw", "normal", "min_dist", "max_dist"):
            pts[k][i + 1] = pts[k][i]
        pts["desc"][i + 1] = pts["desc"][i]
        pts["desc"][i + 1, 0] ^= 1
        pts["flags"][i + 1] = 1
        pts["flags"][i] |= 1
    return rivals


# ---------------------------------------------------------------- lib/host_frustum_smoke: the class members on stand-in objects
def write_flat(path, arrays):
    """named flat arrays (host/flatfile.h): uint8 kept, float -> float32, integer -> int32"""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint8:
                kind, raw = 2, a.reshape(-1)
            elif a.dtype.kind == "f":
                kind, raw = 1, a.astype(np.float32).reshape(-1)
            else:
                kind, raw = 0, a.astype(np.int32).reshape(-1)
            f.write(name.encode().ljust(24, b"\0")[:24]); f.write(struct.pack("<ii", kind, raw.size)); f.write(raw.tobytes())


def read_flat(path):
    import struct
    out = {}
    with open(path, "rb") as f:
        (n,) = struct.unpack("<i", f.read(4))
        for _ in range(n):
            name = f.read(24).split(b"\0")[0].decode()
            kind, cnt = struct.unpack("<ii", f.read(8))
            dt = (np.int32, np.float32, np.uint8)[kind]
            out[name] = np.frombuffer(f.read(cnt * np.dtype(dt).itemsize), dt).copy()
    return out


def initial_state(n, seed=0):
    """what an earlier frame left in the points' mTrack* fields: trk_f [n][8], trk_i [n][4] (host_frustum_smoke.cc)"""
    rng = np.random.default_rng(4000 + seed)
    trk_f = rng.uniform(1.0, 300.0, (n, 8)).astype(f32)
    trk_i = np.stack([rng.integers(0, 8, n), rng.integers(0, 8, n), rng.integers(0, 2, n), rng.integers(0, 2, n)], 1).astype(np.int32)
    return trk_f, trk_i


def smoke_input(fr, pts, trk_f, trk_i, train=None, bad=None, last_seen=None, fmp=None, sensor=0, imu_init=0, ba2=0, frame_id=10, last_reloc=0, state=2):
    """the flat file of host_frustum_smoke for a frame dict, its points and (optionally) a make_train_frame result"""
    n = len(pts["flags"])
    N = 0 if train is None else len(train["kp"])
    a = dict(nleft=[train["nleft"] if train is not None else (0 if fr["rig"] else -1)], cam_type=[fr["cam_type"][0]], cam_type2=[max(int(fr["cam_type"][1]), 0)],
             nlevels=[fr["nlevels"]], far_points=[fr["far_points"]], sensor=[sensor], imu_init=[imu_init], ba2=[ba2], frame_id=[frame_id], last_reloc=[last_reloc],
             state=[state], Tcw=fr["Tcw"], Trl=fr.get("Trl", np.zeros((3, 4), f32)), Tlr=fr.get("Tlr", np.zeros((3, 4), f32)), cam=fr["cam"][0], cam2=fr["cam"][1],
             bounds=np.array(fr["bounds"], f32), mbf=[fr["mbf"]], scale=fr["scale_factors"], log_scale=[fr["log_scale_factor"]], th_far=[fr["th_far_points"]],
             limit=[fr["viewing_cos_limit"]], X=pts["Xw"], normal=pts["normal"], min_dist=pts["min_dist"], max_dist=pts["max_dist"],
             nobs=(pts["flags"] & 1).astype(np.int32) * 3, bad=np.zeros(n, np.int32) if bad is None else bad,
             last_seen=np.zeros(n, np.int32) if last_seen is None else last_seen, skip=((pts["flags"] >> 1) & 1).astype(np.int32), desc=pts["desc"],
             trk_f=trk_f, trk_i=trk_i, kp=np.zeros(0, f32), oct=np.zeros(0, np.int32), desc_kp=np.zeros(0, np.uint8), ur=np.zeros(0, f32),
             mirror=np.zeros(0, np.int32), fmp=np.zeros(0, np.int32))
    if train is not None:
        a.update(kp=np.stack([train["kp"]["x"], train["kp"]["y"]], 1), oct=train["kp"]["octave"], desc_kp=train["desc"],
                 ur=train["u_right"] if train["u_right"] is not None else np.zeros(0, f32),
                 mirror=train["mirror"] if train["mirror"] is not None else np.full(N, -1, np.int32), fmp=np.full(N, -1, np.int32) if fmp is None else fmp)
    return a


def points_from_state(pts, trk_f, trk_i, bad=None, last_seen=None):
    """frustum_model.MP objects for the points of a smoke input"""
    n = len(pts["flags"])
    return [fm.MP(i, bool(bad[i]) if bad is not None else False, int(pts["flags"][i] & 1) * 3, int(last_seen[i]) if last_seen is not None else 0,
                  list(trk_f[i]) + list(trk_i[i])) for i in range(n)]


def state_arrays(mps):
    """(trk_f [n][8], trk_i [n][4], visible [n], last_seen [n]) of a list of frustum_model.MP, as host_frustum_smoke writes them"""
    tf = np.array([[p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR, p.mTrackProjYR, p.mTrackDepth, p.mTrackDepthR, p.mTrackViewCos, p.mTrackViewCosR] for p in mps], f32)
    ti = np.array([[p.mnTrackScaleLevel, p.mnTrackScaleLevelR, int(p.mbTrackInView), int(p.mbTrackInViewR)] for p in mps], np.int32)
    return tf.reshape(-1, 8), ti.reshape(-1, 4), np.array([p.mnVisible for p in mps], np.int32), np.array([p.mnLastFrameSeen for p in mps], np.int32)
