"""Frame::isInFrustum (src/Frame.cc:483-572), Frame::isInFrustumChecks (:1170-1243), the query builder of
ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:54-79, :149-156) and the bookkeeping of
Tracking::SearchLocalPoints (src/Tracking.cc:2358-2430), restated from the reference text in numpy float32 scalars, one operation at a time:

  Pc = R*P + t      cv::gemm's small-matrix path: the row's products summed in float, then (float)((double)sum + (double)t)
  cv::norm, dot     accumulated in double
  project           oracle_match_bind.camera_project_f
  log               the platform's logf through ctypes (numpy carries its own)

Every point gets an outcome code per camera: 0 accepted, 1 skipped, 2 negative depth, 3 u outside, 4 v outside, 5 too near, 6 too far,
7 viewing angle (255: the frame has no such camera).  `rules` can replace each strict comparison by its non-strict twin: the tests use
that to show that their boundary rows tell the right rule from the wrong one."""
import ctypes
import ctypes.util
import numpy as np
import oracle_match_bind as omb

f32, f64 = np.float32, np.float64
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float

TRACK_RECORD_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("proj_yr", "<f4"), ("depth", "<f4"), ("depth_r", "<f4"),
                               ("view_cos", "<f4"), ("view_cos_r", "<f4"), ("level", "<i4"), ("level_r", "<i4"), ("in_view", "u1"),
                               ("in_view_r", "u1"), ("code", "u1"), ("code_r", "u1")])
RIGHT_RULES = dict(bounds_strict=True, distance_strict=True, angle_strict=True)


def logf(x):
    return f32(_libm.logf(float(f32(x))))


def predict_scale(max_raw, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale (src/MapPoint.cc:514-546): None where the reference converts inf / NaN to int (undefined)"""
    with np.errstate(all="ignore"):
        ratio = f32(max_raw) / f32(dist)
        if not (ratio > 0 and np.isfinite(ratio)):
            return None
        n = int(np.ceil(f32(logf(ratio) / f32(log_scale_factor))))
    if n < 0:
        n = 0
    elif n >= nlevels:
        n = nlevels - 1
    return n


def level_by_expression(ratio, log_scale_factor, nlevels):
    """the expression of slam_types.h / MapPoint.cc on a ratio"""
    n = int(np.ceil(f32(logf(ratio) / f32(log_scale_factor))))
    return 0 if n < 0 else (nlevels - 1 if n >= nlevels else n)


def level_by_thresholds(ratio, thresholds):
    return int(np.count_nonzero(f32(ratio) >= np.asarray(thresholds, f32)))


# ---------------------------------------------------------------- CV_32F matrix expressions (host/cvmath.h)
def mul_add(A, x, c=None):
    """A*x (+ c): the small-matrix path"""
    A = np.asarray(A, f32).reshape(3, 3); x = np.asarray(x, f32)
    d = np.zeros(3, f32)
    for i in range(3):
        t = f32(f32(f32(A[i, 0] * x[0]) + f32(A[i, 1] * x[1])) + f32(A[i, 2] * x[2]))
        d[i] = f32(f64(t) + (f64(c[i]) if c is not None else f64(0)))
    return d


def mul33(A, B):
    A = np.asarray(A, f32).reshape(3, 3); B = np.asarray(B, f32).reshape(3, 3)
    D = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            D[i, j] = f32(f32(f32(A[i, 0] * B[0, j]) + f32(A[i, 1] * B[1, j])) + f32(A[i, 2] * B[2, j]))
    return D


def mul_t(A, x, alpha=1.0):
    """alpha * A^T * x: a transposed operand takes the general path (double sums)"""
    A = np.asarray(A, f32).reshape(3, 3); x = np.asarray(x, f32)
    d = np.zeros(3, f32)
    for i in range(3):
        s = f64(0)
        for k in range(3):
            s += f64(A[k, i]) * f64(x[k])
        d[i] = f32(s * alpha)
    return d


def norm3(a):
    s = f64(0)
    for i in range(3):
        s += f64(a[i]) * f64(a[i])
    return np.sqrt(s)


def dot3(a, b):
    s = f64(0)
    for i in range(3):
        s += f64(a[i]) * f64(b[i])
    return s


def pose_matrices(Tcw, Trl=None, Tlr=None):
    """Frame::UpdatePoseMatrices (Frame.cc:456-462) and the right camera's pose of isInFrustumChecks (:1176-1180)"""
    Tcw = np.asarray(Tcw, f32)
    Rcw, tcw = Tcw[:3, :3].copy(), Tcw[:3, 3].copy()
    Ow = mul_t(Rcw, tcw, -1.0)                                 # -mRcw.t()*mtcw
    out = dict(Rcw=Rcw.reshape(9), tcw=tcw, Ow=Ow, Rrw=np.zeros(9, f32), trw=np.zeros(3, f32), Orw=np.zeros(3, f32))
    if Trl is not None:
        Trl = np.asarray(Trl, f32); Tlr = np.asarray(Tlr, f32)
        Rwc = Rcw.T.copy()                                     # mRwc = mRcw.t(): a stored matrix, no transposed operand below
        out["Rrw"] = mul33(Trl[:3, :3], Rcw).reshape(9)
        out["trw"] = mul_add(Trl[:3, :3], tcw, Trl[:3, 3])
        out["Orw"] = mul_add(Rwc, Tlr[:3, 3], Ow)
    return out


# ---------------------------------------------------------------- one point, one camera
def camera_checks(fr, right, X, N, min_raw, max_raw, rules=RIGHT_RULES):
    """The tests both branches share (Frame.cc:497-541, :1189-1225) -> (code, dict(u, v, depth, invz, view_cos, level))"""
    R, t, O = (fr["Rrw"], fr["trw"], fr["Orw"]) if right else (fr["Rcw"], fr["tcw"], fr["Ow"])
    c = 1 if right else 0
    min_x, min_y, max_x, max_y = [f32(v) for v in fr["bounds"]]
    with np.errstate(all="ignore"):
        Pc = mul_add(R, X, t)
        o = dict(u=f32(0), v=f32(0), view_cos=f32(0), level=0)
        o["depth"] = f32(norm3(Pc))
        o["invz"] = f32(1.0) / Pc[2]
        if Pc[2] < f32(0):
            return 2, o
        uv = omb.camera_project_f(int(fr["cam_type"][c]), fr["cam"][c], Pc)
        lt = (lambda a, b: a < b) if rules["bounds_strict"] else (lambda a, b: a <= b)
        if lt(uv[0], min_x) or lt(max_x, uv[0]):
            return 3, o
        if lt(uv[1], min_y) or lt(max_y, uv[1]):
            return 4, o
        o["u"], o["v"] = uv[0], uv[1]
        PO = np.asarray(X, f32) - np.asarray(O, f32)
        dist = f32(norm3(PO))
        lt = (lambda a, b: a < b) if rules["distance_strict"] else (lambda a, b: a <= b)
        if lt(dist, f32(0.8) * f32(min_raw)):
            return 5, o
        if lt(f32(1.2) * f32(max_raw), dist):
            return 6, o
        o["view_cos"] = f32(dot3(PO, N) / f64(dist))
        lt = (lambda a, b: a < b) if rules["angle_strict"] else (lambda a, b: a <= b)
        if lt(o["view_cos"], f32(fr["viewing_cos_limit"])):
            return 7, o
        lv = predict_scale(max_raw, dist, fr["log_scale_factor"], int(fr["nlevels"]))
        o["level"] = 0 if lv is None else lv
        o["undefined"] = lv is None
    return 0, o


def frustum(fr, pts, rules=RIGHT_RULES):
    """isInFrustum over the points of a frame -> (records [n] TRACK_RECORD_DTYPE as orbhip_track_record defines them, nToMatch,
    undefined [n]: rows on which the reference's PredictScale is undefined)"""
    n = len(pts["flags"])
    rec = np.zeros(n, TRACK_RECORD_DTYPE)
    undefined = np.zeros(n, bool)
    rig = bool(fr["rig"])
    n_to_match = 0
    for i in range(n):
        r = rec[i]
        r["level"] = r["level_r"] = -1 if rig else 0
        r["code"], r["code_r"] = 1, (1 if rig else 255)
        if pts["flags"][i] & 2:
            continue
        X, N, mn, mx = pts["Xw"][i], pts["normal"][i], pts["min_dist"][i], pts["max_dist"][i]
        cl, L = camera_checks(fr, False, X, N, mn, mx, rules)
        r["code"] = cl
        if not rig:
            r["proj_x"] = r["proj_y"] = -1
            if cl == 0 or cl >= 5:
                r["proj_x"], r["proj_y"] = L["u"], L["v"]
            if cl == 0:
                r["in_view"] = 1
                r["proj_xr"] = L["u"] - f32(f32(fr["mbf"]) * L["invz"])
                r["depth"], r["level"], r["view_cos"] = L["depth"], L["level"], L["view_cos"]
                undefined[i] = L["undefined"]
        else:
            if cl == 0:
                r["in_view"] = 1
                r["proj_x"], r["proj_y"], r["level"], r["view_cos"], r["depth"] = L["u"], L["v"], L["level"], L["view_cos"], L["depth"]
                undefined[i] |= L["undefined"]
            cr, Rr = camera_checks(fr, True, X, N, mn, mx, rules)
            r["code_r"] = cr
            if cr == 0:
                r["in_view_r"] = 1
                r["proj_xr"], r["proj_yr"], r["level_r"], r["view_cos_r"], r["depth_r"] = Rr["u"], Rr["v"], Rr["level"], Rr["view_cos"], Rr["depth"]
                undefined[i] |= Rr["undefined"]
        if r["in_view"] or r["in_view_r"]:
            n_to_match += 1
    return rec, n_to_match, undefined


def radius_by_viewing_cos(view_cos):
    return f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)


def queries(fr, pts, rec):
    """host/ORBmatcher.cc:70-104 (ORBmatcher.cc:54-79, :149-156 of the reference) on the records -> (q, desc_q, owner)"""
    q, dq, owner = [], [], []
    rig = bool(fr["rig"])
    th = f32(fr["th"])
    sf = np.asarray(fr["scale_factors"], f32)
    stale = pts.get("track_depth")
    for i in range(len(rec)):
        r = rec[i]
        if not r["in_view"] and not r["in_view_r"]:
            continue
        depth = r["depth"] if r["in_view"] else (f32(stale[i]) if stale is not None else f32(0))       # mTrackDepth: stale unless the left camera accepted
        if fr["far_points"] and depth > f32(fr["th_far_points"]):
            continue
        obs = int(pts["flags"][i] & 1)
        if r["in_view"]:
            lv = int(r["level"])
            rad = radius_by_viewing_cos(r["view_cos"])
            if th != f32(1.0):
                rad = f32(rad * th)
            q.append((r["proj_x"], r["proj_y"], f32(rad * sf[lv]), r["proj_xr"], 0.0, lv - 1, lv, obs))
            dq.append(pts["desc"][i]); owner.append(i)
        if rig and r["in_view_r"]:
            lv = int(r["level_r"])
            if lv != -1:
                rad = radius_by_viewing_cos(r["view_cos_r"])
                q.append((r["proj_xr"], r["proj_yr"], f32(rad * sf[lv]), -1.0, 0.0, lv - 1, lv, obs | 2))
                dq.append(pts["desc"][i]); owner.append(i)
    return (np.array(q, omb.PROJ_QUERY_DTYPE).reshape(-1), np.array(dq, np.uint8).reshape(-1, 32), np.array(owner, np.int32).reshape(-1))


# ---------------------------------------------------------------- Tracking::SearchLocalPoints, the bookkeeping
class MP:
    """the MapPoint members Tracking::SearchLocalPoints and Frame::isInFrustum touch"""
    FIELDS = ("mTrackProjX", "mTrackProjY", "mTrackProjXR", "mTrackProjYR", "mTrackDepth", "mTrackDepthR", "mTrackViewCos", "mTrackViewCosR",
              "mnTrackScaleLevel", "mnTrackScaleLevelR", "mbTrackInView", "mbTrackInViewR", "mnVisible", "mnLastFrameSeen")

    def __init__(self, idx, bad, nobs, last_seen, init):
        self.idx, self.bad, self.nobs, self.mnLastFrameSeen, self.mnVisible = idx, bool(bad), int(nobs), int(last_seen), 1
        (self.mTrackProjX, self.mTrackProjY, self.mTrackProjXR, self.mTrackProjYR, self.mTrackDepth, self.mTrackDepthR, self.mTrackViewCos,
         self.mTrackViewCosR) = [f32(v) for v in init[:8]]
        self.mnTrackScaleLevel, self.mnTrackScaleLevelR, self.mbTrackInView, self.mbTrackInViewR = int(init[8]), int(init[9]), bool(init[10]), bool(init[11])

    def state(self):
        return tuple(float(getattr(self, k)) for k in self.FIELDS)


def apply_record(p, r, rig):
    """what Frame::isInFrustum writes into the MapPoint, from the record and its codes"""
    if not rig:
        p.mbTrackInView = bool(r["in_view"])
        p.mTrackProjX, p.mTrackProjY = f32(r["proj_x"]), f32(r["proj_y"])
        if r["code"] == 0:
            p.mTrackProjXR, p.mTrackDepth, p.mnTrackScaleLevel, p.mTrackViewCos = f32(r["proj_xr"]), f32(r["depth"]), int(r["level"]), f32(r["view_cos"])
    else:
        p.mbTrackInView, p.mbTrackInViewR = bool(r["in_view"]), bool(r["in_view_r"])
        p.mnTrackScaleLevel, p.mnTrackScaleLevelR = int(r["level"]), int(r["level_r"])
        if r["code"] == 0:
            p.mTrackProjX, p.mTrackProjY, p.mTrackViewCos, p.mTrackDepth = f32(r["proj_x"]), f32(r["proj_y"]), f32(r["view_cos"]), f32(r["depth"])
        if r["code_r"] == 0:
            p.mTrackProjXR, p.mTrackProjYR, p.mTrackViewCosR, p.mTrackDepthR = f32(r["proj_xr"]), f32(r["proj_yr"]), f32(r["view_cos_r"]), f32(r["depth_r"])


def choose_th(sensor, imu_initialized, inertial_ba2, frame_id, last_reloc_frame_id, state):
    """Tracking.cc:2406-2426.  sensor: System::eSensor (MONOCULAR 0, STEREO 1, RGBD 2, IMU_MONOCULAR 3, IMU_STEREO 4); state:
    Tracking::eTrackingState (RECENTLY_LOST 3, LOST 4)"""
    th = 1
    if sensor == 2:
        th = 3
    if imu_initialized:
        th = 2 if inertial_ba2 else 3
    elif sensor in (3, 4):
        th = 10
    if frame_id < last_reloc_frame_id + 2:
        th = 5
    if state in (3, 4):
        th = 15
    return th


def search_local_points(fr, pts, mps, frame_mp, frame_id, matcher):
    """Tracking::SearchLocalPoints (Tracking.cc:2358-2430).  mps: the local map points (MP, list order = pts order); frame_mp: the frame's
    mvpMapPoints (MP or None per keypoint), updated in place; fr["th"] etc. already chosen; matcher(q, dq) -> (nmatches, train_match) runs
    ORBmatcher::SearchByProjection's device part on the claims of frame_mp.  Returns (matches or None when the matcher was not run,
    mmProjectPoints {point index: (x, y)})."""
    for k, p in enumerate(frame_mp):                            # :2361-2378
        if p is not None:
            if p.bad:
                frame_mp[k] = None
            else:
                p.mnVisible += 1; p.mnLastFrameSeen = frame_id; p.mbTrackInView = False; p.mbTrackInViewR = False
    flags = np.array([(1 if p.nobs > 0 else 0) | (2 if (p.mnLastFrameSeen == frame_id or p.bad) else 0) for p in mps], np.uint8)
    pts = dict(pts, flags=flags, track_depth=np.array([p.mTrackDepth for p in mps], f32))
    rec, n_to_match, _ = frustum(fr, pts)
    project = {}
    for p, r in zip(mps, rec):                                  # :2383-2401
        if r["code"] == 1:
            continue
        apply_record(p, r, bool(fr["rig"]))
        if r["in_view"] or r["in_view_r"]:
            p.mnVisible += 1
        if p.mbTrackInView:
            project[p.idx] = (float(p.mTrackProjX), float(p.mTrackProjY))
    if n_to_match == 0:
        return None, project
    q, dq, owner = queries(fr, pts, rec)
    nm, tm = matcher(q, dq)
    for k in range(len(frame_mp)):
        if tm[k] >= 0:
            frame_mp[k] = mps[owner[tm[k]]]
    return nm, project
