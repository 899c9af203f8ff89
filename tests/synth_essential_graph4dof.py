"""Synthetic 4-DoF essential graphs as LoopClosing::CorrectLoop hands them to Optimizer::OptimizeEssentialGraph4DoF (src/LoopClosing.cc:1218,
src/Optimizer.cc:8335-8557).  TEST INFRASTRUCTURE ONLY.

A visual-inertial rig drives a closed circle a little more than once on a gravity-aligned map: roll and pitch are observable and do
not drift, the odometry drifts in yaw about the world's vertical and in translation.  Keyframe 0 is the loop keyframe (fixed), the last
one the current keyframe.

  vertices    ImuCamPose(pKF): Rcw / tcw and Rwb / twb are what a keyframe stores -- FLOAT, cast to double -- so the loaded Rcw differs from
              Rcb Rwb^T at the 1e-7 level, as in a real map; ImuCamPose(Rwc, twc, pKF) for the current keyframe's neighbourhood
              (CorrectedSim3: double throughout, the current keyframe's corrected pose propagated along the odometry).  One more FIXED
              vertex at the end with an edge to vertex 0: an edge between two fixed vertices
  edges       in the reference's order: the LoopConnections block (current neighbourhood x loop neighbourhood) measured on vScw; then
              per keyframe the mPrevKF edge, older loop edges, covisibility edges to keyframes two and more back -- measured on the
              non-corrected poses.  Several edges between one pair occur (an old loop edge on a chain pair)
  measurement [dRij | dtij] of Siw * Sjw^-1 with both of scale 1: dRij = Ri Rj^T, dtij = ti - dRij tj
Everything is float64 data once made."""
import numpy as np
import essential_graph_model as em7


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _rxy(rx, ry):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


# camera in the body frame: z forward, x right, y down for a body with x forward, z up; plus a small mounting error and a lever arm
RCB = (np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0.0]]) @ _rxy(0.02, -0.015)).astype(np.float32).astype(np.float64)
TCB = np.array([0.06, -0.02, 0.11], np.float32).astype(np.float64)


def _cam(Rwb, twb):
    """Tcw of a body pose (double)."""
    Rcw = RCB @ Rwb.T
    return Rcw, RCB @ (-Rwb.T @ twb) + TCB


def _row(Rwb, twb, Rcw, tcw):
    return np.concatenate([Rwb.reshape(-1), twb, Rcw.reshape(-1), tcw, RCB.reshape(-1), TCB])


def _meas(Ri, ti, Rj, tj):
    Rij = Ri @ Rj.T
    return np.concatenate([Rij.reshape(-1), ti - Rij @ tj])


def make_graph(seed, n_free, yaw_drift=2e-3, trans_drift=1e-2, nbr=3, consistent=False, extra_fixed=True, cov=(2, 3)):
    """-> dict(fixed, edge_v0, edge_v1, edge_meas [E, 12], state [V, 36], truth (Rwb, twb of the drift-free run), n_free, current, loop,
    corrected (bool per vertex), yaw_injected, t_injected (the drift at the current keyframe)).  consistent: no drift and no corrected
    vertices -- every edge has zero residual up to the float storage."""
    rng = np.random.default_rng(seed)
    K = n_free + 1
    ang = 2 * np.pi * 1.08 / max(K - 1, 1)
    radius = 5.0
    Rt, tt, Ro, to = [], [], [], []
    yaw_err, t_err = 0.0, np.zeros(3)
    tilt = [_rxy(0.03 * rng.standard_normal(), 0.03 * rng.standard_normal()) for _ in range(K)]
    for k in range(K):
        a = k * ang
        R = _rz(a + np.pi / 2) @ tilt[k]
        t = np.array([radius * np.cos(a), radius * np.sin(a), 0.05 * np.sin(3 * a)])
        Rt.append(R); tt.append(t)
        if k > 0 and not consistent:
            yaw_err += yaw_drift * (0.7 + 0.6 * rng.random())
            t_err = t_err + trans_drift * np.linalg.norm(tt[k] - tt[k - 1]) * (np.array([0.6, 0.5, 0.2]) + 0.5 * rng.standard_normal(3))
        D = _rz(yaw_err)                                     # the odometry frame has turned and slid against the truth
        Ro.append(D @ R); to.append(D @ t + t_err)
    cur, loop = K - 1, 0
    # non-corrected vertices: what the keyframe stores (float)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rows, Rc, tc = [], [], []
    for k in range(K):
        Rcw, tcw = _cam(Ro[k], to[k])
        Rc.append(f32(Rcw)); tc.append(f32(tcw))
        rows.append(_row(f32(Ro[k]), f32(to[k]), Rc[k], tc[k]))
    nc_R, nc_t = [r.copy() for r in Rc], [t.copy() for t in tc]
    corrected = np.zeros(K + 1, bool)
    if not consistent and K > 3:
        corrected[max(cur - nbr + 1, 2):cur + 1] = True
        # the current keyframe's corrected pose: the true pose relative to the loop keyframe, on the loop keyframe's stored pose
        Rcl, tcl = _cam(Rt[cur], tt[cur])
        Rl, tl = _cam(Rt[loop], tt[loop])
        Rrel = Rcl @ Rl.T
        trel = tcl - Rrel @ tl
        Rcur, tcur = Rrel @ Rc[loop], Rrel @ tc[loop] + trel
        for i in np.flatnonzero(corrected):
            Ri_c = nc_R[i] @ nc_R[cur].T
            ti_c = nc_t[i] - Ri_c @ nc_t[cur]
            Rcw, tcw = Ri_c @ Rcur, Ri_c @ tcur + ti_c
            Rwc, twc = Rcw.T, -Rcw.T @ tcw                   # ImuCamPose(Rwc, twc, pKF)
            Rc[i], tc[i] = Rwc.T, -(Rwc.T @ twc)
            rows[i] = _row(Rwc @ RCB, Rwc @ TCB + twc, Rc[i], tc[i])
    V = K + (1 if extra_fixed else 0)
    if extra_fixed:
        Rx, tx = _rz(0.4) @ _rxy(0.1, -0.2), np.array([0.5, -0.2, 7.0])
        Rcw, tcw = _cam(Rx, tx)
        rows.append(_row(f32(Rx), f32(tx), f32(Rcw), f32(tcw)))
        Rc.append(f32(Rcw)); tc.append(f32(tcw)); nc_R.append(Rc[-1]); nc_t.append(tc[-1])
    fixed = np.zeros(V, np.uint8); fixed[loop] = 1
    if extra_fixed:
        fixed[K] = 1
    e0, e1, ms = [], [], []
    inserted = set()

    def add(i, j, R, t):
        e0.append(i); e1.append(j); ms.append(_meas(R[i], t[i], R[j], t[j]))

    if corrected.any():
        for i in np.flatnonzero(corrected):
            for j in (loop, loop + 1):
                add(i, j, Rc, tc)                            # vScw: corrected poses where there are any (:8390-8400)
                inserted.add((min(i, j), max(i, j)))
    loops = [(K // 2, 1)] if K > 12 else []
    if K > 5:
        loops.append((4, 3))                                 # an old loop edge on a chain pair: two edges between one pair
    for i in range(K):
        if i > 0:
            add(i, i - 1, nc_R, nc_t)                        # mPrevKF
        for a, b in loops:
            if a == i:
                add(a, b, nc_R, nc_t)
        for back in cov:
            j = i - back
            if j < 0 or any((a, b) in ((i, j), (j, i)) for a, b in loops) or (j, i) in inserted:
                continue
            add(i, j, nc_R, nc_t)
    if extra_fixed:
        add(0, K, nc_R, nc_t)                                # between two fixed vertices: not active
        add(1, K, nc_R, nc_t)
    return dict(fixed=fixed, edge_v0=np.array(e0, np.int32), edge_v1=np.array(e1, np.int32), edge_meas=np.array(ms, np.float64).reshape(-1, 12),
                state=np.array(rows), truth=(np.array(Rt), np.array(tt)), n_free=int((fixed == 0).sum()), current=cur, loop=loop, corrected=corrected,
                yaw_injected=yaw_err, t_injected=t_err, nc=(np.array(nc_R[:K]), np.array(nc_t[:K])), cam=(np.array(Rc[:K]), np.array(tc[:K])), loops=loops)


def chain(seed, n_vertices, n_edges=None, yaw=0.02, trans=0.05):
    """The smallest graphs: vertex 0 fixed, vertices on a line, each edge (i, i-1) measured on the stored poses, then the free vertices
    pushed off by a yaw and a translation.  n_edges > n_vertices - 1 repeats pairs (several edges between one pair) and adds (i, i-2)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    R, t = [], []
    for k in range(n_vertices):
        R.append(_rz(0.3 * k) @ _rxy(0.02 * rng.standard_normal(), 0.02 * rng.standard_normal())); t.append(np.array([1.5 * k, 0.3 * rng.standard_normal(), 0.05 * k]))
    cams = [tuple(f32(x) for x in _cam(R[k], t[k])) for k in range(n_vertices)]
    pairs = [(i, i - 1) for i in range(1, n_vertices)] + [(i, i - 2) for i in range(2, n_vertices)]
    n_edges = n_vertices - 1 if n_edges is None else n_edges
    e0, e1, ms = [], [], []
    for k in range(n_edges):
        i, j = pairs[k % len(pairs)]
        noise = _rz(1e-3 * rng.standard_normal()), 1e-3 * rng.standard_normal(3)
        m = _meas(noise[0] @ cams[i][0], cams[i][1] + noise[1], cams[j][0], cams[j][1])
        e0.append(i); e1.append(j); ms.append(m)
    rows = [_row(f32(R[0]), f32(t[0]), *cams[0])]
    for k in range(1, n_vertices):
        D = _rz(yaw * (1 + 0.3 * rng.standard_normal()))
        Rp, tp = D @ R[k], t[k] + trans * rng.standard_normal(3)
        rows.append(_row(f32(Rp), f32(tp), *(f32(x) for x in _cam(Rp, tp))))
    fixed = np.zeros(n_vertices, np.uint8); fixed[0] = 1
    return dict(fixed=fixed, edge_v0=np.array(e0, np.int32), edge_v1=np.array(e1, np.int32), edge_meas=np.array(ms).reshape(-1, 12), state=np.array(rows),
                n_free=n_vertices - 1)


def empty_graph():
    return dict(fixed=np.zeros(0, np.uint8), edge_v0=np.zeros(0, np.int32), edge_v1=np.zeros(0, np.int32), edge_meas=np.zeros((0, 12)),
                state=np.zeros((0, 36)), n_free=0)


def _float_imu_pose(T, Tcb):
    """KeyFrame::GetImuRotation / GetImuPosition as host/slam_types.h states them (src/KeyFrame.cc:161-172): float sums in k order."""
    T, Tcb = np.asarray(T, np.float32), np.asarray(Tcb, np.float32)
    R, t = np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    for i in range(3):
        a = np.float32(0)
        for k in range(3):
            a = np.float32(a + np.float32(T[k, i] * np.float32(Tcb[k, 3] - T[k, 3])))
        t[i] = a
        for j in range(3):
            a = np.float32(0)
            for k in range(3):
                a = np.float32(a + np.float32(T[k, i] * Tcb[k, j]))
            R[i, j] = a
    return R.astype(np.float64), t.astype(np.float64)


def class_scene(seed=3, n_kf=40, bad_kf=None, n_points=300, yaw_drift=2e-3, trans_drift=1e-2):
    """A stand-in inertial map for host_essential_graph4dof_smoke (flat-file arrays) around a make_graph trajectory: keyframe ids 2 k,
    float poses, one IMU calibration, mPrevKF along the trajectory, a spanning tree (only its children matter here), loop edges,
    covisibility weights on both sides of minFeat = 100, a LoopConnections block of which one pair is too weak and the (current, loop)
    pair weak but kept, the pose tables of the current keyframe's neighbourhood, map points of which some are bad; optionally a bad
    keyframe."""
    rng = np.random.default_rng(seed)
    g = make_graph(seed, n_kf - 1, yaw_drift=yaw_drift, trans_drift=trans_drift, extra_fixed=False)
    K = n_kf
    ids = 2 * np.arange(K)
    Tcw = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    Tcw[:, :3, :3] = g["nc"][0].astype(np.float32); Tcw[:, :3, 3] = g["nc"][1].astype(np.float32)
    Tcb = np.eye(4, dtype=np.float32); Tcb[:3, :3] = RCB.astype(np.float32); Tcb[:3, 3] = TCB.astype(np.float32)
    cur, loop = g["current"], g["loop"]
    parent = np.arange(-1, K - 1)
    for k in range(7, K, 7):
        parent[k] = k - 2
    le = list(g["loops"])
    cv = []
    for i in range(K):
        for j in range(max(i - 5, 0), i):
            cv.append((i, j, int(rng.integers(101, 300)) if i - j <= 3 else int(rng.integers(15, 100))))
    corr = np.flatnonzero(g["corrected"][:K])
    lc = [(int(i), j) for i in corr for j in (loop, loop + 1)]
    for (i, j) in lc:
        cv.append((i, j, 40 if (i, j) in ((cur, loop), (int(corr[0]), loop + 1)) else 180))
    bad = np.zeros(K, np.int32)
    if bad_kf is not None:
        bad[bad_kf] = 1
    sim = lambda R, t: np.concatenate([em7.R_to_quat(np.asarray(R, np.float64)), np.asarray(t, np.float64), [1.0]])
    nc = np.stack([sim(Tcw[k, :3, :3], Tcw[k, :3, 3]) for k in range(K)])
    sim_c = np.stack([sim(g["cam"][0][k], g["cam"][1][k]) for k in corr])
    mp_ref = rng.integers(0, K, n_points)
    cam = rng.uniform([-2, -1, 1], [2, 1, 9], (n_points, 3))
    mp_pos = em7.s3_map(em7.s3_inverse(nc)[mp_ref], cam).astype(np.float32)
    mp_bad = (rng.random(n_points) < 0.1).astype(np.int32)
    raw = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint8).reshape(-1)
    arrays = dict(kf_id=ids, kf_bad=bad, kf_parent=parent, kf_prev=np.arange(-1, K - 1), Tcw=Tcw.reshape(-1), Tcb=Tcb.reshape(-1),
                  max_kf_id=[ids[-1]], cur=[cur], loop=[loop],
                  le_a=[a for a, b in le], le_b=[b for a, b in le], cv_a=[c[0] for c in cv], cv_b=[c[1] for c in cv], cv_w=[c[2] for c in cv],
                  lc_a=[a for a, b in lc], lc_b=[b for a, b in lc], sim_kf=corr, sim_c=raw(sim_c), sim_nc=raw(nc[corr]),
                  mp_pos=mp_pos.reshape(-1), mp_ref=mp_ref, mp_bad=mp_bad)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    return dict(arrays=arrays, g=g, K=K, ids=ids, Tcw=Tcw, Tcb=Tcb, nc=nc, sim_c=sim_c, parent=parent, le=le, cv=cv, lc=lc, corr=corr, cur=cur, loop=loop,
                bad=bad.astype(bool), mp_pos=mp_pos, mp_ref=mp_ref, mp_bad=mp_bad.astype(bool))


def gather(sc):
    """Optimizer::OptimizeEssentialGraph4DoF's vertex and edge gathering (src/Optimizer.cc:8335-8557) restated on a class_scene -> (ABI
    graph dict with state, vertex index per keyframe or -1, edges left out, vS = vScw per keyframe).  Sets that the reference walks in
    pointer order are walked in index order here: the edge ORDER may differ from the class's, the edge SET may not."""
    K, bad = sc["K"], sc["bad"]
    vertex = np.where(~bad, np.cumsum(~bad) - 1, -1)
    Rcb, tcb = sc["Tcb"][:3, :3].astype(np.float64), sc["Tcb"][:3, 3].astype(np.float64)
    vS = sc["nc"].copy()
    rows = []
    corr_at = {int(k): n for n, k in enumerate(sc["corr"])}
    for k in range(K):
        if k in corr_at:
            vS[k] = sc["sim_c"][corr_at[k]]
            Swc = em7.s3_inverse(vS[k])
            Rwc, twc = em7.quat_to_R(Swc[:4]), Swc[4:7]
            Rcw = Rwc.T
            rows.append(_row(Rwc @ Rcb, Rwc @ tcb + twc, Rcw, -(Rcw @ twc)))
        else:
            Rwb, twb = _float_imu_pose(sc["Tcw"][k], sc["Tcb"])
            rows.append(_row(Rwb, twb, sc["Tcw"][k, :3, :3].astype(np.float64), sc["Tcw"][k, :3, 3].astype(np.float64)))
        rows[-1][24:33], rows[-1][33:36] = Rcb.reshape(-1), tcb
    w = {}
    for a, b, x in sc["cv"]:
        w[(a, b)] = w[(b, a)] = x
    e0, e1, ms, left = [], [], [], 0

    def add(i, j, Si, Sj):
        nonlocal left
        if vertex[i] < 0 or vertex[j] < 0:
            left += 1
            return
        Sij = em7.s3_mul(Si, em7.s3_inverse(Sj))
        e0.append(vertex[i]); e1.append(vertex[j]); ms.append(np.concatenate([em7.quat_to_R(Sij[:4]).reshape(-1), Sij[4:7]]))

    inserted = set()
    for i, j in sc["lc"]:
        if (i != sc["cur"] or j != sc["loop"]) and w.get((i, j), 0) < 100:
            continue
        add(i, j, vS[i], vS[j]); inserted.add((min(i, j), max(i, j)))
    nc = sc["nc"]                                                # NonCorrectedSim3 where present, else vScw: the same numbers here
    loops = {}
    for a, b in sc["le"]:
        loops.setdefault(a, set()).add(b); loops.setdefault(b, set()).add(a)
    for i in range(K):
        if i > 0:
            add(i, i - 1, nc[i], nc[i - 1])
        for l in sorted(loops.get(i, ())):
            if l < i:
                add(i, l, nc[i], nc[l])
        nb = sorted([(-(w[(i, j)]), k, j) for k, (a, b, x) in enumerate(sc["cv"]) for j in ((b,) if a == i else (a,) if b == i else ()) if x >= 100])
        for _, _, j in nb:
            if j == i - 1 or j == i + 1 or sc["parent"][j] == i or j in loops.get(i, ()) or bad[j] or not j < i or (min(i, j), max(i, j)) in inserted:
                continue
            add(i, j, nc[i], nc[j])
    fixed = np.zeros(int((~bad).sum()), np.uint8); fixed[vertex[sc["loop"]]] = 1
    return dict(fixed=fixed, edge_v0=np.array(e0, np.int32), edge_v1=np.array(e1, np.int32), edge_meas=np.array(ms).reshape(-1, 12),
                state=np.array(rows)[~bad]), vertex, left, vS
