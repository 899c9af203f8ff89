"""Synthetic essential graphs as LoopClosing::CorrectLoop hands them to Optimizer::OptimizeEssentialGraph (src/LoopClosing.cc:1131-1223,
src/Optimizer.cc:2390-2613).  TEST INFRASTRUCTURE ONLY.

A camera drives a closed circle a little more than once; its odometry drifts in rotation, translation and (monocular: free scale) in
scale.  Keyframe 0 is the map's first one (fixed); the last keyframe is the current one, whose loop keyframe is near the start.

  vertices    CorrectedSim3 for the current keyframe's neighbourhood (the Sim3 found against the loop keyframe, propagated as
              g2oCorrectedSiw = g2oSic * g2oCorrectedScw, LoopClosing.cc:1160-1164), Sim3(Rcw, tcw, 1) for everyone else; one more
              FIXED vertex at the end (what a merge overload fixes) with an edge to vertex 0 -- an edge between two fixed vertices
  edges       in the reference's order: the LoopConnections block (current neighbourhood x loop neighbourhood) measured on the CORRECTED
              poses; then per keyframe the spanning-tree edge (a chain with a few branches), older loop edges, covisibility edges to the
              preceding 2..5 keyframes that are neither parent / child nor in sInsertedEdges, and (inertial) the mPrevKF edge --
              measured on NonCorrectedSim3 where an endpoint has an entry.  Duplicates between one pair occur: an old loop edge on a
              tree pair, the mPrevKF edges on the chain.
Everything is float64 data once made."""
import numpy as np
import essential_graph_model as em


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])


def _sim3(q, t, s=1.0):
    return np.concatenate([q, t, [s]])


def make_graph(seed, n_free, fix_scale, rot_drift=0.012, scale_drift=0.012, trans_drift=0.01, inertial=False, n_old_loops=2, consistent=False,
               nbr=3):
    """-> dict(fixed, edge_v0, edge_v1, edge_meas, sim3 (the vertex estimates), truth (the drift-free Siw), n_free, fix_scale, current,
    loop, corrected (bool per vertex), Scw_nc (the non-corrected Sim3 of every vertex)).  consistent: no drift -- every edge has zero
    residual at `truth`."""
    rng = np.random.default_rng(seed)
    K = n_free + 1                                            # keyframes of the trajectory; vertex K is the extra fixed one
    ang = 2 * np.pi * 1.08 / max(K - 1, 1)
    # true relative motion Tc(k+1)c(k) and its drifted measurement (odometry)
    S_true = [_sim3(_rot([0, 0, 1], 0.0), np.zeros(3))]
    S_odo = [S_true[0].copy()]
    radius = 5.0
    scale = 1.0
    for k in range(1, K):
        step = 2 * radius * np.sin(ang / 2)
        rel_q = _rot([0.05 * rng.standard_normal(), 1.0, 0.05 * rng.standard_normal()], -ang)
        rel_t = np.array([-step, 0.02 * rng.standard_normal(), 0.1 * step * rng.standard_normal()])
        rel = _sim3(rel_q, rel_t)
        S_true.append(em.s3_mul(rel, S_true[-1]))
        if consistent:
            S_odo.append(em.s3_mul(rel, S_odo[-1]))
            continue
        dq = _rot(np.array([0.3, 1.0, 0.2]) + 0.3 * rng.standard_normal(3), rot_drift * (0.7 + 0.6 * rng.random()))     # a systematic drift
        if not fix_scale:
            scale *= np.exp(scale_drift * (0.7 + 0.6 * rng.random()))
        rel_d = _sim3(em.quat_mul(dq, rel_q), scale * rel_t * (1 + trans_drift * rng.standard_normal(3)))
        S_odo.append(em.s3_mul(rel_d, S_odo[-1]))
    S_true, S_odo = np.array(S_true), np.array(S_odo)
    cur, loop = K - 1, 0 if K <= 6 else 1
    # the Sim3 between the current and the loop keyframe as Sim3Solver + OptimizeSim3 leave it: the true relative pose in the loop
    # keyframe's (undrifted) map scale, scale = ratio of the two map scales
    rel_true = em.s3_mul(S_true[cur], em.s3_inverse(S_true[loop]))
    Scm = _sim3(rel_true[:4], rel_true[4:7], 1.0 if (fix_scale or consistent) else 1.0 / scale)
    Scw_corr = em.s3_mul(Scm, S_odo[loop])
    corrected = np.zeros(K + 1, bool)
    if not consistent:
        corrected[max(cur - nbr + 1, loop + 2):cur + 1] = True
    est = np.concatenate([S_odo, [_sim3(_rot([1, 0, 0], 0.3), np.array([0.5, -0.2, 7.0]))]])
    nc = est.copy()
    for i in np.flatnonzero(corrected):
        est[i] = em.s3_mul(em.s3_mul(S_odo[i], em.s3_inverse(S_odo[cur])), Scw_corr)
    fixed = np.zeros(K + 1, np.uint8); fixed[0] = 1; fixed[K] = 1

    parent = np.arange(-1, K - 1)
    for k in range(7, K, 7):
        parent[k] = k - 2                                     # k - 1 stays a leaf: a branch of the spanning tree
    loops = []
    if K > 12:
        loops = [(K // 2, 2)] + ([(2 * K // 3, 4)] if n_old_loops > 1 else [])
    if K > 5:
        loops.append((4, 3))                                  # an old loop edge on a tree pair: two edges between one pair

    e0, e1, ms = [], [], []
    inserted = set()

    def add(i, j, Si, Sj):                                    # vertex(0) = i, vertex(1) = j, measurement Sji = Sjw * Swi
        e0.append(i); e1.append(j); ms.append(em.s3_mul(Sj, em.s3_inverse(Si)))

    if corrected.any():
        loop_nb = list(range(max(loop - 1, 0), loop + 2))
        for i in np.flatnonzero(corrected):
            for j in loop_nb:
                add(i, j, est[i], est[j])                     # vScw: the corrected poses (Optimizer.cc:2455-2461)
                inserted.add((min(i, j), max(i, j)))
    for i in range(K):
        if parent[i] >= 0:
            add(i, parent[i], nc[i], nc[parent[i]])
        for a, b in loops:
            if a == i:
                add(a, b, nc[a], nc[b])
        width = 2 + int(rng.integers(0, 4))
        for j in range(i - 2, i - 1 - width, -1):
            if j < 0 or j == parent[i] or parent[j] == i or any((a, b) in ((i, j), (j, i)) for a, b in loops) or (j, i) in inserted:
                continue
            add(i, j, nc[i], nc[j])
        if inertial and i > 0:
            add(i, i - 1, nc[i], nc[i - 1])
    add(0, K, nc[0], nc[K])                                   # between two fixed vertices: not active
    add(1, K, nc[1], nc[K])
    truth = np.concatenate([S_true, nc[K:]])
    return dict(fixed=fixed, edge_v0=np.array(e0, np.int32), edge_v1=np.array(e1, np.int32), edge_meas=np.array(ms, np.float64), sim3=est, truth=truth,
                n_free=n_free, fix_scale=bool(fix_scale), current=cur, loop=loop, corrected=corrected, Scw_nc=nc)


def empty_graph():
    return dict(fixed=np.zeros(0, np.uint8), edge_v0=np.zeros(0, np.int32), edge_v1=np.zeros(0, np.int32), edge_meas=np.zeros((0, 8)),
                sim3=np.zeros((0, 8)), n_free=0, fix_scale=False)


def points_scene(g, est_after, n_points, seed=5):
    """Map points for the correction: float positions near their reference keyframe, d_ref with -1 rows (bad points).
    -> (Xw float32 [n, 3], ref int32 [n], Scw [V, 8] = the vertex estimates before, corrected_Swc [V, 8] = the inverses after)."""
    rng = np.random.default_rng(seed)
    V = len(g["fixed"])
    ref = rng.integers(0, V, n_points).astype(np.int32)
    ref[rng.random(n_points) < 0.05] = -1
    Scw = np.asarray(g["sim3"], np.float64)
    Swc = em.s3_inverse(np.asarray(est_after, np.float64))
    cam = rng.uniform([-2, -1, 1], [2, 1, 9], (n_points, 3))
    Xw = em.s3_map(em.s3_inverse(Scw)[np.maximum(ref, 0)], cam).astype(np.float32)
    return Xw, ref, Scw, Swc


def _float_pose(S):
    """[R | t] of a scale-1 Sim3 as the float 4x4 a keyframe stores."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = em.quat_to_R(S[:4]).astype(np.float32); T[:3, 3] = S[4:7].astype(np.float32)
    return T


def _sim3_of_pose(T):
    """g2o::Sim3(Rcw, tcw, 1) of a float pose: Eigen::Quaterniond(Matrix3d), not normalised."""
    return np.concatenate([em.R_to_quat(T[:3, :3].astype(np.float64)), T[:3, 3].astype(np.float64), [1.0]])


def class_scene(seed=3, n_kf=40, fix_scale=False, bad_kf=None, n_points=300, drift=2e-3):
    """A stand-in map for host_essential_graph_smoke (flat-file arrays) around a make_graph trajectory: keyframe ids 2 k (the first one is
    the map's initial keyframe), float poses, the spanning tree, loop edges, covisibility weights on both sides of minFeat = 100, a
    LoopConnections block of which one pair is too weak, the pose tables of the current keyframe's neighbourhood, map points of which some
    were corrected by the current keyframe (mnCorrectedByKF / mnCorrectedReference), some are bad; optionally a bad keyframe."""
    rng = np.random.default_rng(seed)
    g = make_graph(seed, n_kf - 1, fix_scale, rot_drift=drift, scale_drift=drift)
    K = n_kf
    ids = 2 * np.arange(K)
    Tcw = np.stack([_float_pose(g["Scw_nc"][k]) for k in range(K)])
    cur, loop = g["current"], g["loop"]
    parent = np.arange(-1, K - 1)
    for k in range(7, K, 7):
        parent[k] = k - 2
    le = [(K // 2, 2), (2 * K // 3, 4), (4, 3)]
    cv = []
    for i in range(K):
        for j in range(max(i - 5, 0), i):
            cv.append((i, j, int(rng.integers(101, 300)) if i - j <= 3 else int(rng.integers(15, 100))))
    corr = np.flatnonzero(g["corrected"][:K])
    lc = [(int(i), j) for i in corr for j in (loop - 1, loop, loop + 1)]
    for (i, j) in lc:                                            # weights of the LoopConnections pairs: one too weak, (cur, loop) weak but kept
        cv.append((i, j, 40 if (i, j) in ((cur, loop), (int(corr[0]), loop + 1)) else 180))
    bad = np.zeros(K, np.int32)
    if bad_kf is not None:
        bad[bad_kf] = 1
    mp_ref = rng.integers(0, K, n_points)
    cam = rng.uniform([-2, -1, 1], [2, 1, 9], (n_points, 3))
    nc = np.stack([_sim3_of_pose(Tcw[k]) for k in range(K)])
    mp_pos = em.s3_map(em.s3_inverse(nc)[mp_ref], cam).astype(np.float32)
    mp_bad = (rng.random(n_points) < 0.1).astype(np.int32)
    by_cur = rng.random(n_points) < 0.2
    mp_by = np.where(by_cur, ids[cur], 0)
    mp_cref = np.where(by_cur, ids[rng.choice(corr, n_points)], 0)
    raw = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint8).reshape(-1)
    arrays = dict(kf_id=ids, kf_bad=bad, kf_parent=parent, kf_imu=np.zeros(K, np.int32), kf_prev=np.arange(-1, K - 1), Tcw=Tcw.reshape(-1),
                  init_id=[ids[0]], max_kf_id=[ids[-1]], cur=[cur], loop=[loop], fix_scale=[int(fix_scale)],
                  le_a=[a for a, b in le], le_b=[b for a, b in le], cv_a=[c[0] for c in cv], cv_b=[c[1] for c in cv], cv_w=[c[2] for c in cv],
                  lc_a=[a for a, b in lc], lc_b=[b for a, b in lc], sim_kf=corr, sim_c=raw(g["sim3"][corr]), sim_nc=raw(nc[corr]),
                  mp_pos=mp_pos.reshape(-1), mp_ref=mp_ref, mp_bad=mp_bad, mp_by=mp_by, mp_cref=mp_cref)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    return dict(arrays=arrays, g=g, K=K, ids=ids, Tcw=Tcw, nc=nc, parent=parent, le=le, cv=cv, lc=lc, corr=corr, cur=cur, loop=loop, bad=bad.astype(bool),
                fix_scale=fix_scale, mp_pos=mp_pos, mp_ref=mp_ref, mp_bad=mp_bad.astype(bool), by_cur=by_cur, mp_cref=mp_cref)


def gather(sc):
    """Optimizer::OptimizeEssentialGraph's vertex and edge gathering (src/Optimizer.cc:2379-2588) restated on a class_scene -> (ABI
    graph dict with sim3, vertex index per keyframe or -1, edges left out).  Sets that the reference walks in pointer order are walked in
    index order here: the edge ORDER may differ from the class's, the edge SET may not."""
    K, bad = sc["K"], sc["bad"]
    vertex = np.where(~bad, np.cumsum(~bad) - 1, -1)
    vS = sc["nc"].copy()
    vS[sc["corr"]] = sc["g"]["sim3"][sc["corr"]]
    w = {}
    for a, b, x in sc["cv"]:
        w[(a, b)] = w[(b, a)] = x
    e0, e1, ms, left = [], [], [], 0

    def add(i, j, Si, Sj):
        nonlocal left
        if vertex[i] < 0 or vertex[j] < 0:
            left += 1
            return
        e0.append(vertex[i]); e1.append(vertex[j]); ms.append(em.s3_mul(Sj, em.s3_inverse(Si)))

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
        p = sc["parent"][i]
        if p >= 0:
            add(i, p, nc[i], nc[p])
        for l in sorted(loops.get(i, ())):
            if l < i:
                add(i, l, nc[i], nc[l])
        nb = sorted([(-(w[(i, j)]), k, j) for k, (a, b, x) in enumerate(sc["cv"]) for j in ((b,) if a == i else (a,) if b == i else ()) if x >= 100])
        for _, _, j in nb:
            if j == p or sc["parent"][j] == i or j in loops.get(i, ()) or bad[j] or not j < i or (min(i, j), max(i, j)) in inserted:
                continue
            add(i, j, nc[i], nc[j])
    fixed = np.zeros(int((~bad).sum()), np.uint8); fixed[vertex[0]] = 1
    return dict(fixed=fixed, edge_v0=np.array(e0, np.int32), edge_v1=np.array(e1, np.int32), edge_meas=np.array(ms), sim3=vS[~bad]), vertex, left
