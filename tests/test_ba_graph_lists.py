"""The host lists of the bundle adjustments (csrc/ba_graph_lists.h) in a stand-alone host program under the address and
undefined-behaviour sanitizers: free numbering, point-major and pose-major edge lists, twin chains, Schur GEMM tasks / stages / masks,
pair-list sizes, exchange offsets, the slices of a landmark-sharded batch and every refusal.  The program reads crafted graphs from a
text file and prints every array; they are compared with a restatement of the rules written here in plain Python.  No GPU, no library."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-slam3-mac_amd", "csrc")
BADARG = -1

MAIN = r"""
#include "ba_graph_lists.h"
#include <cstdio>
#include <string>
template <class T> static void line(const char *name, const std::vector<T> &v) { printf("%s", name); for (const T &x : v) printf(" %lld", (long long)x); printf("\n"); }
static void dline(const char *name, const std::vector<double> &v) { printf("%s", name); for (double x : v) printf(" %.17g", x); printf("\n"); }
struct G { std::vector<uint8_t> fixed, type; std::vector<int32_t> ep, el, pcam; std::vector<double> obs, is2, poses, points; std::vector<orbhip_ba_camera> cams; };
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char name[64];
    int world, rank, mode, ng;
    while (fscanf(f, "%63s %d %d %d %d", name, &world, &rank, &mode, &ng) == 5) {
        std::vector<G> gs(ng);
        std::vector<orbhip_ba_graph> graphs(ng);
        std::vector<const double *> poses(ng), points(ng);
        for (int g = 0; g < ng; g++) {
            G &S = gs[g];
            orbhip_ba_graph &H = graphs[g];
            memset(&H, 0, sizeof(H));
            int np, nl, ne, cam_model, ncam, null_tables, no_stereo;
            double trl_w;
            if (fscanf(f, "%d %d %d %d %lf %d %d %d", &np, &nl, &ne, &cam_model, &trl_w, &ncam, &null_tables, &no_stereo) != 8) return 3;
            S.fixed.resize(np > 0 ? np : 0);
            for (auto &x : S.fixed) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = (uint8_t)v; }
            S.ep.resize(ne); S.el.resize(ne); S.type.resize(ne);
            for (int e = 0; e < ne; e++) { int a, b, c; if (fscanf(f, "%d %d %d", &a, &b, &c) != 3) return 3; S.ep[e] = a; S.el[e] = b; S.type[e] = (uint8_t)c; }
            S.cams.resize(ncam);
            for (int c = 0; c < ncam; c++) {
                orbhip_ba_camera &K = S.cams[c];
                memset(&K, 0, sizeof(K));
                int cm; double w;
                if (fscanf(f, "%lf %d", &w, &cm) != 2) return 3;
                K.fx = 500 + c; K.fy = 510 + c; K.cx = 320 + c; K.cy = 240 + c; K.bf = 40 + c; K.camera_model = cm; K.Trl[3] = w; K.Trl[4] = 0.1 * c;
                K.fx2 = 400 + c; K.fy2 = 410 + c; K.cx2 = 300 + c; K.cy2 = 200 + c; K.camera2_model = 1 - cm;
                for (int k = 0; k < 4; k++) { K.kb[k] = 0.01 * (k + 1) + c; K.kb2[k] = 0.02 * (k + 1) + c; }
            }
            S.pcam.resize(ncam > 0 && np > 0 ? np : 0);
            for (auto &x : S.pcam) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = v; }
            for (int e = 0; e < ne; e++) { for (int k = 0; k < 3; k++) S.obs.push_back(10.0 * e + k + 100.0 * g); S.is2.push_back(1.0 + e + 0.5 * g); }
            for (int i = 0; i < np; i++) {                       // odd poses carry a quaternion with negative w; none is normalised
                const double q[7] = {0.1 * i, 0.2, -0.3, (i & 1) ? -0.9 : 0.9, 1.0 * i, 2.0 * i, 3.0 * i + g};
                S.poses.insert(S.poses.end(), q, q + 7);
            }
            for (int l = 0; l < nl; l++) { S.points.push_back(l); S.points.push_back(l + 0.5); S.points.push_back(l + 0.25 + g); }
            H.n_poses = np; H.n_points = nl; H.n_edges = ne;
            H.pose_fixed = S.fixed.data(); H.edge_pose = S.ep.data(); H.edge_point = S.el.data(); H.edge_obs = S.obs.data(); H.edge_inv_sigma2 = S.is2.data();
            H.edge_stereo = no_stereo ? nullptr : S.type.data();
            H.fx = 700 + g; H.fy = 710; H.cx = 330; H.cy = 250; H.bf = 35; H.camera_model = cam_model; H.Trl[3] = trl_w; H.Trl[6] = 0.25;
            H.fx2 = 600; H.fy2 = 610; H.cx2 = 310; H.cy2 = 210; H.camera2_model = 1;
            for (int k = 0; k < 4; k++) { H.kb[k] = 0.1 * (k + 1); H.kb2[k] = 0.2 * (k + 1); }
            H.n_cameras = ncam;
            if (!null_tables) { H.cameras = S.cams.data(); H.pose_camera = S.pcam.data(); }
            poses[g] = S.poses.data(); points[g] = S.points.data();
        }
        BaGraphLists L;
        BaShard S;
        int rc;
        const char *msg = nullptr;
        if (world > 1) {
            rc = S.build(graphs.data(), ng, points.data(), rank, world);
            msg = S.err;
            if (rc == ORBHIP_OK) { rc = L.build(S.sub.data(), ng, poses.data(), S.pts.data(), &S.has, world, mode); msg = L.err; }
        } else { rc = L.build(graphs.data(), ng, poses.data(), points.data(), nullptr, world, mode); msg = L.err; }
        printf("case %s %d %s\n", name, rc, msg ? msg : "-");
        if (rc != ORBHIP_OK) continue;
        if (world > 1) {
            std::vector<int> sl, pts_at;
            for (int g = 0; g < ng; g++) { sl.push_back(S.slices[g].pt0); sl.push_back(S.slices[g].npts); sl.push_back(S.slices[g].e0); sl.push_back(S.slices[g].ne);
                                           pts_at.push_back((int)(S.pts[g] - points[g])); }
            line("slices", sl); line("pts_at", pts_at);
        }
        std::vector<long long> gd;
        std::vector<double> gcal;
        for (const BaGraphDev &D : L.gd) {
            const long long v[] = {D.n_poses, D.n_points, D.n_edges, D.nf, D.n, D.ld, D.pose_off, D.point_off, D.edge_off, D.free_off, D.ptstart_off, D.posestart_off,
                                   (long long)D.s_off, (long long)D.spart_off, D.gemm_off, D.stage_off, D.n_stages, D.gemm_ps, D.ks, D.nt16, D.ngrp,
                                   (long long)D.pair_off, (long long)D.pent_off, D.cam_off, D.cam_model, D.cam2_model};
            gd.insert(gd.end(), v, v + sizeof(v) / sizeof(v[0]));
            const double c[] = {D.fx, D.fy, D.cx, D.cy, D.bf, D.kb[0], D.kb[3], D.Trl[3], D.Trl[6], D.fx2, D.fy2, D.cx2, D.cy2, D.kb2[0], D.kb2[3]};
            gcal.insert(gcal.end(), c, c + sizeof(c) / sizeof(c[0]));
        }
        line("gd", gd); dline("gcal", gcal);
        std::vector<double> cams;
        for (const BaCamDev &K : L.cams) { const double c[] = {K.fx, K.bf, (double)K.cam_model, K.kb[3], K.Trl[3], K.Trl[4], K.cy2, K.kb2[0], (double)K.cam2_model}; cams.insert(cams.end(), c, c + 9); }
        dline("cams", cams);
        line("pose_cam", L.posecam); line("hidx", L.hidx); line("edge_pose", L.epose); line("edge_point", L.epoint); line("edge_stereo", L.est);
        line("edge_dup", L.edup); line("edge_next", L.enext); line("edge_task", L.etask); line("pt_start", L.ptstart); line("pose_start", L.posestart);
        line("pose_edges", L.poseedges); line("pm_point", L.pmpoint); line("pm_task", L.pmtask); line("pm_type", L.pmtype); line("ptmask", L.ptmask);
        line("x1_off", L.x1off); line("x2_off", L.x2off);
        dline("edge_obs", L.eobs); dline("edge_is2", L.eis2); dline("pm_is2", L.pmis2); dline("pm_obs", L.pmobs); dline("poses0", L.poses0); dline("points0", L.points0);
        std::vector<int> t4;
        for (const BaInt4 &t : L.gtask) { t4.push_back(t.x); t4.push_back(t.y); t4.push_back(t.z); t4.push_back(t.w); }
        line("gemm_task", t4);
        t4.clear();
        for (const BaInt4 &t : L.gstage) { t4.push_back(t.x); t4.push_back(t.y); t4.push_back(t.z); t4.push_back(t.w); }
        line("gemm_stage", t4);
        const long long sc[] = {L.sumP, L.sumL, L.sumE, L.sumF, L.max_edges, L.max_points, L.max_nf, L.max_ld, (long long)L.s_total, (long long)L.spart_total, L.any_big, L.general,
                                L.pair_lists, (long long)L.pair_total_start, (long long)L.pair_total_ent, L.max_npair, L.max_row_blocks, (long long)L.x_need};
        line("scalars", std::vector<long long>(sc, sc + sizeof(sc) / sizeof(sc[0])));
        dline("flops", {L.flops_per_launch, L.flops_issued, L.flops_dense});
    }
    fclose(f);
    return 0;
}
"""

GD = ["n_poses", "n_points", "n_edges", "nf", "n", "ld", "pose_off", "point_off", "edge_off", "free_off", "ptstart_off", "posestart_off", "s_off", "spart_off",
      "gemm_off", "stage_off", "n_stages", "gemm_ps", "ks", "nt16", "ngrp", "pair_off", "pent_off", "cam_off", "cam_model", "cam2_model"]
SCALARS = ["sumP", "sumL", "sumE", "sumF", "max_edges", "max_points", "max_nf", "max_ld", "s_total", "spart_total", "any_big", "general", "pair_lists",
           "pair_total_start", "pair_total_ent", "max_npair", "max_row_blocks", "x_need"]
# the constants the rules below are stated with (csrc/ba_graph_lists.h)
GEMM_PS, GEMM_C, GEMM_NCH, GEMM_WAVES, GEMM_LDS_PAD, GEMM_STAGE_EDGES, GEMM_TARGET_WGS, PANEL = 8, 3, 8, 8, 16, 85, 256, 126 * 1024
LDLT_MAXN = 480


def graph(fixed, edges, n_points, cam_model=0, trl_w=0.0, cams=(), pose_cam=(), null_tables=0, no_stereo=0, n_poses=None):
    return dict(fixed=list(fixed), edges=list(edges), n_points=n_points, cam_model=cam_model, trl_w=trl_w, cams=list(cams), pose_cam=list(pose_cam),
                null_tables=null_tables, no_stereo=no_stereo, n_poses=len(fixed) if n_poses is None else n_poses)


def case(name, graphs, world=1, rank=0, mode=1):
    return dict(name=name, graphs=graphs, world=world, rank=rank, mode=mode)


def all_see(n_poses, n_points, fixed=()):
    """every pose sees every point, one monocular edge each"""
    return graph([1 if i in fixed else 0 for i in range(n_poses)], [(i, l, 0) for l in range(n_points) for i in range(n_poses)], n_points)


def ring(n_poses, n_points, per_point=3):
    """point l is seen by per_point consecutive poses starting at l mod n_poses"""
    return graph([0] * n_poses, [((l + k) % n_poses, l, 0) for l in range(n_points) for k in range(per_point)], n_points)


# 4 poses: 0 fixed, 1 and 2 free, 3 free without an edge; 5 points: 0 seen only by the fixed pose, 1 twice by pose 1 (types 0 and 2)
TINY_EDGES = [(0, 0, 0), (1, 1, 0), (1, 1, 2), (2, 1, 1), (0, 2, 0), (2, 2, 0), (1, 3, 1), (2, 4, 0), (1, 4, 0)]
TINY = graph([1, 0, 0, 0], TINY_EDGES, 5, trl_w=1.0)
SECOND = graph([0, 1, 0], [(0, 0, 1), (2, 0, 0), (1, 1, 0), (2, 1, 0), (0, 2, 0)], 3)
CAMS = graph([0, 0, 1], [(0, 0, 0), (1, 0, 0), (2, 1, 0), (0, 1, 0)], 2, cams=[(1.0, 0), (0.5, 1)], pose_cam=[1, 0, 1], no_stereo=1)
SHARD = graph([1, 0, 0, 0], [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 2, 0), (1, 2, 0), (3, 3, 0), (0, 4, 0), (3, 4, 0), (2, 4, 0)], 5)
CASES = [
    case("tiny_pairs", [TINY], mode=1), case("tiny_gemm", [TINY], mode=2),
    case("cut_ps", [all_see(1, 9)], mode=2), case("cut_edges", [all_see(20, 5)], mode=2), case("cut_ld", [graph([0] * 80, [(i, l, 0) for l in range(6) for i in range(80) if i % 6 == l], 6)], mode=2),
    case("big", [ring(81, 90)], mode=2), case("big_sharded", [ring(81, 90)], world=2, rank=0, mode=2), case("too_big", [ring(683, 683, 1)]),
    case("two", [TINY, SECOND], mode=2), case("two_pairs", [TINY, SECOND], mode=1), case("cams", [CAMS]),
    case("shard0", [SHARD, SECOND], world=2, rank=0), case("shard1", [SHARD, SECOND], world=2, rank=1),
    case("shard_few", [graph([0], [(0, 0, 0)], 1)], world=2, rank=1),
    case("no_poses", [graph([], [], 1, n_poses=0)]),
    case("not_major", [graph([0, 0], [(0, 1, 0), (1, 0, 0)], 2)]),
    case("bad_id", [graph([0, 0], [(0, 0, 0), (2, 1, 0)], 2)]),
    case("bad_type", [graph([0, 0], [(0, 0, 0), (1, 1, 3)], 2)]),
    case("no_trl", [graph([0, 0], [(0, 0, 0), (1, 1, 2)], 2)]),
    case("null_tables", [graph([0, 0], [(0, 0, 0)], 1, cams=[(1.0, 0)], pose_cam=[0, 0], null_tables=1)]),
    case("bad_pose_cam", [graph([0, 0], [(0, 0, 0)], 1, cams=[(1.0, 0)], pose_cam=[0, 1])]),
]


def spec_text(cases):
    out = []
    for c in cases:
        out.append("%s %d %d %d %d" % (c["name"], c["world"], c["rank"], c["mode"], len(c["graphs"])))
        for g in c["graphs"]:
            out.append("%d %d %d %d %r %d %d %d" % (g["n_poses"], g["n_points"], len(g["edges"]), g["cam_model"], g["trl_w"], len(g["cams"]), g["null_tables"], g["no_stereo"]))
            out.append(" ".join(map(str, g["fixed"])))
            out.append(" ".join("%d %d %d" % e for e in g["edges"]))
            out.append(" ".join("%r %d" % c2 for c2 in g["cams"]))
            out.append(" ".join(map(str, g["pose_cam"])))
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ba_lists")
    src, exe, spec = tmp / "main.cc", str(tmp / "ba_lists"), tmp / "cases.txt"
    src.write_text(MAIN)
    spec.write_text(spec_text(CASES))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe, str(spec)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], dict(rc=int(w[2]), msg=ln.split(None, 3)[3]))
        elif w[0] in ("gcal", "cams", "edge_obs", "edge_is2", "pm_is2", "pm_obs", "poses0", "points0", "flops"):
            cur[w[0]] = [float(x) for x in w[1:]]
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    assert list(out) == [c["name"] for c in CASES]
    return out


# ---------------------------------------------------------------------------------------------------------------- the rules, restated
def shard(g, gi, rank, world):
    """rank r keeps points [r L / world, (r + 1) L / world) with their edges; points re-based, poses untouched"""
    L = g["n_points"]
    p0, p1 = rank * L // world, (rank + 1) * L // world
    ids = [e for e, (_, l, _) in enumerate(g["edges"]) if p0 <= l < p1]
    sub = dict(g, edges=[(g["edges"][e][0], g["edges"][e][1] - p0, g["edges"][e][2]) for e in ids], n_points=p1 - p0)
    sub["obs_edge0"], sub["pt0"] = (ids[0] if ids else sum(1 for _, l, _ in g["edges"] if l < p0)), p0
    sub["in_system"] = sorted({p for p, _, _ in g["edges"]})          # a pose with an edge on ANY rank
    return sub, (p0, p1 - p0, sub["obs_edge0"], len(ids))


def restate(c):
    """Every list of the batch from the rules of ba_graph_lists.h's header comment and DESIGN, graph by graph."""
    G, world, mode = len(c["graphs"]), c["world"], c["mode"]
    graphs, slices = [], []
    for gi, g in enumerate(c["graphs"]):
        if world > 1:
            g, sl = shard(g, gi, c["rank"], world)
            slices += sl
        graphs.append(g)
    R = {k: [] for k in ("gd", "pose_cam", "hidx", "edge_pose", "edge_point", "edge_stereo", "edge_dup", "edge_next", "edge_task", "pt_start", "pose_start", "pose_edges",
                         "pm_point", "pm_task", "pm_type", "ptmask", "x1_off", "x2_off", "edge_obs", "edge_is2", "pm_is2", "pm_obs", "poses0", "points0", "gemm_task",
                         "gemm_stage")}
    R["slices"] = slices
    sums = dict(P=0, L=0, E=0, F=0, s=0, sp=0, x1=0, x2=0, ncam=0)
    stats = world > 1 or mode == 2                    # the tile masks and flop counts serve the GEMM form only
    info, general, any_big = [], False, False
    dense = issued = 0.0
    for gi, g in enumerate(graphs):
        E, NL, NP = g["edges"], g["n_points"], g["n_poses"]
        e0g, pt0g = g.get("obs_edge0", 0), g.get("pt0", 0)
        seen = set(g["in_system"]) if "in_system" in g else {p for p, _, _ in E}
        free = [i for i in range(NP) if not g["fixed"][i] and i in seen]
        h = {p: k for k, p in enumerate(free)}
        nf = len(free)
        n, ld = 6 * nf, max(96, -(-6 * nf // 96) * 96)
        big = n > LDLT_MAXN
        any_big |= big
        types = [0 if g["no_stereo"] else t for _, _, t in E]
        # twins: an edge whose (point, pose) an earlier edge has is a duplicate; every edge points to the next one of its chain
        dup, nxt, last = [0] * len(E), [-1] * len(E), {}
        for e, (p, l, _) in enumerate(E):
            if (p, l) in last:
                dup[e], nxt[last[(p, l)]] = 1, e
            last[(p, l)] = e
        general |= any(dup) or 2 in types or g["cam_model"] != 0 or bool(g["cams"])
        by_pose = [[e for e, (p, _, _) in enumerate(E) if p == fp] for fp in free]
        pe = [e for l in by_pose for e in l]
        pose_start = [0]
        for l in by_pose:
            pose_start.append(pose_start[-1] + len(l))
        pm = pe + [0] * (len(E) - len(pe))                              # filler: edge 0
        blocks = [e for e, (p, _, _) in enumerate(E) if p in h and not dup[e]]       # one Hpl block per (point, free pose)
        task0 = len(R["gemm_task"]) // 4
        etask = [task0 + blocks.index(e) if e in blocks else -1 for e in range(len(E))]
        gemm_ps = min(GEMM_PS, PANEL // (8 * 2 * 3 * (ld + GEMM_LDS_PAD)))
        stages, cur = [], [0, 0, 0, 0]
        for l in range(NL):
            nb = sum(1 for e in blocks if E[e][1] == l)
            if cur[1] == gemm_ps or cur[3] + nb > GEMM_STAGE_EDGES:
                stages.append(tuple(cur))
                cur = [l, 0, cur[2] + cur[3], 0]
            cur[1] += 1
            cur[3] += nb
        if cur[1]:
            stages.append(tuple(cur))
        nt = ld // 16
        ngrp = -(-sum(-(-(nt - tr) // GEMM_C) for tr in range(nt)) // (GEMM_WAVES * GEMM_NCH))
        ks = max(1, min(-(-GEMM_TARGET_WGS // (G * ngrp)), max(1, len(stages) // 4)))
        if big:
            ks = 1
        mask = [0] * NL
        if stats and not big:
            for e, (p, l, _) in enumerate(E):
                if p in h:
                    mask[l] |= 1 << (6 * h[p] // 16) | 1 << ((6 * h[p] + 5) // 16)
        if stats:
            issued += sum(bin(m).count("1") * (bin(m).count("1") + 1) / 2 for m in mask) * 2048.0
        dense += nt * (nt + 1) / 2 * 2048.0 * NL
        cam_off = -1
        if g["cams"]:
            cam_off = sums["ncam"]
            sums["ncam"] += len(g["cams"])
        info.append(dict(nf=nf, blocks=blocks, E=E, h=h))
        R["gd"].append(dict(n_poses=NP, n_points=NL, n_edges=len(E), nf=nf, n=n, ld=ld, pose_off=sums["P"], point_off=sums["L"], edge_off=sums["E"], free_off=sums["F"],
                            ptstart_off=sums["L"] + gi, posestart_off=sums["F"] + gi, s_off=sums["s"], spart_off=sums["sp"], gemm_off=task0, stage_off=len(R["gemm_stage"]) // 4,
                            n_stages=len(stages), gemm_ps=gemm_ps, ks=ks, nt16=nt, ngrp=ngrp, pair_off=0, pent_off=0, cam_off=cam_off, cam_model=g["cam_model"], cam2_model=1))
        R["pose_cam"] += g["pose_cam"] if g["cams"] else [0] * NP
        R["hidx"] += [h.get(i, -1) for i in range(NP)]
        R["edge_pose"] += [p for p, _, _ in E]
        R["edge_point"] += [l for _, l, _ in E]
        R["edge_stereo"] += types
        R["edge_dup"] += dup
        R["edge_next"] += nxt
        R["edge_task"] += etask
        R["pt_start"] += [sum(1 for _, l, _ in E if l < k) for k in range(NL + 1)]
        R["pose_start"] += pose_start
        R["pose_edges"] += pm
        R["pm_point"] += [E[e][1] for e in pm]
        R["pm_type"] += [types[e] for e in pm]
        R["pm_task"] += [etask[e] for e in pe] + [-1] * (len(E) - len(pe))
        R["ptmask"] += mask
        R["x1_off"].append(sums["x1"])
        R["x2_off"].append(sums["x2"])
        obs = lambda e: [10.0 * (e + e0g) + k + 100.0 * gi for k in range(3)]
        is2 = lambda e: 1.0 + (e + e0g) + 0.5 * gi
        R["edge_obs"] += [x for e in range(len(E)) for x in obs(e)]
        R["edge_is2"] += [is2(e) for e in range(len(E))]
        R["pm_obs"] += [x for e in pm for x in obs(e)]
        R["pm_is2"] += [is2(e) for e in pm]
        for i in range(NP):
            q = [0.1 * i, 0.2, -0.3, -0.9 if i & 1 else 0.9]
            if q[3] < 0:
                q = [-x for x in q]
            nn = math.sqrt(sum(x * x for x in q))
            R["poses0"] += [x / nn for x in q] + [1.0 * i, 2.0 * i, 3.0 * i + gi]
        R["points0"] += [x for l in range(pt0g, pt0g + NL) for x in (l, l + 0.5, l + 0.25 + gi)]
        R["gemm_task"] += [x for e in blocks for x in (e, 6 * h[E[e][0]], E[e][1], gi)]
        R["gemm_stage"] += [x for s in stages for x in s]
        sums["x1"] += 42 * nf + 2
        sums["x2"] += ld * ld + 6 * nf
        sums["s"] += ld * ld
        sums["sp"] += ks * ld * ld                                         # Spart is sized by the GEMM's split, whichever form runs
        sums["P"] += NP; sums["L"] += NL; sums["E"] += len(E); sums["F"] += nf
    pair_lists = any_big or (world == 1 and mode != 2)
    pstart = pent = max_npair = max_row = 0
    if pair_lists:
        for d, i in zip(R["gd"], info):
            d["ks"], d["pair_off"], d["pent_off"] = 1, pstart, pent
            per_point = {}
            for e in i["blocks"]:
                per_point[i["E"][e][1]] = per_point.get(i["E"][e][1], 0) + 1
            pent += sum(nb * (nb + 1) // 2 for nb in per_point.values())
            pstart += i["nf"] * (i["nf"] + 1) // 2 + 1
            max_npair = max(max_npair, i["nf"] * (i["nf"] + 1) // 2)
            max_row = max([max_row] + [sum(1 for e in i["blocks"] if i["E"][e][0] == p) for p in i["h"]])
    R["scalars"] = dict(sumP=sums["P"], sumL=sums["L"], sumE=sums["E"], sumF=sums["F"], max_edges=max(d["n_edges"] for d in R["gd"]), max_points=max(d["n_points"] for d in R["gd"]),
                        max_nf=max(d["nf"] for d in R["gd"]), max_ld=max(d["ld"] for d in R["gd"]), s_total=sums["s"], spart_total=sums["sp"], any_big=int(any_big),
                        general=int(general), pair_lists=int(pair_lists), pair_total_start=pstart, pair_total_ent=pent, max_npair=max_npair, max_row_blocks=max_row,
                        x_need=max(sums["x1"], sums["x2"], 3 * G))
    R["flops"] = (issued, dense)
    return R


def gd_of(got, g):
    return dict(zip(GD, got["gd"][g * len(GD):(g + 1) * len(GD)]))


def check_against_restatement(got, c):
    assert (got["rc"], got["msg"]) == (0, "-")
    R = restate(c)
    for g, want in enumerate(R["gd"]):
        assert gd_of(got, g) == want, (c["name"], g)
    for k in ("pose_cam", "hidx", "edge_pose", "edge_point", "edge_stereo", "edge_dup", "edge_next", "edge_task", "pt_start", "pose_start", "pose_edges", "pm_point", "pm_task",
              "pm_type", "ptmask", "x1_off", "x2_off", "gemm_task", "gemm_stage", "edge_obs", "edge_is2", "pm_is2", "pm_obs", "points0"):
        assert got[k] == R[k], (c["name"], k)
    assert got["poses0"] == pytest.approx(R["poses0"], rel=0, abs=1e-15)
    assert dict(zip(SCALARS, got["scalars"])) == R["scalars"], c["name"]
    assert (got["flops"][0], got["flops"][2]) == R["flops"]
    if c["world"] > 1:
        assert got["slices"] == list(R["slices"])
    return R


@pytest.mark.parametrize("name", ["tiny_pairs", "tiny_gemm", "cut_ps", "cut_edges", "cut_ld", "big", "two", "two_pairs", "cams", "shard0", "shard1"])
def test_every_array_follows_the_rules(printed, name):
    check_against_restatement(printed[name], next(c for c in CASES if c["name"] == name))


def test_tiny_graph_spelled_out(printed):
    for name in ("tiny_gemm", "tiny_pairs"):
        got = printed[name]
        d = gd_of(got, 0)
        assert (d["nf"], d["n"], d["ld"], d["nt16"], d["ngrp"], d["ks"], d["gemm_ps"], d["n_stages"]) == (2, 12, 96, 6, 1, 1, 8, 1)
        assert got["hidx"] == [-1, 0, 1, -1]                                   # pose 3 is free but has no edge: nothing in the system
        assert got["pt_start"] == [0, 1, 4, 6, 7, 9] and got["pose_start"] == [0, 4, 7]
        assert got["pose_edges"] == [1, 2, 6, 8, 3, 5, 7, 0, 0]
        assert got["pm_point"] == [1, 1, 3, 4, 1, 2, 4, 0, 0] and got["pm_type"] == [0, 2, 1, 0, 1, 0, 0, 0, 0]         # the last two: edge 0 once more
        assert got["pm_is2"] == [2.0, 3.0, 7.0, 9.0, 4.0, 6.0, 8.0, 1.0, 1.0] and got["pm_obs"][-6:] == [0.0, 1.0, 2.0, 0.0, 1.0, 2.0]
        assert got["edge_dup"] == [0, 0, 1, 0, 0, 0, 0, 0, 0] and got["edge_next"] == [-1, 2, -1, -1, -1, -1, -1, -1, -1]
        assert got["edge_task"] == [-1, 0, -1, 1, -1, 2, 3, 4, 5]              # the point of the fixed pose: none; the twin: one block for the pair
        assert got["gemm_task"] == [1, 0, 1, 0, 3, 6, 1, 0, 5, 6, 2, 0, 6, 0, 3, 0, 7, 6, 4, 0, 8, 0, 4, 0]
        assert got["gemm_stage"] == [0, 5, 0, 6]
        assert got["pm_task"] == [0, -1, 3, 5, 1, 2, 4, -1, -1]
        assert got["x1_off"] == [0] and got["x2_off"] == [0]
        s = dict(zip(SCALARS, got["scalars"]))
        assert s["general"] == 1 and s["any_big"] == 0 and s["x_need"] == 96 * 96 + 12 and (s["sumP"], s["sumL"], s["sumE"], s["sumF"]) == (4, 5, 9, 2)
    assert printed["tiny_gemm"]["ptmask"] == [0, 1, 1, 1, 1] and printed["tiny_pairs"]["ptmask"] == [0] * 5
    s = dict(zip(SCALARS, printed["tiny_pairs"]["scalars"]))
    # points 1 and 4 hold two blocks (3 entries each), points 2 and 3 one; both free poses hold three blocks
    assert (s["pair_lists"], s["pair_total_ent"], s["pair_total_start"], s["max_npair"], s["max_row_blocks"]) == (1, 8, 4, 3, 3)
    s = dict(zip(SCALARS, printed["tiny_gemm"]["scalars"]))
    assert (s["pair_lists"], s["pair_total_ent"], s["pair_total_start"], s["max_row_blocks"]) == (0, 0, 0, 0)


def test_stage_cuts(printed):
    assert printed["cut_ps"]["gemm_stage"] == [0, 8, 0, 8, 8, 1, 8, 1]                 # nine points with one block each: GEMM_PS = 8 points, then one
    assert printed["cut_edges"]["gemm_stage"] == [0, 4, 0, 80, 4, 1, 80, 20]           # 80 + 20 > GEMM_STAGE_EDGES: cut before the fifth point
    d = gd_of(printed["cut_ld"], 0)
    assert (d["nf"], d["ld"], d["gemm_ps"]) == (80, 480, 5)
    assert printed["cut_ld"]["gemm_stage"] == [0, 5, 0, 67, 5, 1, 67, 13]               # 13 or 14 blocks per point, 80 in all: only gemm_ps = 5 cuts


def test_big_windows(printed):
    got = printed["big"]
    d, s = gd_of(got, 0), dict(zip(SCALARS, got["scalars"]))
    assert (d["nf"], d["n"], d["ld"], d["ks"]) == (81, 486, 576, 1) and s["any_big"] == 1 and s["pair_lists"] == 1
    assert got["ptmask"] == [0] * 90
    assert (printed["big_sharded"]["rc"], printed["big_sharded"]["msg"]) == (BADARG, "landmark-sharded solve: at most 80 free keyframes per window")
    assert (printed["too_big"]["rc"], printed["too_big"]["msg"]) == (BADARG, "more than 682 free keyframes in one window")


def test_second_graph_of_a_batch(printed):
    d = gd_of(printed["two"], 1)
    assert (d["pose_off"], d["point_off"], d["edge_off"], d["free_off"], d["ptstart_off"], d["posestart_off"]) == (4, 5, 9, 2, 6, 3)
    assert (d["s_off"], d["spart_off"], d["gemm_off"], d["stage_off"]) == (96 * 96, 96 * 96, 6, 1)
    assert printed["two"]["x1_off"] == [0, 86] and printed["two"]["x2_off"] == [0, 96 * 96 + 12]
    assert printed["two"]["edge_task"][9:] == [6, 7, -1, 8, 9] and printed["two"]["gemm_task"][24:28] == [0, 0, 0, 1]
    d = gd_of(printed["two_pairs"], 1)
    assert (d["pair_off"], d["pent_off"]) == (4, 8)


def test_camera_table(printed):
    got = printed["cams"]
    assert gd_of(got, 0)["cam_off"] == 0 and got["pose_cam"] == [1, 0, 1] and dict(zip(SCALARS, got["scalars"]))["general"] == 1
    # per camera c: fx, bf, cam_model, kb[3], Trl[3], Trl[4], cy2, kb2[0], cam2_model as the program filled them
    assert got["cams"] == pytest.approx([500.0, 40.0, 0.0, 0.04, 1.0, 0.0, 200.0, 0.02, 1.0, 501.0, 41.0, 1.0, 1.04, 0.5, 0.1, 201.0, 1.02, 0.0], rel=0, abs=1e-12)
    assert got["gcal"] == pytest.approx([700.0, 710.0, 330.0, 250.0, 35.0, 0.1, 0.4, 0.0, 0.25, 600.0, 610.0, 310.0, 210.0, 0.2, 0.8], rel=0, abs=1e-12)
    assert printed["tiny_gemm"]["cams"] == [] and gd_of(printed["tiny_gemm"], 0)["cam_off"] == -1 and printed["tiny_gemm"]["pose_cam"] == [0] * 4


def test_sharding(printed):
    r0, r1 = printed["shard0"], printed["shard1"]
    # 5 points over 2 ranks: [0, 2) and [2, 5); the second graph's 3 points: [0, 1) and [1, 3)
    assert r0["slices"] == [0, 2, 0, 3, 0, 1, 0, 2] and r1["slices"] == [2, 3, 3, 6, 1, 2, 2, 3]
    assert r0["pts_at"] == [0, 0] and r1["pts_at"] == [6, 3]
    assert r0["edge_point"] == [0, 0, 1, 0, 0] and r1["edge_point"] == [0, 0, 1, 2, 2, 2, 0, 0, 1]
    # pose 3 of the first graph has no edge on rank 0 and is numbered there all the same
    assert r0["hidx"] == r1["hidx"] == [-1, 0, 1, 2, 0, -1, 1]
    assert (printed["shard_few"]["rc"], printed["shard_few"]["msg"]) == (BADARG, "a sharded graph needs at least one point per rank")


@pytest.mark.parametrize("name,msg", [("no_poses", "-"), ("not_major", "edges must be point-major with valid ids"), ("bad_id", "edges must be point-major with valid ids"),
                                      ("bad_type", "edge_stereo must be 0, 1 or 2"), ("no_trl", "edges of type 2 need Trl (mTrl) and the second camera"),
                                      ("null_tables", "n_cameras > 0 needs cameras and pose_camera"), ("bad_pose_cam", "pose_camera out of range")])
def test_refusals(printed, name, msg):
    assert (printed[name]["rc"], printed[name]["msg"]) == (BADARG, msg)


def test_estimates_are_normalised(printed):
    p = printed["tiny_gemm"]["poses0"]
    for i in range(4):
        q, nn = p[7 * i:7 * i + 4], math.sqrt(0.01 * i * i + 0.04 + 0.09 + 0.81)
        sign = -1.0 if i & 1 else 1.0                                            # odd poses came with w < 0: the whole quaternion is flipped
        assert q == pytest.approx([sign * 0.1 * i / nn, sign * 0.2 / nn, sign * -0.3 / nn, 0.9 / nn], rel=0, abs=1e-15)
        assert p[7 * i + 4:7 * i + 7] == [1.0 * i, 2.0 * i, 3.0 * i]
