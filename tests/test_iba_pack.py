"""The host packing of the inertial bundle adjustments (csrc/iba_pack.h) in a stand-alone host program under the address and
undefined-behaviour sanitizers (and, for the threaded packing, the thread sanitizer): unknown numbering, per-keyframe edge lists and
their chunks, pair lists with twins and their chunks, edge colours, the rebase of chunks of windows packed on several threads, the
upload blob, every refusal, and FullInertialBA's activity filter.  The program reads crafted windows from a text file and prints every
array of every window, taken out of the blob through the offsets table and the window's own offsets; they are compared with a
restatement of the rules written here in plain Python / numpy.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-slam3-mac_amd", "csrc")
BADARG, CAPACITY = -1, -4
LOCAL, FULL, FULL_SHARED = 0, 1, 2
KF, PRE, CHUNK = 21, 67, 256
WIN_BYTES = 22 * 4 + 2 * 8 + 17 * 8 + 3 * 4 + 4 + 24 * 8       # IbaWin: 22 ints, 2 long long, 17 doubles, 3 ints and 4 bytes of padding, 24 doubles

MAIN = r"""
#include "iba_pack.h"
template <class T> static void line(int w, const char *name, const T *p, size_t n) { printf("w%d %s", w, name); for (size_t i = 0; i < n; i++) printf(" %lld", (long long)p[i]); printf("\n"); }
static void dline(int w, const char *name, const double *p, size_t n) { printf("w%d %s", w, name); for (size_t i = 0; i < n; i++) printf(" %.17g", p[i]); printf("\n"); }
static unsigned long long fnv(const void *p, size_t n) { unsigned long long h = 1469598103934665603ull; for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull; return h; }
struct Win { std::vector<uint8_t> fixed, imu, type, close, rob; std::vector<int32_t> ekf, ept, k1, k2; std::vector<double> obs, is2, pre, info, ig, ia, kfs, pts; };
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char name[64], kind[16];
    int mode, nthr, nw;
    while (fscanf(f, "%63s %15s %d %d %d", name, kind, &mode, &nthr, &nw) == 5) {
        std::vector<Win> ws(nw);
        std::vector<orbhip_iba_window> wins(nw);
        std::vector<const double *> kfp(nw), ptp(nw);
        for (int w = 0; w < nw; w++) {
            Win &S = ws[w];
            orbhip_iba_window &g = wins[w];
            memset(&g, 0, sizeof(g));
            int nk, nl, ne, nm, cam2;
            if (fscanf(f, "%d %d %d %d %d", &nk, &nl, &ne, &nm, &cam2) != 5) return 3;
            S.fixed.resize(nk); S.imu.resize(nk);
            for (auto &x : S.fixed) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = (uint8_t)v; }
            for (auto &x : S.imu) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = (uint8_t)v; }
            S.ekf.resize(ne); S.ept.resize(ne); S.type.resize(ne);
            for (int e = 0; e < ne; e++) { int a, b, c; if (fscanf(f, "%d %d %d", &a, &b, &c) != 3) return 3; S.ekf[e] = a; S.ept[e] = b; S.type[e] = (uint8_t)c; }
            S.k1.resize(nm); S.k2.resize(nm);
            for (int m = 0; m < nm; m++) { int a, b; if (fscanf(f, "%d %d", &a, &b) != 2) return 3; S.k1[m] = a; S.k2[m] = b; }
            for (int e = 0; e < ne; e++) { for (int k = 0; k < 3; k++) S.obs.push_back(10.0 * e + k); S.is2.push_back(1.0 + e); S.close.push_back(e % 3 == 0 ? 7 : 0); }
            for (int m = 0; m < nm; m++) {
                for (int k = 0; k < IBA_PRE; k++) S.pre.push_back(1000.0 * m + k);
                for (int k = 0; k < 81; k++) S.info.push_back(100.0 * m + k);
                for (int k = 0; k < 9; k++) { S.ig.push_back(10.0 * m + k + 0.5); S.ia.push_back(10.0 * m + k + 0.25); }
                S.rob.push_back(m % 2 ? 5 : 0);
            }
            for (int i = 0; i < IBA_KF * nk; i++) S.kfs.push_back(1000.0 * w + i);
            for (int i = 0; i < 3 * nl; i++) S.pts.push_back(100.0 * w + i + 0.5);
            g.n_kf = nk; g.kf_fixed = S.fixed.data(); g.kf_imu = S.imu.data();
            for (int i = 0; i < 9; i++) g.Rcb[i] = 0.1 * (i + 1) + w;
            for (int i = 0; i < 3; i++) g.tcb[i] = 1.0 + i + w;
            for (int i = 0; i < 12; i++) g.Trl[i] = 0.05 * (i + 1) - 0.2;
            g.fx = 500 + w; g.fy = 510; g.cx = 320; g.cy = 240; g.bf = 40; g.camera_model = 1; g.has_cam2 = cam2;
            g.fx2 = 400 + w; g.fy2 = 410; g.cx2 = 300; g.cy2 = 200; g.camera2_model = 1;
            for (int k = 0; k < 4; k++) { g.kb[k] = 0.5 * (k + 1); g.kb2[k] = 0.25 * (k + 1); }
            g.n_points = nl; g.n_edges = ne; g.edge_kf = S.ekf.data(); g.edge_point = S.ept.data(); g.edge_obs = S.obs.data(); g.edge_stereo = S.type.data();
            g.edge_inv_sigma2 = S.is2.data(); g.edge_close = S.close.data();
            g.n_inertial = nm; g.in_kf1 = S.k1.data(); g.in_kf2 = S.k2.data(); g.in_preint = S.pre.data(); g.in_info = S.info.data(); g.in_info_g = S.ig.data();
            g.in_info_a = S.ia.data(); g.in_robust = S.rob.data();
            kfp[w] = S.kfs.data(); ptp[w] = S.pts.data();
        }
        if (!strcmp(kind, "filter")) {
            for (int w = 0; w < nw; w++) {
                FibaMap F;
                orbhip_iba_window o;
                const int rc = fiba_filter(wins[w], mode != 0, F, o);
                printf("case %s %d -\n", name, rc);
                if (rc != ORBHIP_OK) continue;
                const long long sc[] = {o.n_kf, o.n_points, o.n_edges, o.n_inertial, o.edge_close == nullptr, o.kf_fixed == wins[w].kf_fixed, o.has_cam2};
                line(w, "scalars", sc, 7);
                line(w, "edge_kf", o.edge_kf, o.n_edges); line(w, "edge_point", o.edge_point, o.n_edges); line(w, "edge_stereo", o.edge_stereo, o.n_edges);
                dline(w, "edge_is2", o.edge_inv_sigma2, o.n_edges); dline(w, "edge_obs", o.edge_obs, 3 * (size_t)o.n_edges);
                line(w, "in_kf1", o.in_kf1, o.n_inertial); line(w, "in_kf2", o.in_kf2, o.n_inertial); line(w, "in_robust", o.in_robust, o.n_inertial);
                dline(w, "in_pre", o.in_preint, (size_t)IBA_PRE * o.n_inertial); dline(w, "in_info", o.in_info, 81 * (size_t)o.n_inertial);
                dline(w, "in_info_g", o.in_info_g, 9 * (size_t)o.n_inertial); dline(w, "in_info_a", o.in_info_a, 9 * (size_t)o.n_inertial);
            }
            continue;
        }
        IbaPacked R;
        const int rc = iba_pack_windows(wins.data(), nw, kfp.data(), ptp.data(), mode, nthr, R);
        printf("case %s %d %s\n", name, rc, R.err.empty() ? "-" : R.err.c_str());
        if (rc != ORBHIP_OK) continue;
        const IbaBlobOffsets &O = R.o;
        const uint8_t *B = R.blob.data();
        const long long sums[] = {(long long)R.sumKF, (long long)R.sumL, (long long)R.sumE, (long long)R.sumM, (long long)R.sumX, (long long)R.sumH, (long long)R.n_kftask,
                                  (long long)R.n_pairtask, R.max_n, (long long)R.blob.size(), (long long)R.kfs.size(), (long long)R.pts.size()};
        line(-1, "sums", sums, 12);
        line(-1, "offsets", (const size_t *)&O, sizeof(O) / sizeof(size_t));
        const unsigned long long hs[] = {fnv(B, R.blob.size()), fnv(R.hw.data(), sizeof(IbaWin) * R.hw.size()), fnv(R.kfs.data(), 8 * R.kfs.size()), fnv(R.pts.data(), 8 * R.pts.size()),
                                         (unsigned long long)(memcmp(B + O.win, R.hw.data(), sizeof(IbaWin) * R.hw.size()) == 0)};
        printf("w-1 hashes %llu %llu %llu %llu %llu\n", hs[0], hs[1], hs[2], hs[3], hs[4]);
        for (int w = 0; w < nw; w++) {
            const IbaWin &W = R.hw[w];
            const long long v[] = {W.n_kf, W.L, W.E, W.M, W.n, W.nfree, W.ncolors, W.npairs, W.nktask, W.nptask, W.kf_off, W.pt_off, W.e_off, W.m_off, W.x_off, W.free_off,
                                   W.ptstart_off, W.kfe_off, W.ktask_off, W.ktstart_off, W.ptask_off, W.ptstart2_off, W.pent_off, W.h_off, W.cam_model, W.has_cam2, W.cam2_model};
            line(w, "win", v, sizeof(v) / sizeof(v[0]));
            const double c[] = {W.fx, W.fy, W.cx, W.cy, W.bf, W.kb[0], W.kb[3], W.fx2, W.fy2, W.cx2, W.cy2, W.kb2[0], W.kb2[3]};
            dline(w, "cal", c, 13); dline(w, "Rcb", W.Rcb, 9); dline(w, "tcb", W.tcb, 3); dline(w, "Rcb2", W.Rcb2, 9); dline(w, "tcb2", W.tcb2, 3);
            line(w, "kf_xoff", (const int *)(B + O.kf_xoff) + W.kf_off, W.n_kf); line(w, "kf_imu", B + O.kf_imu + W.kf_off, W.n_kf);
            line(w, "free_kf", (const int *)(B + O.free_kf) + W.free_off, W.nfree);
            line(w, "edge_kf", (const int *)(B + O.edge_kf) + W.e_off, W.E); line(w, "edge_point", (const int *)(B + O.edge_point) + W.e_off, W.E);
            line(w, "edge_stereo", B + O.edge_stereo + W.e_off, W.E); line(w, "edge_close", B + O.edge_close + W.e_off, W.E);
            dline(w, "edge_obs", (const double *)(B + O.edge_obs) + 3 * (size_t)W.e_off, 3 * (size_t)W.E); dline(w, "edge_is2", (const double *)(B + O.edge_is2) + W.e_off, W.E);
            line(w, "pt_start", (const int *)(B + O.pt_start) + W.ptstart_off, W.L + 1);
            const int *kts = (const int *)(B + O.kf_task_start) + W.ktstart_off, *pts2 = (const int *)(B + O.pair_task_start) + W.ptstart2_off;
            line(w, "kf_task_start", kts, W.nfree + 1); line(w, "pair_task_start", pts2, W.npairs + 1);
            const int *kt = (const int *)(B + O.kf_task) + 4 * (size_t)W.ktask_off, *pt = (const int *)(B + O.pair_task) + 4 * (size_t)W.ptask_off;
            line(w, "kf_task", kt, 4 * (size_t)W.nktask); line(w, "pair_task", pt, 4 * (size_t)W.nptask);
            const size_t nkfe = W.nktask ? (size_t)kt[4 * (W.nktask - 1) + 2] : 0;            // the last chunk's end
            size_t npent = 0;
            for (int t = 0; t < W.nptask; t++) npent = std::max(npent, (size_t)pt[4 * t + 2]);
            line(w, "kf_edges", (const int *)(B + O.kf_edges) + W.kfe_off, nkfe); line(w, "pair_ent", (const int *)(B + O.pair_ent) + 2 * (size_t)W.pent_off, 2 * npent);
            line(w, "in_kf1", (const int *)(B + O.in_kf1) + W.m_off, W.M); line(w, "in_kf2", (const int *)(B + O.in_kf2) + W.m_off, W.M);
            line(w, "in_color", (const int *)(B + O.in_color) + W.m_off, W.M); line(w, "in_robust", B + O.in_robust + W.m_off, W.M);
            dline(w, "in_pre", (const double *)(B + O.in_pre) + (size_t)IBA_PRE * W.m_off, (size_t)IBA_PRE * W.M); dline(w, "in_info", (const double *)(B + O.in_info) + 81 * (size_t)W.m_off, 81 * (size_t)W.M);
            dline(w, "in_info_g", (const double *)(B + O.in_info_g) + 9 * (size_t)W.m_off, 9 * (size_t)W.M); dline(w, "in_info_a", (const double *)(B + O.in_info_a) + 9 * (size_t)W.m_off, 9 * (size_t)W.M);
            dline(w, "kfs", R.kfs.data() + (size_t)IBA_KF * W.kf_off, (size_t)IBA_KF * W.n_kf); dline(w, "pts", R.pts.data() + 3 * (size_t)W.pt_off, 3 * (size_t)W.L);
        }
    }
    fclose(f);
    return 0;
}
"""

WIN = ["n_kf", "L", "E", "M", "n", "nfree", "ncolors", "npairs", "nktask", "nptask", "kf_off", "pt_off", "e_off", "m_off", "x_off", "free_off", "ptstart_off", "kfe_off",
       "ktask_off", "ktstart_off", "ptask_off", "ptstart2_off", "pent_off", "h_off", "cam_model", "has_cam2", "cam2_model"]
# the 25 arrays of the blob in the order they are laid out, with their element sizes
OFFSETS = [("win", None), ("kf_xoff", 4), ("kf_imu", 1), ("free_kf", 4), ("edge_kf", 4), ("edge_point", 4), ("edge_obs", 8), ("edge_is2", 8), ("edge_stereo", 1),
           ("edge_close", 1), ("pt_start", 4), ("kf_edges", 4), ("pair_ent", 8), ("kf_task", 16), ("kf_task_start", 4), ("pair_task", 16), ("pair_task_start", 4),
           ("in_kf1", 4), ("in_kf2", 4), ("in_color", 4), ("in_robust", 1), ("in_pre", 8), ("in_info", 8), ("in_info_g", 8), ("in_info_a", 8)]
DOUBLES = ("cal", "Rcb", "tcb", "Rcb2", "tcb2", "edge_obs", "edge_is2", "in_pre", "in_info", "in_info_g", "in_info_a", "kfs", "pts")


def window(fixed, imu, edges, n_points, inertial=(), cam2=0):
    return dict(fixed=list(fixed), imu=list(imu), edges=list(edges), n_points=n_points, inertial=list(inertial), cam2=cam2)


def case(name, wins, mode=LOCAL, nthr=1, kind="pack"):
    return dict(name=name, wins=wins, mode=mode, nthr=nthr, kind=kind)


# keyframes: 0 fixed (IMU), 1 free without IMU (6 unknowns), 2 and 3 free with IMU (15 each); keyframe 2 sees point 1 through both cameras
# (types 0 and 2).  A chain of three inertial edges needs four keyframes with IMU states, so a second fixed one (4, no visual edge) ends
# it: 0-2, 2-3, 3-4
TINY = window([1, 0, 0, 0, 1], [1, 0, 1, 1, 1], [(0, 0, 0), (1, 0, 1), (2, 1, 0), (2, 1, 2), (3, 1, 0), (1, 2, 0), (3, 2, 1)], 3, [(0, 2), (2, 3), (3, 4)], cam2=1)
SEAM_A = window([0, 0], [0, 0], [(k, l, 0) for l in range(257) for k in (0, 1) if k == 1 or l < 256], 257)        # 256 and 257 edges; the pair shares 256 points
SEAM_B = window([0, 0], [0, 0], [(k, l, 0) for l in range(257) for k in (0, 1)], 257)                              # the pair shares 257 points
EMPTY = window([1, 0], [1, 1], [], 0)
SMALL = window([0, 1, 0], [1, 1, 0], [(0, 0, 0), (2, 0, 0), (1, 1, 1), (2, 1, 0)], 2, [(1, 0)])
SIX = [TINY, SMALL, EMPTY, SEAM_A, SMALL, TINY]
MANY_KF = window([0] * 33, [1] * 33, [], 0)                                                                         # 33 x 15 = 495 unknowns
MANY_IN = window([1, 0], [1, 1], [], 0, [(0, 1)] * 513)
STAR = window([0] + [1] * 257, [1] * 258, [], 0, [(0, k) for k in range(1, 258)])                                    # 257 inertial edges at keyframe 0: colour 256
# the filter: point 0 is seen only by the fixed keyframes 0 and 1; inertial edges 0-1 (both fixed), 1-2, 2-3
FILT = window([1, 1, 0, 0], [1, 1, 1, 1], [(0, 0, 0), (1, 0, 1), (0, 1, 0), (2, 1, 0), (3, 2, 1), (1, 2, 0)], 3, [(0, 1), (1, 2), (2, 3)])
CASES = [
    case("tiny", [TINY]), case("tiny_full", [TINY], FULL), case("tiny_shared", [TINY], FULL_SHARED),
    case("seams", [SEAM_A, SEAM_B]), case("empty", [EMPTY]),
    case("six_1", SIX, nthr=1), case("six_3", SIX, nthr=3),
    case("many_kf", [MANY_KF]), case("many_kf_full", [SMALL, MANY_KF], FULL), case("many_in", [MANY_IN]), case("star", [STAR]),
    case("no_imu", [window([0, 0], [1, 0], [], 0, [(0, 1)])]), case("not_major", [window([0], [1], [(0, 1, 0), (0, 0, 0)], 2)]),
    case("filter", [FILT], 0, kind="filter"), case("filter_shared", [FILT], 1, kind="filter"),
]


def spec_text(cases):
    out = []
    for c in cases:
        out.append("%s %s %d %d %d" % (c["name"], c["kind"], c["mode"], c["nthr"], len(c["wins"])))
        for g in c["wins"]:
            out.append("%d %d %d %d %d" % (len(g["fixed"]), g["n_points"], len(g["edges"]), len(g["inertial"]), g["cam2"]))
            out += [" ".join(map(str, g["fixed"])), " ".join(map(str, g["imu"])), " ".join("%d %d %d" % e for e in g["edges"]), " ".join("%d %d" % m for m in g["inertial"])]
    return "\n".join(out) + "\n"


def build(tmp, sanitize, tag):
    src, exe = tmp / "main.cc", str(tmp / ("iba_pack_" + tag))
    src.write_text(MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-Wall", "-Werror", "-pthread", "-I", CSRC, "-o", exe, str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def run(exe, spec):
    r = subprocess.run([exe, str(spec)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stdout and "runtime error" not in r.stdout and "WARNING" not in r.stdout, r.stdout[-3000:]
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], dict(rc=int(w[2]), msg=ln.split(None, 3)[3], text=[]))
            continue
        cur["text"].append(ln)
        cur.setdefault(int(w[0][1:]), {})[w[1]] = [float(x) for x in w[2:]] if w[1] in DOUBLES else [int(x) for x in w[2:]]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("iba_pack")


@pytest.fixture(scope="module")
def printed(tmp):
    spec = tmp / "cases.txt"
    spec.write_text(spec_text(CASES))
    out = run(build(tmp, "address,undefined", "asan"), spec)
    assert list(out) == [c["name"] for c in CASES]
    return out


# ---------------------------------------------------------------------------------------------------------------- the rules, restated
def restate_window(g, w, mode, at):
    """One window's arrays; `at` holds what the windows in front of it put into the batch (its offsets)."""
    K, E, M = len(g["fixed"]), g["edges"], g["inertial"]
    free = [k for k in range(K) if not g["fixed"][k]]
    f_of = {k: f for f, k in enumerate(free)}
    xoff, n = [], 0
    for k in range(K):
        xoff.append(-1 if g["fixed"][k] else n)
        if not g["fixed"][k]:
            n += (9 if mode == FULL_SHARED else 15) if g["imu"][k] else 6
    if mode == FULL_SHARED:
        n += 6                                                             # the shared biases come last
    chunks = lambda lo, hi: [(o, min(o + CHUNK, hi)) for o in range(lo, hi, CHUNK)]
    kf_edges, kf_task, kf_task_start = [], [], []
    for f, k in enumerate(free):
        mine = [e for e, (ek, _, _) in enumerate(E) if ek == k]
        kf_task_start.append(len(kf_task))
        kf_task += [(f, a, b, 0) for a, b in chunks(len(kf_edges), len(kf_edges) + len(mine))]
        kf_edges += mine
    kf_task_start.append(len(kf_task))
    # per pair of free keyframes (i <= j, row-major) the edges of every landmark both see, in landmark order; a keyframe's two edges to one
    # landmark give the pair (i, i) both orders besides each edge with itself
    pairs = [(i, j) for i in range(len(free)) for j in range(i, len(free))]
    ent = {p: [] for p in pairs}
    for l in range(g["n_points"]):
        fe = [(f_of[k], e) for e, (k, pl, _) in enumerate(E) if pl == l and k in f_of]
        for a in range(len(fe)):
            for b in range(a, len(fe)):
                (fa, ea), (fb, eb) = fe[a], fe[b]
                if fa > fb:
                    (fa, ea), (fb, eb) = (fb, eb), (fa, ea)
                ent[(fa, fb)].append((ea, eb))
                if a != b and fa == fb:
                    ent[(fa, fb)].append((fe[b][1], fe[a][1]))
    pair_ent, pair_task, pair_task_start = [], [], []
    for q, p in enumerate(pairs):
        pair_task_start.append(len(pair_task))
        pair_task += [(q, a, b, int(p[0] == p[1])) for a, b in chunks(len(pair_ent), len(pair_ent) + len(ent[p]))]
        pair_ent += ent[p]
    pair_task_start.append(len(pair_task))
    used, count, colour = {}, {}, []
    for k1, k2 in M:                                                       # greedy: the smallest colour neither keyframe has; rank inside the colour above bit 8
        c = 0
        while c in used.get(k1, ()) or c in used.get(k2, ()):
            c += 1
        used.setdefault(k1, set()).add(c); used.setdefault(k2, set()).add(c)
        colour.append(c | count.get(c, 0) << 8)
        count[c] = count.get(c, 0) + 1
    Rcb, tcb, Trl = 0.1 * np.arange(1, 10).reshape(3, 3) + w, np.arange(1.0, 4.0) + w, (0.05 * np.arange(1, 13) - 0.2).reshape(3, 4)
    R = dict(
        win=dict(n_kf=K, L=g["n_points"], E=len(E), M=len(M), n=n, nfree=len(free), ncolors=len(count), npairs=len(pairs), nktask=len(kf_task), nptask=len(pair_task),
                 kf_off=at["kf"], pt_off=at["l"], e_off=at["e"], m_off=at["m"], x_off=at["x"], free_off=at["free"], ptstart_off=at["l"] + at["w"], kfe_off=at["kfe"],
                 ktask_off=at["ktask"], ktstart_off=at["free"] + at["w"], ptask_off=at["ptask"], ptstart2_off=at["pairs"] + at["w"], pent_off=at["pent"], h_off=at["h"],
                 cam_model=1, has_cam2=g["cam2"], cam2_model=g["cam2"]),
        cal=[500.0 + w, 510.0, 320.0, 240.0, 40.0, 0.5, 2.0] + ([400.0 + w, 410.0, 300.0, 200.0, 0.25, 1.0] if g["cam2"] else [0.0] * 6),
        Rcb=Rcb.ravel().tolist(), tcb=tcb.tolist(),
        Rcb2=(Trl[:, :3] @ Rcb).ravel().tolist() if g["cam2"] else [0.0] * 9, tcb2=(Trl[:, :3] @ tcb + Trl[:, 3]).tolist() if g["cam2"] else [0.0] * 3,
        kf_xoff=xoff, kf_imu=[int(bool(x)) for x in g["imu"]], free_kf=free, edge_kf=[k for k, _, _ in E], edge_point=[l for _, l, _ in E], edge_stereo=[t for _, _, t in E],
        edge_close=[int(e % 3 == 0) for e in range(len(E))], edge_obs=[10.0 * e + k for e in range(len(E)) for k in range(3)], edge_is2=[1.0 + e for e in range(len(E))],
        pt_start=[sum(1 for _, l, _ in E if l < k) for k in range(g["n_points"] + 1)], kf_task_start=kf_task_start, pair_task_start=pair_task_start,
        kf_task=[x for t in kf_task for x in t], pair_task=[x for t in pair_task for x in t], kf_edges=kf_edges, pair_ent=[x for p in pair_ent for x in p],
        in_kf1=[a for a, _ in M], in_kf2=[b for _, b in M], in_color=colour, in_robust=[m % 2 for m in range(len(M))],
        in_pre=[1000.0 * m + k for m in range(len(M)) for k in range(PRE)], in_info=[100.0 * m + k for m in range(len(M)) for k in range(81)],
        in_info_g=[10.0 * m + k + 0.5 for m in range(len(M)) for k in range(9)], in_info_a=[10.0 * m + k + 0.25 for m in range(len(M)) for k in range(9)],
        kfs=[1000.0 * w + i for i in range(KF * K)], pts=[100.0 * w + i + 0.5 for i in range(3 * g["n_points"])])
    at = dict(w=at["w"] + 1, kf=at["kf"] + K, l=at["l"] + g["n_points"], e=at["e"] + len(E), m=at["m"] + len(M), x=at["x"] + n, h=at["h"] + n * n, free=at["free"] + len(free),
              kfe=at["kfe"] + len(kf_edges), ktask=at["ktask"] + len(kf_task), ptask=at["ptask"] + len(pair_task), pairs=at["pairs"] + len(pairs), pent=at["pent"] + len(pair_ent),
              max_n=max(at["max_n"], n))
    return R, at


def check_against_restatement(got, c):
    assert (got["rc"], got["msg"]) == (0, "-")
    at = dict(w=0, kf=0, l=0, e=0, m=0, x=0, h=0, free=0, kfe=0, ktask=0, ptask=0, pairs=0, pent=0, max_n=0)
    for w, g in enumerate(c["wins"]):
        R, at = restate_window(g, w, c["mode"], at)
        assert dict(zip(WIN, got[w]["win"])) == R.pop("win"), (c["name"], w)
        for k in ("Rcb2", "tcb2"):
            np.testing.assert_allclose(got[w][k], R.pop(k), rtol=1e-14, atol=0, err_msg="%s %d %s" % (c["name"], w, k))
        for k, want in R.items():
            assert got[w][k] == want, (c["name"], w, k)
    nw = len(c["wins"])
    counts = dict(kf_xoff=at["kf"], kf_imu=at["kf"], free_kf=at["free"], edge_kf=at["e"], edge_point=at["e"], edge_obs=3 * at["e"], edge_is2=at["e"], edge_stereo=at["e"],
                  edge_close=at["e"], pt_start=at["l"] + nw, kf_edges=at["kfe"], pair_ent=at["pent"], kf_task=at["ktask"], kf_task_start=at["free"] + nw, pair_task=at["ptask"],
                  pair_task_start=at["pairs"] + nw, in_kf1=at["m"], in_kf2=at["m"], in_color=at["m"], in_robust=at["m"], in_pre=PRE * at["m"], in_info=81 * at["m"],
                  in_info_g=9 * at["m"], in_info_a=9 * at["m"])
    sums = got[-1]["sums"]
    assert sums[:9] == [at["kf"], at["l"], at["e"], at["m"], at["x"], at["h"], at["ktask"], at["ptask"], at["max_n"]] and sums[10:] == [KF * at["kf"], 3 * at["l"]]
    # the blob: every array at the next multiple of 256 bytes, at least one element long
    off, offsets = 0, got[-1]["offsets"]
    assert len(offsets) == len(OFFSETS) == 25
    for (name, size), o in zip(OFFSETS, offsets):
        assert o == off, (c["name"], name)
        nbytes = max(WIN_BYTES * nw if size is None else size * max(counts[name], 1), 1)
        off = -(-(o + nbytes) // 256) * 256
    assert sums[9] == offsets[-1] + 8 * max(counts["in_info_a"], 1)
    assert got[-1]["hashes"][4] == 1                                          # the windows as the blob holds them are the windows returned


@pytest.mark.parametrize("name", ["tiny", "tiny_full", "tiny_shared", "seams", "empty", "six_1", "six_3"])
def test_every_array_follows_the_rules(printed, name):
    check_against_restatement(printed[name], next(c for c in CASES if c["name"] == name))


def test_tiny_window_spelled_out(printed):
    got = printed["tiny"][0]
    w = dict(zip(WIN, got["win"]))
    assert (w["n"], w["nfree"], w["ncolors"], w["npairs"], w["has_cam2"]) == (36, 3, 2, 6, 1)
    assert got["kf_xoff"] == [-1, 0, 6, 21, -1] and got["free_kf"] == [1, 2, 3]
    assert got["kf_edges"] == [1, 5, 2, 3, 4, 6] and got["kf_task"] == [0, 0, 2, 0, 1, 2, 4, 0, 2, 4, 6, 0]
    # pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); the twin of keyframe 2 (block 1) at point 1: edges 2 and 3 with themselves and both orders
    assert got["pair_task"] == [0, 0, 2, 1, 2, 2, 3, 0, 3, 3, 7, 1, 4, 7, 9, 0, 5, 9, 11, 1] and got["pair_task_start"] == [0, 1, 1, 2, 3, 4, 5]
    assert got["pair_ent"] == [1, 1, 5, 5, 5, 6, 2, 2, 2, 3, 3, 2, 3, 3, 2, 4, 3, 4, 4, 4, 6, 6]
    assert got["in_color"] == [0, 1, 0 | 1 << 8]                              # a chain of three: colours 0, 1, 0, the second edge of colour 0 with rank 1
    assert got["in_robust"] == [0, 1, 0] and got["edge_close"] == [1, 0, 0, 1, 0, 0, 1]
    Trl = (0.05 * np.arange(1, 13) - 0.2).reshape(3, 4)
    np.testing.assert_allclose(np.array(got["Rcb2"]).reshape(3, 3), Trl[:, :3] @ (0.1 * np.arange(1, 10).reshape(3, 3)), rtol=1e-14)
    np.testing.assert_allclose(got["tcb2"], Trl[:, :3] @ np.arange(1.0, 4.0) + Trl[:, 3], rtol=1e-14)


def test_modes(printed):
    assert printed["tiny_full"][0]["kf_xoff"] == [-1, 0, 6, 21, -1] and dict(zip(WIN, printed["tiny_full"][0]["win"]))["n"] == 36
    assert printed["tiny_shared"][0]["kf_xoff"] == [-1, 0, 6, 15, -1] and dict(zip(WIN, printed["tiny_shared"][0]["win"]))["n"] == 6 + 9 + 9 + 6


def test_chunk_seams(printed):
    a, b = printed["seams"][0], printed["seams"][1]
    assert a["kf_task_start"] == [0, 1, 3] and a["kf_task"] == [0, 0, 256, 0, 1, 256, 512, 0, 1, 512, 513, 0]              # 256 edges: one chunk; 257: two
    assert a["pair_task_start"] == [0, 1, 2, 4]                                                                            # (0,0) 256, (0,1) 256, (1,1) 257 entries
    assert a["pair_task"] == [0, 0, 256, 1, 1, 256, 512, 0, 2, 512, 768, 1, 2, 768, 769, 1]
    assert b["kf_task_start"] == [0, 2, 4] and b["pair_task_start"] == [0, 2, 4, 6] and b["pair_task"][8:16] == [1, 257, 513, 0, 1, 513, 514, 0]


def test_empty_parts(printed):
    got = printed["empty"][0]
    w = dict(zip(WIN, got["win"]))
    assert (w["L"], w["E"], w["M"], w["n"], w["nfree"], w["npairs"], w["nktask"], w["nptask"], w["ncolors"]) == (0, 0, 0, 15, 1, 1, 0, 0, 0)
    assert got["pt_start"] == [0] and got["kf_task_start"] == [0, 0] and got["pair_task_start"] == [0, 0] and got["kf_edges"] == got["pair_ent"] == got["pts"] == []


def test_refusals(printed):
    big = "inertial BA: more than 480 keyframe unknowns (32 inertial keyframes)"
    assert (printed["many_kf"]["rc"], printed["many_kf"]["msg"]) == (CAPACITY, big)
    assert (printed["many_kf_full"]["rc"], printed["many_kf_full"]["msg"]) == (
        CAPACITY, "full inertial BA: map 1 has 495 reduced unknowns (33 free keyframes, 0 inertial edges); the limits are 480 and 512")
    assert (printed["many_in"]["rc"], printed["many_in"]["msg"]) == (CAPACITY, big)
    assert (printed["star"]["rc"], printed["star"]["msg"]) == (CAPACITY, "-")                  # colour 256 does not fit the eight bits below the rank
    assert (printed["no_imu"]["rc"], printed["no_imu"]["msg"]) == (BADARG, "-")
    assert (printed["not_major"]["rc"], printed["not_major"]["msg"]) == (BADARG, "-")


def test_chunked_packing_is_the_single_threaded_packing(printed, tmp):
    assert printed["six_1"]["text"] == printed["six_3"]["text"]                # windows, blob hash, offsets table, kfs / pts: identical
    assert printed["six_1"][-1]["hashes"][4] == 1
    # the three-thread run once more under the thread sanitizer
    spec = tmp / "six_3.txt"
    spec.write_text(spec_text([c for c in CASES if c["name"] == "six_3"]))
    out = run(build(tmp, "thread", "tsan"), spec)
    assert out["six_3"]["text"] == printed["six_3"]["text"]


def test_fiba_filter(printed):
    plain, shared = printed["filter"], printed["filter_shared"]
    for got in (plain, shared):
        assert got["rc"] == 0
        g = got[0]
        assert g["scalars"][:3] == [4, 3, 4] and g["scalars"][4:] == [1, 1, 0]                 # indices stay: 4 keyframes, 3 points; edge_close dropped
        assert g["edge_kf"] == [0, 2, 3, 1] and g["edge_point"] == [1, 1, 2, 2] and g["edge_stereo"] == [0, 0, 1, 0]      # point 0: only fixed keyframes see it
        assert g["edge_is2"] == [3.0, 4.0, 5.0, 6.0] and g["edge_obs"] == [10.0 * e + k for e in (2, 3, 4, 5) for k in range(3)]
        assert all(r == 1 for r in g["in_robust"])
    kept = [1, 2]                                                              # without shared biases the edge between the fixed keyframes 0 and 1 is inactive
    g = plain[0]
    assert g["scalars"][3] == 2 and g["in_kf1"] == [1, 2] and g["in_kf2"] == [2, 3] and g["in_robust"] == [1, 1]
    assert g["in_pre"] == [1000.0 * m + k for m in kept for k in range(PRE)] and g["in_info"] == [100.0 * m + k for m in kept for k in range(81)]
    assert g["in_info_g"] == [10.0 * m + k + 0.5 for m in kept for k in range(9)] and g["in_info_a"] == [10.0 * m + k + 0.25 for m in kept for k in range(9)]
    g = shared[0]
    assert g["scalars"][3] == 3 and g["in_kf1"] == [0, 1, 2] and g["in_kf2"] == [1, 2, 3] and g["in_robust"] == [1, 1, 1]
    assert g["in_pre"] == [1000.0 * m + k for m in range(3) for k in range(PRE)]
    assert g["in_info_g"] == [0.0] * 27 and g["in_info_a"] == [0.0] * 27
