// iba_pack.h -- the host's packing of inertial-BA windows (iba_kernels.hip: LocalInertialBA, FullInertialBA): SoA arrays, per-keyframe
// edge lists, per-pair block lists, task lists and edge colours of every window, chunks of windows packed on several host threads and
// laid out in one upload blob, and FullInertialBA's activity filter.  The kernels sum in exactly these orders, so the lists are part of
// the result's bits.  Nothing from HIP is included: a host compiler builds this header alone (tests/test_iba_pack.py does, under the
// address, undefined-behaviour and thread sanitizers); iba_create_impl allocates, uploads and fills the kernel's argument block.
// IbaWin's camera fields are also the rig of the inertial pose-only optimisation (pose_inertial_kernels.hip, through iba_edges.h).
#pragma once
#include "../../include/orbhip.h"
#include "ba_ldlt_limits.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#define IBA_KF ORBHIP_IBA_KF
#define IBA_PRE ORBHIP_IBA_PREINT
#define IBA_THREADS 512        // threads of a workgroup; also the most inertial edges of a window (one thread each)
#define IBA_KF_CHUNK 256
#define IBA_PAIR_CHUNK 256
// mode: IBA_LOCAL (LocalInertialBA), IBA_FULL (FullInertialBA, biases per keyframe), IBA_FULL_SHARED (bInit: 9 unknowns per inertial
// keyframe, the 6 shared bias unknowns last)
enum { IBA_LOCAL = 0, IBA_FULL = 1, IBA_FULL_SHARED = 2 };

struct IbaWin {
    int n_kf, L, E, M, n, nfree, ncolors, npairs, nktask, nptask;
    int kf_off, pt_off, e_off, m_off, x_off, free_off, ptstart_off, kfe_off, ktask_off, ktstart_off, ptask_off, ptstart2_off;
    long long pent_off, h_off;
    double Rcb[9], tcb[3], fx, fy, cx, cy, bf;
    int cam_model, has_cam2, cam2_model;            // camera 0; a second camera of the rig (EdgeMono(1) edges, edge type 2)
    double kb[4], Rcb2[9], tcb2[3], fx2, fy2, cx2, cy2, kb2[4];
};

// HIP's int4 / int2 as the host sees them (iba_kernels.hip asserts size and alignment)
struct alignas(16) IbaInt4 { int x, y, z, w; };
struct alignas(8) IbaInt2 { int x, y; };

// Host-side packing of windows [w0, w1) into one IbaPack.  Every offset stored in hw[w] is relative to THIS pack; iba_pack_windows packs
// chunks of windows on several host threads (packing was 2.5x the device time of a batch) and rebases them when it lays the chunks out
// in the upload blob.
struct IbaPack {
    std::vector<int> kf_xoff, free_kf, edge_kf, edge_point, pt_start, kf_edges, in1, in2, in_color, kf_task_start, pair_task_start;
    std::vector<IbaInt2> pair_ent;
    std::vector<IbaInt4> kf_task, pair_task;
    std::vector<uint8_t> kf_imu, edge_stereo, edge_close, in_robust;
    std::vector<double> edge_obs, edge_is2, in_pre, in_info, in_info_g, in_info_a, kfs, pts;
    size_t sumKF = 0, sumL = 0, sumE = 0, sumM = 0, sumX = 0, sumH = 0;
    int max_n = 0, rc = ORBHIP_OK;
    const char *err = nullptr;
    char err_buf[160];
    std::vector<int> tmp_pstart, tmp_kcount, tmp_kpos, tmp_pcount, tmp_ppos;
    std::vector<std::pair<int, int>> tmp_fe;
};
static inline int iba_pack_range(const orbhip_iba_window *wins, int w0, int w1, const double *const *kf_state_inout, const double *const *points_inout, IbaWin *hw, IbaPack &P, int mode = IBA_LOCAL)
{
    auto &kf_xoff = P.kf_xoff; auto &free_kf = P.free_kf; auto &edge_kf = P.edge_kf; auto &edge_point = P.edge_point; auto &pt_start = P.pt_start;
    auto &kf_edges = P.kf_edges; auto &in1 = P.in1; auto &in2 = P.in2; auto &in_color = P.in_color; auto &kf_task_start = P.kf_task_start;
    auto &pair_task_start = P.pair_task_start; auto &pair_ent = P.pair_ent; auto &kf_task = P.kf_task; auto &pair_task = P.pair_task;
    auto &kf_imu = P.kf_imu; auto &edge_stereo = P.edge_stereo; auto &edge_close = P.edge_close; auto &in_robust = P.in_robust;
    auto &edge_obs = P.edge_obs; auto &edge_is2 = P.edge_is2; auto &in_pre = P.in_pre; auto &in_info = P.in_info; auto &in_info_g = P.in_info_g;
    auto &in_info_a = P.in_info_a; auto &kfs = P.kfs; auto &pts = P.pts;
    auto &tmp_pstart = P.tmp_pstart; auto &tmp_kcount = P.tmp_kcount; auto &tmp_kpos = P.tmp_kpos; auto &tmp_pcount = P.tmp_pcount; auto &tmp_ppos = P.tmp_ppos;
    auto &tmp_fe = P.tmp_fe;
    size_t &sumKF = P.sumKF, &sumL = P.sumL, &sumE = P.sumE, &sumM = P.sumM, &sumX = P.sumX, &sumH = P.sumH;
    int &max_n = P.max_n;
    {
        size_t te = 0, tl = 0, tk = 0;
        for (int w = w0; w < w1; w++) { te += (size_t)std::max(wins[w].n_edges, 0); tl += (size_t)std::max(wins[w].n_points, 0); tk += (size_t)std::max(wins[w].n_kf, 0); }
        edge_kf.reserve(te); edge_point.reserve(te); edge_obs.reserve(3 * te); edge_is2.reserve(te); edge_stereo.reserve(te); edge_close.reserve(te);
        kf_edges.reserve(te); pair_ent.reserve(3 * te); pt_start.reserve(tl + (size_t)(w1 - w0)); pts.reserve(3 * tl); kfs.reserve(IBA_KF * tk);
    }
    for (int w = w0; w < w1; w++) {
        const orbhip_iba_window &g = wins[w];
        if (g.n_kf <= 0 || g.n_points < 0 || g.n_edges < 0 || g.n_inertial < 0 || !g.kf_fixed || !g.kf_imu || !kf_state_inout[w] ||
            (g.n_points && !points_inout[w]) ||
            (g.n_edges && (!g.edge_kf || !g.edge_point || !g.edge_obs || !g.edge_stereo || !g.edge_inv_sigma2)) ||
            (g.n_inertial && (!g.in_kf1 || !g.in_kf2 || !g.in_preint || !g.in_info || !g.in_info_g || !g.in_info_a || !g.in_robust)))
            return ORBHIP_E_BADARG;
        IbaWin &W = hw[w];
        memset(&W, 0, sizeof(W));
        W.n_kf = g.n_kf; W.L = g.n_points; W.E = g.n_edges; W.M = g.n_inertial;
        W.kf_off = (int)sumKF; W.pt_off = (int)sumL; W.e_off = (int)sumE; W.m_off = (int)sumM; W.x_off = (int)sumX; W.h_off = (long long)sumH;
        W.free_off = (int)free_kf.size(); W.ptstart_off = (int)pt_start.size();
        W.kfe_off = (int)kf_edges.size(); W.pent_off = (long long)pair_ent.size();
        W.ktask_off = (int)kf_task.size(); W.ktstart_off = (int)kf_task_start.size();
        W.ptask_off = (int)pair_task.size(); W.ptstart2_off = (int)pair_task_start.size();
        memcpy(W.Rcb, g.Rcb, sizeof(W.Rcb)); memcpy(W.tcb, g.tcb, sizeof(W.tcb));
        W.fx = g.fx; W.fy = g.fy; W.cx = g.cx; W.cy = g.cy; W.bf = g.bf;
        W.cam_model = g.camera_model == 1 ? 1 : 0; memcpy(W.kb, g.kb, sizeof(W.kb));
        W.has_cam2 = g.has_cam2 ? 1 : 0;
        if (W.has_cam2) {                                  // Rcb[1] = Rrl Rcb[0], tcb[1] = Rrl tcb[0] + trl (G2oTypes.cc:60-63)
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) W.Rcb2[3 * r + c] = g.Trl[4 * r] * g.Rcb[c] + g.Trl[4 * r + 1] * g.Rcb[3 + c] + g.Trl[4 * r + 2] * g.Rcb[6 + c];
                W.tcb2[r] = g.Trl[4 * r] * g.tcb[0] + g.Trl[4 * r + 1] * g.tcb[1] + g.Trl[4 * r + 2] * g.tcb[2] + g.Trl[4 * r + 3];
            }
            W.fx2 = g.fx2; W.fy2 = g.fy2; W.cx2 = g.cx2; W.cy2 = g.cy2; W.cam2_model = g.camera2_model == 1 ? 1 : 0; memcpy(W.kb2, g.kb2, sizeof(W.kb2));
        }
        std::vector<int> fidx(g.n_kf, -1);
        int n = 0;
        for (int k = 0; k < g.n_kf; k++) {
            kf_imu.push_back(g.kf_imu[k] ? 1 : 0);
            if (g.kf_fixed[k]) { kf_xoff.push_back(-1); continue; }
            kf_xoff.push_back(n); fidx[k] = W.nfree++; free_kf.push_back(k);
            n += g.kf_imu[k] ? (mode == IBA_FULL_SHARED ? 9 : 15) : 6;
        }
        if (mode == IBA_FULL_SHARED) n += 6;
        W.n = n;
        if (mode != IBA_LOCAL && (n > BA_LDLT_MAXN || g.n_inertial > IBA_THREADS)) {
            snprintf(P.err_buf, sizeof(P.err_buf), "full inertial BA: map %d has %d reduced unknowns (%d free keyframes, %d inertial edges); the limits are %d and %d",
                     w, n, W.nfree, g.n_inertial, BA_LDLT_MAXN, IBA_THREADS);
            P.err = P.err_buf;
            return ORBHIP_E_CAPACITY;
        }
        if (n > BA_LDLT_MAXN || g.n_inertial > IBA_THREADS) { P.err = "inertial BA: more than 480 keyframe unknowns (32 inertial keyframes)"; return ORBHIP_E_CAPACITY; }
        max_n = std::max(max_n, n);
        // edges: grouped by point (the reference creates them point by point, Optimizer.cc:4914-5034)
        std::vector<int> &pstart = tmp_pstart; pstart.assign(g.n_points + 1, 0);
        std::vector<int> &kcount = tmp_kcount; kcount.assign(W.nfree + 1, 0);
        const size_t e_base = edge_kf.size();
        edge_kf.resize(e_base + g.n_edges); edge_point.resize(e_base + g.n_edges); edge_obs.resize(3 * (e_base + g.n_edges));
        edge_is2.resize(e_base + g.n_edges); edge_stereo.resize(e_base + g.n_edges); edge_close.resize(e_base + g.n_edges);
        for (int e = 0; e < g.n_edges; e++) {
            const int k = g.edge_kf[e], l = g.edge_point[e];
            if (k < 0 || k >= g.n_kf || l < 0 || l >= g.n_points || (e && l < g.edge_point[e - 1])) return ORBHIP_E_BADARG;
            pstart[l + 1]++;
            if (fidx[k] >= 0) kcount[fidx[k] + 1]++;
            edge_kf[e_base + e] = k; edge_point[e_base + e] = l;
            if (g.edge_stereo[e] > 2 || (g.edge_stereo[e] == 2 && !g.has_cam2)) return ORBHIP_E_BADARG;
            edge_stereo[e_base + e] = g.edge_stereo[e];
            edge_close[e_base + e] = g.edge_close ? (g.edge_close[e] ? 1 : 0) : 0;
        }
        if (g.n_edges) {
            memcpy(edge_obs.data() + 3 * e_base, g.edge_obs, 24 * (size_t)g.n_edges);
            memcpy(edge_is2.data() + e_base, g.edge_inv_sigma2, 8 * (size_t)g.n_edges);
        }
        for (int l = 0; l < g.n_points; l++) pstart[l + 1] += pstart[l];
        pt_start.insert(pt_start.end(), pstart.begin(), pstart.end());
        // per-keyframe edge lists (counting sort, edge order kept), cut into chunks of <= IBA_KF_CHUNK edges (one wave pair each)
        for (int f = 0; f < W.nfree; f++) kcount[f + 1] += kcount[f];
        {
            const size_t kbase = kf_edges.size();
            kf_edges.resize(kbase + kcount[W.nfree]);
            std::vector<int> &kpos = tmp_kpos; kpos.assign(kcount.begin(), kcount.end() - 1);
            for (int e = 0; e < g.n_edges; e++) { const int f = fidx[g.edge_kf[e]]; if (f >= 0) kf_edges[kbase + kpos[f]++] = e; }
        }
        for (int f = 0; f < W.nfree; f++) {
            kf_task_start.push_back((int)kf_task.size() - W.ktask_off);
            for (int o = kcount[f]; o < kcount[f + 1]; o += IBA_KF_CHUNK)
                kf_task.push_back(IbaInt4{f, o, std::min<int>(o + IBA_KF_CHUNK, kcount[f + 1]), 0});
        }
        kf_task_start.push_back((int)kf_task.size() - W.ktask_off);
        W.nktask = (int)kf_task.size() - W.ktask_off;
        // pair lists: for every point, every (i <= j) pair of the free keyframes that see it (two counting passes, point order kept)
        W.npairs = W.nfree * (W.nfree + 1) / 2;
        auto pair_id = [&](int i, int j) { return i * W.nfree - i * (i - 1) / 2 + (j - i); };
        std::vector<int> &pcount = tmp_pcount; pcount.assign(W.npairs + 1, 0);
        std::vector<std::pair<int, int>> &fe = tmp_fe;
        for (int pass = 0; pass < 2; pass++) {
            const size_t pbase = pair_ent.size() - (pass ? (size_t)pcount[W.npairs] : 0);
            std::vector<int> &ppos = tmp_ppos;
            if (pass) ppos.assign(pcount.begin(), pcount.end() - 1);
            for (int l = 0; l < g.n_points; l++) {
                fe.clear();
                for (int e = pstart[l]; e < pstart[l + 1]; e++) if (fidx[g.edge_kf[e]] >= 0) fe.push_back({fidx[g.edge_kf[e]], e});
                for (size_t a2 = 0; a2 < fe.size(); a2++)
                    for (size_t b2 = a2; b2 < fe.size(); b2++) {
                        const bool sw = fe[a2].first > fe[b2].first;
                        const int i = sw ? fe[b2].first : fe[a2].first, j = sw ? fe[a2].first : fe[b2].first;
                        // a keyframe's left and right edges to one point (i == j, two edges) add W_a D^-1 W_b^T AND its transpose to the
                        // diagonal block (g2o keeps ONE Hpl block per (pose, point) pair: both edges accumulate into it)
                        const bool twin = b2 != a2 && i == j;
                        if (!pass) pcount[pair_id(i, j) + 1] += twin ? 2 : 1;
                        else {
                            pair_ent[pbase + ppos[pair_id(i, j)]++] = IbaInt2{sw ? fe[b2].second : fe[a2].second, sw ? fe[a2].second : fe[b2].second};
                            if (twin) pair_ent[pbase + ppos[pair_id(i, j)]++] = IbaInt2{fe[b2].second, fe[a2].second};
                        }
                    }
            }
            if (!pass) {
                for (int q = 0; q < W.npairs; q++) pcount[q + 1] += pcount[q];
                pair_ent.resize(pair_ent.size() + pcount[W.npairs]);
            }
        }
        for (int i = 0, q = 0; i < W.nfree; i++)
            for (int j = i; j < W.nfree; j++, q++) {
                pair_task_start.push_back((int)pair_task.size() - W.ptask_off);
                for (int o = pcount[q]; o < pcount[q + 1]; o += IBA_PAIR_CHUNK)
                    pair_task.push_back(IbaInt4{q, o, std::min<int>(o + IBA_PAIR_CHUNK, pcount[q + 1]), i == j ? 1 : 0});
            }
        pair_task_start.push_back((int)pair_task.size() - W.ptask_off);
        W.nptask = (int)pair_task.size() - W.ptask_off;
        // inertial edges + greedy colouring (edges of one colour share no keyframe)
        std::vector<std::vector<int>> used(g.n_kf);
        std::vector<int> col_count;
        for (int m = 0; m < g.n_inertial; m++) {
            const int k1 = g.in_kf1[m], k2 = g.in_kf2[m];
            if (k1 < 0 || k1 >= g.n_kf || k2 < 0 || k2 >= g.n_kf || k1 == k2 || !g.kf_imu[k1] || !g.kf_imu[k2]) return ORBHIP_E_BADARG;
            int c = 0;
            auto taken = [&](int col) { for (int u : used[k1]) if (u == col) return true; for (int u : used[k2]) if (u == col) return true; return false; };
            while (taken(c)) c++;
            used[k1].push_back(c); used[k2].push_back(c);
            W.ncolors = std::max(W.ncolors, c + 1);
            if ((int)col_count.size() <= c) col_count.resize(c + 1, 0);
            if (c > 255) return ORBHIP_E_CAPACITY;               // (a keyframe with more than 255 inertial edges)
            // colour | rank inside the colour << 8: workgroup 0 deals the edges of a colour to its waves by rank
            in1.push_back(k1); in2.push_back(k2); in_color.push_back(c | (col_count[c]++ << 8)); in_robust.push_back(g.in_robust[m] ? 1 : 0);
        }
        if (g.n_inertial) {
            in_pre.insert(in_pre.end(), g.in_preint, g.in_preint + (size_t)IBA_PRE * g.n_inertial);
            in_info.insert(in_info.end(), g.in_info, g.in_info + 81 * (size_t)g.n_inertial);
            in_info_g.insert(in_info_g.end(), g.in_info_g, g.in_info_g + 9 * (size_t)g.n_inertial);
            in_info_a.insert(in_info_a.end(), g.in_info_a, g.in_info_a + 9 * (size_t)g.n_inertial);
        }
        kfs.insert(kfs.end(), kf_state_inout[w], kf_state_inout[w] + (size_t)IBA_KF * g.n_kf);
        if (g.n_points) pts.insert(pts.end(), points_inout[w], points_inout[w] + 3 * (size_t)g.n_points);
        sumKF += g.n_kf; sumL += g.n_points; sumE += g.n_edges; sumM += g.n_inertial; sumX += n; sumH += (size_t)n * n;
    }
    return ORBHIP_OK;
}

// ------------------------------------------------------------------ a batch of windows, packed
// The constant device data of a batch as the host uploads it: every array is the concatenation of the chunks' pieces at a 256-byte
// aligned offset of `blob`; IbaBlobOffsets names the offsets in the order they are laid out.
struct IbaBlobOffsets {
    size_t win, kf_xoff, kf_imu, free_kf, edge_kf, edge_point, edge_obs, edge_is2, edge_stereo, edge_close, pt_start, kf_edges, pair_ent, kf_task,
           kf_task_start, pair_task, pair_task_start, in_kf1, in_kf2, in_color, in_robust, in_pre, in_info, in_info_g, in_info_a;
};
struct IbaPacked {
    std::vector<IbaWin> hw;                          // [n_windows], offsets batch-global
    std::vector<uint8_t> blob;
    IbaBlobOffsets o;
    std::vector<double> kfs, pts;                    // initial states, concatenated
    size_t sumKF = 0, sumL = 0, sumE = 0, sumM = 0, sumX = 0, sumH = 0, n_kftask = 0, n_pairtask = 0;
    int max_n = 0;
    std::string err;                                 // the refusal's message, empty where the code says it all
};
// Packs chunks of windows on n_threads host threads (windows are independent), rebases every window's offsets by what the chunks in
// front of it hold, and copies the chunks' pieces into the blob on the same threads.  The result does not depend on n_threads.
static inline int iba_pack_windows(const orbhip_iba_window *wins, int n_windows, const double *const *kf_states, const double *const *points, int mode, int n_threads, IbaPacked &R)
{
    const int nthr = std::max(1, n_threads);
    std::vector<IbaWin> &hw = R.hw;
    hw.assign(n_windows, IbaWin());
    std::vector<IbaPack> packs(nthr);
    auto chunk_lo = [&](int c) { return (int)((long long)n_windows * c / nthr); };
    {
        std::vector<std::thread> th;
        for (int c = 1; c < nthr; c++)
            th.emplace_back([&, c] { packs[c].rc = iba_pack_range(wins, chunk_lo(c), chunk_lo(c + 1), kf_states, points, hw.data(), packs[c], mode); });
        packs[0].rc = iba_pack_range(wins, chunk_lo(0), chunk_lo(1), kf_states, points, hw.data(), packs[0], mode);
        for (auto &t : th) t.join();
    }
    for (int c = 0; c < nthr; c++)
        if (packs[c].rc != ORBHIP_OK) { if (packs[c].err) R.err = packs[c].err; return packs[c].rc; }
    // rebase every window's offsets by what the chunks in front of it hold
    struct Base { size_t kf, l, e, m, x, h, fr, pst, kfe, pent, ktask, ktstart, ptask, ptstart2; };
    std::vector<Base> base(nthr);
    {
        Base b = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = 0; c < nthr; c++) {
            const IbaPack &P = packs[c];
            base[c] = b;
            for (int w = chunk_lo(c); w < chunk_lo(c + 1); w++) {
                IbaWin &W = hw[w];
                W.kf_off += (int)b.kf; W.pt_off += (int)b.l; W.e_off += (int)b.e; W.m_off += (int)b.m; W.x_off += (int)b.x; W.h_off += (long long)b.h;
                W.free_off += (int)b.fr; W.ptstart_off += (int)b.pst; W.kfe_off += (int)b.kfe; W.pent_off += (long long)b.pent;
                W.ktask_off += (int)b.ktask; W.ktstart_off += (int)b.ktstart; W.ptask_off += (int)b.ptask; W.ptstart2_off += (int)b.ptstart2;
            }
            b.kf += P.sumKF; b.l += P.sumL; b.e += P.sumE; b.m += P.sumM; b.x += P.sumX; b.h += P.sumH; b.fr += P.free_kf.size(); b.pst += P.pt_start.size();
            b.kfe += P.kf_edges.size(); b.pent += P.pair_ent.size(); b.ktask += P.kf_task.size(); b.ktstart += P.kf_task_start.size();
            b.ptask += P.pair_task.size(); b.ptstart2 += P.pair_task_start.size();
            R.max_n = std::max(R.max_n, P.max_n);
        }
        R.sumKF = b.kf; R.sumL = b.l; R.sumE = b.e; R.sumM = b.m; R.sumX = b.x; R.sumH = b.h; R.n_kftask = b.ktask; R.n_pairtask = b.ptask;
    }
    // the upload blob: every array is the concatenation of the chunks' pieces; the pieces are copied in place by the same threads
    std::vector<uint8_t> &bytes = R.blob;
    bytes.clear();
    auto alloc = [&](size_t nbytes) {
        const size_t off = (bytes.size() + 255) & ~(size_t)255;
        bytes.resize(off + std::max<size_t>(nbytes, 1));
        return off;
    };
    std::vector<std::function<void(int)>> copies;
    auto lay = [&](auto member, size_t elem_bytes) {
        size_t total = 0;
        std::vector<size_t> offs(nthr);
        for (int c = 0; c < nthr; c++) { offs[c] = total; total += (packs[c].*member).size(); }
        const size_t o = alloc(elem_bytes * std::max<size_t>(total, 1));
        copies.push_back([&, member, offs, o, elem_bytes](int c) {
            const auto &v = packs[c].*member;
            if (!v.empty()) memcpy(bytes.data() + o + elem_bytes * offs[c], v.data(), elem_bytes * v.size());
        });
        return o;
    };
    IbaBlobOffsets &O = R.o;
    O.win = alloc(sizeof(IbaWin) * (size_t)n_windows);
    O.kf_xoff = lay(&IbaPack::kf_xoff, 4); O.kf_imu = lay(&IbaPack::kf_imu, 1); O.free_kf = lay(&IbaPack::free_kf, 4); O.edge_kf = lay(&IbaPack::edge_kf, 4);
    O.edge_point = lay(&IbaPack::edge_point, 4); O.edge_obs = lay(&IbaPack::edge_obs, 8); O.edge_is2 = lay(&IbaPack::edge_is2, 8);
    O.edge_stereo = lay(&IbaPack::edge_stereo, 1); O.edge_close = lay(&IbaPack::edge_close, 1); O.pt_start = lay(&IbaPack::pt_start, 4);
    O.kf_edges = lay(&IbaPack::kf_edges, 4); O.pair_ent = lay(&IbaPack::pair_ent, 8); O.kf_task = lay(&IbaPack::kf_task, 16);
    O.kf_task_start = lay(&IbaPack::kf_task_start, 4); O.pair_task = lay(&IbaPack::pair_task, 16); O.pair_task_start = lay(&IbaPack::pair_task_start, 4);
    O.in_kf1 = lay(&IbaPack::in1, 4); O.in_kf2 = lay(&IbaPack::in2, 4); O.in_color = lay(&IbaPack::in_color, 4); O.in_robust = lay(&IbaPack::in_robust, 1);
    O.in_pre = lay(&IbaPack::in_pre, 8); O.in_info = lay(&IbaPack::in_info, 8); O.in_info_g = lay(&IbaPack::in_info_g, 8); O.in_info_a = lay(&IbaPack::in_info_a, 8);
    R.kfs.assign((size_t)IBA_KF * R.sumKF, 0.0); R.pts.assign(3 * R.sumL, 0.0);
    {
        auto copy_chunk = [&](int c) {
            for (auto &f : copies) f(c);
            if (!packs[c].kfs.empty()) memcpy(R.kfs.data() + (size_t)IBA_KF * base[c].kf, packs[c].kfs.data(), 8 * packs[c].kfs.size());
            if (!packs[c].pts.empty()) memcpy(R.pts.data() + 3 * base[c].l, packs[c].pts.data(), 8 * packs[c].pts.size());
        };
        std::vector<std::thread> th;
        for (int c = 1; c < nthr; c++) th.emplace_back([&, c] { copy_chunk(c); });
        if (n_windows) memcpy(bytes.data() + O.win, hw.data(), sizeof(IbaWin) * (size_t)n_windows);
        copy_chunk(0);
        for (auto &t : th) t.join();
    }
    return ORBHIP_OK;
}

// ------------------------------------------------------------------ FullInertialBA's filter
// A map as the kernel takes it: g2o's activity rule applied on the host.  The visual edges of a point that only fixed keyframes see
// are dropped (bAllFixed: the point is no vertex), without shared biases so are inertial edges between two fixed keyframes (no free
// vertex: not active); every inertial edge is robust.  Indices of keyframes and points are kept.
struct FibaMap {
    std::vector<int32_t> edge_kf, edge_point, in_kf1, in_kf2;
    std::vector<double> edge_obs, edge_is2, in_pre, in_info, in_info_g, in_info_a;
    std::vector<uint8_t> edge_stereo, in_robust;
};
static inline int fiba_filter(const orbhip_iba_window &g, bool shared, FibaMap &F, orbhip_iba_window &out)
{
    out = g;
    if (g.n_kf <= 0 || g.n_points < 0 || g.n_edges < 0 || g.n_inertial < 0 || !g.kf_fixed || !g.kf_imu ||
        (g.n_edges && (!g.edge_kf || !g.edge_point || !g.edge_obs || !g.edge_stereo || !g.edge_inv_sigma2)) ||
        (g.n_inertial && (!g.in_kf1 || !g.in_kf2 || !g.in_preint || !g.in_info || (!shared && (!g.in_info_g || !g.in_info_a)))))
        return ORBHIP_E_BADARG;
    std::vector<uint8_t> free_seen(std::max(g.n_points, 1), 0);
    for (int e = 0; e < g.n_edges; e++) {
        const int k = g.edge_kf[e], l = g.edge_point[e];
        if (k < 0 || k >= g.n_kf || l < 0 || l >= g.n_points) return ORBHIP_E_BADARG;
        if (!g.kf_fixed[k]) free_seen[l] = 1;
    }
    for (int e = 0; e < g.n_edges; e++) {
        if (!free_seen[g.edge_point[e]]) continue;
        F.edge_kf.push_back(g.edge_kf[e]); F.edge_point.push_back(g.edge_point[e]); F.edge_stereo.push_back(g.edge_stereo[e]);
        F.edge_is2.push_back(g.edge_inv_sigma2[e]);
        F.edge_obs.insert(F.edge_obs.end(), g.edge_obs + 3 * (size_t)e, g.edge_obs + 3 * (size_t)e + 3);
    }
    for (int m = 0; m < g.n_inertial; m++) {
        const int k1 = g.in_kf1[m], k2 = g.in_kf2[m];
        if (k1 < 0 || k1 >= g.n_kf || k2 < 0 || k2 >= g.n_kf) return ORBHIP_E_BADARG;
        if (!shared && g.kf_fixed[k1] && g.kf_fixed[k2]) continue;
        F.in_kf1.push_back(k1); F.in_kf2.push_back(k2); F.in_robust.push_back(1);
        F.in_pre.insert(F.in_pre.end(), g.in_preint + (size_t)IBA_PRE * m, g.in_preint + (size_t)IBA_PRE * (m + 1));
        F.in_info.insert(F.in_info.end(), g.in_info + 81 * (size_t)m, g.in_info + 81 * (size_t)(m + 1));
        for (int i = 0; i < 9; i++) {
            F.in_info_g.push_back(shared ? 0.0 : g.in_info_g[9 * (size_t)m + i]);
            F.in_info_a.push_back(shared ? 0.0 : g.in_info_a[9 * (size_t)m + i]);
        }
    }
    out.n_edges = (int)F.edge_kf.size(); out.edge_kf = F.edge_kf.data(); out.edge_point = F.edge_point.data(); out.edge_obs = F.edge_obs.data();
    out.edge_stereo = F.edge_stereo.data(); out.edge_inv_sigma2 = F.edge_is2.data(); out.edge_close = nullptr;
    out.n_inertial = (int)F.in_kf1.size(); out.in_kf1 = F.in_kf1.data(); out.in_kf2 = F.in_kf2.data(); out.in_preint = F.in_pre.data();
    out.in_info = F.in_info.data(); out.in_info_g = F.in_info_g.data(); out.in_info_a = F.in_info_a.data(); out.in_robust = F.in_robust.data();
    return ORBHIP_OK;
}
