// ba_graph_lists.h -- the host's lists of a batch of bundle-adjustment graphs (ba_kernels.hip, the host side): free-pose numbering, point-major and
// pose-major edge lists, twin-edge chains, the Schur GEMM's tasks and stages, tile masks, pair-list sizes and exchange offsets, and the
// slice of every graph a rank of a landmark-sharded batch owns.  The kernels sum in exactly these orders, so the lists are part of the
// result's bits.  Nothing from HIP is included: a host compiler builds this header alone (tests/test_ba_graph_lists.py does, under the
// address and undefined-behaviour sanitizers); ba_create_impl allocates, uploads and launches.
#pragma once
#include "../../include/orbhip.h"
#include "ba_ldlt_limits.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// ------------------------------------------------------------------ constants the lists depend on
#define BA_BIG_MAXN 4096       // unknowns of the largest window (global-memory Schur complement + blocked LDL^T beyond BA_LDLT_MAXN)
// Schur GEMM (k_ba_schur_gemm): stages of <= GEMM_PS points and <= GEMM_STAGE_EDGES Hpl blocks; every row strip of the upper tile
// triangle is cut into chunks of GEMM_C tiles, GEMM_NCH chunks per wave, GEMM_WAVES waves per workgroup
#define GEMM_PS 8
#define GEMM_C 3               // tiles per chunk
#define GEMM_NCH 8             // chunks per wave
#define GEMM_WAVES 8
#define GEMM_LDS_PAD 16        // = 32 dwords mod 64
#define GEMM_STAGE_EDGES 85    // 6 column tasks per Hpl block, one task per thread
#ifndef GEMM_TARGET_WGS
#define GEMM_TARGET_WGS 256     // one resident workgroup per CU (VGPR-bound); more splits only add Spart traffic (512: -2 %)
#endif
#define GEMM_PANEL_LDS_BYTES (126 * 1024)   // of the CU's 160 KB: the rest holds the raw blocks, task descriptors, C^-1 rows, masks
#if defined(__HIPCC__)
static inline __host__ __device__ int gemm_strip_chunks(int nt, int tr) { return (nt - tr + GEMM_C - 1) / GEMM_C; }
#else
static inline int gemm_strip_chunks(int nt, int tr) { return (nt - tr + GEMM_C - 1) / GEMM_C; }
#endif

// ------------------------------------------------------------------ device structures the host fills
// One calibration (round 4: the reference gives every edge its keyframe's own, Optimizer.cc:1961, :1990-1994, :2021-2023).  The edge
// functions of ba_edges.h are templates over the calibration object: a BaCamDev, or a BaGraphDev (one calibration per graph), which
// carries the same fields under the same names.
struct BaCamDev {
    double fx, fy, cx, cy, bf;
    int cam_model;
    double kb[4];
    double Trl[7], fx2, fy2, cx2, cy2, kb2[4];
    int cam2_model;
};

struct BaGraphDev {
    int n_poses, n_points, n_edges, nf, n, ld;      // n = 6*nf, ld = n rounded up to 96
    int pose_off, point_off, edge_off, free_off;     // offsets into the concatenated arrays
    int ptstart_off, posestart_off;                  // into pt_start / pose_start (+g extra entries)
    size_t s_off, spart_off, xl_off;                 // element offsets
    int gemm_off, stage_off, n_stages;               // Schur GEMM work lists: first entry of gemm_task / gemm_stage, number of stages
    int gemm_ps;                                     // points per stage (<= GEMM_PS; fewer when ld is large: the LDS panel is [2][gemm_ps][3][ld+16])
    int ks;                                          // split-K factor of the Schur GEMM (ranges of stages)
    int nt16;                                        // 16-column tiles per side (ld / 16)
    int ngrp;                                        // chunk groups (each workgroup keeps <= GEMM_WAVES*GEMM_NCH chunks of GEMM_C tiles in registers)
    double fx, fy, cx, cy, bf;
    int cam_model;                                   // 0 Pinhole, 1 KannalaBrandt8 (monocular edges)
    double kb[4];
    double Trl[7], fx2, fy2, cx2, cy2, kb2[4];       // second camera of a rigid pair (edge type 2, EdgeSE3ProjectXYZToBody)
    int cam2_model;
    // windows with more than 80 free keyframes (n > BA_LDLT_MAXN): global-memory Schur complement and blocked LDL^T
    size_t pair_off, pent_off;                       // into big_pair_start (nf (nf + 1) / 2 + 1 entries) / big_pair_ent
    int cam_off;                                     // >= 0: per-keyframe calibration -- pose i of this graph uses cams[cam_off + pose_cam[pose_off + i]] (round 4)
};

// HIP's int4 / int2 as the host sees them (ba_kernels.hip asserts size and alignment)
struct alignas(16) BaInt4 { int x, y, z, w; };
struct alignas(8) BaInt2 { int x, y; };

// ------------------------------------------------------------------ the lists of a batch
// Every array ba_create_impl uploads, the normalised initial estimates and the sizes its allocations need.  ba_create_impl keeps one
// per thread: the vectors keep their capacity from call to call -- LocalMapping solves one window per keyframe from the same thread,
// and fresh multi-megabyte vectors cost more in page faults than in arithmetic.
struct BaGraphLists {
    std::vector<BaGraphDev> gd;
    std::vector<BaCamDev> cams;                      // [sum of n_cameras]
    std::vector<int> posecam;                        // [sumP] index into the graph's cameras (0 without a table)
    std::vector<int> x1off, x2off;                   // [G] payload offsets of exchanges 1 and 2 of a sharded solve
    std::vector<int> hidx;                           // [sumP] free index or -1
    std::vector<int> epose, epoint, enext, etask;    // [sumE] as given; next edge of a (point, pose) chain or -1; the edge's Hpl block (batch-global) or -1
    std::vector<uint8_t> est, edup;                  // [sumE] type; 1 = an earlier edge of the point has the same pose
    std::vector<double> eobs, eis2;                  // [sumE*3], [sumE]
    std::vector<int> ptstart, posestart;             // per graph n_points + 1 / nf + 1 entries
    std::vector<int> poseedges;                      // [sumE] graph-local edges grouped by free pose (entries past posestart[nf]: 0)
    std::vector<int> pmpoint, pmtask;                // the static edge data in that pose-major order (filler past posestart[nf]: edge 0's, task -1)
    std::vector<uint8_t> pmtype;
    std::vector<double> pmis2, pmobs;
    std::vector<uint32_t> ptmask;                    // [sumL] bit t: the point's Hpl column is non-zero inside columns [16t, 16t + 16)
    std::vector<BaInt4> gtask, gstage;               // {graph-local edge, 6*h, point, graph}; {first point, points, first task, tasks}
    std::vector<double> poses0, points0;             // initial estimates, quaternions normalised with w >= 0
    int sumP, sumL, sumE, sumF, max_edges, max_points, max_nf, max_ld;
    size_t s_total, spart_total;                     // doubles of S / Spart
    bool any_big, general, pair_lists;               // a window beyond BA_LDLT_MAXN; KannalaBrandt8, second-camera edges, twins or a camera table; Schur complement from pair lists
    size_t pair_total_start, pair_total_ent;         // entries of big_pair_start / big_pair_ent over the batch
    int max_npair, max_row_blocks;                   // most pairs of a graph; most Hpl blocks any free pose holds (LDS of k_ba_schur_rows)
    size_t x_need;                                   // doubles per rank slot of the exchange buffer
    double flops_per_launch, flops_issued, flops_dense;      // MFMA flops of one Schur GEMM launch: tiles that hold data, tiles issued, all tiles
    const char *err;                                 // the refusal's message, nullptr where the code says it all

    void clear()
    {
        gd.clear(); cams.clear(); posecam.clear(); x1off.clear(); x2off.clear(); hidx.clear(); epose.clear(); epoint.clear(); enext.clear(); etask.clear();
        est.clear(); edup.clear(); eobs.clear(); eis2.clear(); ptstart.clear(); posestart.clear(); poseedges.clear(); pmpoint.clear(); pmtask.clear();
        pmtype.clear(); pmis2.clear(); pmobs.clear(); ptmask.clear(); gtask.clear(); gstage.clear(); poses0.clear(); points0.clear();
        sumP = sumL = sumE = sumF = max_edges = max_points = max_nf = max_ld = max_npair = max_row_blocks = 0;
        s_total = spart_total = pair_total_start = pair_total_ent = x_need = 0;
        any_big = general = pair_lists = false;
        flops_per_launch = flops_issued = flops_dense = 0;
        err = nullptr;
    }
    int refuse(const char *msg) { err = msg; return ORBHIP_E_BADARG; }

    // pose_in_system[g] (optional): which poses take part in the reduced system even without an edge in THIS graph -- a sharded
    // batch sees only a slice of the edges but must number the free poses like every other rank.
    // mode: 2 = the Schur complement from the MFMA panel GEMM, else from the per-block-pair lists (k_ba_schur_big) -- measured faster at
    // every batch size; the GEMM also in the landmark-sharded mode, and never for big windows.
    int build(const orbhip_ba_graph *graphs, int n_graphs, const double *const *poses, const double *const *points,
              const std::vector<std::vector<uint8_t>> *pose_in_system, int world, int mode)
    {
        clear();
        size_t x1 = 0, x2 = 0, s = 0, sp = 0;
        std::vector<std::vector<int>> g_local_h;                 // hessian index of every pose, per graph (pair-list sizes)
        const bool want_gemm_stats = !(world == 1 && mode != 2);    // the MFMA flop counts of the GEMM form (bench / profiling): not needed by the pair-list form
        {   // every per-edge / per-point / per-pose array is sized once (round 4: ~25 push_back per edge were 1 ms of a one-shot solve)
            size_t te = 0, tl = 0, tp = 0;
            for (int g = 0; g < n_graphs; g++) { te += (size_t)std::max(graphs[g].n_edges, 0); tl += (size_t)std::max(graphs[g].n_points, 0); tp += (size_t)std::max(graphs[g].n_poses, 0); }
            hidx.reserve(tp); epose.reserve(te); epoint.reserve(te); eobs.reserve(3 * te); eis2.reserve(te); est.reserve(te); edup.reserve(te); enext.reserve(te);
            ptstart.reserve(tl + n_graphs); posestart.reserve(tp + n_graphs); poseedges.reserve(te); ptmask.reserve(tl); gtask.reserve(te); gstage.reserve(tl / 4 + 16);
            etask.reserve(te); pmpoint.reserve(te); pmtask.reserve(te); pmtype.reserve(te); pmis2.reserve(te); pmobs.reserve(3 * te);
            poses0.reserve(7 * tp); points0.reserve(3 * tl);
        }
        for (int g = 0; g < n_graphs; g++) {
            const orbhip_ba_graph &H = graphs[g];
            if (H.n_poses <= 0 || H.n_points <= 0 || H.n_edges < 0) return ORBHIP_E_BADARG;
            BaGraphDev D;
            memset(&D, 0, sizeof(D));
            D.n_poses = H.n_poses; D.n_points = H.n_points; D.n_edges = H.n_edges;
            D.pose_off = sumP; D.point_off = sumL; D.edge_off = sumE; D.free_off = sumF;
            D.fx = H.fx; D.fy = H.fy; D.cx = H.cx; D.cy = H.cy; D.bf = H.bf;
            D.cam_model = H.camera_model; for (int k = 0; k < 4; k++) D.kb[k] = H.kb[k];
            for (int k = 0; k < 7; k++) D.Trl[k] = H.Trl[k];
            D.fx2 = H.fx2; D.fy2 = H.fy2; D.cx2 = H.cx2; D.cy2 = H.cy2; D.cam2_model = H.camera2_model; for (int k = 0; k < 4; k++) D.kb2[k] = H.kb2[k];
            D.cam_off = -1;
            if (H.n_cameras > 0) {                                   // per-keyframe calibration (Optimizer.cc:1961, :1990-1994, :2021-2023)
                if (!H.cameras || !H.pose_camera) return refuse("n_cameras > 0 needs cameras and pose_camera");
                D.cam_off = (int)cams.size();
                for (int c = 0; c < H.n_cameras; c++) {
                    const orbhip_ba_camera &Cc = H.cameras[c];
                    BaCamDev K;
                    memset(&K, 0, sizeof(K));                        // (padding: the table is uploaded byte for byte)
                    K.fx = Cc.fx; K.fy = Cc.fy; K.cx = Cc.cx; K.cy = Cc.cy; K.bf = Cc.bf; K.cam_model = Cc.camera_model;
                    for (int k = 0; k < 4; k++) { K.kb[k] = Cc.kb[k]; K.kb2[k] = Cc.kb2[k]; }
                    for (int k = 0; k < 7; k++) K.Trl[k] = Cc.Trl[k];
                    K.fx2 = Cc.fx2; K.fy2 = Cc.fy2; K.cx2 = Cc.cx2; K.cy2 = Cc.cy2; K.cam2_model = Cc.camera2_model;
                    cams.push_back(K);
                }
                for (int i = 0; i < H.n_poses; i++) {
                    if (H.pose_camera[i] < 0 || H.pose_camera[i] >= H.n_cameras) return refuse("pose_camera out of range");
                    posecam.push_back(H.pose_camera[i]);
                }
                general = true;                                      // the camera table is read by the general instantiations only
            } else posecam.insert(posecam.end(), (size_t)H.n_poses, 0);
            std::vector<int> has(H.n_poses, 0), local_h(H.n_poses, -1);
            for (int e = 0; e < H.n_edges; e++) {
                if (H.edge_pose[e] < 0 || H.edge_pose[e] >= H.n_poses || H.edge_point[e] < 0 || H.edge_point[e] >= H.n_points ||
                    (e > 0 && H.edge_point[e] < H.edge_point[e - 1])) return refuse("edges must be point-major with valid ids");
                has[H.edge_pose[e]] = 1;
            }
            if (pose_in_system) for (int i = 0; i < H.n_poses; i++) has[i] = (*pose_in_system)[g][i];
            int nf = 0;
            for (int i = 0; i < H.n_poses; i++) { local_h[i] = (!H.pose_fixed[i] && has[i]) ? nf++ : -1; hidx.push_back(local_h[i]); }
            D.nf = nf; D.n = 6 * nf; D.ld = std::max(96, (D.n + 95) / 96 * 96);   // multiple of 16 (MFMA tiles) and of 32 (1-KiB LDS-DMA pieces)
            if (D.n > BA_BIG_MAXN) return refuse("more than 682 free keyframes in one window");
            const bool big_graph = D.n > BA_LDLT_MAXN;               // > 80 free keyframes: global-memory Schur complement + blocked LDL^T
            if (big_graph && world > 1) return refuse("landmark-sharded solve: at most 80 free keyframes per window");
            any_big = any_big || big_graph;
            D.ptstart_off = (int)ptstart.size();
            std::vector<int> cnt(H.n_points + 1, 0);
            for (int e = 0; e < H.n_edges; e++) cnt[H.edge_point[e] + 1]++;
            for (int l = 0; l < H.n_points; l++) cnt[l + 1] += cnt[l];
            ptstart.insert(ptstart.end(), cnt.begin(), cnt.end());
            D.posestart_off = (int)posestart.size();
            std::vector<int> pc(nf + 1, 0);
            for (int e = 0; e < H.n_edges; e++) if (local_h[H.edge_pose[e]] >= 0) pc[local_h[H.edge_pose[e]] + 1]++;
            for (int h = 0; h < nf; h++) pc[h + 1] += pc[h];
            std::vector<int> fill(pc.begin(), pc.end() - 1), pel(H.n_edges, 0);
            for (int e = 0; e < H.n_edges; e++) { const int h = local_h[H.edge_pose[e]]; if (h >= 0) pel[fill[h]++] = e; }
            posestart.insert(posestart.end(), pc.begin(), pc.end());
            poseedges.insert(poseedges.end(), pel.begin(), pel.end());
            {                                                         // pose-major copy of the static edge data (entries past pc[nf] unused)
                const size_t o = pmpoint.size(), ne = (size_t)H.n_edges;
                pmpoint.resize(o + ne); pmtype.resize(o + ne); pmis2.resize(o + ne); pmobs.resize(3 * (o + ne));
                for (size_t k = 0; k < ne; k++) {
                    const int e = (int)k < pc[nf] ? pel[k] : 0;
                    pmpoint[o + k] = H.edge_point[e]; pmtype[o + k] = H.edge_stereo ? H.edge_stereo[e] : 0; pmis2[o + k] = H.edge_inv_sigma2[e];
                    pmobs[3 * (o + k)] = H.edge_obs[3 * e]; pmobs[3 * (o + k) + 1] = H.edge_obs[3 * e + 1]; pmobs[3 * (o + k) + 2] = H.edge_obs[3 * e + 2];
                }
            }
            {   // edge types: 0 mono, 1 stereo, 2 second camera (needs a rigid transform mTrl with a non-zero quaternion)
                bool any2 = false;
                for (int e = 0; e < H.n_edges && H.edge_stereo; e++) {
                    if (H.edge_stereo[e] > 2) return refuse("edge_stereo must be 0, 1 or 2");
                    any2 = any2 || H.edge_stereo[e] == 2;
                }
                const double qn = H.Trl[0] * H.Trl[0] + H.Trl[1] * H.Trl[1] + H.Trl[2] * H.Trl[2] + H.Trl[3] * H.Trl[3];
                if (any2 && H.n_cameras <= 0 && !(qn > 0.0)) return refuse("edges of type 2 need Trl (mTrl) and the second camera");
                for (int e = 0; e < H.n_edges && any2 && H.n_cameras > 0 && H.cameras && H.pose_camera; e++) {
                    if (H.edge_stereo[e] != 2) continue;
                    const int ci = H.pose_camera[H.edge_pose[e]];
                    if (ci < 0 || ci >= H.n_cameras) continue;       // (reported above)
                    const double *t = H.cameras[ci].Trl;
                    if (!(t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3] > 0.0)) return refuse("edges of type 2 need their keyframe's Trl (mTrl) and second camera");
                }
            }
            {   // chains of edges that share (point, pose): edges are point-major, so only a point's own edges are compared
                std::vector<int> nxt(H.n_edges, -1); std::vector<uint8_t> dup(H.n_edges, 0);
                for (int e0 = 0; e0 < H.n_edges;) {
                    int e1 = e0;
                    while (e1 < H.n_edges && H.edge_point[e1] == H.edge_point[e0]) e1++;
                    for (int a = e0; a < e1; a++)
                        for (int c = a + 1; c < e1; c++)
                            if (H.edge_pose[c] == H.edge_pose[a]) { if (nxt[a] < 0) nxt[a] = c; dup[c] = 1; break; }
                    e0 = e1;
                }
                edup.insert(edup.end(), dup.begin(), dup.end()); enext.insert(enext.end(), nxt.begin(), nxt.end());
                for (int e = 0; e < H.n_edges; e++) if (dup[e] || (H.edge_stereo && H.edge_stereo[e] == 2)) general = true;
                if (H.camera_model != 0) general = true;
            }
            epose.insert(epose.end(), H.edge_pose, H.edge_pose + H.n_edges); epoint.insert(epoint.end(), H.edge_point, H.edge_point + H.n_edges);
            eobs.insert(eobs.end(), H.edge_obs, H.edge_obs + 3 * (size_t)H.n_edges); eis2.insert(eis2.end(), H.edge_inv_sigma2, H.edge_inv_sigma2 + H.n_edges);
            if (H.edge_stereo) est.insert(est.end(), H.edge_stereo, H.edge_stereo + H.n_edges); else est.insert(est.end(), (size_t)H.n_edges, (uint8_t)0);
            const int nt = D.ld / 16, ntiles = nt * (nt + 1) / 2;
            int nchunks = 0;
            for (int tr = 0; tr < nt; tr++) nchunks += gemm_strip_chunks(nt, tr);
            D.nt16 = nt; D.ngrp = (nchunks + GEMM_WAVES * GEMM_NCH - 1) / (GEMM_WAVES * GEMM_NCH);
            {   // Schur GEMM work lists: Hpl blocks (free pose, first edge of a twin chain) point-major, cut into stages
                D.gemm_off = (int)gtask.size(); D.stage_off = (int)gstage.size();
                D.gemm_ps = (int)std::min<size_t>(GEMM_PS, GEMM_PANEL_LDS_BYTES / (sizeof(double) * 2 * 3 * (size_t)(D.ld + GEMM_LDS_PAD)));
                if (D.gemm_ps < 1) return refuse("too many free keyframes for the LDS panel of the Schur GEMM");
                const uint8_t *dupv = edup.data() + (edup.size() - H.n_edges);
                int e = 0, pt0 = 0, npts = 0, t0 = (int)gtask.size() - D.gemm_off, ntask = 0;
                for (int l = 0; l < H.n_points; l++) {
                    int e1 = e, nblk = 0;
                    while (e1 < H.n_edges && H.edge_point[e1] == l) { if (local_h[H.edge_pose[e1]] >= 0 && !dupv[e1]) nblk++; e1++; }
                    if (nblk > GEMM_STAGE_EDGES && !big_graph) return refuse("a point has more Hpl blocks than free keyframes fit (ld <= 512)");
                    if (npts == D.gemm_ps || ntask + nblk > GEMM_STAGE_EDGES) {       // (big windows: the stage lists are built but not used)
                        gstage.push_back(BaInt4{pt0, npts, t0, ntask});
                        pt0 = l; npts = 0; t0 += ntask; ntask = 0;
                    }
                    for (int k = e; k < e1; k++) {
                        const bool blk = local_h[H.edge_pose[k]] >= 0 && !dupv[k];
                        etask.push_back(blk ? (int)gtask.size() : -1);
                        if (blk) gtask.push_back(BaInt4{k, 6 * local_h[H.edge_pose[k]], l, g});
                    }
                    npts++; ntask += nblk; e = e1;
                }
                if (npts) gstage.push_back(BaInt4{pt0, npts, t0, ntask});
                D.n_stages = (int)gstage.size() - D.stage_off;
            }
            {   // pose-major copy of edge_task (k_ba_bschur)
                const int *et = etask.data() + (etask.size() - H.n_edges);
                const int *pl = poseedges.data() + (poseedges.size() - H.n_edges);
                const int npm = posestart[posestart.size() - 1];
                for (int k = 0; k < H.n_edges; k++) pmtask.push_back(k < npm ? et[pl[k]] : -1);
            }
            // split the stages so that every CU has a workgroup
            int ks = (GEMM_TARGET_WGS + n_graphs * D.ngrp - 1) / (n_graphs * D.ngrp);
            ks = std::max(1, std::min(ks, std::max(1, D.n_stages / 4)));
            if (big_graph) ks = 1;                                   // k_ba_schur_big writes the whole block matrix once
            D.ks = ks;
            g_local_h.push_back(local_h);
            {   // static block-sparsity masks: 16-column tiles of the point's Hpl column that hold a non-zero block
                double issued = 0;
                ptmask.insert(ptmask.end(), (size_t)H.n_points, 0u);
                uint32_t *pmv = ptmask.data() + (ptmask.size() - H.n_points);
                for (int e = 0; e < H.n_edges && want_gemm_stats; e++) {
                    const int h = local_h[H.edge_pose[e]];
                    if (h >= 0 && !big_graph) pmv[H.edge_point[e]] |= (1u << ((6 * h) >> 4)) | (1u << ((6 * h + 5) >> 4));
                }
                double chunks = 0;                                                         // the kernel's issue rule: row tile hit AND a column tile of the chunk hit
                for (int l = 0; l < H.n_points && want_gemm_stats; l++) {
                    if (!pmv[l]) continue;                                                 // (a big window has nt > 32 tiles and no masks: nothing to shift)
                    const double k = __builtin_popcount(pmv[l]); issued += k * (k + 1) / 2;
                    for (int tr = 0; tr < nt; tr++) {
                        if (!((pmv[l] >> tr) & 1u)) continue;
                        for (int tc = tr; tc < nt; tc += GEMM_C) {
                            const int len = std::min(GEMM_C, nt - tc);
                            const uint32_t hit = pmv[l] & (((1u << len) - 1u) << tc);
                            if (hit) chunks += __builtin_popcount(hit);
                        }
                    }
                }
                flops_per_launch += issued * 2048.0;                                       // one 16x16x4 f64 MFMA (2048 flop) per (point, upper tile) that holds data
                flops_issued += chunks * 2048.0;
                flops_dense += (double)ntiles * 2048.0 * (double)H.n_points;                // same tiles without the masks
            }
            x1off.push_back((int)x1); x1 += (size_t)nf * 42 + 2;
            x2off.push_back((int)x2); x2 += (size_t)D.ld * D.ld + (size_t)nf * 6;
            D.s_off = s; s += (size_t)D.ld * D.ld;
            D.spart_off = sp; sp += (size_t)ks * D.ld * D.ld;
            max_edges = std::max(max_edges, H.n_edges); max_points = std::max(max_points, H.n_points);
            max_nf = std::max(max_nf, nf); max_ld = std::max(max_ld, D.ld);
            // initial estimates: SE3Quat ctor normalises the rotation (se3quat.h:58-64)
            for (int i = 0; i < H.n_poses; i++) {
                double q[7];
                memcpy(q, poses[g] + 7 * i, sizeof(q));
                if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
                const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
                for (int k = 0; k < 4; k++) q[k] /= nn;
                poses0.insert(poses0.end(), q, q + 7);
            }
            points0.insert(points0.end(), points[g], points[g] + 3 * (size_t)H.n_points);
            sumP += H.n_poses; sumL += H.n_points; sumE += H.n_edges; sumF += nf;
            gd.push_back(D);
        }
        s_total = s; spart_total = sp;
        pair_lists = any_big || (world == 1 && mode != 2);
        if (pair_lists) {
            for (int g = 0; g < n_graphs; g++) {
                BaGraphDev &D = gd[g];
                D.ks = 1;                                            // k_ba_schur_big writes slice 0 only
                const orbhip_ba_graph &H = graphs[g];
                const std::vector<int> &lh = g_local_h[g];
                const int nf = D.nf, npair = nf * (nf + 1) / 2;
                D.pair_off = pair_total_start; D.pent_off = pair_total_ent;
                const int *et = etask.data() + D.edge_off;
                // the lists themselves are built on the device (k_ba_pair_lists); the host only needs their sizes -- a point with nb blocks
                // puts one entry into nb (nb + 1) / 2 lists -- and the longest row of blocks (the LDS the row-owner Schur kernel takes)
                std::vector<int> seen(nf, 0);
                size_t tot = 0;
                for (int e0 = 0; e0 < H.n_edges;) {
                    int e1 = e0, nb = 0;
                    while (e1 < H.n_edges && H.edge_point[e1] == H.edge_point[e0]) { if (et[e1] >= 0) { nb++; seen[lh[H.edge_pose[e1]]]++; } e1++; }
                    tot += (size_t)nb * (nb + 1) / 2;
                    e0 = e1;
                }
                for (int k = 0; k < nf; k++) max_row_blocks = std::max(max_row_blocks, seen[k]);
                pair_total_start += (size_t)npair + 1; pair_total_ent += tot;
                max_npair = std::max(max_npair, npair);
            }
        }
        x_need = std::max(std::max(x1, x2), (size_t)3 * n_graphs);
        return ORBHIP_OK;
    }
};

// ------------------------------------------------------------------ landmark-sharded batches
// Every rank passes the SAME full graphs and estimates; rank r keeps points [r*L/world, (r+1)*L/world) of every graph with their edges
// (contiguous: edges are point-major) and all poses.  sub[g] is graph g cut to that slice (edge_point re-based into ept[g]), has[g] the
// poses with an edge on ANY rank: BaGraphLists::build's pose_in_system.
struct BaSlice { int pt0, npts, e0, ne; };
struct BaShard {
    std::vector<orbhip_ba_graph> sub;
    std::vector<std::vector<int32_t>> ept;
    std::vector<std::vector<uint8_t>> has;
    std::vector<const double *> pts;
    std::vector<BaSlice> slices;
    const char *err = nullptr;

    int build(const orbhip_ba_graph *graphs, int n_graphs, const double *const *points, int rank, int world)
    {
        sub.assign(graphs, graphs + n_graphs);
        ept.assign(n_graphs, {}); has.assign(n_graphs, {}); pts.assign(n_graphs, nullptr); slices.assign(n_graphs, BaSlice{0, 0, 0, 0});
        for (int g = 0; g < n_graphs; g++) {
            const orbhip_ba_graph &H = graphs[g];
            if (H.n_poses <= 0 || H.n_points < world || H.n_edges < 0) { err = "a sharded graph needs at least one point per rank"; return ORBHIP_E_BADARG; }
            has[g].assign(H.n_poses, 0);
            for (int e = 0; e < H.n_edges; e++) {
                if (H.edge_pose[e] < 0 || H.edge_pose[e] >= H.n_poses || H.edge_point[e] < 0 || H.edge_point[e] >= H.n_points ||
                    (e > 0 && H.edge_point[e] < H.edge_point[e - 1])) { err = "edges must be point-major with valid ids"; return ORBHIP_E_BADARG; }
                has[g][H.edge_pose[e]] = 1;
            }
            const int p0 = (int)((long long)rank * H.n_points / world), p1 = (int)((long long)(rank + 1) * H.n_points / world);
            int e0 = 0;
            while (e0 < H.n_edges && H.edge_point[e0] < p0) e0++;
            int e1 = e0;
            while (e1 < H.n_edges && H.edge_point[e1] < p1) e1++;
            slices[g] = {p0, p1 - p0, e0, e1 - e0};
            ept[g].resize(e1 - e0);
            for (int e = e0; e < e1; e++) ept[g][e - e0] = H.edge_point[e] - p0;
            orbhip_ba_graph &S = sub[g];
            S.n_points = p1 - p0; S.n_edges = e1 - e0;
            S.edge_pose = H.edge_pose + e0; S.edge_point = ept[g].data(); S.edge_obs = H.edge_obs + 3 * (size_t)e0;
            S.edge_inv_sigma2 = H.edge_inv_sigma2 + e0; S.edge_stereo = H.edge_stereo ? H.edge_stereo + e0 : nullptr;
            pts[g] = points[g] + 3 * (size_t)p0;
        }
        return ORBHIP_OK;
    }
};
