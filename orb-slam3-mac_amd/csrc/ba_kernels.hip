// ba_kernels.hip -- batched local bundle adjustment on gfx950: the numerical core of
// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1699-2344), i.e. g2o's
// Levenberg-Marquardt + Schur complement (BlockSolver_6_3), for G independent graphs at once.
//
//   B1  SE3Quat exp / oplus                  Thirdparty/g2o/g2o/types/se3quat.h:104-110,223-257      (ba_edges.h, shared with
//   B2  residuals + chi2                     include/OptimizableTypes.h:99-110, types_six_dof_expmap.cpp:190-197     pose_kernels.hip,
//   B3  Jacobians                            src/OptimizableTypes.cpp:139-160, types_six_dof_expmap.cpp:228-274      the pose-only BA)
//   B4  Huber-weighted quadratic form        g2o/core/base_binary_edge.hpp:55-120, robust_kernel_impl.cpp:65-91
//   B5  system layout, lambda on diagonals   g2o/core/block_solver.hpp:502-604
//   B6  Schur complement + reduced solve     g2o/core/block_solver.hpp:354-486, solvers/linear_solver_eigen.h:94-125
//   B7  LM control                           g2o/core/optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp:354-419
//   B8  two-pass schedule + outlier gates    src/Optimizer.cc:2041-2181
//
// Design: everything FP64.  The LM state machine of every graph lives on the device
// (BaState); the host only "ticks" a fixed kernel sequence (one LM trial per tick per
// graph) and polls one integer.  Edges arrive point-major (the reference's insertion
// order), so per-point assembly needs no atomics; pose blocks use a host-built pose-major
// edge list (deterministic reductions).  The only dense contraction, S -= (W D^-1) W^T, runs
// on the FP64 matrix cores (v_mfma_f64_16x16x4_f64) over a K-padded dense W panel.
//
// This file is the host side only: the arena plan, create (upload, pair-list launches), the tick -- the kernel sequence and its capture
// as a graph -- solve, download and the C ABI.  The device side:
//   ba_batch.h              BaState, BaBatch, ba_cam_ref, launch constants, the declaration of every kernel
//   ba_edge_kernels.hip     B2 - B5  k_ba_levels, _errors, _reduce, _build_points, _build_poses, _maxdiag, _finalize
//   ba_schur_kernels.hip    B6       k_ba_pair_lists, _pair_scan, _point_prep, _schur_gemm, _schur_finish, _bschur, _schur_big, _schur_rows;
//                                    the FP64 MFMA peak probe
//   ba_reduced_kernels.hip  B6       k_ba_ldlt, k_ba_big_init / _diag / _rows / _trail / _backsub; orbhip_debug_ldlt_prof (debug build)
//   ba_lm_kernels.hip       B7, B8   k_ba_pretrial, _backsub_points, _update_poses, _control
//   ba_shard_kernels.hip             k_ba_shard_pack1 / _sum1 / _pack2 / _sum2 / _pack34 / _sum34
//   ba_graph_lists.h                 the host's lists (no HIP), which create uploads
#include "orb_internal.h"
#include "ctx_internal.h"
#include "ba_ldlt.h"             // ba_ldlt_lds_bytes, LD_NB
#include "dense_ldlt_big.h"      // dense_big_rows_lds, dense_big_bsub_lds
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)
#include <cmath>
#include <cstring>
#include <vector>
#include <chrono>
#include <algorithm>

struct orbhip_ba_batch {
    orbhip_ctx *ctx;
    BaBatch B;
    std::vector<BaGraphDev> gd;
    std::vector<void *> allocs;              // ONE device arena per batch (round 4; ~60 separate hipMalloc before), absent when the
    bool ctx_arena, ctx_word;                // one-shot call borrowed the context's cached arena / pinned word instead
    std::vector<double> poses0, points0;     // normalised initial estimates (host copy)
    int *h_n_active;                         // pinned
    size_t wd_total, s_total, spart_total;
    int ticks_last;
    bool no_discard;                         // merge variant: no >= 50 % outlier bail-out
    bool profile;                            // time the Schur GEMM launches with hipEvents
    hipEvent_t ev0, ev1;
    float gemm_ms_total; int gemm_launches;
    double gemm_flops_per_launch;            // MFMA flops actually issued by one launch (all graphs)
    double gemm_flops_dense;                 // what the same upper tiles would cost without block-sparsity skipping
    double gemm_flops_issued;                // MFMA flops issued by one launch (every tile of a chunk whose row tile and one column tile the point touches)
    // landmark-sharded batches: the slice of every full graph this rank owns
    bool general;                            // some graph needs KannalaBrandt8, second-camera edges or twin-edge chains
    std::vector<BaSlice> slices;
    size_t x_need;                           // doubles per rank slot of the exchange buffer
    // one LM tick (about 20 dependent launches) captured as a hipGraph: small batches are launch bound
    hipGraphExec_t tick_graph; bool tick_graph_valid; BaBatch tick_B;
    int max_row_blocks;                      // most Hpl blocks any free pose of the batch holds (LDS of k_ba_schur_rows)
};

// Device memory of a batch: every array is a slice of ONE arena.  ba_create_impl first declares all slices (uploads first: their
// offsets are contiguous), then takes the arena -- its own hipMalloc, or for a one-shot solve (Optimizer::LocalBundleAdjustment's
// shape: create, solve, download, destroy) the context's cached grow-only arena -- gathers the upload slices in the context's
// page-locked staging area and sends them in ONE host-to-device copy.  Round 3 issued ~60 hipMalloc, ~27 synchronous copies from
// pageable vectors and ~60 hipFree per window: 1.8 + 0.96 ms of a 7 ms call (host_smoke latency).
struct BaPlan {
    struct It { void **dst; const void *src; size_t bytes, off; };
    std::vector<It> items;
    size_t total = 0, up_end = 0;
    void add(void **dst, const void *src, size_t bytes)
    {
        items.push_back({dst, src, bytes, total});
        total += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        if (src) up_end = total;
    }
};
extern "C" void orbhip_ba_default_params(orbhip_ba_params *p)
{
    p->iters1 = 5; p->iters2 = 10; p->huber_mono2 = 5.991; p->huber_stereo2 = 7.815;
    p->user_lambda_init = 0.0; p->tau = 1e-50; p->max_trials = 100;
    p->stage2_exclude_outliers = 0; p->stage2_drop_robust = 0; p->no_discard = 0; p->gate_mono2 = 0; p->gate_stereo2 = 0;
}

// Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag), Optimizer.cc:6255-6800
extern "C" void orbhip_ba_merge_params(orbhip_ba_params *p)
{
    orbhip_ba_default_params(p);
    p->huber_mono2 = 5.99; p->gate_mono2 = 5.991; p->gate_stereo2 = 7.815;       // :6395, :6554, :6571
    p->stage2_exclude_outliers = 1; p->stage2_drop_robust = 1; p->no_discard = 1;
}

// Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust), Optimizer.cc:62-330: ONE optimize(nIterations),
// thHuber2D = sqrt(5.99) / thHuber3D = sqrt(7.815) (:133-134) when bRobust, no outlier stage, results always written back
extern "C" void orbhip_ba_global_params(orbhip_ba_params *p, int iterations, int robust)
{
    orbhip_ba_default_params(p);
    p->iters1 = iterations; p->iters2 = 0; p->no_discard = 1;
    p->huber_mono2 = robust ? 5.99 : 1e300; p->huber_stereo2 = robust ? 7.815 : 1e300;     // delta -> inf: rho(x) = x, no kernel
    p->gate_mono2 = 5.991; p->gate_stereo2 = 7.815;                                          // informational outlier flags only
}

extern "C" void orbhip_ba_batch_destroy(orbhip_ba_batch *b)
{
    if (!b) return;
    (void)hipStreamSynchronize(orbhip_ctx_stream_internal(b->ctx));
    for (void *p : b->allocs) (void)hipFree(p);
    if (b->ctx_arena) orbhip_ctx_ba_arena_release_internal(b->ctx);
    if (b->h_n_active && !b->ctx_word) (void)hipHostFree(b->h_n_active);
    if (b->ev0) { (void)hipEventDestroy(b->ev0); (void)hipEventDestroy(b->ev1); }
    if (b->tick_graph_valid) (void)hipGraphExecDestroy(b->tick_graph);
    delete b;
}

static_assert(sizeof(BaInt4) == sizeof(int4) && alignof(BaInt4) == alignof(int4) && sizeof(BaInt2) == sizeof(int2) && alignof(BaInt2) == alignof(int2),
              "ba_graph_lists.h's four-int and two-int structs must be HIP's int4 and int2");

// The lists come from ba_graph_lists.h (host only); here they get their device memory, are uploaded, and the pair lists are launched.
static int ba_create_impl(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs, const double *const *poses, const double *const *points,
                          const std::vector<std::vector<uint8_t>> *pose_in_system, int rank, int world, orbhip_ba_batch **out, bool oneshot = false)
{
    if (!ctx || !graphs || n_graphs <= 0 || !poses || !points || !out) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    int mode = orbhip_ctx_ba_schur_mode_internal(ctx);
    if (const char *ev = getenv("ORBHIP_BA_PAIRS")) mode = atoi(ev) ? 1 : 2;                                                    // development override
    static thread_local BaGraphLists L;                          // (keeps its vectors' capacity from call to call: see the struct)
    const int rc = L.build(graphs, n_graphs, poses, points, pose_in_system, world, mode);
    if (rc != ORBHIP_OK) { if (L.err) orbhip_set_last_error_internal(L.err); return rc; }
    orbhip_ba_batch *b = new orbhip_ba_batch();
    b->ctx = ctx; b->h_n_active = nullptr; b->ctx_arena = false; b->ctx_word = false; b->ticks_last = 0; b->tick_graph = nullptr; b->tick_graph_valid = false;
    b->profile = false; b->ev0 = b->ev1 = nullptr; b->gemm_ms_total = 0; b->gemm_launches = 0;
    b->gemm_flops_per_launch = L.flops_per_launch; b->gemm_flops_dense = L.flops_dense; b->gemm_flops_issued = L.flops_issued;
    b->gd = L.gd; b->poses0 = L.poses0; b->points0 = L.points0;
    b->general = L.general; b->s_total = L.s_total; b->spart_total = L.spart_total; b->max_row_blocks = L.max_row_blocks; b->x_need = L.x_need;
    BaBatch &B = b->B;
    memset(&B, 0, sizeof(B));
    B.G = n_graphs; B.rank = rank; B.world = world;
    B.max_edges = L.max_edges; B.max_points = L.max_points; B.max_nf = L.max_nf; B.max_ld = L.max_ld;
    B.sumP = L.sumP; B.sumL = L.sumL; B.sumE = L.sumE; B.sumF = L.sumF;
    B.big = L.any_big ? 1 : 0; B.pair_schur = L.pair_lists ? 1 : 0;
    const size_t sumP = (size_t)L.sumP, sumL = (size_t)L.sumL, sumE = (size_t)L.sumE, sumF = (size_t)L.sumF, n_pent = std::max<size_t>(L.pair_total_ent, 1);
    BaPlan plan;
#define UP(dst, vec) plan.add((void **)&(dst), (vec).empty() ? (const void *)&plan : (const void *)(vec).data(), (vec).size() * sizeof((vec)[0]))
#define AL(dst, T, n) plan.add((void **)&(dst), nullptr, (size_t)(n) * sizeof(T))
    UP(B.gd, L.gd); UP(B.cams, L.cams); UP(B.pose_cam, L.posecam); UP(B.hidx, L.hidx); UP(B.edge_pose, L.epose); UP(B.edge_point, L.epoint); UP(B.edge_obs, L.eobs);
    UP(B.edge_is2, L.eis2); UP(B.edge_stereo, L.est); UP(B.edge_dup, L.edup); UP(B.edge_next, L.enext); UP(B.pt_start, L.ptstart); UP(B.pose_start, L.posestart);
    UP(B.pose_edges, L.poseedges); UP(B.ptmask, L.ptmask); UP(B.gemm_task, L.gtask); UP(B.gemm_stage, L.gstage); UP(B.edge_task, L.etask); UP(B.x1_off, L.x1off);
    UP(B.x2_off, L.x2off); UP(B.pm_point, L.pmpoint); UP(B.pm_task, L.pmtask); UP(B.pm_type, L.pmtype); UP(B.pm_is2, L.pmis2); UP(B.pm_obs, L.pmobs);
    if (L.any_big) {
        AL(B.big_y, double, sumF * 6); AL(B.big_d, double, sumF * 6); AL(B.big_U, double, (size_t)n_graphs * LD_NB * LD_NB);
        AL(B.big_fail, int, n_graphs);
    }
    if (L.pair_lists) {
        AL(B.big_pair_start, int, L.pair_total_start); AL(B.big_pair_ent, int2, n_pent); AL(B.big_pair_pt, int, n_pent); AL(B.big_pair_jr, int2, n_pent);
    }
    AL(B.st, BaState, n_graphs);
    AL(B.poses, double, 2 * sumP * 7); AL(B.points, double, 2 * sumL * 3);
    AL(B.err, double, sumE * 3); AL(B.chi2, double, sumE); AL(B.rho0, double, sumE);
    AL(B.Hll, double, sumL * 6); AL(B.bl, double, sumL * 3); AL(B.Dinv, double, sumL * 6); AL(B.db, double, sumL * 3);
    AL(B.Hpp, double, sumF * 36); AL(B.bp, double, sumF * 6); AL(B.bs, double, sumF * 6);
    AL(B.Wsp, double, L.gtask.size() * 18); AL(B.Linv, double, sumL * 6); AL(B.S, double, L.s_total); AL(B.Spart, double, L.spart_total);
    AL(B.xp, double, sumF * 6); AL(B.xl, double, sumL * 3);
    AL(B.scale_pt, double, sumL); AL(B.scale_pose, double, sumF);
    AL(B.chi, double, n_graphs); AL(B.scale, double, n_graphs); AL(B.maxdiag, double, n_graphs);
    AL(B.n_active, int, 1); AL(B.outlier, uint8_t, sumE); AL(B.level, uint8_t, sumE);
    AL(B.bacc, double, sumF * 6); AL(B.x_abort, int, 1); AL(B.edges_total, double, n_graphs);
#undef UP
#undef AL
    {
        hipStream_t st = orbhip_ctx_stream_internal(ctx);
        uint8_t *arena = nullptr;
        if (oneshot && (arena = (uint8_t *)orbhip_ctx_ba_arena_acquire_internal(ctx, plan.total))) b->ctx_arena = true;
        else {
            void *p = nullptr;
            if (hipMalloc(&p, plan.total) != hipSuccess) { orbhip_ba_batch_destroy(b); orbhip_set_last_error_internal("device allocation failed"); return ORBHIP_E_HIP; }
            b->allocs.push_back(p); arena = (uint8_t *)p;
        }
        uint8_t *stage = (uint8_t *)orbhip_ctx_pinned_internal(ctx, plan.up_end);
        if (!stage) { orbhip_ba_batch_destroy(b); orbhip_set_last_error_internal("page-locked staging allocation failed"); return ORBHIP_E_HIP; }
        for (const BaPlan::It &it : plan.items) {
            *it.dst = arena + it.off;
            if (it.src && it.bytes) memcpy(stage + it.off, it.src, it.bytes);
        }
        // the staging area belongs to the context and the next host-pointer call may reuse it: the copy is waited for here
        bool up_ok = hipMemcpyAsync(arena, stage, plan.up_end, hipMemcpyHostToDevice, st) == hipSuccess;
        if (up_ok && L.pair_lists && L.max_npair > 0) {          // the pair lists, from the lists just uploaded (stream order)
            const dim3 grid((unsigned)((L.max_npair + 3) / 4), (unsigned)n_graphs);
            hipLaunchKernelGGL(k_ba_pair_lists<0>, grid, dim3(256), 0, st, B);
            hipLaunchKernelGGL(k_ba_pair_scan, dim3((unsigned)n_graphs), dim3(256), 0, st, B);
            hipLaunchKernelGGL(k_ba_pair_lists<1>, grid, dim3(256), 0, st, B);
            up_ok = hipGetLastError() == hipSuccess;
        }
        if (!up_ok || hipStreamSynchronize(st) != hipSuccess) {
            orbhip_ba_batch_destroy(b); orbhip_set_last_error_internal("upload of the graph failed"); return ORBHIP_E_HIP;
        }
        if (oneshot && (b->h_n_active = orbhip_ctx_pinned_word_internal(ctx))) b->ctx_word = true;
        else if (hipHostMalloc((void **)&b->h_n_active, sizeof(int)) != hipSuccess) { b->h_n_active = nullptr; orbhip_ba_batch_destroy(b); orbhip_set_last_error_internal("device allocation failed"); return ORBHIP_E_HIP; }
    }
    *out = b;
    return ORBHIP_OK;
}

extern "C" int orbhip_ba_batch_create(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs,
                                      double *const *poses, double *const *points, orbhip_ba_batch **out)
{
    return ba_create_impl(ctx, graphs, n_graphs, poses, points, nullptr, 0, 1, out);
}

// Landmark-sharded batch (optional single-graph mode): rank r's slice of every graph (BaShard, ba_graph_lists.h), all poses
extern "C" int orbhip_ba_batch_create_sharded(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs, double *const *poses,
                                              double *const *points, int rank, int world, orbhip_ba_batch **out)
{
    if (!ctx || !graphs || n_graphs <= 0 || !poses || !points || !out || world < 1 || rank < 0 || rank >= world) return ORBHIP_E_BADARG;
    BaShard S;
    int rc = S.build(graphs, n_graphs, points, rank, world);
    if (rc != ORBHIP_OK) { orbhip_set_last_error_internal(S.err); return rc; }
    rc = ba_create_impl(ctx, S.sub.data(), n_graphs, poses, S.pts.data(), &S.has, rank, world, out);
    if (rc == ORBHIP_OK) (*out)->slices = S.slices;
    return rc;
}

extern "C" size_t orbhip_ba_batch_exchange_doubles(const orbhip_ba_batch *b) { return b ? b->x_need : 0; }

// Runs optimize(iters1) + optimize(iters2) + outlier classification for every graph of the batch,
// starting from the initial estimates given at creation.  Device-resident; returns after completion.
static int ba_solve_impl(orbhip_ba_batch *b, const orbhip_ba_params *params, volatile const uint8_t *abort_flag, orbhip_ba_exchange_fn xch, void *xuser)
{
    if (!b || !params) return ORBHIP_E_BADARG;
    const bool sharded = b->B.world > 1;
    if (sharded && (!xch || !b->B.xbuf)) { orbhip_set_last_error_internal("a sharded batch needs orbhip_ba_batch_set_exchange_buffer and an exchange callback"); return ORBHIP_E_BADARG; }
    if (hipSetDevice(orbhip_ctx_device_internal(b->ctx)) != hipSuccess) return ORBHIP_E_HIP;
    if (!sharded && abort_flag && *abort_flag) return ORBHIP_E_ABORTED;       // Optimizer.cc:2041-2043 (sharded: the flag travels through exchange 3)
    hipStream_t s = orbhip_ctx_stream_internal(b->ctx);
    BaBatch &B = b->B;
    B.delta_m = (double)(float)sqrt(params->huber_mono2); B.dsqr_m = (double)(float)(B.delta_m * B.delta_m);
    B.delta_s = (double)(float)sqrt(params->huber_stereo2); B.dsqr_s = (double)(float)(B.delta_s * B.delta_s);
    B.gate_m = params->gate_mono2 > 0 ? params->gate_mono2 : params->huber_mono2;
    B.gate_s = params->gate_stereo2 > 0 ? params->gate_stereo2 : params->huber_stereo2;
    B.ex2 = params->stage2_exclude_outliers; B.nr2 = params->stage2_drop_robust; b->no_discard = params->no_discard != 0;
    B.user_lambda = params->user_lambda_init; B.tau = params->tau;
    B.iters[0] = params->iters1; B.iters[1] = params->iters2; B.max_trials = params->max_trials;
    // reset state + estimates
    std::vector<BaState> st(B.G);
    for (auto &x : st) {
        memset(&x, 0, sizeof(x));
        x.need_build = 1; x.need_lambda_init = 1; x.active = 1; x.ok = 1; x.chi_first = -1.0; x.robust = 1;
    }
    if (params->iters1 <= 0) for (auto &x : st) { x.pass = 1; }
    int n_active = B.G;
    if (params->iters1 <= 0 && params->iters2 <= 0) { for (auto &x : st) x.active = 0; n_active = 0; }
    ORB_HIP_TRY(hipMemcpyAsync(B.st, st.data(), sizeof(BaState) * B.G, hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemcpyAsync(B.poses, b->poses0.data(), sizeof(double) * b->poses0.size(), hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemcpyAsync(B.points, b->points0.data(), sizeof(double) * b->points0.size(), hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemcpyAsync(B.n_active, &n_active, sizeof(int), hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemsetAsync(B.xp, 0, sizeof(double) * (size_t)B.sumF * 6, s));
    ORB_HIP_TRY(hipMemsetAsync(B.xl, 0, sizeof(double) * (size_t)B.sumL * 3, s));
    ORB_HIP_TRY(hipMemsetAsync(B.level, 0, (size_t)std::max(B.sumE, 1), s));
    ORB_HIP_TRY(hipMemsetAsync(B.x_abort, 0, sizeof(int), s));
    ORB_HIP_TRY(hipStreamSynchronize(s));     // st / n_active host buffers must outlive the copies
    // sharded: the caller's all-gather runs between two kernels; the stream is drained around it
#define XCHG(stage, cnt) do { ORB_HIP_TRY(hipStreamSynchronize(s)); if (xch(xuser, (stage), (size_t)(cnt)) != 0) { orbhip_set_last_error_internal("exchange callback failed"); return ORBHIP_E_HIP; } } while (0)
    const size_t x1n = b->x_need, x3n = (size_t)3 * B.G;
    const int G = B.G;
    const dim3 ge((B.max_edges + 255) / 256, G), gp128((B.max_points + 127) / 128, G), gp256((B.max_points + 255) / 256, G);
    const dim3 gf(std::max(B.max_nf, 1), G);
    int max_items = 0, max_poses = 0;
    for (auto &D : b->gd) { max_items = std::max(max_items, D.ks * D.ngrp); max_poses = std::max(max_poses, D.n_poses); }
    size_t gemm_lds = 0;
    for (auto &D : b->gd) gemm_lds = std::max(gemm_lds, sizeof(double) * (2 * (size_t)D.gemm_ps * 3 * (size_t)(D.ld + GEMM_LDS_PAD) + GEMM_LDS_TAIL));
    if (orb_lds_optin(reinterpret_cast<const void *>(k_ba_schur_gemm), orbhip_ctx_device_internal(b->ctx), gemm_lds)) { orbhip_set_last_error_internal("LDS opt-in (k_ba_schur_gemm)"); return ORBHIP_E_HIP; }
    const size_t ldlt_lds = B.big ? 0 : ba_ldlt_lds_bytes(B.max_ld);
    if (!B.big && orb_lds_optin(reinterpret_cast<const void *>(k_ba_ldlt), orbhip_ctx_device_internal(b->ctx), ldlt_lds)) { orbhip_set_last_error_internal("LDS opt-in (k_ba_ldlt)"); return ORBHIP_E_HIP; }
    const size_t rows_lds = dense_big_rows_lds(), bsub_lds = dense_big_bsub_lds(B.max_ld);
    int max_n = 0, max_nfp = 0;
    for (auto &D : b->gd) { max_n = std::max(max_n, D.n); max_nfp = std::max(max_nfp, D.nf * (D.nf + 1) / 2); }
    if (B.big) {
        if (orb_lds_optin(reinterpret_cast<const void *>(k_ba_big_rows), orbhip_ctx_device_internal(b->ctx), rows_lds) ||
            orb_lds_optin(reinterpret_cast<const void *>(k_ba_big_backsub), orbhip_ctx_device_internal(b->ctx), bsub_lds)) { orbhip_set_last_error_internal("LDS opt-in (big LDLT)"); return ORBHIP_E_HIP; }
    }
    // the row-owner form of the pair Schur kernel: whenever every pose's blocks fit the LDS (ORBHIP_BA_SCHUR_ROWS=0: keep k_ba_schur_big, for A/B runs)
    const size_t srow_lds = sizeof(double) * 18 * (size_t)std::max(b->max_row_blocks, 1);
    bool schur_rows = B.pair_schur && b->max_row_blocks <= SROW_MAX_BLOCKS && !(getenv("ORBHIP_BA_SCHUR_ROWS") && atoi(getenv("ORBHIP_BA_SCHUR_ROWS")) == 0);
    if (schur_rows && orb_lds_optin(reinterpret_cast<const void *>(k_ba_schur_rows), orbhip_ctx_device_internal(b->ctx), srow_lds)) { orbhip_set_last_error_internal("LDS opt-in (k_ba_schur_rows)"); return ORBHIP_E_HIP; }
    const int max_ticks = (params->iters1 + params->iters2) * params->max_trials + 4;
    int tick = 0;
    // one LM tick: every graph that is still active evaluates, builds, solves and tries one step (inactive graphs return at once)
    auto launch_tick = [&](int ab) -> int {
        if (B.ex2) hipLaunchKernelGGL(k_ba_levels, ge, dim3(256), 0, s, B);
        if (b->general) hipLaunchKernelGGL(k_ba_errors<true>, ge, dim3(256), 0, s, B, 0); else hipLaunchKernelGGL(k_ba_errors<false>, ge, dim3(256), 0, s, B, 0);
        hipLaunchKernelGGL(k_ba_reduce, dim3(G), dim3(1024), 0, s, B, 0);
        if (b->general) hipLaunchKernelGGL(k_ba_build_points<true>, dim3((B.max_points + 15) / 16, G), dim3(256), 0, s, B);
        else hipLaunchKernelGGL(k_ba_build_points<false>, dim3((B.max_points + 15) / 16, G), dim3(256), 0, s, B);
        if (b->general) hipLaunchKernelGGL(k_ba_build_poses<true>, gf, dim3(64), 0, s, B); else hipLaunchKernelGGL(k_ba_build_poses<false>, gf, dim3(64), 0, s, B);
        hipLaunchKernelGGL(k_ba_maxdiag, dim3(G), dim3(256), 0, s, B);
        if (sharded) {                                           // exchange 1: Hpp, bp, chi2, max |Hll diag|
            hipLaunchKernelGGL(k_ba_shard_pack1, dim3(G), dim3(256), 0, s, B);
            XCHG(1, x1n);
            hipLaunchKernelGGL(k_ba_shard_sum1, dim3(G), dim3(256), 0, s, B);
        }
        hipLaunchKernelGGL(k_ba_pretrial, dim3((G + 63) / 64), dim3(64), 0, s, B);
        hipLaunchKernelGGL(k_ba_point_prep, gp256, dim3(256), 0, s, B);
        if (b->profile) ORB_HIP_TRY(hipEventRecord(b->ev0, s));
        if (B.pair_schur && max_nfp > 0) {                       // (a batch whose poses are all fixed has no reduced system: points only)
            if (G >= 8 && schur_rows) hipLaunchKernelGGL(k_ba_schur_rows, dim3((unsigned)(B.max_nf * (((G + 7) / 8) * 8))), dim3(SROW_THREADS), srow_lds, s, B, B.max_nf);
            else if (G >= 8) hipLaunchKernelGGL(k_ba_schur_big<16>, dim3((unsigned)(((max_nfp + 3) / 4) * (((G + 7) / 8) * 8))), dim3(64), 0, s, B, (max_nfp + 3) / 4);
            else hipLaunchKernelGGL(k_ba_schur_big<64>, dim3((unsigned)(max_nfp * G)), dim3(64), 0, s, B, max_nfp);
        }
        else if (!B.pair_schur) hipLaunchKernelGGL(k_ba_schur_gemm, dim3(max_items, G), dim3(64 * GEMM_WAVES), gemm_lds, s, B);
        if (b->profile) ORB_HIP_TRY(hipEventRecord(b->ev1, s));
        if (!B.pair_schur) hipLaunchKernelGGL(k_ba_bschur, gf, dim3(64), 0, s, B);      // (the pair kernel's diagonal rows produced bs)
        if (sharded) {                                           // exchange 2: the shared Schur block (sum_ks Spart) and W db
            hipLaunchKernelGGL(k_ba_shard_pack2, dim3((B.max_ld * B.max_ld + 255) / 256, G), dim3(256), 0, s, B);
            XCHG(2, x1n);
            hipLaunchKernelGGL(k_ba_shard_sum2, dim3(G), dim3(256), 0, s, B);
        }
        if (!B.pair_schur) hipLaunchKernelGGL(k_ba_schur_finish, dim3((B.max_ld * B.max_ld + 255) / 256, G), dim3(256), 0, s, B);      // (the pair kernel wrote the finished S)
        if (!B.big) hipLaunchKernelGGL(k_ba_ldlt, dim3(G), dim3(1024), ldlt_lds, s, B);
        else {
            hipLaunchKernelGGL(k_ba_big_init, dim3((max_n + 255) / 256, G), dim3(256), 0, s, B);
            for (int p0 = 0; p0 < max_n; p0 += LD_NB) {
                const int m2 = max_n - p0 - LD_NB;
                hipLaunchKernelGGL(k_ba_big_diag, dim3(G), dim3(64), 0, s, B, p0);
                if (m2 > 0) {
                    hipLaunchKernelGGL(k_ba_big_rows, dim3((m2 + 255) / 256, G), dim3(256), rows_lds, s, B, p0);
                    const int nt = (m2 + 63) / 64;
                    hipLaunchKernelGGL(k_ba_big_trail, dim3(nt, nt, G), dim3(256), 0, s, B, p0);
                }
            }
            hipLaunchKernelGGL(k_ba_big_backsub, dim3(G), dim3(1024), bsub_lds, s, B);
        }
        hipLaunchKernelGGL(k_ba_backsub_points, dim3((B.max_points + 15) / 16, G), dim3(256), 0, s, B);
        hipLaunchKernelGGL(k_ba_update_poses, dim3((max_poses + 63) / 64, G), dim3(64), 0, s, B);
        if (b->general) hipLaunchKernelGGL(k_ba_errors<true>, ge, dim3(256), 0, s, B, 1); else hipLaunchKernelGGL(k_ba_errors<false>, ge, dim3(256), 0, s, B, 1);
        hipLaunchKernelGGL(k_ba_reduce, dim3(G), dim3(1024), 0, s, B, 1);
        if (sharded) {                                           // exchange 3: trial chi2, computeScale, abort flag
            hipLaunchKernelGGL(k_ba_shard_pack34, dim3((G + 63) / 64), dim3(64), 0, s, B, 3, ab);
            XCHG(3, x3n);
            hipLaunchKernelGGL(k_ba_shard_sum34, dim3((G + 63) / 64), dim3(64), 0, s, B, 3);
        }
        hipLaunchKernelGGL(k_ba_control, dim3((G + 63) / 64), dim3(64), 0, s, B, ab);
        return ORBHIP_OK;
    };
    // Replay form of a tick (no exchange, no event timing, abort flag down): captured once per batch and parameter set.  The
    // kernels of a graph that has finished return at once, so several ticks may be queued per host round trip.
    const bool trace = getenv("ORBHIP_BA_TRACE") != nullptr;      // development: graph 0's LM state after every tick on stderr (one tick per round trip)
    // (a one-shot solve would capture, instantiate and destroy a graph for ~8 replays: ORBHIP_BA_ONESHOT_GRAPH=0 / 1 decides)
    static const int oneshot_graph = getenv("ORBHIP_BA_ONESHOT_GRAPH") ? atoi(getenv("ORBHIP_BA_ONESHOT_GRAPH")) : 0;
    const bool use_graph = !sharded && !b->profile && !trace && (!b->ctx_arena || oneshot_graph);
    if (use_graph && !(b->tick_graph_valid && memcmp(&b->tick_B, &B, sizeof(BaBatch)) == 0)) {
        if (b->tick_graph_valid) { (void)hipGraphExecDestroy(b->tick_graph); b->tick_graph_valid = false; }
        hipGraph_t graph = nullptr;
        ORB_HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = launch_tick(0);
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        if (rc != ORBHIP_OK || ce != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); orbhip_set_last_error_internal("tick capture"); return ORBHIP_E_HIP; }
        const hipError_t ie = hipGraphInstantiate(&b->tick_graph, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) { orbhip_set_last_error_internal("hipGraphInstantiate(tick)"); return ORBHIP_E_HIP; }
        b->tick_graph_valid = true; b->tick_B = B;
    }
    const int ticks_per_sync = use_graph ? (G <= 16 ? 4 : 2) : 1;
    while (tick < max_ticks && n_active > 0) {
        const int ab = (abort_flag && *abort_flag) ? 1 : 0;
        if (use_graph && !ab) {
            for (int k = 0; k < ticks_per_sync && tick < max_ticks; k++, tick++) ORB_HIP_TRY(hipGraphLaunch(b->tick_graph, s));
        } else {
            const int rc = launch_tick(ab);
            if (rc != ORBHIP_OK) return rc;
            tick++;
        }
        ORB_HIP_TRY(hipMemcpyAsync(b->h_n_active, B.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        ORB_HIP_TRY(hipGetLastError());                  // a rejected launch fails here, loudly, instead of spinning to max_ticks
        n_active = *b->h_n_active;
        if (trace) {
            BaState t0;
            ORB_HIP_TRY(hipMemcpy(&t0, B.st, sizeof(BaState), hipMemcpyDeviceToHost));
            fprintf(stderr, "[orbhip ba] tick %d: pass %d iter %d qmax %d lambda %.6e chi %.9e rho %.6e ok %d nbad %d active %d trials %d\n", tick, t0.pass, t0.iter, t0.qmax,
                    t0.lambda, t0.current_chi, t0.rho_dbg, t0.ok, t0.nbad, t0.active, t0.lm_trials);
        }
        if (b->profile) {
            float ms = 0;
            ORB_HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
            b->gemm_ms_total += ms; b->gemm_launches++;
        }
    }
    b->ticks_last = tick;
    hipLaunchKernelGGL(k_ba_finalize, ge, dim3(256), 0, s, B);
    if (sharded) {                                               // exchange 4: outlier and edge counts for the >= 50 % rule
        hipLaunchKernelGGL(k_ba_shard_pack34, dim3((G + 63) / 64), dim3(64), 0, s, B, 4, 0);
        XCHG(4, x3n);
        hipLaunchKernelGGL(k_ba_shard_sum34, dim3((G + 63) / 64), dim3(64), 0, s, B, 4);
    }
    ORB_HIP_TRY(hipStreamSynchronize(s));
    ORB_HIP_TRY(hipGetLastError());
#undef XCHG
    return ORBHIP_OK;
}

extern "C" int orbhip_ba_batch_solve(orbhip_ba_batch *b, const orbhip_ba_params *params, volatile const uint8_t *abort_flag)
{
    if (b && b->B.world > 1) { orbhip_set_last_error_internal("sharded batch: use orbhip_ba_batch_solve_sharded"); return ORBHIP_E_BADARG; }
    return ba_solve_impl(b, params, abort_flag, nullptr, nullptr);
}

extern "C" int orbhip_ba_batch_set_exchange_buffer(orbhip_ba_batch *b, double *d_buf, size_t capacity_doubles)
{
    if (!b || !d_buf || capacity_doubles < (size_t)b->B.world * b->x_need) return ORBHIP_E_BADARG;
    b->B.xbuf = d_buf; b->B.xcount = b->x_need;
    return ORBHIP_OK;
}

extern "C" int orbhip_ba_batch_solve_sharded(orbhip_ba_batch *b, const orbhip_ba_params *params, volatile const uint8_t *abort_flag,
                                             orbhip_ba_exchange_fn exchange, void *user)
{
    if (!b || !exchange) return ORBHIP_E_BADARG;
    if (b->B.world == 1) return ba_solve_impl(b, params, abort_flag, nullptr, nullptr);
    return ba_solve_impl(b, params, abort_flag, exchange, user);
}

// D2H of the results of the last solve.  poses_out[g]/points_out[g] are written unless the graph
// was discarded (>= 50 % outliers, Optimizer.cc:2177-2181); outlier/stats may be NULL.
extern "C" int orbhip_ba_batch_download(orbhip_ba_batch *b, double *const *poses_out, double *const *points_out,
                                        uint8_t *const *edge_outlier_out, orbhip_ba_stats *stats_out)
{
    if (!b) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(b->ctx)) != hipSuccess) return ORBHIP_E_HIP;
    BaBatch &B = b->B;
    std::vector<BaState> st(B.G);
    std::vector<double> poses((size_t)2 * B.sumP * 7), points((size_t)2 * B.sumL * 3);
    std::vector<uint8_t> outl(B.sumE ? B.sumE : 1);
    if (hipMemcpy(st.data(), B.st, sizeof(BaState) * B.G, hipMemcpyDeviceToHost) != hipSuccess) return ORBHIP_E_HIP;
    if (hipMemcpy(poses.data(), B.poses, poses.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return ORBHIP_E_HIP;
    if (hipMemcpy(points.data(), B.points, points.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return ORBHIP_E_HIP;
    if (B.sumE && hipMemcpy(outl.data(), B.outlier, B.sumE, hipMemcpyDeviceToHost) != hipSuccess) return ORBHIP_E_HIP;
    std::vector<double> etot(B.G, 0.0);
    if (B.world > 1 && hipMemcpy(etot.data(), B.edges_total, sizeof(double) * B.G, hipMemcpyDeviceToHost) != hipSuccess) return ORBHIP_E_HIP;
    for (int g = 0; g < B.G; g++) {
        const BaGraphDev &D = b->gd[g];
        const double n_edges_all = B.world > 1 ? etot[g] : (double)D.n_edges;          // sharded: counts of all ranks (exchange 4)
        const int discarded = (!b->no_discard && n_edges_all > 0 && st[g].n_outliers >= n_edges_all * 0.5) ? 1 : 0;
        const size_t pt0 = b->slices.empty() ? 0 : (size_t)b->slices[g].pt0, e0 = b->slices.empty() ? 0 : (size_t)b->slices[g].e0;
        if (!discarded) {                                      // sharded: this rank's points / edges land at their place in the full arrays
            if (poses_out && poses_out[g]) memcpy(poses_out[g], poses.data() + ((size_t)st[g].cur * B.sumP + D.pose_off) * 7, sizeof(double) * 7 * D.n_poses);
            if (points_out && points_out[g]) memcpy(points_out[g] + 3 * pt0, points.data() + ((size_t)st[g].cur * B.sumL + D.point_off) * 3, sizeof(double) * 3 * D.n_points);
        }
        if (edge_outlier_out && edge_outlier_out[g]) memcpy(edge_outlier_out[g] + e0, outl.data() + D.edge_off, D.n_edges);
        if (stats_out) {
            orbhip_ba_stats &o = stats_out[g];
            o.iterations_run[0] = st[g].iters_run[0]; o.iterations_run[1] = st[g].iters_run[1];
            o.lm_trials = st[g].lm_trials; o.n_outliers = st[g].n_outliers; o.discarded = discarded;
            o.chi2_initial = st[g].chi_first; o.chi2_final = st[g].chi_last;
        }
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_ba_batch_ticks(const orbhip_ba_batch *b) { return b ? b->ticks_last : ORBHIP_E_BADARG; }

extern "C" int orbhip_ba_batch_set_profiling(orbhip_ba_batch *b, int enable)
{
    if (!b) return ORBHIP_E_BADARG;
    if (enable && !b->ev0) {
        if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) return ORBHIP_E_HIP;
    }
    b->profile = enable != 0; b->gemm_ms_total = 0; b->gemm_launches = 0;
    return ORBHIP_OK;
}

// Accumulated device time / launch count of the Schur GEMM kernel since profiling was enabled,
// and the MFMA flops one launch really issues (upper 16x16 tiles, static block-sparsity masks).
extern "C" int orbhip_ba_batch_gemm_profile(const orbhip_ba_batch *b, float *total_ms, int *launches, double *flops_per_launch)
{
    if (!b || !total_ms || !launches || !flops_per_launch) return ORBHIP_E_BADARG;
    *total_ms = b->gemm_ms_total; *launches = b->gemm_launches; *flops_per_launch = b->gemm_flops_per_launch;
    return ORBHIP_OK;
}
extern "C" double orbhip_ba_batch_gemm_dense_flops(const orbhip_ba_batch *b) { return b ? b->gemm_flops_dense : 0.0; }
extern "C" double orbhip_ba_batch_gemm_issued_flops(const orbhip_ba_batch *b) { return b ? b->gemm_flops_issued : 0.0; }

extern "C" int orbhip_ba_solve_batch(orbhip_ctx *ctx, const orbhip_ba_graph *graphs, int n_graphs,
                                     const orbhip_ba_params *params, volatile const uint8_t *abort_flag,
                                     double *const *poses_inout, double *const *points_inout,
                                     uint8_t *const *edge_outlier_out, orbhip_ba_stats *stats_out)
{
    if (abort_flag && *abort_flag) return ORBHIP_E_ABORTED;
    orbhip_ba_batch *b = nullptr;
    static const bool prof = getenv("ORBHIP_HOST_PROF") != nullptr;       // where a one-shot call spends its time (host_smoke latency)
    const auto t0 = std::chrono::steady_clock::now();
    int rc = ba_create_impl(ctx, graphs, n_graphs, poses_inout, points_inout, nullptr, 0, 1, &b, true);     // borrows the context's cached arena
    if (rc) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = orbhip_ba_batch_solve(b, params, abort_flag);
    const auto t2 = std::chrono::steady_clock::now();
    if (rc == ORBHIP_OK) rc = orbhip_ba_batch_download(b, poses_inout, points_inout, edge_outlier_out, stats_out);
    const auto t3 = std::chrono::steady_clock::now();
    orbhip_ba_batch_destroy(b);
    if (prof) {
        const auto t4 = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::milli>(c - a).count(); };
        fprintf(stderr, "[orbhip ba] one-shot solve of %d graph(s): create %.3f  solve %.3f  download %.3f  destroy %.3f ms\n", n_graphs, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4));
    }
    return rc;
}
