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
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "ba_ldlt.h"
#include "dense_ldlt_big.h"
#include "ba_edges.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <thread>
#include <algorithm>
#include <atomic>

typedef double v4d __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ device structures
// (BaGraphDev, BaCamDev: ba_graph_lists.h, with the host code that fills them)
struct BaState {
    double lambda, ni, current_chi, ini_chi, chi_first, chi_last;
    int pass, iter, qmax, nbad;
    int need_build, need_lambda_init, active, cur;   // cur: which pose/point buffer is current
    int ok;                                          // last LDLT status
    int errors_fresh;                                // the stored errors / chi2 are those of the current estimate (the last trial was accepted)
    int iters_run[2], lm_trials, n_outliers;
    int robust;                                      // 0 after setRobustKernel(0) (merge variant, second pass)
    int apply_levels;                                // set when pass 1 starts: k_ba_levels classifies the edges once
    double rho_dbg;
};

struct BaBatch {      // kernel argument (by value)
    int G, max_edges, max_points, max_nf, max_ld;
    const BaGraphDev *gd;
    const BaCamDev *cams; const int *pose_cam;       // per-keyframe calibration tables ([sum of n_cameras], [sumP]); see BaGraphDev::cam_off
    BaState *st;
    // graph topology
    const int *hidx;            // [sumP]
    const int *edge_pose, *edge_point;   // [sumE] local indices
    const double *edge_obs, *edge_is2;   // [sumE*3], [sumE]
    const uint8_t *edge_stereo;
    // a point seen by the same keyframe in both cameras of a rig has TWO edges to one pose; g2o maps both onto the same
    // Hpl block (they accumulate).  edge_dup[e] = 1: an earlier edge of the same point has the same pose (its Hpl share is
    // added by that first edge); edge_next[e] = the next such edge of the chain or -1.
    const uint8_t *edge_dup;
    const int *edge_next;
    const int *pt_start;        // per graph n_points+1
    const int *pose_start;      // per graph nf+1  (free poses only, by hessian index)
    const int *pose_edges;      // [sumE'] edge ids (graph-local) grouped by free pose
    // static edge data once more in that pose-major order, so that k_ba_build_poses streams it (only the point is a gather)
    const int *pm_point, *pm_task; const uint8_t *pm_type; const double *pm_is2, *pm_obs;
    // estimates, double buffered: buffer b at poses + b*sumP*7
    double *poses, *points;
    int sumP, sumL, sumE, sumF;
    // per-edge
    double *err, *chi2, *rho0;
    // system
    double *Hll, *bl, *Dinv, *db;        // [sumL*6] [sumL*3] [sumL*6] [sumL*3]
    double *Hpp, *bp, *bs;               // [sumF*36] [sumF*6] [sumF*6]
    double *Wsp;                         // [tasks][18] Hpl block of edge_task[e], [b*6 + a] = (J_T^T w Omega J_X)[a][b] (first edge of a twin chain: the sum)
    const int *edge_task;                // [sumE] index of the edge's Hpl block in Wsp / gemm_task (batch-global), -1: fixed pose or later twin
    double *Linv;                        // [sumL*6] rows of C^-1 (lower), D = Hll + lambda I = C C^T: l00 l10 l11 l20 l21 l22
    // Schur GEMM work lists (static): the edges with a free pose and no earlier twin, point-major, cut into stages of
    // <= GEMM_PS points and <= GEMM_STAGE_EDGES edges
    const int4 *gemm_task;               // {graph-local edge, 6*h, point, graph}
    const int4 *gemm_stage;              // per stage {first point, number of points, first task, number of tasks}
    const uint32_t *ptmask;              // [sumL] bit t: the point's Hpl column is non-zero inside columns [16t, 16t+16) (static)
    double *S, *Spart;                   // per graph [ld*ld], [ks][ld*ld]
    double *xp, *xl;                     // [sumF*6], [sumL*3]
    double *scale_pt, *scale_pose;       // partial sums of computeScale
    double *chi, *scale, *maxdiag;       // [G]
    int *n_active;                       // [1]
    uint8_t *outlier;                    // [sumE]
    uint8_t *level;                      // [sumE] 1 = excluded from the optimisation (setLevel(1), merge variant)
    // params
    double delta_m, dsqr_m, delta_s, dsqr_s, gate_m, gate_s, user_lambda, tau;
    int iters[2], max_trials;
    int ex2, nr2;                        // merge variant: exclude first-pass outliers / drop the robust kernel in pass 2
    // landmark-sharded solve (optional single-graph mode): this rank owns a slice of every graph's points and their
    // edges, poses are replicated; partial sums meet in xbuf [world][xcount] (slot r = rank r's payload, filled by the caller's
    // all-gather) and are reduced in rank order on every rank, so all ranks take identical LM decisions.
    int rank, world;
    double *xbuf;
    size_t xcount;
    const int *x1_off, *x2_off;          // [G] payload offsets of exchange 1 (Hpp, bp, chi2, max |Hll diag|) and 2 (sum_ks Spart, W db)
    double *bacc;                        // [sumF*6] sum over this rank's edges of W db (k_ba_bschur)
    int *x_abort;                        // [1] any rank saw the abort flag (exchange 3)
    double *edges_total;                 // [G] number of edges over all ranks (>= 50 % outlier rule)
    // big windows (any graph of the batch with n > BA_LDLT_MAXN): per graph, per pair of free poses i <= j (row-major over the upper
    // triangle) the Hpl blocks of the points both see -- the Schur complement is summed per 6x6 block in a fixed order
    int big;
    int pair_schur;                                          // the Schur complement comes from the pair lists (k_ba_schur_big); always with big
    const int *big_pair_start; const int2 *big_pair_ent; const int *big_pair_pt;      // big_pair_pt: the point of every entry     // entries: {Hpl block of pose i, Hpl block of pose j} (batch-global block ids)
    const int2 *big_pair_jr;                                 // of every entry: {Hpl block of pose j, rank of pose i's block in pose i's own (diagonal) list} (k_ba_schur_rows)
    double *big_y, *big_d, *big_U;                           // [sumF*6] forward-substituted right-hand side, pivots; [G][32*32] unscaled diagonal-block columns
    int *big_fail;                                           // [G] a zero / non-finite pivot was met
};

// The calibration the edges of pose `pi` (local index) of graph G project through: the keyframe's own camera when the graph carries a
// camera table, else the graph's single calibration.  A REFERENCE, not a copy: BaGraphDev's calibration fields (fx ... cam2_model) are
// laid out exactly like a BaCamDev, so both cases are one pointer and a field is loaded where it is used (a 30-double copy per edge
// cost the general build kernel its second wave per SIMD: 232 -> 280 registers)
static_assert(offsetof(BaGraphDev, cam2_model) - offsetof(BaGraphDev, fx) == offsetof(BaCamDev, cam2_model) && offsetof(BaGraphDev, kb) - offsetof(BaGraphDev, fx) == offsetof(BaCamDev, kb) &&
              offsetof(BaGraphDev, Trl) - offsetof(BaGraphDev, fx) == offsetof(BaCamDev, Trl) && offsetof(BaGraphDev, kb2) - offsetof(BaGraphDev, fx) == offsetof(BaCamDev, kb2),
              "BaGraphDev's calibration fields must mirror BaCamDev");
template <bool GENERAL>
__device__ __forceinline__ const BaCamDev &ba_cam_ref(const BaBatch &B, const BaGraphDev &G, int pi)
{
    if (GENERAL && G.cam_off >= 0) return B.cams[G.cam_off + B.pose_cam[G.pose_off + pi]];
    return *reinterpret_cast<const BaCamDev *>(&G.fx);
}

// (SE3 and edge math, B1 - B3: ba_edges.h; Huber, B4: geom3.h)

// ------------------------------------------------------------------ kernels
// which: 0 -> evaluate at the CURRENT estimate for graphs that need a (re)build;
//        1 -> evaluate at the TRIAL estimate for every active graph.
// GENERAL = false: every graph of the batch is Pinhole without second-camera edges and without twin edges (the usual local BA)
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_ba_errors(BaBatch B, int which)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || (which == 0 && (!st.need_build || (st.errors_fresh && B.world == 1)))) return;      // after an accepted trial the stored errors ARE the current ones
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int buf = which == 0 ? st.cur : (st.cur ^ 1);
    const int ge = G.edge_off + e;
    if (B.level[ge]) { B.rho0[ge] = 0; return; }      // not an active edge: its stored error / chi2 stay as last computed
    const double *pose = B.poses + ((size_t)buf * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)buf * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    double P[3], er[3];
    const int type = B.edge_stereo[ge], stereo = type == 1;          // 0 mono, 1 stereo, 2 second camera (ToBody)
    const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, B.edge_pose[ge]);
    if (GENERAL && type == 2) tobody_error(cam, pose, X, B.edge_obs + 3 * (size_t)ge, P, er);
    else edge_error<GENERAL>(cam, pose, X, B.edge_obs + 3 * (size_t)ge, stereo, P, er);
    const double chi2 = (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]) * B.edge_is2[ge];
    double r0, r1;
    if (!st.robust) { r0 = chi2; r1 = 1.; }
    else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
    B.err[3 * (size_t)ge] = er[0]; B.err[3 * (size_t)ge + 1] = er[1]; B.err[3 * (size_t)ge + 2] = er[2];
    B.chi2[ge] = chi2;
    B.rho0[ge] = r0;
}

// Deterministic per-graph sums: chi = sum rho0 over edges (activeRobustChi2, sparse_optimizer.cpp:100-114);
// mode 1 additionally sums computeScale partials (levenberg.cpp:187-194).
__global__ __launch_bounds__(1024) void k_ba_reduce(BaBatch B, int which)
{
    // 1024 threads, four loads in flight per thread, DPP tree per wave, the 16 wave sums added in order: a fixed association (round 1: 256
    // threads walking 78 dependent loads each and an 8-step LDS tree -- 21 us of a single-window LM tick, twice per tick)
    __shared__ double red[16];
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || (which == 0 && (!st.need_build || (st.errors_fresh && B.world == 1)))) return;      // after an accepted trial the stored errors ARE the current ones
    const BaGraphDev &G = B.gd[g];
    auto block_sum = [&](double v) {
        v = wave_sum_f64_dpp(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        double t = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) t += red[w];
        return t;
    };
    {
        const double *r = B.rho0 + G.edge_off;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int e = tid;
        for (; e + 3072 < G.n_edges; e += 4096) { s0 += r[e]; s1 += r[e + 1024]; s2 += r[e + 2048]; s3 += r[e + 3072]; }
        for (; e < G.n_edges; e += 1024) s0 += r[e];
        const double chi = block_sum((s0 + s1) + (s2 + s3));
        if (tid == 0) B.chi[g] = chi;
    }
    if (which == 0 && tid == 0) B.st[g].apply_levels = 0;      // k_ba_levels (earlier in this tick) has consumed it
    if (which == 1) {
        double t = 0;
        for (int l = tid; l < G.n_points; l += 1024) t += B.scale_pt[G.point_off + l];
        if (B.rank == 0) for (int h = tid; h < G.nf; h += 1024) t += B.scale_pose[G.free_off + h];   // replicated: counted once
        const double sc = block_sum(t);
        if (tid == 0) B.scale[g] = sc;
    }
}

// buildSystem, landmark side: 16 lanes per point share its (contiguous) edges -- one edge per lane and trip, so the
// Jacobians of a point's ~10 observations are evaluated side by side and their scattered Hpl writes are in flight
// together; Hll / bl are reduced over the 16 lanes in a fixed (butterfly) order.
// Hll (sym 6), bl, and the edge's Hpl block Wsp[e][6*b + a] = (J_T^T w Omega J_X)[a][b].
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_ba_build_points(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    const int sub = threadIdx.x & 15;
    const int l = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int *ps = B.pt_start + G.ptstart_off;
    if (l >= G.n_points) return;                      // whole 16-lane groups leave together
    const int e0 = ps[l], e1 = ps[l + 1];
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + l) * 3;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // H (6, upper) then b (3)
    for (int e = e0 + sub; e < e1; e += 16) {
        const int ge = G.edge_off + e;
        const int pi = B.edge_pose[ge];
        const int hi = B.hidx[G.pose_off + pi];
        const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + pi) * 7;
        const int type = B.edge_stereo[ge], stereo = type == 1;
        double P[3], R[9], Jx[9], Jt[18];
#pragma unroll
        for (int k = 6; k < 9; k++) Jx[k] = 0;
#pragma unroll
        for (int k = 12; k < 18; k++) Jt[k] = 0;                                     // monocular edge: third row empty
        const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, pi);
        if (GENERAL && type == 2) tobody_jacobians(cam, pose, X, Jx, Jt);
        else {
            quat_rot(pose, X, P);
            P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
            quat_to_R(pose, R);
            edge_jacobians<GENERAL>(cam, P, R, stereo, Jx, Jt);
        }
        const double chi2 = B.chi2[ge];
        double r0, r1;
        if (!st.robust) r1 = 1.;
        else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
        const double w = B.level[ge] ? 0.0 : r1 * B.edge_is2[ge];          // level-1 edge: contributes nothing (its Hpl block is zeroed)
        const double es[3] = {B.err[3 * (size_t)ge], B.err[3 * (size_t)ge + 1], stereo ? B.err[3 * (size_t)ge + 2] : 0.0};
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double j0 = Jx[3 * d], j1 = Jx[3 * d + 1], j2 = Jx[3 * d + 2];
            const double we = -w * es[d];
            acc[6] += j0 * we; acc[7] += j1 * we; acc[8] += j2 * we;
            acc[0] += j0 * w * j0; acc[1] += j0 * w * j1; acc[2] += j0 * w * j2;
            acc[3] += j1 * w * j1; acc[4] += j1 * w * j2; acc[5] += j2 * w * j2;
        }
        if (hi >= 0 && (!GENERAL || !B.edge_dup[ge])) {
            double Wb[18];
#pragma unroll
            for (int bb = 0; bb < 3; bb++)
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    double h = 0;
#pragma unroll
                    for (int d = 0; d < 3; d++) h += Jt[6 * d + a] * w * Jx[3 * d + bb];
                    Wb[6 * bb + a] = h;
                }
            for (int e2 = GENERAL ? B.edge_next[ge] : -1; e2 >= 0; e2 = B.edge_next[G.edge_off + e2]) {      // the same keyframe's other camera (rare)
                const int g2 = G.edge_off + e2;
                const int type2 = B.edge_stereo[g2], st2 = type2 == 1;
                double P2[3], R2[9], Jx2[9], Jt2[18];
                for (int k = 6; k < 9; k++) Jx2[k] = 0;
                for (int k = 12; k < 18; k++) Jt2[k] = 0;
                if (type2 == 2) tobody_jacobians(cam, pose, X, Jx2, Jt2);
                else {
                    quat_rot(pose, X, P2);
                    P2[0] += pose[4]; P2[1] += pose[5]; P2[2] += pose[6];
                    quat_to_R(pose, R2);
                    edge_jacobians(cam, P2, R2, st2, Jx2, Jt2);
                }
                double q0, q1;
                if (!st.robust) q1 = 1.;
                else if (st2) huber(B.chi2[g2], B.delta_s, B.dsqr_s, &q0, &q1); else huber(B.chi2[g2], B.delta_m, B.dsqr_m, &q0, &q1);
                const double w2 = B.level[g2] ? 0.0 : q1 * B.edge_is2[g2];
                for (int bb = 0; bb < 3; bb++)
                    for (int a = 0; a < 6; a++) {
                        double h = 0;
                        for (int d = 0; d < 3; d++) h += Jt2[6 * d + a] * w2 * Jx2[3 * d + bb];
                        Wb[6 * bb + a] += h;
                    }
            }
            // (round 4: parking the blocks of a workgroup's 16 points in LDS and writing the contiguous range out with consecutive lanes on
            // consecutive 16 bytes was SLOWER: 0.55 against 0.42 ms per 256 windows -- two more barriers and the LDS round trip)
            double *wo = B.Wsp + (size_t)B.edge_task[ge] * 18;
#pragma unroll
            for (int k = 0; k < 18; k++) wo[k] = Wb[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        acc[k] = row16_allreduce_f64_dpp(acc[k]);          // the point's 16 lanes = one DPP row
    }
    if (sub == 0) {
        double *Ho = B.Hll + (size_t)(G.point_off + l) * 6, *bo = B.bl + (size_t)(G.point_off + l) * 3;
#pragma unroll
        for (int i = 0; i < 6; i++) Ho[i] = acc[i];
        bo[0] = acc[6]; bo[1] = acc[7]; bo[2] = acc[8];
    }
}

// buildSystem, pose side: one wave per free pose over its edges (pose-major list).
template <bool GENERAL>
__global__ __launch_bounds__(64) void k_ba_build_poses(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    const int h = blockIdx.x;
    if (h >= G.nf) return;
    const int lane = threadIdx.x;
    const int *qs = B.pose_start + G.posestart_off;
    const int *pe = B.pose_edges + G.edge_off;
    double acc[27];
    for (int i = 0; i < 27; i++) acc[i] = 0;
    // every edge of this list has the same pose; the edge's error / chi2 are recomputed from the pose-major copy of its static data
    // (bit-identical to k_ba_errors: same inputs, same code) instead of being gathered from the point-major arrays
    const int pose_i = qs[h] < qs[h + 1] ? B.edge_pose[G.edge_off + pe[qs[h]]] : 0;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + pose_i) * 7;
    const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, pose_i);
    for (int k = qs[h] + lane; k < qs[h + 1]; k += 64) {
        const size_t gk = (size_t)G.edge_off + k;
        const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.pm_point[gk]) * 3;
        const int type = B.pm_type[gk], stereo = type == 1;
        double P[3], R[9], Jx[9], Jt[18], es[3];
#pragma unroll
        for (int q = 12; q < 18; q++) Jt[q] = 0;                  // monocular edge: third row empty (the loops below run all 3 rows)
        if (GENERAL && type == 2) { tobody_error(cam, pose, X, B.pm_obs + 3 * gk, P, es); tobody_jacobians(cam, pose, X, Jx, Jt); }
        else {
            edge_error<GENERAL>(cam, pose, X, B.pm_obs + 3 * gk, stereo, P, es);
            quat_to_R(pose, R);
            edge_jacobians<GENERAL>(cam, P, R, stereo, Jx, Jt);
        }
        const double is2 = B.pm_is2[gk];
        const double chi2 = (es[0] * es[0] + es[1] * es[1] + es[2] * es[2]) * is2;
        double r0, r1;
        if (!st.robust) r1 = 1.;
        else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
        const double w = (B.ex2 && B.level[G.edge_off + pe[k]]) ? 0.0 : r1 * is2;      // levels exist only in the merge variant
#pragma unroll
        for (int d = 0; d < 3; d++) {                             // compile-time indices: acc stays in registers
            const double we = -w * es[d];
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double ja = Jt[6 * d + a];
                acc[21 + a] += ja * we;
#pragma unroll
                for (int bb = a; bb < 6; bb++) acc[idx++] += ja * w * Jt[6 * d + bb];
            }
        }
    }
    for (int i = 0; i < 27; i++) {
        double v = acc[i];
        v = wave_sum_f64_dpp(v);
        acc[i] = v;
    }
    if (lane == 0) {
        double *Hp = B.Hpp + (size_t)(G.free_off + h) * 36;
        int idx = 0;
        for (int a = 0; a < 6; a++)
            for (int bb = a; bb < 6; bb++) { Hp[6 * a + bb] = acc[idx]; Hp[6 * bb + a] = acc[idx]; idx++; }
        for (int a = 0; a < 6; a++) B.bp[(size_t)(G.free_off + h) * 6 + a] = acc[21 + a];
    }
}

// computeLambdaInit (levenberg.cpp:171-185): max |diag| over pose and landmark blocks
__global__ __launch_bounds__(256) void k_ba_maxdiag(BaBatch B)
{
    __shared__ double red[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build || !st.need_lambda_init) return;
    const BaGraphDev &G = B.gd[g];
    const int *ps = B.pt_start + G.ptstart_off;
    double m = 0;
    if (B.world == 1)                                   // sharded: Hpp is still a partial sum here (k_ba_shard_sum1 finishes the max)
        for (int h = tid; h < G.nf; h += 256)
            for (int a = 0; a < 6; a++) m = fmax(m, fabs(B.Hpp[(size_t)(G.free_off + h) * 36 + 7 * a]));
    for (int l = tid; l < G.n_points; l += 256)
        if (ps[l + 1] > ps[l]) {
            const double *H = B.Hll + (size_t)(G.point_off + l) * 6;
            m = fmax(m, fmax(fabs(H[0]), fmax(fabs(H[3]), fabs(H[5]))));
        }
    red[tid] = m;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (tid < d) red[tid] = fmax(red[tid], red[tid + d]); __syncthreads(); }
    if (tid == 0) B.maxdiag[g] = red[0];
}

// start of an outer LM iteration (levenberg.cpp:71-92) for graphs that just (re)built
__global__ void k_ba_pretrial(BaBatch B)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B.G) return;
    BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    st.current_chi = B.chi[g];
    st.ini_chi = st.current_chi;
    if (st.chi_first < 0) st.chi_first = st.current_chi;
    if (st.need_lambda_init) {
        st.lambda = B.user_lambda > 0 ? B.user_lambda : B.tau * B.maxdiag[g];
        st.ni = 2; st.nbad = 0;
        st.need_lambda_init = 0;
    }
    st.qmax = 0;
    st.need_build = 0;
}

// per trial: D = Hll + lambda I, D^-1 (symmetric), db = D^-1 bl   (block_solver.hpp:395-404)
__global__ __launch_bounds__(256) void k_ba_point_prep(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= G.n_points) return;
    const int *ps = B.pt_start + G.ptstart_off;
    double *Di = B.Dinv + (size_t)(G.point_off + l) * 6, *db = B.db + (size_t)(G.point_off + l) * 3;
    if (ps[l + 1] == ps[l]) { for (int i = 0; i < 6; i++) { Di[i] = 0; B.Linv[(size_t)(G.point_off + l) * 6 + i] = 0; } db[0] = db[1] = db[2] = 0; return; }
    const double *H = B.Hll + (size_t)(G.point_off + l) * 6;
    const double a00 = H[0] + st.lambda, a01 = H[1], a02 = H[2], a11 = H[3] + st.lambda, a12 = H[4], a22 = H[5] + st.lambda;
    const double c0 = a11 * a22 - a12 * a12, c1 = a12 * a02 - a01 * a22, c2 = a01 * a12 - a11 * a02;
    const double id = 1.0 / (a00 * c0 + a01 * c1 + a02 * c2);
    const double i00 = c0 * id, i01 = c1 * id, i02 = c2 * id;
    const double i11 = (a00 * a22 - a02 * a02) * id, i12 = (a02 * a01 - a00 * a12) * id, i22 = (a00 * a11 - a01 * a01) * id;
    Di[0] = i00; Di[1] = i01; Di[2] = i02; Di[3] = i11; Di[4] = i12; Di[5] = i22;
    {   // D = C C^T (Cholesky), Linv = C^-1: the Schur GEMM multiplies Z = C^-1 W, so that W^T D^-1 W = Z^T Z
        const double c00 = sqrt(a00), l00 = 1.0 / c00;
        const double c10 = a01 * l00, c20 = a02 * l00;
        const double c11 = sqrt(a11 - c10 * c10), l11 = 1.0 / c11;
        const double c21 = (a12 - c20 * c10) * l11;
        const double c22 = sqrt(a22 - c20 * c20 - c21 * c21), l22 = 1.0 / c22;
        const double l10 = -c10 * l00 * l11, l21 = -c21 * l11 * l22, l20 = -(l21 * c10 + l22 * c20) * l00;
        double *Lo = B.Linv + (size_t)(G.point_off + l) * 6;
        Lo[0] = l00; Lo[1] = l10; Lo[2] = l11; Lo[3] = l20; Lo[4] = l21; Lo[5] = l22;
    }
    const double *b = B.bl + (size_t)(G.point_off + l) * 3;
    db[0] = i00 * b[0] + i01 * b[1] + i02 * b[2];
    db[1] = i01 * b[0] + i11 * b[1] + i12 * b[2];
    db[2] = i02 * b[0] + i12 * b[1] + i22 * b[2];
}

// Schur GEMM on the FP64 matrix cores:  S_sub = W^T D^-1 W = Z^T Z  with  Z = C^-1 W,  D = C C^T  (k_ba_point_prep), over the
// K-padded dense panel Z[4l+b][c] (K = 4 per point: 3 + pad), v_mfma_f64_16x16x4_f64:
//   A[i][k] (lane i=l&15,k=l>>4), B[k][j] (lane j=l&15,k=l>>4), C/D 4 regs: col = l&15, row = (l>>4) + 4*reg.
// One 512-thread workgroup (8 waves, up to 256 VGPRs each) owns a range of STAGES (<= GEMM_PS points, <= GEMM_STAGE_EDGES Hpl
// blocks) of one graph.  The dense panel exists only in LDS: per stage every thread fetches ONE column of ONE sparse Hpl block
// (3 doubles of Wsp, loaded a stage ahead into registers), multiplies it by the point's C^-1 and scatters it into the cleared stage
// buffer -- HBM sees the 144-byte blocks (0.7 GB per 256 graphs) instead of a 79 %-zero dense panel (3.5 GB), and both MFMA
// fragments come straight from the same LDS panel (no D^-1 arithmetic between load and MFMA).  The upper 16x16 output tiles stay
// in accumulator registers for the whole launch.
// Tile ownership: every row strip of the upper triangle is cut into CHUNKS of GEMM_C consecutive tiles; chunk i belongs to wave
// i % 8, slot i / 8 (GEMM_NCH slots per wave).  Block sparsity: a point is seen by ~10 of ~48 free keyframes; which (point, chunk,
// tile) combinations of a stage hold data is decided once per stage by all 64 lanes (lane = 8*point + chunk) and three ballots;
// a hit chunk loads its A fragment and GEMM_C B fragments back to back and issues the MFMAs of its non-empty tiles.
// LDS rows are padded to ld+16 doubles so that the K-rows of a fragment fall into different bank halves.
// (GEMM_PS, GEMM_C, GEMM_NCH, GEMM_WAVES, GEMM_LDS_PAD, GEMM_STAGE_EDGES, GEMM_TARGET_WGS, GEMM_PANEL_LDS_BYTES and gemm_strip_chunks: ba_graph_lists.h,
// with the host code that cuts the stages by them)
#define GEMM_LDS_TAIL 32       // a short chunk reads up to GEMM_C-1 tiles past the end of a row (never multiplied)
static_assert(GEMM_PS * GEMM_NCH <= 64 && GEMM_NCH * GEMM_C <= 32, "one lane per (stage point, chunk); one valid bit per tile");
static_assert(6 * GEMM_STAGE_EDGES <= 64 * GEMM_WAVES && 6 * GEMM_PS <= 64 * GEMM_WAVES, "one column task per thread");
__global__ __launch_bounds__(64 * GEMM_WAVES) void k_ba_schur_gemm(BaBatch B)
{
    extern __shared__ double glds[];               // [2][gemm_ps][3][ld + pad] Z rows of the stage, double buffered (+ tail)
    __shared__ __attribute__((aligned(16))) double s_raw[2][GEMM_STAGE_EDGES * 18];   // the stage's Hpl blocks as they lie in Wsp
    __shared__ __attribute__((aligned(16))) int4 s_task[2][GEMM_STAGE_EDGES];
    __shared__ __attribute__((aligned(16))) double s_linv[2][GEMM_PS][6];
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[3][GEMM_PS];
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nt = G.nt16;
    if ((int)blockIdx.x >= G.ks * G.ngrp) return;
    const int ksi = blockIdx.x / G.ngrp, grp = blockIdx.x - ksi * G.ngrp;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const int ld = G.ld, ldp = ld + GEMM_LDS_PAD;
    // this wave's chunks: offsets of the row tile / first column tile inside an LDS row (wave-uniform -> scalar registers)
    int aoff[GEMM_NCH], boffc[GEMM_NCH];
    uint32_t cvalid = 0;                                 // tiles that exist: bit c*GEMM_C + j
    v4d acc[GEMM_NCH * GEMM_C];
#pragma unroll
    for (int c = 0; c < GEMM_NCH; c++) {
        int id = (grp * GEMM_NCH + c) * GEMM_WAVES + wv, tr = 0;
        while (tr < nt && id >= gemm_strip_chunks(nt, tr)) { id -= gemm_strip_chunks(nt, tr); tr++; }
        if (tr < nt) {
            const int tc = tr + id * GEMM_C, len = min(GEMM_C, nt - tc);
            aoff[c] = 16 * tr; boffc[c] = 16 * tc; cvalid |= ((1u << len) - 1u) << (c * GEMM_C);
        } else { aoff[c] = 0; boffc[c] = 0; }
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) acc[c * GEMM_C + j] = (v4d){0, 0, 0, 0};
    }
    // the same table per LANE for the once-per-stage hit evaluation: lane = 8*point + chunk decides (point, chunk) for all
    // GEMM_PS x GEMM_NCH = 64 combinations at once; the ballots replace ~20 scalar instructions per (point, chunk)
    uint32_t lrow = 0, lcolbit[GEMM_C];
    {
        const int c = lane % GEMM_NCH;
        int id = (grp * GEMM_NCH + c) * GEMM_WAVES + wv, tr = 0;
        while (tr < nt && id >= gemm_strip_chunks(nt, tr)) { id -= gemm_strip_chunks(nt, tr); tr++; }
        const int tc = tr + id * GEMM_C;
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) lcolbit[j] = (tr < nt && tc + j < nt) ? 1u << (tc + j) : 0u;
        if (tr < nt) lrow = 1u << tr;
    }
    const int per = (G.n_stages + G.ks - 1) / G.ks;
    const int sb = ksi * per, se = min(G.n_stages, sb + per);
    const int4 *stg = B.gemm_stage + G.stage_off;          // {first point, points, first task, tasks}
    const int4 *tsk = B.gemm_task + G.gemm_off;            // {edge, 6*h, point, -}
    const double live = lk < 3 ? 1.0 : 0.0;                // K-row 3 is the pad: A is zero there, B re-reads row 2 (finite)
    const int boff = min(lk, 2) * ldp + li;
    const size_t stage_doubles = (size_t)G.gemm_ps * 3 * ldp;
    // stage s -> LDS by asynchronous global -> LDS copies (no staging registers): its Hpl blocks (contiguous in Wsp), task
    // descriptors, C^-1 rows and occupancy masks; issued two stages ahead of the multiply
    auto dma16 = [&](const void *src, void *dst, int bytes) {          // wave-strided 1-KiB pieces, 16 B per lane
        for (int piece = wv; piece * 1024 < bytes; piece += GEMM_WAVES)
            if (piece * 1024 + lane * 16 < bytes)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)src + piece * 1024 + lane * 16),
                                                 (__attribute__((address_space(3))) void *)((char *)dst + piece * 1024), 16, 0, 0);
    };
    auto load_stage = [&](int s) {
        const int4 sd = stg[s];
        const int b2 = s & 1;
        dma16(B.Wsp + (size_t)(G.gemm_off + sd.z) * 18, &s_raw[b2][0], sd.w * 144);
        dma16(tsk + sd.z, &s_task[b2][0], sd.w * 16);
        if (wv == 0) {
            if (lane * 16 < sd.y * 48)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)(B.Linv + (size_t)(G.point_off + sd.x) * 6) + lane * 16),
                                                 (__attribute__((address_space(3))) void *)&s_linv[b2][0][0], 16, 0, 0);
        } else if (wv == 1) {
            if (lane < sd.y)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(B.ptmask + G.point_off + sd.x + lane),
                                                 (__attribute__((address_space(3))) void *)&s_mask[s % 3][0], 4, 0, 0);
        }
    };
    auto clear = [&](int buf) {                            // the stage buffer starts from zero
        double2 *z = reinterpret_cast<double2 *>(glds + buf * stage_doubles);
        for (int i = tid; i < (int)(stage_doubles / 2); i += 64 * GEMM_WAVES) z[i] = make_double2(0.0, 0.0);
    };
    auto scatter = [&](int s, int buf) {                   // Z = C^-1 W, one column of one block per thread
        const int b2 = s & 1, ntask = stg[s].w, pt0 = stg[s].x;
        if (tid < 6 * ntask) {
            const int i = tid / 6, a = tid - 6 * i;
            const int4 t = s_task[b2][i];
            const double *w = &s_raw[b2][18 * i + a];
            const double w0 = w[0], w1 = w[6], w2 = w[12];
            const int wp = t.z - pt0;
            const double *L = s_linv[b2][wp];
            double *dst = glds + buf * stage_doubles + (size_t)wp * 3 * ldp + t.y + a;
            dst[0] = L[0] * w0;
            dst[ldp] = L[1] * w0 + L[2] * w1;
            dst[2 * ldp] = L[3] * w0 + L[4] * w1 + L[5] * w2;
        }
    };
    if (sb < se) {
        load_stage(sb);
        if (sb + 1 < se) load_stage(sb + 1);
        clear(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        scatter(sb, 0);
    }
    int cur = 0;
    for (int s = sb; s < se; s++, cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's copies of stage s+1 have landed
        __syncthreads();                                    // stage s is scattered; everyone is done with the other buffer and has its copies
        if (s + 1 < se) clear(cur ^ 1);
        __syncthreads();
        if (s + 1 < se) { scatter(s + 1, cur ^ 1); }
        if (s + 2 < se) load_stage(s + 2);                  // reuses the raw / task / C^-1 slots of stage s (scattered one iteration ago)
        const int np = stg[s].y;
        const double *stage = glds + cur * stage_doubles;
        // which (point, chunk, tile) combinations of this stage hold data: one evaluation per lane, GEMM_C ballots
        unsigned long long hit[GEMM_C];
        {
            const int pl = lane / GEMM_NCH;
            const uint32_t m = pl < np ? s_mask[s % 3][pl] : 0u;
            const bool rh = (m & lrow) != 0;
#pragma unroll
            for (int j = 0; j < GEMM_C; j++) hit[j] = __ballot(rh && (m & lcolbit[j]));
        }
        for (int p = 0; p < np; p++) {
            uint32_t tj[GEMM_C], any = 0;
#pragma unroll
            for (int j = 0; j < GEMM_C; j++) { tj[j] = (uint32_t)(hit[j] >> (GEMM_NCH * p)) & ((1u << GEMM_NCH) - 1u); any |= tj[j]; }
            if (any == 0) continue;                         // the point touches none of this wave's chunks
            const double *rows = stage + (size_t)p * 3 * ldp + boff;
#pragma unroll
            for (int c = 0; c < GEMM_NCH; c++) {
                if (any & (1u << c)) {
                    const double az = rows[aoff[c]];
                    double bf[GEMM_C];
#pragma unroll
                    for (int j = 0; j < GEMM_C; j++) bf[j] = rows[boffc[c] + 16 * j];   // tiles past nt: pad garbage, never multiplied
                    __builtin_amdgcn_sched_barrier(0);          // all 1 + GEMM_C LDS reads in flight before the first wait
                    const double a = live * az;
#pragma unroll
                    for (int j = 0; j < GEMM_C; j++)
                        if (tj[j] & (1u << c))                  // the fragments are already in registers: an empty tile costs one scalar test
                            acc[c * GEMM_C + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bf[j], acc[c * GEMM_C + j], 0, 0, 0);
                }
            }
        }
    }
    double *Sp = B.Spart + G.spart_off + (size_t)ksi * ld * ld;
#pragma unroll
    for (int c = 0; c < GEMM_NCH; c++) {
#pragma unroll
        for (int j = 0; j < GEMM_C; j++) {
            if ((cvalid >> (c * GEMM_C + j)) & 1u) {
#pragma unroll
                for (int r = 0; r < 4; r++) Sp[(size_t)(aoff[c] + lk + 4 * r) * ld + boffc[c] + 16 * j + li] = acc[c * GEMM_C + j][r];
            }
        }
    }
}

// S = blockdiag(Hpp + lambda I) - sum_ks Spart (mirrored from the upper tiles); padding rows -> identity
__global__ __launch_bounds__(256) void k_ba_schur_finish(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.ld * G.ld) return;
    const int r = idx / G.ld, c = idx - r * G.ld;
    double v = 0;
    if (r >= G.n || c >= G.n) v = (r == c) ? 1.0 : 0.0;
    else {
        if (r / 6 == c / 6) v = B.Hpp[(size_t)(G.free_off + r / 6) * 36 + (r % 6) * 6 + (c % 6)] + (r == c ? st.lambda : 0.0);
        const int ur = (r / 16 <= c / 16) ? r : c, uc = (r / 16 <= c / 16) ? c : r;   // upper-tile source
        double s = 0;
        if (B.world == 1) {
            const double *Sp = B.Spart + G.spart_off + (size_t)ur * G.ld + uc;
            for (int k = 0; k < G.ks; k++) s += Sp[(size_t)k * G.ld * G.ld];
        } else {
            const double *X = B.xbuf + B.x2_off[g] + (size_t)ur * G.ld + uc;          // every rank's sum_ks Spart, rank order
            for (int r = 0; r < B.world; r++) s += X[(size_t)r * B.xcount];
        }
        v -= s;
    }
    B.S[G.s_off + idx] = v;
}

// bs = bp - sum_{edges of pose} W_e * db_point   (block_solver.hpp:409-416,435-438), one wave per free pose
__global__ __launch_bounds__(64) void k_ba_bschur(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int h = blockIdx.x;
    if (h >= G.nf) return;
    const int lane = threadIdx.x;
    const int *qs = B.pose_start + G.posestart_off;
    const int *pe = B.pose_edges + G.edge_off;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = qs[h] + lane; k < qs[h + 1]; k += 64) {
        const int task = B.pm_task[(size_t)G.edge_off + k];                // pose-major copies: only the block and db are gathers
        if (task < 0) continue;                                            // one Hpl block per (point, pose)
        const int l = B.pm_point[(size_t)G.edge_off + k];
        const double *db = B.db + (size_t)(G.point_off + l) * 3;
        const double *w = B.Wsp + (size_t)task * 18;
        for (int a = 0; a < 6; a++) acc[a] += w[a] * db[0] + w[6 + a] * db[1] + w[12 + a] * db[2];
    }
    for (int a = 0; a < 6; a++) {
        double v = acc[a];
        v = wave_sum_f64_dpp(v);
        acc[a] = v;
    }
    if (lane == 0)
        for (int a = 0; a < 6; a++) {
            B.bacc[(size_t)(G.free_off + h) * 6 + a] = acc[a];
            B.bs[(size_t)(G.free_off + h) * 6 + a] = B.bp[(size_t)(G.free_off + h) * 6 + a] - acc[a];      // sharded: redone by k_ba_shard_sum2
        }
}

__global__ __launch_bounds__(1024) void k_ba_ldlt(BaBatch B)
{
    const int g = blockIdx.x;
    BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const bool ok = ldlt_solve_wg(B.S + G.s_off, G.ld, G.n, B.bs + (size_t)G.free_off * 6, B.xp + (size_t)G.free_off * 6, B.max_ld);
    if (threadIdx.x == 0) st.ok = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Windows with more than 80 free keyframes (n = 6 nf > BA_LDLT_MAXN; the reference has no cap: Optimizer.cc:1703-1819 takes
// every covisible keyframe, the merge variant :6255 two whole neighbourhoods).  The reduced system no longer fits the
// single-workgroup kernels, so it is built and factored in global memory by many workgroups:
//   k_ba_schur_big      S_ij = sum over the points seen by free poses i and j of W_i D^-1 W_j^T, one wave per 6x6 block pair,
//                       fixed summation order (block_solver.hpp:381-432 restated per output block)
//   k_ba_big_diag / _rows / _trail   right-looking blocked LDL^T, 32-column panels: diagonal block (one wave), the rows below
//                       (one row per thread, many workgroups), rank-32 trailing update (64x64 tiles, many workgroups)
//   k_ba_big_backsub    D^-1, L^T x = y
// The stages' bodies are dense_ldlt_big.h's, shared with the pose graphs; the kernels here pick the window by blockIdx, skip an inactive
// one and hand its pointers over.  The arithmetic per entry is the LDS-panel kernel's (same ldlt_rows), so small and big windows factor alike.
// LPP = lanes per pair: 16 (four pairs per wave; batches) or 64 (one pair per wave: with a handful of windows the chip is empty and the
// per-pair chain -- entries / lanes dependent gather rounds -- is what a tick waits for)
template <int LPP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ba_schur_big(BaBatch B, int nblk)
{
    constexpr int PPW = 64 / LPP;                                  // pairs per wave
    // FOUR block pairs per wave, 16 lanes each: the 36 sums of a pair are reduced inside its 16-lane DPP row (4 rotate-add steps
    // instead of 6 scan steps + a readlane over the wave) and four pairs share the issue slots -- 2.6x fewer instructions per pair
    // than one wave per pair, which made this kernel faster than the MFMA panel GEMM for every batch size.
    // blockIdx -> (graph, block of 4 pairs): all blocks of a graph run on ONE XCD (workgroups are dealt round-robin over the 8 XCDs), one
    // graph after the other per XCD, so that the graph's Hpl blocks (2.9 MB at 50 x 2000 x 10; every block is read ~11 times, once per
    // pair it belongs to) stay in that XCD's 4 MB L2 instead of being fetched again from HBM
    int g, blk;
    if (B.G >= 8) { const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3; g = xcd + 8 * (slot / nblk); blk = slot - (slot / nblk) * nblk; }
    else { g = blockIdx.x / nblk; blk = blockIdx.x - g * nblk; }               // few graphs: every graph over the whole chip
    if (g >= B.G) return;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nf = G.nf;
    const int lane = threadIdx.x, sub = lane & (LPP - 1);
    const int pair = blk * PPW + lane / LPP;
    if (pair >= nf * (nf + 1) / 2) return;                          // whole rows leave together (row-local DPP below)
    int i = 0, bp = pair;
    while (bp >= nf - i) { bp -= nf - i; i++; }
    const int j = i + bp;
    const int *ps = B.big_pair_start + G.pair_off + pair;
    const int2 *ent = B.big_pair_ent + G.pent_off;
    const int *entl = B.big_pair_pt + G.pent_off;
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0.0;
    // the list entry (two block indices + point) of the NEXT trip is fetched a trip ahead: index load and block gathers are two dependent
    // L2 round trips, this takes the first one off the chain
    const int e_end = ps[1];
    int en = ps[0] + sub;
    int2 tn = make_int2(0, 0); int ln = 0;
    if (en < e_end) { tn = ent[en]; ln = entl[en]; }
    for (int e = en; e < e_end; e += LPP) {
        const int2 t = tn;
        const int l = ln;
        if (e + LPP < e_end) { tn = ent[e + LPP]; ln = entl[e + LPP]; }
        const double *Di = B.Dinv + (size_t)(G.point_off + l) * 6;       // (Hll + lambda I)^-1, upper triangle
        const double i00 = Di[0], i01 = Di[1], i02 = Di[2], i11 = Di[3], i12 = Di[4], i22 = Di[5];
        const double *wa = B.Wsp + (size_t)t.x * 18, *wb = B.Wsp + (size_t)t.y * 18;
        double y0[6], y1[6], y2[6];                                     // Y = W_a D^-1 (block_solver.hpp:398-407), then acc += Y W_b^T
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double a0 = wa[a], a1 = wa[6 + a], a2 = wa[12 + a];
            y0[a] = a0 * i00 + a1 * i01 + a2 * i02;
            y1[a] = a0 * i01 + a1 * i11 + a2 * i12;
            y2[a] = a0 * i02 + a1 * i12 + a2 * i22;
        }
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double b0 = wb[c], b1 = wb[6 + c], b2 = wb[12 + c];
#pragma unroll
            for (int r = 0; r < 6; r++) acc[6 * r + c] += y0[r] * b0 + y1[r] * b1 + y2[r] * b2;
        }
    }
    // the finished block goes straight into S = blockdiag(Hpp + lambda I) - sum, both triangles (no partial-sum buffer, no finish
    // kernel on this path; rows / columns >= n of the padded matrix are never read by the factorisations)
    double *S = B.S + G.s_off;
    const double lambda = st.lambda;
    const double *Hd = B.Hpp + (size_t)(G.free_off + i) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) {
        const double v = LPP == 16 ? row16_allreduce_f64_dpp(acc[k]) : wave_sum_f64_dpp(acc[k]);      // every lane of the group holds the sum
        if (sub == 0) {
            const int r = k / 6, c = k - 6 * r;
            const double out = (i == j ? Hd[k] + (r == c ? lambda : 0.0) : 0.0) - v;
            S[(size_t)(6 * i + r) * G.ld + 6 * j + c] = out;
            if (i != j) S[(size_t)(6 * j + c) * G.ld + 6 * i + r] = out;
        }
    }
    // bs = bp - W D^-1 b_l (block_solver.hpp:409-416, 435-438): the diagonal pair lists every Hpl block of pose i exactly once; a second,
    // short pass over it (its blocks are in L2 now) -- inside the loop above the extra branch and registers cost more than they saved
    if (i == j) {
        double wdb[6] = {0, 0, 0, 0, 0, 0};
        for (int e = ps[0] + sub; e < ps[1]; e += LPP) {
            const double *w = B.Wsp + (size_t)ent[e].x * 18, *db = B.db + (size_t)(G.point_off + entl[e]) * 3;
            const double d0 = db[0], d1 = db[1], d2 = db[2];
#pragma unroll
            for (int a = 0; a < 6; a++) wdb[a] += w[a] * d0 + w[6 + a] * d1 + w[12 + a] * d2;
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double v = LPP == 16 ? row16_allreduce_f64_dpp(wdb[a]) : wave_sum_f64_dpp(wdb[a]);
            if (sub == 0) { B.bacc[(size_t)(G.free_off + i) * 6 + a] = v; B.bs[(size_t)(G.free_off + i) * 6 + a] = B.bp[(size_t)(G.free_off + i) * 6 + a] - v; }
        }
    }
}

// The same sums, one 256-thread workgroup per ROW i of the block matrix (round 3).  k_ba_schur_big gathers, per list entry, BOTH Hpl blocks
// and the point's D^-1 from L2: 5-6 cache lines for 162 multiply-adds, 9 GB per launch at 256 windows, and the gather path (one line per
// lane per load instruction) is what the kernel waits for.  All pairs (i, j >= i) share pose i's side: the workgroup computes
// Y_il = W_il D_l^-1 for every block of pose i ONCE into LDS (the diagonal pair's list enumerates them in point order; an entry carries
// the rank of its i-side block in that list), then its sixteen 16-lane groups take the pairs of the row round-robin and gather only W_jl:
// 2 lines per entry, a third of the multiply-adds gone.  Expressions and summation order are k_ba_schur_big<16>'s, so the two kernels
// agree bit for bit on every off-diagonal block (the diagonal blocks and bs are summed in another association, see below).  Rows are dealt
// like the pairs were: a graph's rows on one XCD, longest rows first.
#define SROW_THREADS 384                              // 6 waves: 170 VGPRs each at 3 waves per SIMD, two workgroups per CU while a row is <= 500 blocks
#define SROW_GROUPS (SROW_THREADS / 16)
#define SROW_MAX_BLOCKS 1024                          // 147 KB of LDS; batches with a fuller row keep k_ba_schur_big
__global__ __launch_bounds__(SROW_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_ba_schur_rows(BaBatch B, int max_nf)
{
    extern __shared__ __attribute__((aligned(16))) double srow_y[];          // [blocks of pose i][18]: y0[6] y1[6] y2[6]
    __shared__ double s_part[SROW_GROUPS * 27];                              // the diagonal block's and W db's partial sums, one set per 16-lane group
    __shared__ int s_next;                                                   // next pair of the row nobody has taken
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int g = xcd + 8 * (slot / max_nf), i = slot - (slot / max_nf) * max_nf;
    if (g >= B.G) return;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int nf = G.nf;
    if (i >= nf) return;
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const int *ps = B.big_pair_start + G.pair_off + (i * nf - i * (i - 1) / 2);      // pairs (i, i), (i, i + 1), ...
    const int2 *ent = B.big_pair_ent + G.pent_off;
    const int *entl = B.big_pair_pt + G.pent_off;
    const int2 *entjr = B.big_pair_jr + G.pent_off;
    if (tid == 0) s_next = i + 1 + SROW_GROUPS;
    // ---- pose i's own blocks, one per thread: Y into LDS, and the diagonal pair (i, i) on the way -- its list IS this enumeration, and as
    // one 16-lane group's chain (400 entries at 50 x 2000 x 10) it would outlast every other pair of the row by a factor of five while the
    // workgroup holds its LDS.  S_ii and bs = bp - W D^-1 b_l are summed per thread, per 16-lane group (DPP), then over the groups in order.
    {
        const int d0 = ps[0], nblk = ps[1] - d0;
        double dacc[21], wdb[6];                       // S_ii is symmetric: its lower triangle, row-major
#pragma unroll
        for (int k = 0; k < 21; k++) dacc[k] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) wdb[a] = 0.0;
        for (int p = tid; p < nblk; p += SROW_THREADS) {
            const int l = entl[d0 + p];
            const double *Di = B.Dinv + (size_t)(G.point_off + l) * 6, *db = B.db + (size_t)(G.point_off + l) * 3;
            const double i00 = Di[0], i01 = Di[1], i02 = Di[2], i11 = Di[3], i12 = Di[4], i22 = Di[5];
            const double d0b = db[0], d1b = db[1], d2b = db[2];
            const double2 *wa2 = reinterpret_cast<const double2 *>(B.Wsp + (size_t)ent[d0 + p].x * 18);       // 144-byte blocks: 16-byte aligned
            double wa[18], y0[6], y1[6], y2[6];
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 v = wa2[k]; wa[2 * k] = v.x; wa[2 * k + 1] = v.y; }
            double *y = srow_y + 18 * p;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double a0 = wa[a], a1 = wa[6 + a], a2 = wa[12 + a];
                y0[a] = a0 * i00 + a1 * i01 + a2 * i02;
                y1[a] = a0 * i01 + a1 * i11 + a2 * i12;
                y2[a] = a0 * i02 + a1 * i12 + a2 * i22;
                y[a] = y0[a]; y[6 + a] = y1[a]; y[12 + a] = y2[a];
                wdb[a] += a0 * d0b + a1 * d1b + a2 * d2b;
            }
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c <= r; c++) dacc[r * (r + 1) / 2 + c] += y0[r] * wa[c] + y1[r] * wa[6 + c] + y2[r] * wa[12 + c];
        }
#pragma unroll
        for (int k = 0; k < 21; k++) { const double v = row16_allreduce_f64_dpp(dacc[k]); if (sub == 0) s_part[27 * grp + k] = v; }
#pragma unroll
        for (int a = 0; a < 6; a++) { const double v = row16_allreduce_f64_dpp(wdb[a]); if (sub == 0) s_part[27 * grp + 21 + a] = v; }
    }
    __syncthreads();
    double *S = B.S + G.s_off;
    if (tid < 27) {
        double v = 0.0;
        for (int q = 0; q < SROW_GROUPS; q++) v += s_part[27 * q + tid];
        if (tid < 21) {
            int r = 0, c = tid;
            while (c > r) { c -= r + 1; r++; }
            const double out = B.Hpp[(size_t)(G.free_off + i) * 36 + 6 * r + c] + (r == c ? st.lambda : 0.0) - v;
            S[(size_t)(6 * i + r) * G.ld + 6 * i + c] = out;
            S[(size_t)(6 * i + c) * G.ld + 6 * i + r] = out;
        } else {
            const size_t o = (size_t)(G.free_off + i) * 6 + tid - 21;
            B.bacc[o] = v; B.bs[o] = B.bp[o] - v;
        }
    }
    // ---- the pairs (i, j > i), handed out dynamically (list lengths differ by an order of magnitude): the first one per group by index, then
    // from the counter
    for (int j = i + 1 + grp; j < nf; j = row16_allreduce_add_dpp(sub == 0 ? atomicAdd(&s_next, 1) : 0)) {
        const int e0 = ps[j - i], e_end = ps[j - i + 1];
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; k++) acc[k] = 0.0;
        const int en = e0 + sub;                                       // the NEXT trip's list entry is fetched a trip ahead
        int2 tn = make_int2(0, 0);
        if (en < e_end) tn = entjr[en];
        for (int e = en; e < e_end; e += 16) {
            const int bj = tn.x, pos = tn.y;
            if (e + 16 < e_end) tn = entjr[e + 16];
            const double2 *wb2 = reinterpret_cast<const double2 *>(B.Wsp + (size_t)bj * 18);
            double wb[18];
#pragma unroll
            for (int k = 0; k < 9; k++) { const double2 v = wb2[k]; wb[2 * k] = v.x; wb[2 * k + 1] = v.y; }
            const double *y = srow_y + 18 * pos;
            double y0[6], y1[6], y2[6];
#pragma unroll
            for (int a = 0; a < 6; a++) { y0[a] = y[a]; y1[a] = y[6 + a]; y2[a] = y[12 + a]; }
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const double b0 = wb[c], b1 = wb[6 + c], b2 = wb[12 + c];
#pragma unroll
                for (int r = 0; r < 6; r++) acc[6 * r + c] += y0[r] * b0 + y1[r] * b1 + y2[r] * b2;
            }
        }
#pragma unroll
        for (int k = 0; k < 36; k++) {
            const double v = row16_allreduce_f64_dpp(acc[k]);
            if (sub == 0) {
                const int r = k / 6, c = k - 6 * r;
                S[(size_t)(6 * i + r) * G.ld + 6 * j + c] = -v;
                S[(size_t)(6 * j + c) * G.ld + 6 * i + r] = -v;
            }
        }
    }
}

// the window's system as the shared stages see it (dense_ldlt_big.h)
__device__ __forceinline__ DenseSys ba_big_sys(const BaBatch &B, int g)
{
    const BaGraphDev &G = B.gd[g];
    const size_t o = (size_t)G.free_off * 6;
    return DenseSys{B.S + G.s_off, G.ld, G.n, B.bs + o, B.xp + o, B.big_y + o, B.big_d + o, B.big_U + (size_t)g * LD_NB * LD_NB, B.big_fail + g};
}

__global__ __launch_bounds__(256) void k_ba_big_init(BaBatch B)
{
    const int g = blockIdx.y;
    if (!B.st[g].active) return;
    dense_big_init(ba_big_sys(B, g), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_ba_big_diag(BaBatch B, int p0)
{
    const int g = blockIdx.x;
    if (!B.st[g].active) return;
    dense_big_diag(ba_big_sys(B, g), p0);
}

__global__ __launch_bounds__(256) void k_ba_big_rows(BaBatch B, int p0)
{
    extern __shared__ double brl[];
    const int g = blockIdx.y;
    if (!B.st[g].active) return;
    dense_big_rows(ba_big_sys(B, g), p0, blockIdx.x, brl);
}

__global__ __launch_bounds__(256) void k_ba_big_trail(BaBatch B, int p0)
{
    const int g = blockIdx.z;
    if (!B.st[g].active) return;
    dense_big_trail(ba_big_sys(B, g), p0, blockIdx.y, blockIdx.x);
}

__global__ __launch_bounds__(1024) void k_ba_big_backsub(BaBatch B)
{
    extern __shared__ double bbl[];
    const int g = blockIdx.x;
    BaState &st = B.st[g];
    if (!st.active) return;
    const bool ok = dense_big_backsub(ba_big_sys(B, g), B.max_ld, bbl);
    if (threadIdx.x == 0) st.ok = ok ? 1 : 0;
}

// landmark back-substitution (block_solver.hpp:461-481) + trial update of every vertex
// (sparse_optimizer.cpp:422-435) + computeScale partials (levenberg.cpp:187-194)
__global__ __launch_bounds__(256) void k_ba_backsub_points(BaBatch B)
{
    // 16 lanes per point: one observing pose per lane and trip
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int sub = threadIdx.x & 15;
    const int l = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (l >= G.n_points) return;
    const int *ps = B.pt_start + G.ptstart_off;
    const size_t gl = (size_t)G.point_off + l;
    double *xl = B.xl + gl * 3;
    const double *Xc = B.points + ((size_t)st.cur * B.sumL + gl) * 3;
    double *Xn = B.points + ((size_t)(st.cur ^ 1) * B.sumL + gl) * 3;
    if (ps[l + 1] == ps[l]) { if (sub == 0) { Xn[0] = Xc[0]; Xn[1] = Xc[1]; Xn[2] = Xc[2]; B.scale_pt[gl] = 0; } return; }
    const double *bl = B.bl + gl * 3;
    double x0 = xl[0], x1 = xl[1], x2 = xl[2];                     // a failed solve keeps the previous increment
    if (st.ok) {
        double c0 = 0, c1 = 0, c2 = 0;
        for (int e = ps[l] + sub; e < ps[l + 1]; e += 16) {
            const int h = B.hidx[G.pose_off + B.edge_pose[G.edge_off + e]];
            if (h < 0 || B.edge_dup[G.edge_off + e]) continue;              // one Hpl block per (point, pose)
            const double *xp = B.xp + (size_t)(G.free_off + h) * 6;
            const double *w = B.Wsp + (size_t)B.edge_task[G.edge_off + e] * 18;
#pragma unroll
            for (int a = 0; a < 6; a++) { c0 -= w[a] * xp[a]; c1 -= w[6 + a] * xp[a]; c2 -= w[12 + a] * xp[a]; }
        }
        c0 = row16_allreduce_f64_dpp(c0); c1 = row16_allreduce_f64_dpp(c1); c2 = row16_allreduce_f64_dpp(c2);
        c0 += bl[0]; c1 += bl[1]; c2 += bl[2];
        const double *Di = B.Dinv + gl * 6;
        x0 = Di[0] * c0 + Di[1] * c1 + Di[2] * c2;
        x1 = Di[1] * c0 + Di[3] * c1 + Di[4] * c2;
        x2 = Di[2] * c0 + Di[4] * c1 + Di[5] * c2;
    }
    if (sub == 0) {
        xl[0] = x0; xl[1] = x1; xl[2] = x2;
        Xn[0] = Xc[0] + x0; Xn[1] = Xc[1] + x1; Xn[2] = Xc[2] + x2;
        B.scale_pt[gl] = x0 * (st.lambda * x0 + bl[0]) + x1 * (st.lambda * x1 + bl[1]) + x2 * (st.lambda * x2 + bl[2]);
    }
}

__global__ __launch_bounds__(64) void k_ba_update_poses(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= G.n_poses) return;
    const double *pc = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + p) * 7;
    double *pn = B.poses + ((size_t)(st.cur ^ 1) * B.sumP + G.pose_off + p) * 7;
    const int h = B.hidx[G.pose_off + p];
    if (h < 0) { for (int i = 0; i < 7; i++) pn[i] = pc[i]; return; }
    const double *x = B.xp + (size_t)(G.free_off + h) * 6;
    se3_oplus(x, pc, pn);
    const double *bp = B.bp + (size_t)(G.free_off + h) * 6;
    double s = 0;
    for (int a = 0; a < 6; a++) s += x[a] * (st.lambda * x[a] + bp[a]);
    B.scale_pose[G.free_off + h] = s;
}

// LM accept/reject + iteration bookkeeping: levenberg.cpp:121-169, sparse_optimizer.cpp:372-418,
// Optimizer.cc:2048-2122 (two passes).  One thread per graph.
__global__ void k_ba_control(BaBatch B, int abort_arg)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B.G) return;
    const int abort_flag = B.world > 1 ? *B.x_abort : abort_arg;       // sharded: every rank must see the same flag
    BaState &st = B.st[g];
    if (!st.active) return;
    double temp_chi = B.chi[g];
    if (!st.ok) temp_chi = DBL_MAX;
    double rho = st.current_chi - temp_chi;
    const double scale = B.scale[g] + 1e-3;
    rho /= scale;
    if (rho > 0 && isfinite(temp_chi)) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        const double sf = fmax(1. / 3., alpha);
        st.lambda *= sf; st.ni = 2; st.current_chi = temp_chi;
        st.cur ^= 1;                                   // discardTop: the trial becomes the estimate
        st.errors_fresh = 1;
    } else {
        st.lambda *= st.ni; st.ni *= 2;                // pop: keep the old estimate
        st.errors_fresh = 0;                           // the stored errors belong to the rejected trial
    }
    st.qmax++; st.lm_trials++;
    st.rho_dbg = rho;
    if (rho < 0 && st.qmax < B.max_trials && !abort_flag) return;      // retry with the larger lambda
    // outer iteration finished
    st.iters_run[st.pass]++;
    st.chi_last = st.current_chi;
    int ok = 1;
    if (st.qmax == B.max_trials || rho == 0) ok = 0;
    else {
        if ((st.ini_chi - st.current_chi) * 1e3 < st.ini_chi) st.nbad++; else st.nbad = 0;
        if (st.nbad >= 3) ok = 0;
    }
    st.iter++;
    st.need_build = 1;
    if (!ok || st.iter >= B.iters[st.pass] || abort_flag) {
        if (st.pass == 0 && !abort_flag && B.iters[1] > 0) {
            st.pass = 1; st.iter = 0; st.need_lambda_init = 1; st.errors_fresh = 0;      // levels / robust kernel change: re-evaluate
            if (B.ex2) st.apply_levels = 1;                // Optimizer.cc:6546-6579 (merge variant)
            if (B.nr2) st.robust = 0;
        }
        else { st.active = 0; atomicSub(B.n_active, 1); }
    }
}

// Merge variant, between the passes (Optimizer.cc:6546-6579): chi2 of the last evaluation > gate or depth <= 0 at the
// current estimate => setLevel(1).  Runs at the start of the tick after the pass switch (apply_levels).
// ---- landmark-sharded solve: pack this rank's partial sums into its slot of xbuf / reduce all slots in rank order
__global__ __launch_bounds__(256) void k_ba_shard_pack1(BaBatch B)
{
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    double *X = B.xbuf + (size_t)B.rank * B.xcount + B.x1_off[g];
    for (int i = tid; i < G.nf * 36; i += 256) X[i] = B.Hpp[(size_t)G.free_off * 36 + i];
    for (int i = tid; i < G.nf * 6; i += 256) X[G.nf * 36 + i] = B.bp[(size_t)G.free_off * 6 + i];
    if (tid == 0) { X[G.nf * 42] = B.chi[g]; X[G.nf * 42 + 1] = B.maxdiag[g]; }
}
__global__ __launch_bounds__(256) void k_ba_shard_sum1(BaBatch B)
{
    __shared__ double red[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    const double *X = B.xbuf + B.x1_off[g];
    double m = 0;
    for (int i = tid; i < G.nf * 36; i += 256) {
        double v = 0;
        for (int r = 0; r < B.world; r++) v += X[(size_t)r * B.xcount + i];
        B.Hpp[(size_t)G.free_off * 36 + i] = v;
        if (i % 36 % 7 == 0) m = fmax(m, fabs(v));
    }
    for (int i = tid; i < G.nf * 6; i += 256) {
        double v = 0;
        for (int r = 0; r < B.world; r++) v += X[(size_t)r * B.xcount + G.nf * 36 + i];
        B.bp[(size_t)G.free_off * 6 + i] = v;
    }
    red[tid] = m;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (tid < d) red[tid] = fmax(red[tid], red[tid + d]); __syncthreads(); }
    if (tid == 0) {
        double c = 0, mh = red[0];
        for (int r = 0; r < B.world; r++) { c += X[(size_t)r * B.xcount + G.nf * 42]; mh = fmax(mh, X[(size_t)r * B.xcount + G.nf * 42 + 1]); }
        B.chi[g] = c;
        if (st.need_lambda_init) B.maxdiag[g] = mh;
    }
}
__global__ __launch_bounds__(256) void k_ba_shard_pack2(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const int idx = blockIdx.x * 256 + threadIdx.x, n2 = G.ld * G.ld;
    double *X = B.xbuf + (size_t)B.rank * B.xcount + B.x2_off[g];
    if (idx < n2) {
        const double *Sp = B.Spart + G.spart_off + idx;
        double s = 0;
        for (int k = 0; k < G.ks; k++) s += Sp[(size_t)k * n2];
        X[idx] = s;
    }
    if (idx < G.nf * 6) X[n2 + idx] = B.bacc[(size_t)G.free_off * 6 + idx];
}
__global__ __launch_bounds__(256) void k_ba_shard_sum2(BaBatch B)
{
    const int g = blockIdx.x;
    const BaState &st = B.st[g];
    if (!st.active) return;
    const BaGraphDev &G = B.gd[g];
    const double *X = B.xbuf + B.x2_off[g] + (size_t)G.ld * G.ld;
    for (int i = threadIdx.x; i < G.nf * 6; i += 256) {
        double a = 0;
        for (int r = 0; r < B.world; r++) a += X[(size_t)r * B.xcount + i];
        B.bs[(size_t)G.free_off * 6 + i] = B.bp[(size_t)G.free_off * 6 + i] - a;
    }
}
// stage 3: trial chi2, computeScale partial, abort flag; stage 4: outlier / edge counts.  payload 3 doubles per graph.
__global__ void k_ba_shard_pack34(BaBatch B, int stage, int abort_arg)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B.G) return;
    double *X = B.xbuf + (size_t)B.rank * B.xcount + 3 * (size_t)g;
    if (stage == 3) { X[0] = B.chi[g]; X[1] = B.scale[g]; X[2] = (double)abort_arg; }
    else { X[0] = (double)B.st[g].n_outliers; X[1] = (double)B.gd[g].n_edges; X[2] = 0; }
}
__global__ void k_ba_shard_sum34(BaBatch B, int stage)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B.G) return;
    double a = 0, b2 = 0, c = 0;
    for (int r = 0; r < B.world; r++) { const double *X = B.xbuf + (size_t)r * B.xcount + 3 * (size_t)g; a += X[0]; b2 += X[1]; c = fmax(c, X[2]); }
    if (stage == 3) { if (B.st[g].active) { B.chi[g] = a; B.scale[g] = b2; } if (g == 0) *B.x_abort = c > 0 ? 1 : 0; }
    else { B.st[g].n_outliers = (int)a; B.edges_total[g] = b2; }
}

__global__ __launch_bounds__(256) void k_ba_levels(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.apply_levels) return;
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int ge = G.edge_off + e;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    const BaCamDev &cam = ba_cam_ref<true>(B, G, B.edge_pose[ge]);      // (mTrl of the edge's own keyframe)
    const double z = edge_depth(cam, pose, X, B.edge_stereo[ge]);
    const double gate = B.edge_stereo[ge] == 1 ? B.gate_s : B.gate_m;
    if ((B.chi2[ge] > gate) || !(z > 0.0)) B.level[ge] = 1;
}

// outlier gates, Optimizer.cc:2126-2173: stored chi2 of the last evaluation; depth at the final estimate
__global__ __launch_bounds__(256) void k_ba_finalize(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int ge = G.edge_off + e;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    const BaCamDev &cam = ba_cam_ref<true>(B, G, B.edge_pose[ge]);      // (mTrl of the edge's own keyframe)
    const double z = edge_depth(cam, pose, X, B.edge_stereo[ge]);
    const double gate = B.edge_stereo[ge] == 1 ? B.gate_s : B.gate_m;
    const int out = (B.chi2[ge] > gate) || !(z > 0.0);
    B.outlier[ge] = (uint8_t)out;
    if (out) atomicAdd(&B.st[g].n_outliers, 1);
}

// ------------------------------------------------------------------ host side

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

// ---------------------------------------------------------------------------------------------------------------- pair lists, built on the device
// The lists k_ba_schur_big / k_ba_schur_rows walk -- per graph and pair of free poses (i <= j, row-major over the upper triangle) the Hpl
// blocks of the points both see, in point order -- come from the pose-major edge lists that are uploaded anyway: a wave owns a pair, runs
// over pose i's edges 64 at a time (they are in point order) and finds each point among pose j's by a lower bound (the first edge of a
// (point, pose) chain is the one that carries the block).  Same entries in the same order as the host enumeration of round 3/4 -- every
// summation order downstream is unchanged -- without the 0.5 ms the host spent per 50 x 2000 x 10 window and the 2 MB it uploaded.
// FILL = 0: entries per pair into big_pair_start; k_ba_pair_scan turns them into starts; FILL = 1: the entries.
template <int FILL>
__global__ __launch_bounds__(256) void k_ba_pair_lists(BaBatch B)
{
    const BaGraphDev &G = B.gd[blockIdx.y];
    const int nf = G.nf, npair = nf * (nf + 1) / 2;
    const int lane = threadIdx.x & 63, pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= npair) return;
    int i = 0, j = pi;
    while (j >= nf - i) { j -= nf - i; i++; }
    j += i;
    const int *qs = B.pose_start + G.posestart_off, *pe = B.pose_edges + G.edge_off, *et = B.edge_task + G.edge_off, *ep = B.edge_point + G.edge_off;
    const int a0 = qs[i], a1 = qs[i + 1], c0 = qs[j], c1 = qs[j + 1];
    int *pstart = const_cast<int *>(B.big_pair_start) + G.pair_off;
    int2 *ent = const_cast<int2 *>(B.big_pair_ent) + G.pent_off, *jr = const_cast<int2 *>(B.big_pair_jr) + G.pent_off;
    int *ptl = const_cast<int *>(B.big_pair_pt) + G.pent_off;
    int out = FILL ? pstart[pi] : 0, rank = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int p0 = a0; p0 < a1; p0 += 64) {
        const int p = p0 + lane;
        int ta = -1, pt = -1;
        if (p < a1) { const int ea = pe[p]; ta = et[ea]; pt = ep[ea]; }
        const unsigned long long bb = __ballot(ta >= 0);
        const int myrank = rank + __popcll(bb & lt);             // place of the block in pose i's own (diagonal) list
        rank += __popcll(bb);
        int tc = -1;
        if (ta >= 0) {
            if (i == j) tc = ta;
            else {
                int lo = c0, hi = c1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (ep[pe[mid]] < pt) lo = mid + 1; else hi = mid; }
                if (lo < c1) { const int ec = pe[lo]; if (ep[ec] == pt) tc = et[ec]; }
            }
        }
        const unsigned long long hb = __ballot(tc >= 0);
        if (FILL && tc >= 0) {
            const int q = out + __popcll(hb & lt);
            ent[q] = make_int2(ta, tc); ptl[q] = pt; jr[q] = make_int2(tc, myrank);
        }
        out += __popcll(hb);
    }
    if (!FILL && lane == 0) pstart[pi] = out;
}
// counts -> exclusive starts, one workgroup per graph; entry npair = the graph's total
__global__ __launch_bounds__(256) void k_ba_pair_scan(BaBatch B)
{
    const BaGraphDev &G = B.gd[blockIdx.x];
    const int npair = G.nf * (G.nf + 1) / 2;
    int *ps = const_cast<int *>(B.big_pair_start) + G.pair_off;
    __shared__ int part[256];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int k0 = 0; k0 <= npair; k0 += 256) {
        const int k = k0 + threadIdx.x;
        const int v = k < npair ? ps[k] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        const int base = carry;
        if (k <= npair) ps[k] = base + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry = base + part[255];
        __syncthreads();
    }
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
#ifdef LDLT_PROF
extern "C" int orbhip_debug_ldlt_prof(long long *out8, int reset)      // debug build only (EXTRA=-DLDLT_PROF): cumulative cycles of ldlt_solve_wg's phases
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ldlt_prof), 64) != hipSuccess) return ORBHIP_E_HIP;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_ldlt_prof), z, 64) != hipSuccess) return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
#endif

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

// FP64 matrix-core peak of this device, measured: every wave issues independent
// v_mfma_f64_16x16x4_f64 chains (the local micro-architecture guide lists no FP64 MFMA peak).
__global__ __launch_bounds__(256) void k_mfma_f64_peak(double *sink, int iters)
{
    v4d acc[8];
    for (int i = 0; i < 8; i++) acc[i] = (v4d){0, 0, 0, 0};
    const double a = 1.0 + threadIdx.x * 1e-9, bb = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; it++)
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[i], 0, 0, 0);
    double s = 0;
    for (int i = 0; i < 8; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[0] = s;
}

extern "C" int orbhip_mfma_f64_peak_tflops(orbhip_ctx *ctx, double *tflops_out)
{
    if (!ctx || !tflops_out) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    double *sink = nullptr;
    if (hipMalloc((void **)&sink, 8) != hipSuccess) return ORBHIP_E_HIP;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int blocks = 256 * 8, iters = 4096;
    hipLaunchKernelGGL(k_mfma_f64_peak, dim3(blocks), dim3(256), 0, s, sink, 64);          // warm-up
    (void)hipEventRecord(e0, s);
    hipLaunchKernelGGL(k_mfma_f64_peak, dim3(blocks), dim3(256), 0, s, sink, iters);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(sink);
    const double flops = (double)blocks * 4.0 * iters * 8.0 * 2048.0;
    *tflops_out = flops / (ms * 1e-3) / 1e12;
    return ORBHIP_OK;
}

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
