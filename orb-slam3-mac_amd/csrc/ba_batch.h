// ba_batch.h -- what the files of the local bundle adjustment share: the LM state of a graph on the device (BaState), the kernel
// argument (BaBatch, by value), the calibration an edge projects through (ba_cam_ref), the launch constants the host needs beyond
// ba_graph_lists.h's, and the declaration of every kernel.  The kernels are defined in ba_edge_kernels.hip, ba_schur_kernels.hip,
// ba_reduced_kernels.hip, ba_lm_kernels.hip and ba_shard_kernels.hip and launched from ba_kernels.hip (the host side): a kernel defined in
// one object and launched from another needs no relocatable device code, only its declaration here, with the launch bounds of the
// definition.  No `#pragma clang fp contract` here: every .hip sets it after its project headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "ba_graph_lists.h"      // BaGraphDev, BaCamDev, the GEMM_* constants

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

// ------------------------------------------------------------------ launch constants (the rest: ba_graph_lists.h)
#define GEMM_LDS_TAIL 32       // a short chunk reads up to GEMM_C-1 tiles past the end of a row (never multiplied)
// k_ba_schur_rows
#define SROW_THREADS 384                              // 6 waves: 170 VGPRs each at 3 waves per SIMD, two workgroups per CU while a row is <= 500 blocks
#define SROW_GROUPS (SROW_THREADS / 16)
#define SROW_MAX_BLOCKS 1024                          // 147 KB of LDS; batches with a fuller row keep k_ba_schur_big

// ------------------------------------------------------------------ kernels, in the order of a tick
// ba_edge_kernels.hip: edge evaluation and assembly
__global__ __launch_bounds__(256) void k_ba_levels(BaBatch B);
template <bool GENERAL> __global__ __launch_bounds__(256) void k_ba_errors(BaBatch B, int which);
__global__ __launch_bounds__(1024) void k_ba_reduce(BaBatch B, int which);
template <bool GENERAL> __global__ __launch_bounds__(256) void k_ba_build_points(BaBatch B);
template <bool GENERAL> __global__ __launch_bounds__(64) void k_ba_build_poses(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_maxdiag(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_finalize(BaBatch B);
// ba_schur_kernels.hip: the device pair lists (at creation) and the three forms of the Schur complement
template <int FILL> __global__ __launch_bounds__(256) void k_ba_pair_lists(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_pair_scan(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_point_prep(BaBatch B);
__global__ __launch_bounds__(64 * GEMM_WAVES) void k_ba_schur_gemm(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_schur_finish(BaBatch B);
__global__ __launch_bounds__(64) void k_ba_bschur(BaBatch B);
template <int LPP> __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ba_schur_big(BaBatch B, int nblk);
__global__ __launch_bounds__(SROW_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_ba_schur_rows(BaBatch B, int max_nf);
// ba_reduced_kernels.hip: the two forms of the reduced LDL^T
__global__ __launch_bounds__(1024) void k_ba_ldlt(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_big_init(BaBatch B);
__global__ __launch_bounds__(64) void k_ba_big_diag(BaBatch B, int p0);
__global__ __launch_bounds__(256) void k_ba_big_rows(BaBatch B, int p0);
__global__ __launch_bounds__(256) void k_ba_big_trail(BaBatch B, int p0);
__global__ __launch_bounds__(1024) void k_ba_big_backsub(BaBatch B);
// ba_lm_kernels.hip: LM control and the trial update
__global__ void k_ba_pretrial(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_backsub_points(BaBatch B);
__global__ __launch_bounds__(64) void k_ba_update_poses(BaBatch B);
__global__ void k_ba_control(BaBatch B, int abort_arg);
// ba_shard_kernels.hip: the exchanges of a landmark-sharded solve
__global__ __launch_bounds__(256) void k_ba_shard_pack1(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_shard_sum1(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_shard_pack2(BaBatch B);
__global__ __launch_bounds__(256) void k_ba_shard_sum2(BaBatch B);
__global__ void k_ba_shard_pack34(BaBatch B, int stage, int abort_arg);
__global__ void k_ba_shard_sum34(BaBatch B, int stage);
