// pose_graph4dof_kernels.hip -- Optimizer::OptimizeEssentialGraph4DoF (reference src/Optimizer.cc:8305-8610, the branch
// LoopClosing::CorrectLoop takes for an inertial map whose IMU is initialised) on gfx950: a pose graph of VertexPose4DoF / Edge4DoF
// (include/G2oTypes.h:152-186, :833-859) under g2o's Levenberg-Marquardt.  The map points' correction after it is k_pg_points
// (pose_graph_kernels.hip) with Sim3(R, t, 1) rows; there is no point kernel here.
//
//   Q1  vertex state and oplus: ImuCamPose::UpdateW            src/G2oTypes.cc:222-256 through G2oTypes.h:175-185
//   Q2  residual [LogSO3(Rcw_i Rcw_j^T dRij^T) ; Rcw_i (-Rcw_j^T tcw_j) + tcw_i - dtij]      G2oTypes.h:847-852, G2oTypes.cc:1009-1023
//   Q3  numeric Jacobians, delta = 1e-9, through oplus         g2o/core/base_binary_edge.hpp:136-200
//   Q4  quadratic form with a diagonal information, no kernel  base_binary_edge.hpp:55-90
//   Q5  lambda start tau * max |H(j, j)|                        g2o/core/optimization_algorithm_levenberg.cpp:171-185
//   Q6  LM control                                             optimization_algorithm_levenberg.cpp:61-169
//
// A vertex keeps Rwb0, DR, twb, Rcb, tcb, Rcw, tcw and Rwb = DR Rwb0, as ImuCamPose does.  Rcw / tcw are LOADED (the keyframe's float pose
// or the corrected Sim3) and become Rcb Rwb^T, Rcb (-Rwb^T twb) + tcb only at a vertex's first oplus: the nominal error of iteration 0 is
// taken at the loaded ones, its perturbed errors at the derived ones, a fixed vertex keeps the loaded ones throughout.
// UpdateW's `its >= 5` step is left out: it writes 0.0 into DR(0,2), DR(1,2), DR(2,0), DR(2,1) and discards what NormalizeRotation
// returns.  DR is a product of ExpSO3(0, 0, z), whose four entries are a * 0 + b * 0: zero already, so the step changes no value
// (tests/test_essential_graph4dof_model.py runs the model with and without it over more than six accepted iterations: the same bits).
//
// The dense H + lambda I machinery is that of pose_graph_kernels.hip with 4 unknowns per vertex: k_pg4_assemble / _fill / _ldlt /
// _big_* / _reduce are this file's instances of the bodies in pose_graph_common.h and dense_ldlt_big.h (no kernel is shared across
// translation units, see the Makefile), and the host side -- graph checks, lists, arena, dense solve chain, LM control -- is
// pose_graph_common.h's.  Here: the 4-DoF vertex and edge (linearise, the lambda start, update, errors) and the entry point.
// One LM trial is a short chain of launches; the control flow runs on the host with one 24-byte read-back per trial.
//
//   k_pg4_linearize  32 lanes per edge: lane 0 the nominal error, lanes 1..16 one perturbed error each (+-delta on the 4 coordinates of
//                    each free endpoint, 17 evaluations); columns by differences through LDS; J^T W J blocks and -J^T W e to the edge's row
//   k_pg4_assemble   one wave per 4x4 block of H (lower block triangle) and per 4-vector of b, contributions summed in edge order
//   k_pg4_maxdiag    Q5: max |H(j, j)| over the diagonal blocks, a strided pass and a binary tree
//   k_pg4_fill / _ldlt / _big_*      S = H + lambda I and its L D L^T: one workgroup up to BA_LDLT_MAXN unknowns, many up to 4096
//   k_pg4_update     Q1 with the solved x;  k_pg4_errors / _reduce: chi2 = sum e^T W e and computeScale, two stages in a fixed order
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "geom3.h"
#include "ba_ldlt.h"
#include "so3_f64.h"
#include "pose_graph_common.h"
#pragma clang fp contract(fast)       // as the other double-precision optimisers
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

#define PG4_ROW 64            // doubles per edge row: e 6 | Ji^T W Ji 16 | Ji^T W Jj 16 | Jj^T W Jj 16 | -Ji^T W e 4 | -Jj^T W e 4 | pad 2
#define PG4_O_II 6
#define PG4_O_IJ 22
#define PG4_O_JJ 38
#define PG4_O_BI 54
#define PG4_O_BJ 58
#define PG4_USED 62
#define PG4_EPB 8             // edges per 256-lane workgroup of k_pg4_linearize
#define PG4_VS 54             // doubles per vertex on the device
#define PG4_RWB0 0
#define PG4_DR 9
#define PG4_TWB 18
#define PG4_RCB 21
#define PG4_TCB 30
#define PG4_RCW 33
#define PG4_TCW 42
#define PG4_RWB 45
#define PG4_ABI 36            // doubles per vertex of the ABI: Rwb 9 | twb 3 | Rcw 9 | tcw 3 | Rcb 9 | tcb 3

struct Pg4Dev : PgDevCommon {              // est [nv][PG4_VS], meas [ne][12] (dRij row-major, dtij), rows [ne][PG4_ROW], Hb [nblk][16]
    double info[6];                         // the diagonal of the edges' information
};

// Q1: VertexPose4DoF::oplusImpl(u) = ImuCamPose::UpdateW(0, 0, u0, u1, u2, u3)
__device__ __forceinline__ void pg4_oplus(const double *Rwb0, double *DR, double *twb, const double *Rcb, const double *tcb, const double *u,
                                          double *Rwb, double *Rcw, double *tcw)
{
    const double w[3] = {0.0, 0.0, u[0]};
    double dR[9], T[9], tbw[3];
    so3_exp(w, dR, 1e-5, true);
    mm3(dR, DR, T);
#pragma unroll
    for (int k = 0; k < 9; k++) DR[k] = T[k];
    mm3(DR, Rwb0, Rwb);
#pragma unroll
    for (int k = 0; k < 3; k++) twb[k] += u[1 + k];
    mtv3(Rwb, twb, tbw);                                     // tbw = -Rbw twb
#pragma unroll
    for (int k = 0; k < 3; k++) tbw[k] = -tbw[k];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rcw[3 * i + j] = Rcb[3 * i] * Rwb[3 * j] + Rcb[3 * i + 1] * Rwb[3 * j + 1] + Rcb[3 * i + 2] * Rwb[3 * j + 2];
    mv3(Rcb, tbw, tcw);
#pragma unroll
    for (int k = 0; k < 3; k++) tcw[k] += tcb[k];
}

// Q2: one edge's computeError; M = dRij (9, row-major), dtij (3)
__device__ __forceinline__ void pg4_error(const double *Ri, const double *ti, const double *Rj, const double *tj, const double *M, double *e)
{
    double A[9], B[9], p[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) A[3 * i + j] = Ri[3 * i] * Rj[3 * j] + Ri[3 * i + 1] * Rj[3 * j + 1] + Ri[3 * i + 2] * Rj[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[3 * i + j] = A[3 * i] * M[3 * j] + A[3 * i + 1] * M[3 * j + 1] + A[3 * i + 2] * M[3 * j + 2];
    so3_log(B, e);
    mtv3(Rj, tj, p);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = -p[k];
    mv3(Ri, p, q);
#pragma unroll
    for (int k = 0; k < 3; k++) e[3 + k] = q[k] + ti[k] - M[9 + k];
}

__global__ __launch_bounds__(256) void k_pg4_linearize(Pg4Dev G)
{
    __shared__ double errs[PG4_EPB][17][6], Jl[PG4_EPB][6][8];
    const int tid = threadIdx.x, le = tid >> 5, sub = tid & 31;
    const int e = blockIdx.x * PG4_EPB + le;
    const bool live = e < G.ne;
    bool free_i = false, free_j = false;
    if (live) {
        const int vi = G.v0[e], vj = G.v1[e];
        free_i = G.free_idx[vi] >= 0; free_j = G.free_idx[vj] >= 0;
        const int k = sub - 1, side = k >> 3, c = (k & 7) >> 1;
        if (sub == 0 || (sub < 17 && (side == 0 ? free_i : free_j))) {
            double Ri[9], ti[3], Rj[9], tj[3], M[12], er[6];
            const double *Ei = G.est + (size_t)vi * PG4_VS, *Ej = G.est + (size_t)vj * PG4_VS;
#pragma unroll
            for (int q = 0; q < 9; q++) { Ri[q] = Ei[PG4_RCW + q]; Rj[q] = Ej[PG4_RCW + q]; }
#pragma unroll
            for (int q = 0; q < 3; q++) { ti[q] = Ei[PG4_TCW + q]; tj[q] = Ej[PG4_TCW + q]; }
#pragma unroll
            for (int q = 0; q < 12; q++) M[q] = G.meas[12 * (size_t)e + q];
            if (sub > 0) {
                // Q3: the vertex's own oplus on a copy of its state, add[c] = +-delta
                const double *E = side == 0 ? Ei : Ej;
                double Rwb0[9], DR[9], twb[3], Rcb[9], tcb[3], Rwb[9], u[4];
#pragma unroll
                for (int q = 0; q < 9; q++) { Rwb0[q] = E[PG4_RWB0 + q]; DR[q] = E[PG4_DR + q]; Rcb[q] = E[PG4_RCB + q]; }
#pragma unroll
                for (int q = 0; q < 3; q++) { twb[q] = E[PG4_TWB + q]; tcb[q] = E[PG4_TCB + q]; }
                const double dl = (k & 1) ? -1e-9 : 1e-9;
#pragma unroll
                for (int q = 0; q < 4; q++) u[q] = q == c ? dl : 0.0;
                if (side == 0) pg4_oplus(Rwb0, DR, twb, Rcb, tcb, u, Rwb, Ri, ti);
                else pg4_oplus(Rwb0, DR, twb, Rcb, tcb, u, Rwb, Rj, tj);
            }
            pg4_error(Ri, ti, Rj, tj, M, er);
#pragma unroll
            for (int r = 0; r < 6; r++) errs[le][sub][r] = er[r];
        }
    }
    __syncthreads();
    if (live) {
        const double scalar = 1.0 / (2 * 1e-9);
        for (int idx = sub; idx < 48; idx += 32) {
            const int r = idx >> 3, col = idx & 7;
            const bool fr = col < 4 ? free_i : free_j;
            Jl[le][r][col] = fr ? scalar * (errs[le][1 + 2 * col][r] - errs[le][2 + 2 * col][r]) : 0.0;
        }
    }
    __syncthreads();
    if (!live) return;
    double *row = G.rows + (size_t)e * PG4_ROW;
    for (int idx = sub; idx < PG4_USED; idx += 32) {
        double v;
        if (idx < 6) v = errs[le][0][idx];
        else if (idx < PG4_O_BI) {
            const int w = (idx - 6) >> 4, k = (idx - 6) & 15, a = k >> 2, c = k & 3;
            const int ca = w == 2 ? 4 + a : a, cc = w == 0 ? c : 4 + c;
            v = 0;
            for (int r = 0; r < 6; r++) v += Jl[le][r][ca] * G.info[r] * Jl[le][r][cc];
        } else {
            const int a = idx - PG4_O_BI;                 // 0..7: column of J
            v = 0;
            for (int r = 0; r < 6; r++) v += Jl[le][r][a] * (-(G.info[r] * errs[le][0][r]));
        }
        row[idx] = v;
    }
}

// the shared bodies (pose_graph_common.h, dense_ldlt_big.h) at this graph's edge-row layout
struct PgRow4 { enum { D = 4, ROW = PG4_ROW, II = PG4_O_II, IJ = PG4_O_IJ, JJ = PG4_O_JJ, BI = PG4_O_BI, BJ = PG4_O_BJ }; };

__global__ __launch_bounds__(64) void k_pg4_assemble(Pg4Dev G) { pg_assemble_body<PgRow4>(G); }

// Q5: the diagonal blocks are the first nf blocks of Hb
__global__ __launch_bounds__(256) void k_pg4_maxdiag(Pg4Dev G)
{
    __shared__ double sm[256];
    const int tid = threadIdx.x;
    double m = 0;
    for (int j = tid; j < G.n; j += 256) m = fmax(fabs(G.Hb[(size_t)(j >> 2) * 16 + (j & 3) * 5]), m);
    sm[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sm[tid] = fmax(sm[tid], sm[tid + w]);
        __syncthreads();
    }
    if (tid == 0) G.result[3] = sm[0];
}

__global__ __launch_bounds__(64) void k_pg4_fill(Pg4Dev G, double lambda) { pg_fill_body<PgRow4>(G, lambda); }
__global__ __launch_bounds__(1024) void k_pg4_ldlt(Pg4Dev G) { pg_ldlt_body(G); }

// ---- n > BA_LDLT_MAXN: the many-workgroup factorisation, as k_pg_big_* (pose_graph_kernels.hip)
__global__ __launch_bounds__(256) void k_pg4_big_init(Pg4Dev G) { dense_big_init(pg_dense_sys(G), blockIdx.x); }
__global__ __launch_bounds__(64) void k_pg4_big_diag(Pg4Dev G, int p0) { dense_big_diag(pg_dense_sys(G), p0); }
__global__ __launch_bounds__(256) void k_pg4_big_rows(Pg4Dev G, int p0)
{
    extern __shared__ double brl4[];
    dense_big_rows(pg_dense_sys(G), p0, blockIdx.x, brl4);
}
__global__ __launch_bounds__(256) void k_pg4_big_trail(Pg4Dev G, int p0) { dense_big_trail(pg_dense_sys(G), p0, blockIdx.y, blockIdx.x); }
__global__ __launch_bounds__(1024) void k_pg4_big_backsub(Pg4Dev G)
{
    extern __shared__ double bbl4[];
    const bool ok = dense_big_backsub(pg_dense_sys(G), G.n, bbl4);
    if (threadIdx.x == 0) G.result[2] = ok ? 1.0 : 0.0;
}

// Q6 / sparse_optimizer.cpp:422-435: the trial estimate of every free vertex
__global__ __launch_bounds__(64) void k_pg4_update(Pg4Dev G)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= G.nf) return;
    double *E = G.est + (size_t)G.free_list[f] * PG4_VS;
    double Rwb0[9], DR[9], twb[3], Rcb[9], tcb[3], Rwb[9], Rcw[9], tcw[3], u[4];
#pragma unroll
    for (int q = 0; q < 9; q++) { Rwb0[q] = E[PG4_RWB0 + q]; DR[q] = E[PG4_DR + q]; Rcb[q] = E[PG4_RCB + q]; }
#pragma unroll
    for (int q = 0; q < 3; q++) { twb[q] = E[PG4_TWB + q]; tcb[q] = E[PG4_TCB + q]; }
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = G.x[4 * f + q];
    pg4_oplus(Rwb0, DR, twb, Rcb, tcb, u, Rwb, Rcw, tcw);
#pragma unroll
    for (int q = 0; q < 9; q++) { E[PG4_DR + q] = DR[q]; E[PG4_RCW + q] = Rcw[q]; E[PG4_RWB + q] = Rwb[q]; }
#pragma unroll
    for (int q = 0; q < 3; q++) { E[PG4_TWB + q] = twb[q]; E[PG4_TCW + q] = tcw[q]; }
}

__global__ __launch_bounds__(64) void k_pg4_errors(Pg4Dev G)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= G.ne) return;
    const double *Ei = G.est + (size_t)G.v0[e] * PG4_VS, *Ej = G.est + (size_t)G.v1[e] * PG4_VS;
    double Ri[9], ti[3], Rj[9], tj[3], M[12], er[6];
#pragma unroll
    for (int q = 0; q < 9; q++) { Ri[q] = Ei[PG4_RCW + q]; Rj[q] = Ej[PG4_RCW + q]; }
#pragma unroll
    for (int q = 0; q < 3; q++) { ti[q] = Ei[PG4_TCW + q]; tj[q] = Ej[PG4_TCW + q]; }
#pragma unroll
    for (int q = 0; q < 12; q++) M[q] = G.meas[12 * (size_t)e + q];
    pg4_error(Ri, ti, Rj, tj, M, er);
    double c = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) c += er[r] * (G.info[r] * er[r]);
    G.chi_e[e] = c;
}

__global__ __launch_bounds__(256) void k_pg4_reduce(Pg4Dev G, double lambda) { pg_reduce_body(G, lambda); }

thread_local int g_pg4_last_path = -1;      // which factorisation the calling thread's last solved graph took: 0 one workgroup, 1 many
#define PG4_FN "orbhip_optimize_essential_graph4dof_host: "
const PgKernels<Pg4Dev> PG4_KERNELS = {"k_pg4", k_pg4_fill, k_pg4_ldlt, k_pg4_big_init, k_pg4_big_diag, k_pg4_big_rows, k_pg4_big_trail, k_pg4_big_backsub, k_pg4_reduce};

int pg4_check(const orbhip_pose_graph4dof *graphs, int n_graphs, const orbhip_pose_graph4dof_params *p, double *const *state)
{
    if (!(p->iterations >= 1)) return pg_fail(ORBHIP_E_BADARG, PG4_FN "iterations < 1");
    if (!(p->max_trials >= 1)) return pg_fail(ORBHIP_E_BADARG, PG4_FN "max_trials < 1");
    if (!std::isfinite(p->lambda_init)) return pg_fail(ORBHIP_E_BADARG, PG4_FN "lambda_init is not finite");
    if (!(p->lambda_init > 0) && !(std::isfinite(p->tau) && p->tau > 0))
        return pg_fail(ORBHIP_E_BADARG, PG4_FN "tau is not finite and positive (and lambda_init <= 0 asks for the computed start)");
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(p->info_diag[k])) return pg_fail(ORBHIP_E_BADARG, PG4_FN "info_diag[%d] is not finite", k);
    if ((long)p->iterations * p->max_trials > (1L << 24)) return pg_fail(ORBHIP_E_BADARG, PG4_FN "iterations * max_trials beyond 2^24");
    return pg_check_graphs(PG4_FN, "state_inout", graphs, n_graphs, state, PG4_ABI, 12, 4);
}

int pg4_solve_one(orbhip_ctx *ctx, const orbhip_pose_graph4dof &graph, const orbhip_pose_graph4dof_params *p, double *state, orbhip_pose_graph_stats *st,
                  double *trace)
{
    PgRun<Pg4Dev> R;
    R.fn = PG4_FN; R.K = PG4_KERNELS;
    memset(&R.D, 0, sizeof(R.D));
    for (int k = 0; k < 6; k++) R.D.info[k] = p->info_diag[k];
    int rc = pg_setup(ctx, graph, 4, 12, PG4_VS, PG4_ROW, R, [&](double *est) {
        for (int v = 0; v < graph.n_vertices; v++) {
            const double *a = state + PG4_ABI * (size_t)v;
            double *d = est + PG4_VS * (size_t)v;
            for (int k = 0; k < 9; k++) { d[PG4_RWB0 + k] = a[k]; d[PG4_RWB + k] = a[k]; d[PG4_DR + k] = (k % 4 == 0) ? 1.0 : 0.0; d[PG4_RCW + k] = a[12 + k]; d[PG4_RCB + k] = a[24 + k]; }
            for (int k = 0; k < 3; k++) { d[PG4_TWB + k] = a[9 + k]; d[PG4_TCW + k] = a[21 + k]; d[PG4_TCB + k] = a[33 + k]; }
        }
    });
    if (rc) return rc;
    const PgLists &H = R.H;
    const Pg4Dev &D = R.D;
    orbhip_pose_graph_stats S;
    memset(&S, 0, sizeof(S));
    S.n_free = H.nf; S.n_unknowns = H.n; S.lambda = 0;
    if (H.nf == 0 || H.ne == 0) { if (st) *st = S; return ORBHIP_OK; }
    hipStream_t s = R.s;

    g_pg4_last_path = R.big ? 1 : 0;
    PgLmOps ops;
    ops.chi2 = [&](double lambda, double *out3) -> int {
        hipLaunchKernelGGL(k_pg4_errors, dim3((H.ne + 63) / 64), dim3(64), 0, s, D);
        return pg_reduce_read(R, lambda, out3);
    };
    ops.build = [&]() -> int {
        hipLaunchKernelGGL(k_pg4_linearize, dim3((H.ne + PG4_EPB - 1) / PG4_EPB), dim3(256), 0, s, D);
        hipLaunchKernelGGL(k_pg4_assemble, dim3(H.nblk + H.nf), dim3(64), 0, s, D);
        return ORBHIP_OK;
    };
    ops.lambda_start = [&](double *lambda) -> int {                                // computeLambdaInit (:171-185)
        if (p->lambda_init > 0) { *lambda = p->lambda_init; return ORBHIP_OK; }
        hipLaunchKernelGGL(k_pg4_maxdiag, dim3(1), dim3(256), 0, s, D);
        if (hipGetLastError() != hipSuccess) return pg_fail(ORBHIP_E_HIP, PG4_FN "a kernel launch failed");
        ORB_HIP_TRY(hipMemcpyAsync(R.rb, D.result + 3, sizeof(double), hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        *lambda = p->tau * R.rb[0];
        return ORBHIP_OK;
    };
    ops.solve = [&](double lambda) -> int { return pg_solve(R, lambda); };
    ops.update = [&](double lambda, double *out3) -> int {
        hipLaunchKernelGGL(k_pg4_update, dim3((H.nf + 63) / 64), dim3(64), 0, s, D);
        return ops.chi2(lambda, out3);
    };
    if ((rc = pg_lm_run(R, ops, p->iterations, p->max_trials, trace, S))) return rc;
    if (S.end_reason != ORBHIP_PG_END_SOLVE_FAILED) {
        if ((rc = pg_read_est(R))) return rc;
        for (int f = 0; f < H.nf; f++) {                                           // a fixed vertex keeps its bytes
            const int v = H.free_list[f];
            const double *d = R.rb + PG4_VS * (size_t)v;
            double *a = state + PG4_ABI * (size_t)v;
            for (int k = 0; k < 9; k++) { a[k] = d[PG4_RWB + k]; a[12 + k] = d[PG4_RCW + k]; }
            for (int k = 0; k < 3; k++) { a[9 + k] = d[PG4_TWB + k]; a[21 + k] = d[PG4_TCW + k]; }
        }
    }
    if (st) *st = S;
    return ORBHIP_OK;
}

}  // namespace

extern "C" int orbhip_debug_pose_graph4dof_last_path(void) { return g_pg4_last_path; }

extern "C" void orbhip_pose_graph4dof_default_params(orbhip_pose_graph4dof_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->iterations = 20; p->lambda_init = 0; p->tau = 1e-50; p->max_trials = 100;
    // src/Optimizer.cc:8378-8381 sets (0,0) twice and never (2,2): yaw keeps weight 1
    p->info_diag[0] = 1e3; p->info_diag[1] = 1e3; p->info_diag[2] = 1; p->info_diag[3] = 1; p->info_diag[4] = 1; p->info_diag[5] = 1;
}

extern "C" int orbhip_optimize_essential_graph4dof_host(orbhip_ctx *ctx, const orbhip_pose_graph4dof *graphs, int n_graphs,
        const orbhip_pose_graph4dof_params *params, double *const *state_inout, orbhip_pose_graph_stats *stats_out, double *trace_out)
{
    if (!ctx || !graphs || n_graphs < 0 || !params || !state_inout)
        return pg_fail(ORBHIP_E_BADARG, PG4_FN "ctx / graphs / params / state_inout is NULL or n_graphs < 0");
    int rc = pg4_check(graphs, n_graphs, params, state_inout);
    if (rc) return rc;
    const size_t stride = (size_t)params->iterations * params->max_trials * ORBHIP_PG_TRACE;
    for (int g = 0; g < n_graphs; g++)
        if ((rc = pg4_solve_one(ctx, graphs[g], params, state_inout[g], stats_out ? stats_out + g : nullptr, trace_out ? trace_out + g * stride : nullptr))) return rc;
    return ORBHIP_OK;
}
