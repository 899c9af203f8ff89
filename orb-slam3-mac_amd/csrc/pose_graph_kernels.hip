// pose_graph_kernels.hip -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2347-2663, the overload LoopClosing::CorrectLoop
// calls) on gfx950: a Sim3 pose graph of VertexSim3Expmap / EdgeSim3 (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:48-131) under
// g2o's Levenberg-Marquardt, and the correction of the map points that follows it.
//
//   P1  g2o::Sim3 exp / log / operator* / inverse / map       sim3.h:70-142,148-230,233-236,266-272,144-146 (sim3_group.h)
//   P2  residual log(Sji * S_i * S_j^-1)                       types_seven_dof_expmap.h:106-114
//   P3  numeric Jacobians, delta = 1e-9, through oplus         g2o/core/base_binary_edge.hpp:136-200, types_seven_dof_expmap.h:60-69
//   P4  quadratic form, identity information, no kernel        base_binary_edge.hpp:55-90
//   P5  LM control                                             g2o/core/optimization_algorithm_levenberg.cpp:61-194
//   P6  point correction                                       src/Optimizer.cc:2636-2660
//
// One LM trial is a short chain of launches on the context's stream; the control flow of P5 runs on the host, which reads three doubles
// back per trial (chi2, computeScale, the solve's flag).  A loop closure happens once in minutes and its optimisation takes tens of
// milliseconds: the ~10 us of a read-back per trial are not what it waits for.
//
//   k_pg_linearize   32 lanes per edge: lane 0 the nominal error, lanes 1..28 one perturbed error each (+-delta on the 7 coordinates of each
//                    free endpoint); columns by differences through LDS; J^T J blocks and -J^T e to the edge's scratch row
//   k_pg_assemble    one wave per 7x7 block of H (lower block triangle) and per 7-vector of b: sums the block's edge contributions in the
//                    host's list order (= edge order).  No atomics.  H stays in block form over the trials of an iteration
//   k_pg_fill        dense lower triangle S = H + lambda I for one trial (the factorisation is in place)
//   k_pg_ldlt        n <= BA_LDLT_MAXN: ldlt_solve_wg (ba_ldlt.h) in one workgroup
//   k_pg_big_*       n <= 4096: right-looking blocked LDL^T over many workgroups -- 32-column panels, ldlt_rows for the per-entry
//                    arithmetic, 64x64 trailing tiles: the stages of dense_ldlt_big.h, which k_ba_big_* (ba_reduced_kernels.hip) and k_pg4_big_*
//                    run too (the single-workgroup path's DPP / MFMA forms round differently)
//   k_pg_update      trial estimates Sim3(x_v) * S_v
//   k_pg_errors      chi2 of every active edge;  k_pg_reduce: chi2 and computeScale = sum x (lambda x + b), two stages in a fixed order
//   k_pg_points      P6
//
// k_pg_assemble / _fill / _ldlt / _big_* / _reduce are instances of bodies in pose_graph_common.h and dense_ldlt_big.h, and the host side
// -- graph checks, lists, arena, dense solve chain, LM control -- is pose_graph_common.h's, shared with pose_graph4dof_kernels.hip.  Here:
// the Sim3 edge (linearise, update, errors), the point correction, the stage timer and the entry points.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "geom3.h"
#include "ba_ldlt.h"
#include "sim3_group.h"
#include "pose_graph_common.h"
#pragma clang fp contract(fast)       // as the other double-precision optimisers
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

#define PG_ROW 168            // doubles per edge row: e 7 | Ji^T Ji 49 | Ji^T Jj 49 | Jj^T Jj 49 | -Ji^T e 7 | -Jj^T e 7
#define PG_O_II 7
#define PG_O_IJ 56
#define PG_O_JJ 105
#define PG_O_BI 154
#define PG_O_BJ 161
#define PG_EPB 8              // edges per 256-lane workgroup of k_pg_linearize

struct PgDev : PgDevCommon {               // est [nv][8], meas [ne][8], rows [ne][PG_ROW], Hb [nblk][49]
    int fix_scale;
};

// P2: one edge's computeError
__device__ __forceinline__ void pg_error(const double *C, const double *Si, const double *Sj, double *e)
{
    double Sji[8], T[8], E[8];
    s3_inverse(Sj, Sji);
    s3_mul(C, Si, T);
    s3_mul(T, Sji, E);
    s3_log(E, e);
}

__global__ __launch_bounds__(256) void k_pg_linearize(PgDev G)
{
    __shared__ double errs[PG_EPB][29][7], Jl[PG_EPB][7][14];
    const int tid = threadIdx.x, le = tid >> 5, sub = tid & 31;
    const int e = blockIdx.x * PG_EPB + le;
    const bool live = e < G.ne;
    bool free_i = false, free_j = false;
    if (live) {
        const int vi = G.v0[e], vj = G.v1[e];
        free_i = G.free_idx[vi] >= 0; free_j = G.free_idx[vj] >= 0;
        if (sub < 29) {
            double Si[8], Sj[8], C[8], er[7];
            for (int k = 0; k < 8; k++) { Si[k] = G.est[8 * vi + k]; Sj[k] = G.est[8 * vj + k]; C[k] = G.meas[8 * (size_t)e + k]; }
            if (sub > 0) {
                // P3: vi->oplus(add) with add[c] = +-delta: Sim3(add) * estimate, add[6] = 0 under fix_scale
                const int k = sub - 1, side = k / 14, c = (k % 14) >> 1;
                if (side == 0 ? free_i : free_j) {
                    double u[7] = {0, 0, 0, 0, 0, 0, 0}, E[8], Sn[8];
                    const double dl = (k & 1) ? -1e-9 : 1e-9;
#pragma unroll
                    for (int q = 0; q < 7; q++) u[q] = q == c ? dl : 0.0;
                    if (G.fix_scale) u[6] = 0;
                    s3_exp(u, E);
                    double *T = side == 0 ? Si : Sj;
                    s3_mul(E, T, Sn);
                    for (int q = 0; q < 8; q++) T[q] = Sn[q];
                }
            }
            pg_error(C, Si, Sj, er);
            for (int r = 0; r < 7; r++) errs[le][sub][r] = er[r];
        }
    }
    __syncthreads();
    if (live) {
        const double scalar = 1.0 / (2 * 1e-9);
        for (int idx = sub; idx < 98; idx += 32) {
            const int r = idx / 14, col = idx % 14;
            const bool fr = col < 7 ? free_i : free_j;
            Jl[le][r][col] = fr ? scalar * (errs[le][1 + 2 * col][r] - errs[le][2 + 2 * col][r]) : 0.0;
        }
    }
    __syncthreads();
    if (!live) return;
    double *row = G.rows + (size_t)e * PG_ROW;
    for (int idx = sub; idx < PG_ROW; idx += 32) {
        double v;
        if (idx < 7) v = errs[le][0][idx];
        else if (idx < PG_O_BI) {
            const int w = (idx - 7) / 49, k = (idx - 7) % 49, a = k / 7, c = k % 7;
            const int ca = w == 2 ? 7 + a : a, cc = w == 0 ? c : 7 + c;
            v = 0;
            for (int r = 0; r < 7; r++) v += Jl[le][r][ca] * Jl[le][r][cc];
        } else {
            const int a = idx - PG_O_BI;                  // 0..13: column of J
            v = 0;
            for (int r = 0; r < 7; r++) v += Jl[le][r][a] * (-errs[le][0][r]);
        }
        row[idx] = v;
    }
}

// the shared bodies (pose_graph_common.h, dense_ldlt_big.h) at this graph's edge-row layout
struct PgRow7 { enum { D = 7, ROW = PG_ROW, II = PG_O_II, IJ = PG_O_IJ, JJ = PG_O_JJ, BI = PG_O_BI, BJ = PG_O_BJ }; };

__global__ __launch_bounds__(64) void k_pg_assemble(PgDev G) { pg_assemble_body<PgRow7>(G); }
__global__ __launch_bounds__(64) void k_pg_fill(PgDev G, double lambda) { pg_fill_body<PgRow7>(G, lambda); }
__global__ __launch_bounds__(1024) void k_pg_ldlt(PgDev G) { pg_ldlt_body(G); }

// ---- n > BA_LDLT_MAXN: the many-workgroup factorisation (see the head of the file)
__global__ __launch_bounds__(256) void k_pg_big_init(PgDev G) { dense_big_init(pg_dense_sys(G), blockIdx.x); }
__global__ __launch_bounds__(64) void k_pg_big_diag(PgDev G, int p0) { dense_big_diag(pg_dense_sys(G), p0); }
__global__ __launch_bounds__(256) void k_pg_big_rows(PgDev G, int p0)
{
    extern __shared__ double brl[];
    dense_big_rows(pg_dense_sys(G), p0, blockIdx.x, brl);
}
__global__ __launch_bounds__(256) void k_pg_big_trail(PgDev G, int p0) { dense_big_trail(pg_dense_sys(G), p0, blockIdx.y, blockIdx.x); }
__global__ __launch_bounds__(1024) void k_pg_big_backsub(PgDev G)
{
    extern __shared__ double bbl[];
    const bool ok = dense_big_backsub(pg_dense_sys(G), G.n, bbl);
    if (threadIdx.x == 0) G.result[2] = ok ? 1.0 : 0.0;
}

// P5 / sparse_optimizer.cpp:422-435: the trial estimate of every free vertex, Sim3(x_v) * S_v (types_seven_dof_expmap.h:60-69 -- under
// fix_scale the zero is written through to the solver's x, as the reference's Eigen::Map does)
__global__ __launch_bounds__(64) void k_pg_update(PgDev G)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= G.nf) return;
    const int v = G.free_list[f];
    double u[7], E[8], S[8], Sn[8];
    for (int k = 0; k < 7; k++) u[k] = G.x[7 * f + k];
    if (G.fix_scale) { u[6] = 0; G.x[7 * f + 6] = 0; }
    for (int k = 0; k < 8; k++) S[k] = G.est[8 * v + k];
    s3_exp(u, E);
    s3_mul(E, S, Sn);
    for (int k = 0; k < 8; k++) G.est[8 * v + k] = Sn[k];
}

__global__ __launch_bounds__(64) void k_pg_errors(PgDev G)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= G.ne) return;
    const int vi = G.v0[e], vj = G.v1[e];
    double Si[8], Sj[8], C[8], er[7];
    for (int k = 0; k < 8; k++) { Si[k] = G.est[8 * vi + k]; Sj[k] = G.est[8 * vj + k]; C[k] = G.meas[8 * (size_t)e + k]; }
    pg_error(C, Si, Sj, er);
    double c = 0;
    for (int r = 0; r < 7; r++) c += er[r] * er[r];
    G.chi_e[e] = c;
}

__global__ __launch_bounds__(256) void k_pg_reduce(PgDev G, double lambda) { pg_reduce_body(G, lambda); }

// P6
__global__ __launch_bounds__(256) void k_pg_points(const float *Xw, const int32_t *ref, int n_points, const double *Scw, const double *Swc, int nv, float *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int r = ref[i];
    const float x0 = Xw[3 * (size_t)i], x1 = Xw[3 * (size_t)i + 1], x2 = Xw[3 * (size_t)i + 2];
    if (r < 0 || r >= nv) { out[3 * (size_t)i] = x0; out[3 * (size_t)i + 1] = x1; out[3 * (size_t)i + 2] = x2; return; }
    double A[8], B[8];
    for (int k = 0; k < 8; k++) { A[k] = Scw[8 * (size_t)r + k]; B[k] = Swc[8 * (size_t)r + k]; }
    const double X[3] = {(double)x0, (double)x1, (double)x2};
    double y[3], z[3];
    s3_map(A, X, y);
    s3_map(B, y, z);
    out[3 * (size_t)i] = (float)z[0]; out[3 * (size_t)i + 1] = (float)z[1]; out[3 * (size_t)i + 2] = (float)z[2];
}

// ORBHIP_PG_PROF=1: every stage is bracketed by two events on the stream and its DEVICE time (hipEventElapsedTime, microseconds) is summed
// here: linearise, assemble, fill + factor + solve, update + errors + reductions; then trials, iterations, calls.  Debug only: plain
// process-wide sums, not synchronised -- one profiled caller at a time.
double g_pg_prof[7];
thread_local int g_pg_last_path = -1;       // which factorisation the calling thread's last solved graph took: 0 one workgroup, 1 many
struct PgTimer {
    bool on; hipStream_t s; hipEvent_t e0, e1;
    PgTimer(bool on_, hipStream_t s_) : on(on_), s(s_), e0(nullptr), e1(nullptr) { if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) on = false; }
    ~PgTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    void start() { if (on) (void)hipEventRecord(e0, s); }
    void stop(int i)
    {
        if (!on) return;
        float ms = 0;
        if (hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) g_pg_prof[i] += 1e3 * (double)ms;
    }
};

#define PG_FN "orbhip_optimize_essential_graph_host: "
const PgKernels<PgDev> PG_KERNELS = {"k_pg", k_pg_fill, k_pg_ldlt, k_pg_big_init, k_pg_big_diag, k_pg_big_rows, k_pg_big_trail, k_pg_big_backsub, k_pg_reduce};

int pg_check(const orbhip_pose_graph *graphs, int n_graphs, const orbhip_pose_graph_params *p, double *const *sim3)
{
    if (!(p->iterations >= 1)) return pg_fail(ORBHIP_E_BADARG, PG_FN "iterations < 1");
    if (!(p->max_trials >= 1)) return pg_fail(ORBHIP_E_BADARG, PG_FN "max_trials < 1");
    if (!(std::isfinite(p->lambda_init) && p->lambda_init > 0)) return pg_fail(ORBHIP_E_BADARG, PG_FN "lambda_init is not finite and positive");
    if ((long)p->iterations * p->max_trials > (1L << 24)) return pg_fail(ORBHIP_E_BADARG, PG_FN "iterations * max_trials beyond 2^24");
    return pg_check_graphs(PG_FN, "sim3_inout", graphs, n_graphs, sim3, 8, 8, 7);
}

int pg_solve_one(orbhip_ctx *ctx, const orbhip_pose_graph &graph, const orbhip_pose_graph_params *p, double *sim3, orbhip_pose_graph_stats *st,
                 double *trace)
{
    PgRun<PgDev> R;
    R.fn = PG_FN; R.K = PG_KERNELS;
    memset(&R.D, 0, sizeof(R.D));
    R.D.fix_scale = p->fix_scale ? 1 : 0;
    int rc = pg_setup(ctx, graph, 7, 8, 8, PG_ROW, R, [&](double *est) { memcpy(est, sim3, sizeof(double) * 8 * (size_t)graph.n_vertices); });
    if (rc) return rc;
    const PgLists &H = R.H;
    const PgDev &D = R.D;
    orbhip_pose_graph_stats S;
    memset(&S, 0, sizeof(S));
    S.n_free = H.nf; S.n_unknowns = H.n; S.lambda = 0;
    if (H.nf == 0 || H.ne == 0) { if (st) *st = S; return ORBHIP_OK; }
    hipStream_t s = R.s;

    PgTimer T(getenv("ORBHIP_PG_PROF") && atoi(getenv("ORBHIP_PG_PROF")) != 0, s);
    g_pg_last_path = R.big ? 1 : 0;
    if (T.on) g_pg_prof[6] += 1;
    PgLmOps ops;
    ops.chi2 = [&](double lambda, double *out3) -> int {
        hipLaunchKernelGGL(k_pg_errors, dim3((H.ne + 63) / 64), dim3(64), 0, s, D);
        return pg_reduce_read(R, lambda, out3);
    };
    ops.build = [&]() -> int {
        T.start();
        hipLaunchKernelGGL(k_pg_linearize, dim3((H.ne + PG_EPB - 1) / PG_EPB), dim3(256), 0, s, D);
        T.stop(0); T.start();
        hipLaunchKernelGGL(k_pg_assemble, dim3(H.nblk + H.nf), dim3(64), 0, s, D);
        T.stop(1);
        if (T.on) g_pg_prof[5] += 1;
        return ORBHIP_OK;
    };
    ops.lambda_start = [&](double *lambda) -> int { *lambda = p->lambda_init; return ORBHIP_OK; };      // computeLambdaInit with a user value (:171-174)
    ops.solve = [&](double lambda) -> int {
        T.start();
        const int r = pg_solve(R, lambda);
        if (!r) T.stop(2);
        return r;
    };
    ops.update = [&](double lambda, double *out3) -> int {
        T.start();
        hipLaunchKernelGGL(k_pg_update, dim3((H.nf + 63) / 64), dim3(64), 0, s, D);
        const int r = ops.chi2(lambda, out3);
        if (r) return r;
        T.stop(3);
        if (T.on) g_pg_prof[4] += 1;
        return ORBHIP_OK;
    };
    if ((rc = pg_lm_run(R, ops, p->iterations, p->max_trials, trace, S))) return rc;
    if (S.end_reason != ORBHIP_PG_END_SOLVE_FAILED) {
        if ((rc = pg_read_est(R))) return rc;
        memcpy(sim3, R.rb, R.est_bytes);
    }
    if (st) *st = S;
    return ORBHIP_OK;
}

}  // namespace

extern "C" int orbhip_debug_pose_graph_prof(double *out7, int reset)      // see g_pg_prof
{
    if (out7) memcpy(out7, g_pg_prof, sizeof(g_pg_prof));
    if (reset) memset(g_pg_prof, 0, sizeof(g_pg_prof));
    return ORBHIP_OK;
}

extern "C" int orbhip_debug_pose_graph_last_path(void) { return g_pg_last_path; }

// the dense solve chain of a trial (pg_factor_launch) on a system given by the caller, without k_pg_fill
extern "C" int orbhip_debug_pose_graph_dense_solve_host(orbhip_ctx *ctx, const double *S, int n, const double *rhs, double *x_out, int force_big, int *ok_out)
{
#define PG_DS_FN "orbhip_debug_pose_graph_dense_solve_host: "
    if (!ctx || !S || !rhs || !x_out || !ok_out) return pg_fail(ORBHIP_E_BADARG, PG_DS_FN "ctx / S / rhs / x_out / ok_out is NULL");
    if (n < 1) return pg_fail(ORBHIP_E_BADARG, PG_DS_FN "n < 1");
    if (n > PG_MAXN) return pg_fail(ORBHIP_E_CAPACITY, PG_DS_FN "n = %d, at most %d", n, PG_MAXN);
    PgRun<PgDev> R;
    R.fn = PG_DS_FN; R.K = PG_KERNELS;
    memset(&R.D, 0, sizeof(R.D));
    PgDev &D = R.D;
    D.n = n;
    R.big = n > BA_LDLT_MAXN || force_big != 0;
    g_pg_last_path = R.big ? 1 : 0;
    R.s = orbhip_ctx_stream_internal(ctx); R.dev = orbhip_ctx_device_internal(ctx);
    const size_t nn = (size_t)n * n;
    char *blob = (char *)orbhip_ctx_pinned_internal(ctx, sizeof(double) * (nn + n + 4));
    if (!blob) return ORBHIP_E_HIP;
    size_t total = 0;
    for (int pass = 0; pass < 2; pass++) {                   // the arena's size, then its pointers
        Carve c{pass ? (char *)orbhip_ctx_work_internal(ctx, total) : nullptr};
        if (pass && !c.base) return ORBHIP_E_HIP;
        D.S = c.take<double>(nn); D.b = c.take<double>(n); D.x = c.take<double>(n);
        D.big_y = c.take<double>(n); D.big_d = c.take<double>(n); D.big_U = c.take<double>(LD_NB * LD_NB);
        D.fail = c.take<int32_t>(1); D.result = c.take<double>(4);
        total = c.off;
    }
    R.rb = reinterpret_cast<double *>(blob);
    memcpy(R.rb, S, sizeof(double) * nn);
    memcpy(R.rb + nn, rhs, sizeof(double) * n);
    ORB_HIP_TRY(hipSetDevice(R.dev));
    ORB_HIP_TRY(hipMemcpyAsync(D.S, R.rb, sizeof(double) * nn, hipMemcpyHostToDevice, R.s));
    ORB_HIP_TRY(hipMemcpyAsync(D.b, R.rb + nn, sizeof(double) * n, hipMemcpyHostToDevice, R.s));
    int rc = pg_lds_optin(R);
    if (rc) return rc;
    pg_factor_launch(R);
    if (hipGetLastError() != hipSuccess) return pg_fail(ORBHIP_E_HIP, PG_DS_FN "a kernel launch failed");
    ORB_HIP_TRY(hipMemcpyAsync(R.rb, D.x, sizeof(double) * n, hipMemcpyDeviceToHost, R.s));
    ORB_HIP_TRY(hipMemcpyAsync(R.rb + n, D.result, 4 * sizeof(double), hipMemcpyDeviceToHost, R.s));
    ORB_HIP_TRY(hipStreamSynchronize(R.s));
    *ok_out = R.rb[n + 2] != 0.0 ? 1 : 0;
    if (*ok_out) memcpy(x_out, R.rb, sizeof(double) * n);    // a failed solve leaves x as it was
    return ORBHIP_OK;
#undef PG_DS_FN
}

extern "C" void orbhip_pose_graph_default_params(orbhip_pose_graph_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->iterations = 20; p->lambda_init = 1e-16; p->fix_scale = 0; p->max_trials = 100;
}

extern "C" int orbhip_optimize_essential_graph_host(orbhip_ctx *ctx, const orbhip_pose_graph *graphs, int n_graphs, const orbhip_pose_graph_params *params,
        double *const *sim3_inout, orbhip_pose_graph_stats *stats_out, double *trace_out)
{
    if (!ctx || !graphs || n_graphs < 0 || !params || !sim3_inout)
        return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: ctx / graphs / params / sim3_inout is NULL or n_graphs < 0");
    int rc = pg_check(graphs, n_graphs, params, sim3_inout);
    if (rc) return rc;
    const size_t stride = (size_t)params->iterations * params->max_trials * ORBHIP_PG_TRACE;
    for (int g = 0; g < n_graphs; g++)
        if ((rc = pg_solve_one(ctx, graphs[g], params, sim3_inout[g], stats_out ? stats_out + g : nullptr, trace_out ? trace_out + g * stride : nullptr))) return rc;
    return ORBHIP_OK;
}

extern "C" int orbhip_pose_graph_correct_points_device(orbhip_ctx *ctx, const float *d_Xw, const int32_t *d_ref, int n_points,
        const double *d_Scw, const double *d_corrected_Swc, int n_vertices, float *d_Xw_out)
{
    if (!ctx || n_points < 0 || n_vertices < 0 || (n_points > 0 && (!d_Xw || !d_ref || !d_Xw_out)) || (n_vertices > 0 && (!d_Scw || !d_corrected_Swc)))
        return pg_fail(ORBHIP_E_BADARG, "orbhip_pose_graph_correct_points_device: bad argument");
    if (n_points == 0) return ORBHIP_OK;
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    hipLaunchKernelGGL(k_pg_points, dim3((n_points + 255) / 256), dim3(256), 0, orbhip_ctx_stream_internal(ctx), d_Xw, d_ref, n_points, d_Scw, d_corrected_Swc,
                       n_vertices, d_Xw_out);
    if (hipGetLastError() != hipSuccess) return pg_fail(ORBHIP_E_HIP, "k_pg_points launch");
    return ORBHIP_OK;
}

// the same with HOST pointers: one page-locked blob up, one down; synchronous.  What host/Optimizer_OptimizeEssentialGraph.cc calls
extern "C" int orbhip_pose_graph_correct_points_host(orbhip_ctx *ctx, const float *Xw, const int32_t *ref, int n_points,
        const double *Scw, const double *corrected_Swc, int n_vertices, float *Xw_out)
{
    if (!ctx || n_points < 0 || n_vertices < 0 || (n_points > 0 && (!Xw || !ref || !Xw_out)) || (n_vertices > 0 && (!Scw || !corrected_Swc)))
        return pg_fail(ORBHIP_E_BADARG, "orbhip_pose_graph_correct_points_host: bad argument");
    if (n_points == 0) return ORBHIP_OK;
    const size_t bS = align256(sizeof(double) * 8 * (size_t)n_vertices), bX = align256(sizeof(float) * 3 * (size_t)n_points), bR = align256(sizeof(int32_t) * (size_t)n_points);
    const size_t total = 2 * bS + 2 * bX + bR;
    char *dev = (char *)orbhip_ctx_work_internal(ctx, total), *blob = (char *)orbhip_ctx_pinned_internal(ctx, total);
    if (!dev || !blob) return ORBHIP_E_HIP;
    if (n_vertices) { memcpy(blob, Scw, sizeof(double) * 8 * (size_t)n_vertices); memcpy(blob + bS, corrected_Swc, sizeof(double) * 8 * (size_t)n_vertices); }
    memcpy(blob + 2 * bS, Xw, sizeof(float) * 3 * (size_t)n_points);
    memcpy(blob + 2 * bS + bX, ref, sizeof(int32_t) * (size_t)n_points);
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    ORB_HIP_TRY(hipMemcpyAsync(dev, blob, 2 * bS + bX + bR, hipMemcpyHostToDevice, s));
    float *d_out = (float *)(dev + 2 * bS + bX + bR);
    const int rc = orbhip_pose_graph_correct_points_device(ctx, (const float *)(dev + 2 * bS), (const int32_t *)(dev + 2 * bS + bX), n_points, (const double *)dev,
                                                           (const double *)(dev + bS), n_vertices, d_out);
    if (rc) return rc;
    ORB_HIP_TRY(hipMemcpyAsync(blob, d_out, sizeof(float) * 3 * (size_t)n_points, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    memcpy(Xw_out, blob, sizeof(float) * 3 * (size_t)n_points);
    return ORBHIP_OK;
}
