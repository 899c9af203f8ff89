// pose_graph_common.h -- what the two pose-graph optimisers share: pose_graph_kernels.hip (Sim3, 7 unknowns per vertex) and
// pose_graph4dof_kernels.hip (yaw + translation, 4).  Included by those two files only; everything here is per translation unit (no
// kernel is shared across files, see the Makefile), the kernels themselves are thin instances in the two files.
//
//   device   PgDevCommon, the argument block both kernels' structs derive from; the bodies of k_pg*_assemble / _fill / _reduce as
//            templates over the edge-row layout (block size D, row length, offsets of the row's parts); pg_dense_sys, the view
//            that k_pg*_ldlt (ldlt_solve_wg, ba_ldlt.h) and k_pg*_big_* (dense_ldlt_big.h) work on
//   host     the graph checks with their messages, the list builder (pose_graph_lists.h), the arena / blob layout and the upload,
//            the LDS opt-ins, the dense solve chain, the read-backs and g2o's Levenberg-Marquardt control over a few callbacks
//
// Floating-point contraction: this header stands above its includers' `#pragma clang fp contract(fast)`, so the device bodies that
// do arithmetic open with their own, as geom3.h does.  Summation orders are the lists' (edge order) and fixed trees: part of the bits.
#pragma once
#include "orb_internal.h"
#include "ctx_internal.h"
#include "ba_ldlt.h"
#include "dense_ldlt_big.h"
#include "pose_graph_lists.h"
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace {

#define PG_MAXN 4096          // unknowns the dense factorisation takes

struct PgDevCommon {
    int nv, ne, nf, n, nblk;                // vertices, ACTIVE edges, free vertices, unknowns, blocks of the lower block triangle
    double *est, *est_bk;                   // [nv][est stride]
    const int32_t *free_idx, *free_list;    // [nv] -> free index or -1; [nf] -> vertex
    const int32_t *v0, *v1;                 // [ne]
    const double *meas;                     // [ne][meas stride]
    double *rows, *chi_e;                   // [ne][row length], [ne]
    const int32_t *blk_bi, *blk_bj, *blk_start, *blk_item;       // block (bi >= bj); items: edge << 2 | kind
    const int32_t *vb_start, *vb_item;      // per free vertex; items: edge << 1 | side
    double *Hb, *b, *x;                     // [nblk][D * D], [n], [n]
    double *S;                              // [n][n]
    double *big_y, *big_d, *big_U;          // [n], [n], [32 * 32]
    int32_t *fail;                          // [1] many-workgroup factorisation: a pivot was zero / non-finite
    double *result;                         // [4] chi2, computeScale, solve ok, (4-DoF) max |H(j, j)|
};

// An edge-row layout L has: D (unknowns per vertex), ROW (doubles per edge row) and the offsets in the row of Ji^T Ji (II), Ji^T Jj
// (IJ), Jj^T Jj (JJ), -Ji^T e (BI), -Jj^T e (BJ).

// one wave per D x D block of H (lower block triangle) and per D-vector of b: the contributions summed in the lists' order.  No atomics
template <class L>
__device__ __forceinline__ void pg_assemble_body(const PgDevCommon &G)
{
#pragma clang fp contract(fast)
    constexpr int D = L::D;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x < G.nblk) {
        const int blk = blockIdx.x;
        if (lane >= D * D) return;
        const int tr = (lane % D) * D + lane / D;
        double acc = 0;
        for (int k = G.blk_start[blk]; k < G.blk_start[blk + 1]; k++) {
            const int it = G.blk_item[k], kind = it & 3;
            const double *row = G.rows + (size_t)(it >> 2) * L::ROW;
            acc += kind == 0 ? row[L::II + lane] : kind == 1 ? row[L::IJ + lane] : kind == 2 ? row[L::IJ + tr] : row[L::JJ + lane];
        }
        G.Hb[(size_t)blk * (D * D) + lane] = acc;
    } else {
        const int f = blockIdx.x - G.nblk;
        if (f >= G.nf || lane >= D) return;
        double acc = 0;
        for (int k = G.vb_start[f]; k < G.vb_start[f + 1]; k++) {
            const int it = G.vb_item[k];
            acc += G.rows[(size_t)(it >> 1) * L::ROW + ((it & 1) ? L::BJ : L::BI) + lane];
        }
        G.b[D * f + lane] = acc;
    }
}

// S (zeroed by the caller) <- the lower triangle of H + lambda I
template <class L>
__device__ __forceinline__ void pg_fill_body(const PgDevCommon &G, double lambda)
{
#pragma clang fp contract(fast)
    constexpr int D = L::D;
    const int blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= G.nblk || lane >= D * D) return;
    const int bi = G.blk_bi[blk], bj = G.blk_bj[blk], a = lane / D, c = lane % D;
    if (bi == bj && c > a) return;
    G.S[(size_t)(D * bi + a) * G.n + D * bj + c] = G.Hb[(size_t)blk * (D * D) + lane] + ((bi == bj && a == c) ? lambda : 0.0);
}

// chi2 = sum of the edges' chi2 and computeScale (levenberg.cpp:187-194): per lane a strided sum in index order, then a binary tree
__device__ __forceinline__ void pg_reduce_body(const PgDevCommon &G, double lambda)
{
#pragma clang fp contract(fast)
    __shared__ double sc[256], ss[256];
    const int tid = threadIdx.x;
    double c = 0, s = 0;
    for (int e = tid; e < G.ne; e += 256) c += G.chi_e[e];
    for (int j = tid; j < G.n; j += 256) { const double xj = G.x[j]; s += xj * (lambda * xj + G.b[j]); }
    sc[tid] = c; ss[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { sc[tid] += sc[tid + w]; ss[tid] += ss[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { G.result[0] = sc[0]; G.result[1] = ss[0]; }
}

// the dense system S x = b of one trial, as ldlt_solve_wg and the dense_big_* stages see it
__device__ __forceinline__ DenseSys pg_dense_sys(const PgDevCommon &G)
{
    return DenseSys{G.S, G.n, G.n, G.b, G.x, G.big_y, G.big_d, G.big_U, G.fail};
}

__device__ __forceinline__ void pg_ldlt_body(const PgDevCommon &G)
{
    const bool ok = ldlt_solve_wg(G.S, G.n, G.n, G.b, G.x, G.n);
    if (threadIdx.x == 0) G.result[2] = ok ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- host

thread_local char g_pgc_msg[320];
__attribute__((format(printf, 2, 3))) int pg_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_pgc_msg, sizeof(g_pgc_msg), fmt, ap);
    va_end(ap);
    orbhip_set_last_error_internal(g_pgc_msg);
    return code;
}

// The graph checks of both entry points.  fn: "<function name>: "; state_name: the estimates' array in the messages; state_stride /
// meas_stride: doubles per vertex / per edge; dof: unknowns per vertex.  GRAPH is orbhip_pose_graph or orbhip_pose_graph4dof
template <class GRAPH>
int pg_check_graphs(const char *fn, const char *state_name, const GRAPH *graphs, int n_graphs, double *const *state, int state_stride, int meas_stride, int dof)
{
    for (int g = 0; g < n_graphs; g++) {
        const GRAPH &G = graphs[g];
        if (G.n_vertices < 0) return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: n_vertices < 0", fn, g);
        if (G.n_edges < 0) return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: n_edges < 0", fn, g);
        if (G.n_vertices > 0 && !G.fixed) return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: fixed is NULL", fn, g);
        if (G.n_vertices > 0 && !state[g]) return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: %s is NULL", fn, g, state_name);
        if (G.n_edges > 0 && (!G.edge_v0 || !G.edge_v1 || !G.edge_meas))
            return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: edge_v0 / edge_v1 / edge_meas is NULL", fn, g);
        for (int e = 0; e < G.n_edges; e++) {
            if (G.edge_v0[e] < 0 || G.edge_v0[e] >= G.n_vertices)
                return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: edge_v0[%d] = %d is outside the vertices", fn, g, e, (int)G.edge_v0[e]);
            if (G.edge_v1[e] < 0 || G.edge_v1[e] >= G.n_vertices)
                return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: edge_v1[%d] = %d is outside the vertices", fn, g, e, (int)G.edge_v1[e]);
            if (G.edge_v0[e] == G.edge_v1[e])
                return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: edge_v0[%d] == edge_v1[%d]: an edge from a vertex to itself", fn, g, e, e);
            for (int k = 0; k < meas_stride; k++)
                if (!std::isfinite(G.edge_meas[meas_stride * (size_t)e + k]))
                    return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: edge_meas[%d][%d] is not finite", fn, g, e, k);
        }
        int nf = 0;
        for (int v = 0; v < G.n_vertices; v++) {
            nf += G.fixed[v] ? 0 : 1;
            for (int k = 0; k < state_stride; k++)
                if (!std::isfinite(state[g][state_stride * (size_t)v + k]))
                    return pg_fail(ORBHIP_E_BADARG, "%sgraph %d: %s[%d][%d] is not finite", fn, g, state_name, v, k);
        }
        if ((long)dof * nf > PG_MAXN)
            return pg_fail(ORBHIP_E_CAPACITY, "%sgraph %d: %ld unknowns (%d free keyframes), at most %d (%d): "
                           "a map of this size needs a sparse factorisation; nothing was changed, there is no CPU fallback", fn, g, (long)dof * nf, nf, PG_MAXN, PG_MAXN / dof);
    }
    return ORBHIP_OK;
}

// test-only: the many-workgroup factorisation for every size.  Read at every call
inline bool pg_force_big() { return getenv("ORBHIP_PG_FORCE_BIG") && atoi(getenv("ORBHIP_PG_FORCE_BIG")) != 0; }

// the kernels of one optimiser (DEV is its argument block, derived from PgDevCommon) that the shared host code launches
template <class DEV>
struct PgKernels {
    const char *name;                       // "k_pg" / "k_pg4", for the messages
    void (*fill)(DEV, double);
    void (*ldlt)(DEV);
    void (*big_init)(DEV);
    void (*big_diag)(DEV, int);
    void (*big_rows)(DEV, int);
    void (*big_trail)(DEV, int);
    void (*big_backsub)(DEV);
    void (*reduce)(DEV, double);
};

// one graph's solve: its lists, its argument block (pointers into the context's work arena) and what the launches need
template <class DEV>
struct PgRun {
    const char *fn;                         // "<function name>: "
    PgKernels<DEV> K;
    PgLists H;
    DEV D;
    hipStream_t s;
    int dev;
    bool big;                               // the many-workgroup factorisation
    size_t est_bytes, ldlt_lds;
    double *rb;                             // the page-locked blob, reused for the read-backs
};

// LDS opt-ins of the factorisation the run takes
template <class DEV>
int pg_lds_optin(PgRun<DEV> &R)
{
    R.ldlt_lds = ba_ldlt_lds_bytes(R.D.n);
    if (!R.big) { if (orb_lds_optin(reinterpret_cast<const void *>(R.K.ldlt), R.dev, R.ldlt_lds)) return pg_fail(ORBHIP_E_HIP, "LDS opt-in (%s_ldlt)", R.K.name); }
    else if (orb_lds_optin(reinterpret_cast<const void *>(R.K.big_rows), R.dev, dense_big_rows_lds()) ||
             orb_lds_optin(reinterpret_cast<const void *>(R.K.big_backsub), R.dev, dense_big_bsub_lds(R.D.n)))
        return pg_fail(ORBHIP_E_HIP, "LDS opt-in (%s_big_*)", R.K.name);
    return ORBHIP_OK;
}

// Lists, arena and upload.  R.fn, R.K and R.D's own fields are the caller's; the counts and pointers of R.D are set here.  est_stride /
// row: doubles per vertex / per edge row on the device; fill_est(est) writes the vertices' start into the blob.  R.H.nf == 0 or
// R.H.ne == 0 on return: nothing to optimise, nothing was allocated
template <class DEV, class GRAPH>
int pg_setup(orbhip_ctx *ctx, const GRAPH &graph, int dof, int meas_stride, int est_stride, int row, PgRun<DEV> &R, const std::function<void(double *)> &fill_est)
{
    PgLists &H = R.H;
    pg_build_lists(graph.n_vertices, graph.fixed, graph.n_edges, graph.edge_v0, graph.edge_v1, graph.edge_meas, dof, meas_stride, H);
    if (H.nf == 0 || H.ne == 0) return ORBHIP_OK;
    const int n = H.n;
    R.big = n > BA_LDLT_MAXN || pg_force_big();
    R.s = orbhip_ctx_stream_internal(ctx);
    R.dev = orbhip_ctx_device_internal(ctx);
    R.est_bytes = sizeof(double) * est_stride * (size_t)H.nv;
    DEV &D = R.D;
    D.nv = H.nv; D.ne = H.ne; D.nf = H.nf; D.n = n; D.nblk = H.nblk;
    // one arena: the uploaded part first (same layout in a host blob), then the work buffers
    auto layout = [&](char *base, PgDevCommon &O, size_t &upload_bytes) {
        Carve c{base};
        O.est = c.take<double>(est_stride * (size_t)H.nv);
        O.meas = c.take<double>(meas_stride * (size_t)H.ne);
        O.free_idx = c.take<int32_t>(H.nv); O.free_list = c.take<int32_t>(H.nf);
        O.v0 = c.take<int32_t>(H.ne); O.v1 = c.take<int32_t>(H.ne);
        O.blk_bi = c.take<int32_t>(H.nblk); O.blk_bj = c.take<int32_t>(H.nblk); O.blk_start = c.take<int32_t>(H.nblk + 1);
        O.blk_item = c.take<int32_t>(H.blk_item.size());
        O.vb_start = c.take<int32_t>(H.nf + 1); O.vb_item = c.take<int32_t>(H.vb_item.size());
        O.x = c.take<double>(n);                                             // starts at zero (uploaded)
        upload_bytes = c.off;
        O.est_bk = c.take<double>(est_stride * (size_t)H.nv);
        O.rows = c.take<double>((size_t)H.ne * row); O.chi_e = c.take<double>(H.ne);
        O.Hb = c.take<double>((size_t)H.nblk * dof * dof); O.b = c.take<double>(n);
        O.S = c.take<double>((size_t)n * n);
        O.big_y = c.take<double>(n); O.big_d = c.take<double>(n); O.big_U = c.take<double>(LD_NB * LD_NB);
        O.fail = c.take<int32_t>(1); O.result = c.take<double>(4);
        return c.off;
    };
    size_t up = 0, up2;
    PgDevCommon Hh = D;
    const size_t total = layout(nullptr, Hh, up);
    char *arena = (char *)orbhip_ctx_work_internal(ctx, total);
    if (!arena) return ORBHIP_E_HIP;
    char *blob = (char *)orbhip_ctx_pinned_internal(ctx, up + 64);           // the estimates' read-back fits: they are the first part of it
    if (!blob) return ORBHIP_E_HIP;
    layout(arena, D, up);
    layout(blob, Hh, up2);
    memset(blob, 0, up);
    fill_est(Hh.est);
    memcpy((void *)Hh.meas, H.meas.data(), sizeof(double) * H.meas.size());
    auto cp = [](const int32_t *dst, const std::vector<int32_t> &v) { if (!v.empty()) memcpy((void *)dst, v.data(), sizeof(int32_t) * v.size()); };
    cp(Hh.free_idx, H.free_idx); cp(Hh.free_list, H.free_list); cp(Hh.v0, H.v0); cp(Hh.v1, H.v1);
    cp(Hh.blk_bi, H.blk_bi); cp(Hh.blk_bj, H.blk_bj); cp(Hh.blk_start, H.blk_start); cp(Hh.blk_item, H.blk_item);
    cp(Hh.vb_start, H.vb_start); cp(Hh.vb_item, H.vb_item);
    ORB_HIP_TRY(hipSetDevice(R.dev));
    ORB_HIP_TRY(hipMemcpyAsync(arena, blob, up, hipMemcpyHostToDevice, R.s));
    ORB_HIP_TRY(hipStreamSynchronize(R.s));                                        // the blob is reused for the read-backs
    R.rb = reinterpret_cast<double *>(blob);
    return pg_lds_optin(R);
}

// the factorisation and solve of S x = b on the run's path (S filled by the caller)
template <class DEV>
void pg_factor_launch(const PgRun<DEV> &R)
{
    const DEV &D = R.D;
    const int n = D.n;
    hipStream_t s = R.s;
    if (!R.big) { hipLaunchKernelGGL(R.K.ldlt, dim3(1), dim3(1024), R.ldlt_lds, s, D); return; }
    hipLaunchKernelGGL(R.K.big_init, dim3((n + 255) / 256), dim3(256), 0, s, D);
    for (int p0 = 0; p0 < n; p0 += LD_NB) {
        const int m2 = n - p0 - LD_NB;
        hipLaunchKernelGGL(R.K.big_diag, dim3(1), dim3(64), 0, s, D, p0);
        if (m2 > 0) {
            hipLaunchKernelGGL(R.K.big_rows, dim3((m2 + 255) / 256), dim3(256), dense_big_rows_lds(), s, D, p0);
            const int nt = (m2 + 63) / 64;
            hipLaunchKernelGGL(R.K.big_trail, dim3(nt, nt), dim3(256), 0, s, D, p0);
        }
    }
    hipLaunchKernelGGL(R.K.big_backsub, dim3(1), dim3(1024), dense_big_bsub_lds(n), s, D);
}

// one trial's dense solve: S = H + lambda I, factored in place
template <class DEV>
int pg_solve(const PgRun<DEV> &R, double lambda)
{
    ORB_HIP_TRY(hipMemsetAsync(R.D.S, 0, sizeof(double) * (size_t)R.D.n * R.D.n, R.s));
    hipLaunchKernelGGL(R.K.fill, dim3(R.D.nblk), dim3(64), 0, R.s, R.D, lambda);
    pg_factor_launch(R);
    return ORBHIP_OK;
}

// the two reductions after the caller's error kernel, read back: out3 = chi2, computeScale, the solve's flag
template <class DEV>
int pg_reduce_read(const PgRun<DEV> &R, double lambda, double *out3)
{
    hipLaunchKernelGGL(R.K.reduce, dim3(1), dim3(256), 0, R.s, R.D, lambda);
    if (hipGetLastError() != hipSuccess) return pg_fail(ORBHIP_E_HIP, "%sa kernel launch failed", R.fn);   // any launch since the last read-back
    ORB_HIP_TRY(hipMemcpyAsync(R.rb, R.D.result, 3 * sizeof(double), hipMemcpyDeviceToHost, R.s));
    ORB_HIP_TRY(hipStreamSynchronize(R.s));
    out3[0] = R.rb[0]; out3[1] = R.rb[1]; out3[2] = R.rb[2];
    return ORBHIP_OK;
}

// what the control loop asks of an optimiser; every callback returns an ORBHIP_* code
struct PgLmOps {
    std::function<int(double lambda, double *out3)> chi2;       // errors at the estimates + pg_reduce_read
    std::function<int()> build;                                 // linearise + assemble (buildSystem)
    std::function<int(double *lambda)> lambda_start;            // computeLambdaInit
    std::function<int(double lambda)> solve;
    std::function<int(double lambda, double *out3)> update;     // the trial estimates from x, then chi2
};

// OptimizationAlgorithmLevenberg::solve per iteration (optimization_algorithm_levenberg.cpp:61-194), SparseOptimizer::optimize around it
// (sparse_optimizer.cpp:355-420).  Fills S's chi2 / lambda / counts / end_reason; the estimates stay on the device (pg_read_est)
template <class DEV>
int pg_lm_run(const PgRun<DEV> &R, const PgLmOps &ops, int iterations, int max_trials, double *trace, orbhip_pose_graph_stats &S)
{
    const DEV &D = R.D;
    double lambda = 0, ni = 2, current_chi = 0, r3[3];
    int nbad = 0, reason = ORBHIP_PG_END_ITERATIONS, iters = 0, trials = 0, rc;
    bool any_solved = false;
    for (int iter = 0; iter < iterations; iter++) {
        if ((rc = ops.chi2(0.0, r3))) return rc;                                   // computeActiveErrors + activeRobustChi2
        current_chi = r3[0];
        if (iter == 0) S.chi2_initial = current_chi;
        const double ini_chi = current_chi;
        if ((rc = ops.build())) return rc;
        if (iter == 0) {
            if ((rc = ops.lambda_start(&lambda))) return rc;
            ni = 2; nbad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            ORB_HIP_TRY(hipMemcpyAsync(D.est_bk, D.est, R.est_bytes, hipMemcpyDeviceToDevice, R.s));       // push: the whole state
            if ((rc = ops.solve(lambda))) return rc;
            if ((rc = ops.update(lambda, r3))) return rc;
            const bool ok2 = r3[2] != 0.0;
            any_solved = any_solved || ok2;
            const double temp_chi = ok2 ? r3[0] : DBL_MAX;
            const double used = lambda;
            rho = (current_chi - temp_chi) / (r3[1] + 1e-3);
            const bool good = rho > 0 && std::isfinite(temp_chi);
            if (good) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha); ni = 2; current_chi = temp_chi;                         // discardTop
            } else {
                lambda *= ni; ni *= 2;
                ORB_HIP_TRY(hipMemcpyAsync(D.est, D.est_bk, R.est_bytes, hipMemcpyDeviceToDevice, R.s));   // pop
            }
            if (trace) { double *t = trace + (size_t)trials * ORBHIP_PG_TRACE; t[0] = temp_chi; t[1] = rho; t[2] = used; t[3] = good ? 1.0 : 0.0; }
            qmax++; trials++;
        } while (rho < 0 && qmax < max_trials);
        iters++;
        if (qmax == max_trials || rho == 0) { reason = (iter == 0 && !any_solved) ? ORBHIP_PG_END_SOLVE_FAILED : ORBHIP_PG_END_TERMINATE; break; }
        if ((ini_chi - current_chi) * 1e3 < ini_chi) nbad++; else nbad = 0;
        if (nbad >= 3) { reason = ORBHIP_PG_END_NBAD; break; }
    }
    S.chi2_final = current_chi; S.lambda = lambda; S.iterations = iters; S.trials = trials; S.end_reason = reason;
    return ORBHIP_OK;
}

// the estimates, device layout, into R.rb
template <class DEV>
int pg_read_est(const PgRun<DEV> &R)
{
    ORB_HIP_TRY(hipMemcpyAsync(R.rb, R.D.est, R.est_bytes, hipMemcpyDeviceToHost, R.s));
    ORB_HIP_TRY(hipStreamSynchronize(R.s));
    return ORBHIP_OK;
}

}  // namespace
