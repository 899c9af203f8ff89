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
//                    arithmetic, 64x64 trailing tiles: the structure of k_ba_big_diag / _rows / _trail / _backsub (ba_kernels.hip) on
//                    plain pointers: the same elimination order and per-entry formula (the single-workgroup path's DPP / MFMA forms round differently)
//   k_pg_update      trial estimates Sim3(x_v) * S_v
//   k_pg_errors      chi2 of every active edge;  k_pg_reduce: chi2 and computeScale = sum x (lambda x + b), two stages in a fixed order
//   k_pg_points      P6
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "geom3.h"
#include "ba_ldlt.h"
#include "sim3_group.h"
#pragma clang fp contract(fast)       // as the other double-precision optimisers
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace {

#define PG_MAXN 4096
#define PG_ROW 168            // doubles per edge row: e 7 | Ji^T Ji 49 | Ji^T Jj 49 | Jj^T Jj 49 | -Ji^T e 7 | -Jj^T e 7
#define PG_O_II 7
#define PG_O_IJ 56
#define PG_O_JJ 105
#define PG_O_BI 154
#define PG_O_BJ 161
#define PG_EPB 8              // edges per 256-lane workgroup of k_pg_linearize

struct PgDev {
    int nv, ne, nf, n, nblk, fix_scale;     // vertices, ACTIVE edges, free vertices, unknowns, blocks of the lower block triangle
    double *est, *est_bk;                   // [nv][8]
    const int32_t *free_idx, *free_list;    // [nv] -> free index or -1; [nf] -> vertex
    const int32_t *v0, *v1;                 // [ne]
    const double *meas;                     // [ne][8]
    double *rows, *chi_e;                   // [ne][PG_ROW], [ne]
    const int32_t *blk_bi, *blk_bj, *blk_start, *blk_item;       // block (bi >= bj); items: edge << 2 | kind
    const int32_t *vb_start, *vb_item;      // per free vertex; items: edge << 1 | side
    double *Hb, *b, *x;                     // [nblk][49], [n], [n]
    double *S;                              // [n][n]
    double *big_y, *big_d, *big_U;          // [n], [n], [32 * 32]
    int32_t *fail;                          // [1] many-workgroup factorisation: a pivot was zero / non-finite
    double *result;                         // [4] chi2, computeScale, solve ok
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

__global__ __launch_bounds__(64) void k_pg_assemble(PgDev G)
{
    const int lane = threadIdx.x;
    if ((int)blockIdx.x < G.nblk) {
        const int blk = blockIdx.x;
        if (lane >= 49) return;
        const int tr = (lane % 7) * 7 + lane / 7;
        double acc = 0;
        for (int k = G.blk_start[blk]; k < G.blk_start[blk + 1]; k++) {
            const int it = G.blk_item[k], kind = it & 3;
            const double *row = G.rows + (size_t)(it >> 2) * PG_ROW;
            acc += kind == 0 ? row[PG_O_II + lane] : kind == 1 ? row[PG_O_IJ + lane] : kind == 2 ? row[PG_O_IJ + tr] : row[PG_O_JJ + lane];
        }
        G.Hb[(size_t)blk * 49 + lane] = acc;
    } else {
        const int f = blockIdx.x - G.nblk;
        if (f >= G.nf || lane >= 7) return;
        double acc = 0;
        for (int k = G.vb_start[f]; k < G.vb_start[f + 1]; k++) {
            const int it = G.vb_item[k];
            acc += G.rows[(size_t)(it >> 1) * PG_ROW + ((it & 1) ? PG_O_BJ : PG_O_BI) + lane];
        }
        G.b[7 * f + lane] = acc;
    }
}

// S (zeroed by the caller) <- the lower triangle of H + lambda I
__global__ __launch_bounds__(64) void k_pg_fill(PgDev G, double lambda)
{
    const int blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= G.nblk || lane >= 49) return;
    const int bi = G.blk_bi[blk], bj = G.blk_bj[blk], a = lane / 7, c = lane % 7;
    if (bi == bj && c > a) return;
    G.S[(size_t)(7 * bi + a) * G.n + 7 * bj + c] = G.Hb[(size_t)blk * 49 + lane] + ((bi == bj && a == c) ? lambda : 0.0);
}

__global__ __launch_bounds__(1024) void k_pg_ldlt(PgDev G)
{
    const bool ok = ldlt_solve_wg(G.S, G.n, G.n, G.b, G.x, G.n);
    if (threadIdx.x == 0) G.result[2] = ok ? 1.0 : 0.0;
}

// ---- n > BA_LDLT_MAXN: the many-workgroup factorisation (see the head of the file)
__global__ __launch_bounds__(256) void k_pg_big_init(PgDev G)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < G.n) G.big_y[i] = G.b[i];
    if (i == 0) *G.fail = 0;
}

__global__ __launch_bounds__(64) void k_pg_big_diag(PgDev G, int p0)
{
    __shared__ double P[LD_NB * LD_PP], U[LD_NB * LD_NB], dv[LD_NB], yv[LD_NB];
    __shared__ int s_ok;
    const int lane = threadIdx.x, n = G.n, ld = G.n;
    if (p0 >= n || *G.fail) return;
    const int nb = min(LD_NB, n - p0);
    double *S = G.S, *y = G.big_y, *d = G.big_d;
    if (lane == 0) s_ok = 1;
    if (lane < nb) {
        for (int c = 0; c < nb; c++) P[lane * LD_PP + c] = S[(size_t)(p0 + lane) * ld + p0 + c];
        yv[lane] = y[p0 + lane];
    }
    wave_lds_sync();
    if (lane < nb) ldlt_rows<true>((lds_f64 *)P, (lds_f64 *)U, (lds_f64 *)dv, (lds_f64 *)yv, lane, nb, &s_ok);
    wave_lds_sync();
    if (!s_ok) { if (lane == 0) *G.fail = 1; return; }
    if (lane < nb) {
        for (int c = 0; c <= lane; c++) S[(size_t)(p0 + lane) * ld + p0 + c] = (c == lane) ? dv[c] : P[lane * LD_PP + c];
        d[p0 + lane] = dv[lane]; y[p0 + lane] = yv[lane];
    }
    for (int k = lane; k < LD_NB * LD_NB; k += 64) G.big_U[k] = U[k];
}

__global__ __launch_bounds__(256) void k_pg_big_rows(PgDev G, int p0)
{
    extern __shared__ double brl[];                  // P [32 + 256][LD_PP] (rows 0..31 unused), U [32*32], dv [32], yv [32 + 256]
    __shared__ int s_dummy;
    const int tid = threadIdx.x, n = G.n, ld = G.n;
    if (p0 >= n || *G.fail) return;
    const int nb = min(LD_NB, n - p0), m = n - p0;
    const int r = nb + blockIdx.x * 256 + tid;           // row of the panel (relative to p0)
    if (nb + (int)blockIdx.x * 256 >= m) return;
    double *P = brl, *U = P + (size_t)(LD_NB + 256) * LD_PP, *dv = U + LD_NB * LD_NB, *yv = dv + LD_NB;
    double *S = G.S, *y = G.big_y;
    for (int k = tid; k < LD_NB * LD_NB; k += 256) U[k] = G.big_U[k];
    if (tid < nb) { dv[tid] = G.big_d[p0 + tid]; yv[tid] = y[p0 + tid]; }
    const int rl = LD_NB + tid;                          // this thread's row inside the LDS panel
    if (r < m) {
        for (int c = 0; c < nb; c++) P[rl * LD_PP + c] = S[(size_t)(p0 + r) * ld + p0 + c];
        yv[rl] = y[p0 + r];
    }
    __syncthreads();
    if (r < m) {
        ldlt_rows<false>((lds_f64 *)P, (lds_f64 *)U, (lds_f64 *)dv, (lds_f64 *)yv, rl, nb, &s_dummy);
        for (int c = 0; c < nb; c++) S[(size_t)(p0 + r) * ld + p0 + c] = P[rl * LD_PP + c];
        y[p0 + r] = yv[rl];
    }
}

// trailing update S[i][k] -= sum_c L[i][c] d_c L[k][c] for i >= k >= p0 + nb: 64x64 tiles of the lower triangle, 4x4 per thread
__global__ __launch_bounds__(256) void k_pg_big_trail(PgDev G, int p0)
{
    __shared__ double LI[64 * LD_PP], LK[64 * LD_PP], dv[LD_NB];
    const int tid = threadIdx.x, n = G.n, ld = G.n;
    if (p0 >= n || *G.fail) return;
    const int nb = min(LD_NB, n - p0);
    const int base = p0 + nb, m2 = n - base;
    const int ti = blockIdx.y, tk = blockIdx.x;
    if (tk > ti || 64 * ti >= m2) return;
    double *S = G.S;
    for (int idx = tid; idx < 64 * LD_NB; idx += 256) {
        const int r = idx >> 5, c = idx & 31;
        const int gi = base + 64 * ti + r, gk = base + 64 * tk + r;
        LI[r * LD_PP + c] = (c < nb && gi < n) ? S[(size_t)gi * ld + p0 + c] : 0.0;
        LK[r * LD_PP + c] = (c < nb && gk < n) ? S[(size_t)gk * ld + p0 + c] : 0.0;
    }
    if (tid < LD_NB) dv[tid] = tid < nb ? G.big_d[p0 + tid] : 0.0;
    __syncthreads();
    const int a0 = 4 * (tid >> 4), b0 = 4 * (tid & 15);
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b2 = 0; b2 < 4; b2++) acc[a][b2] = 0.0;
    for (int c = 0; c < nb; c++) {
        const double dc = dv[c];
        double av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) { av[a] = LI[(a0 + a) * LD_PP + c] * dc; bv[a] = LK[(b0 + a) * LD_PP + c]; }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b2 = 0; b2 < 4; b2++) acc[a][b2] += av[a] * bv[b2];
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b2 = 0; b2 < 4; b2++) {
            const int gi = base + 64 * ti + a0 + a, gk = base + 64 * tk + b0 + b2;
            if (gi < n && gk < n && gk <= gi) S[(size_t)gi * ld + gk] -= acc[a][b2];
        }
}

__global__ __launch_bounds__(1024) void k_pg_big_backsub(PgDev G)
{
    extern __shared__ double bbl[];                  // y [n], red [32*32], P [32][LD_PP]
    const int tid = threadIdx.x, nth = blockDim.x, n = G.n, ld = G.n;
    if (*G.fail) { if (tid == 0) G.result[2] = 0.0; return; }      // x untouched (as the reference on failure)
    double *y = bbl, *red = y + n, *P = red + 32 * 32;
    const double *S = G.S, *dval = G.big_d;
    // y <- D^-1 y, then L^T x = y panel by panel from the bottom
    for (int i = tid; i < n; i += nth) y[i] = G.big_y[i] / dval[i];
    __syncthreads();
    const int last_p0 = ((n - 1) / LD_NB) * LD_NB;
    for (int p0 = last_p0; p0 >= 0; p0 -= LD_NB) {
        const int nb = min(LD_NB, n - p0), m = n - p0;
        {
            const int c = tid & 31, rg = tid >> 5;          // 1024 threads = 32 columns x 32 row groups
            double part = 0.0;
            if (c < nb)
                for (int r = nb + rg; r < m; r += 32) part += S[(size_t)(p0 + r) * ld + p0 + c] * y[p0 + r];
            red[rg * 32 + c] = part;
        }
        for (int idx = tid; idx < nb * LD_NB; idx += nth) {   // diagonal block of L into LDS
            const int r = idx >> 5, c = idx & 31;
            if (c < nb) P[r * LD_PP + c] = S[(size_t)(p0 + r) * ld + p0 + c];
        }
        __syncthreads();
        if (tid < nb) {
            double t = 0.0;
            for (int rg = 0; rg < 32; rg++) t += red[rg * 32 + tid];
            y[p0 + tid] -= t;
        }
        __syncthreads();
        if (tid < 64) {                                       // 32x32 triangular solve inside one wave
            for (int jj = nb - 1; jj >= 0; jj--) {
                wave_lds_sync();
                const double xj = y[p0 + jj];
                if (tid < jj) y[p0 + tid] -= P[jj * LD_PP + tid] * xj;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += nth) G.x[i] = y[i];
    if (tid == 0) G.result[2] = 1.0;
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

// chi2 = sum of the edges' chi2 and computeScale (levenberg.cpp:187-194): per lane a strided sum in index order, then a binary tree
__global__ __launch_bounds__(256) void k_pg_reduce(PgDev G, double lambda)
{
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

thread_local char g_pg_msg[256];
int pg_fail(int code, const char *fmt, long a = 0, long b = 0, long c = 0)
{
    snprintf(g_pg_msg, sizeof(g_pg_msg), fmt, a, b, c);
    orbhip_set_last_error_internal(g_pg_msg);
    return code;
}

int pg_check(const orbhip_pose_graph *graphs, int n_graphs, const orbhip_pose_graph_params *p, double *const *sim3)
{
    if (!(p->iterations >= 1)) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: iterations < 1");
    if (!(p->max_trials >= 1)) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: max_trials < 1");
    if (!(std::isfinite(p->lambda_init) && p->lambda_init > 0)) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: lambda_init is not finite and positive");
    if ((long)p->iterations * p->max_trials > (1L << 24)) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: iterations * max_trials beyond 2^24");
    for (int g = 0; g < n_graphs; g++) {
        const orbhip_pose_graph &G = graphs[g];
        if (G.n_vertices < 0) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: n_vertices < 0", g);
        if (G.n_edges < 0) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: n_edges < 0", g);
        if (G.n_vertices > 0 && !G.fixed) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: fixed is NULL", g);
        if (G.n_vertices > 0 && !sim3[g]) return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: sim3_inout is NULL", g);
        if (G.n_edges > 0 && (!G.edge_v0 || !G.edge_v1 || !G.edge_meas))
            return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: edge_v0 / edge_v1 / edge_meas is NULL", g);
        for (int e = 0; e < G.n_edges; e++) {
            if (G.edge_v0[e] < 0 || G.edge_v0[e] >= G.n_vertices)
                return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: edge_v0[%ld] = %ld is outside the vertices", g, e, G.edge_v0[e]);
            if (G.edge_v1[e] < 0 || G.edge_v1[e] >= G.n_vertices)
                return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: edge_v1[%ld] = %ld is outside the vertices", g, e, G.edge_v1[e]);
            if (G.edge_v0[e] == G.edge_v1[e])
                return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: edge_v0[%ld] == edge_v1[%ld]: an edge from a vertex to itself", g, e, e);
            for (int k = 0; k < 8; k++)
                if (!std::isfinite(G.edge_meas[8 * (size_t)e + k]))
                    return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: edge_meas[%ld][%ld] is not finite", g, e, k);
        }
        int nf = 0;
        for (int v = 0; v < G.n_vertices; v++) {
            nf += G.fixed[v] ? 0 : 1;
            for (int k = 0; k < 8; k++)
                if (!std::isfinite(sim3[g][8 * (size_t)v + k]))
                    return pg_fail(ORBHIP_E_BADARG, "orbhip_optimize_essential_graph_host: graph %ld: sim3_inout[%ld][%ld] is not finite", g, v, k);
        }
        if (7L * nf > PG_MAXN)
            return pg_fail(ORBHIP_E_CAPACITY, "orbhip_optimize_essential_graph_host: graph %ld: %ld unknowns (%ld free keyframes), at most 4096 (585): "
                           "a map of this size needs a sparse factorisation; nothing was changed, there is no CPU fallback", g, 7L * nf, nf);
    }
    return ORBHIP_OK;
}

// the host's lists of one graph, built once: free numbering in ABI order, active edges in edge order, per block / per vertex the
// contributions in edge order
struct PgHost {
    int nv = 0, ne = 0, nf = 0, n = 0, nblk = 0;
    std::vector<int32_t> free_idx, free_list, v0, v1, blk_bi, blk_bj, blk_start, blk_item, vb_start, vb_item;
    std::vector<double> meas;
};

void pg_build(const orbhip_pose_graph &G, PgHost &H)
{
    H.nv = G.n_vertices;
    H.free_idx.assign(H.nv, -1);
    for (int v = 0; v < H.nv; v++) if (!G.fixed[v]) { H.free_idx[v] = (int32_t)H.free_list.size(); H.free_list.push_back(v); }
    H.nf = (int)H.free_list.size(); H.n = 7 * H.nf;
    for (int e = 0; e < G.n_edges; e++) {
        const int a = G.edge_v0[e], b = G.edge_v1[e];
        if (H.free_idx[a] < 0 && H.free_idx[b] < 0) continue;                // not active (sparse_optimizer.cpp:234)
        H.v0.push_back(a); H.v1.push_back(b);
        for (int k = 0; k < 8; k++) H.meas.push_back(G.edge_meas[8 * (size_t)e + k]);
    }
    H.ne = (int)H.v0.size();
    // blocks: every diagonal block, then the off-diagonal ones in order of first appearance
    std::map<std::pair<int, int>, int> id;
    std::vector<std::vector<int32_t>> items(H.nf), vb(H.nf);
    for (int f = 0; f < H.nf; f++) { id[{f, f}] = f; H.blk_bi.push_back(f); H.blk_bj.push_back(f); }
    for (int e = 0; e < H.ne; e++) {
        const int fi = H.free_idx[H.v0[e]], fj = H.free_idx[H.v1[e]];
        if (fi >= 0) { items[fi].push_back(e << 2 | 0); vb[fi].push_back(e << 1 | 0); }
        if (fj >= 0) { items[fj].push_back(e << 2 | 3); vb[fj].push_back(e << 1 | 1); }
        if (fi >= 0 && fj >= 0) {
            const std::pair<int, int> key = fi > fj ? std::make_pair(fi, fj) : std::make_pair(fj, fi);
            auto it = id.find(key);
            if (it == id.end()) { it = id.emplace(key, (int)items.size()).first; items.emplace_back(); H.blk_bi.push_back(key.first); H.blk_bj.push_back(key.second); }
            items[it->second].push_back(e << 2 | (fi > fj ? 1 : 2));         // Ji^T Jj is block (fi, fj); below the diagonal as it is, else transposed
        }
    }
    H.nblk = (int)items.size();
    H.blk_start.push_back(0);
    for (auto &l : items) { H.blk_item.insert(H.blk_item.end(), l.begin(), l.end()); H.blk_start.push_back((int32_t)H.blk_item.size()); }
    H.vb_start.push_back(0);
    for (auto &l : vb) { H.vb_item.insert(H.vb_item.end(), l.begin(), l.end()); H.vb_start.push_back((int32_t)H.vb_item.size()); }
}

struct Carve {
    char *base; size_t off = 0;
    template <class T> T *take(size_t count) { T *p = base ? reinterpret_cast<T *>(base + off) : nullptr; off += align256(count * sizeof(T)); return p; }
};

int pg_solve_one(orbhip_ctx *ctx, const orbhip_pose_graph &graph, const orbhip_pose_graph_params *p, double *sim3, orbhip_pose_graph_stats *st,
                 double *trace)
{
    PgHost H;
    pg_build(graph, H);
    orbhip_pose_graph_stats S;
    memset(&S, 0, sizeof(S));
    S.n_free = H.nf; S.n_unknowns = H.n; S.lambda = 0;
    if (H.nf == 0 || H.ne == 0) { if (st) *st = S; return ORBHIP_OK; }
    const int n = H.n;
    const bool force_big = getenv("ORBHIP_PG_FORCE_BIG") && atoi(getenv("ORBHIP_PG_FORCE_BIG")) != 0;       // test-only: the many-workgroup factorisation for every size
    const bool big = n > BA_LDLT_MAXN || force_big;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    const int dev = orbhip_ctx_device_internal(ctx);

    PgDev D;
    memset(&D, 0, sizeof(D));
    D.nv = H.nv; D.ne = H.ne; D.nf = H.nf; D.n = n; D.nblk = H.nblk; D.fix_scale = p->fix_scale ? 1 : 0;
    // one arena: the uploaded part first (same layout in a host blob), then the work buffers
    auto layout = [&](char *base, PgDev &O, size_t &upload_bytes) {
        Carve c{base};
        O.est = c.take<double>(8 * (size_t)H.nv);
        O.meas = c.take<double>(8 * (size_t)H.ne);
        O.free_idx = c.take<int32_t>(H.nv); O.free_list = c.take<int32_t>(H.nf);
        O.v0 = c.take<int32_t>(H.ne); O.v1 = c.take<int32_t>(H.ne);
        O.blk_bi = c.take<int32_t>(H.nblk); O.blk_bj = c.take<int32_t>(H.nblk); O.blk_start = c.take<int32_t>(H.nblk + 1);
        O.blk_item = c.take<int32_t>(H.blk_item.size());
        O.vb_start = c.take<int32_t>(H.nf + 1); O.vb_item = c.take<int32_t>(H.vb_item.size());
        O.x = c.take<double>(n);                                             // starts at zero (uploaded)
        upload_bytes = c.off;
        O.est_bk = c.take<double>(8 * (size_t)H.nv);
        O.rows = c.take<double>((size_t)H.ne * PG_ROW); O.chi_e = c.take<double>(H.ne);
        O.Hb = c.take<double>((size_t)H.nblk * 49); O.b = c.take<double>(n);
        O.S = c.take<double>((size_t)n * n);
        O.big_y = c.take<double>(n); O.big_d = c.take<double>(n); O.big_U = c.take<double>(LD_NB * LD_NB);
        O.fail = c.take<int32_t>(1); O.result = c.take<double>(4);
        return c.off;
    };
    size_t up = 0;
    PgDev dummy = D;
    const size_t total = layout(nullptr, dummy, up);
    char *arena = (char *)orbhip_ctx_work_internal(ctx, total);
    if (!arena) return ORBHIP_E_HIP;
    char *blob = (char *)orbhip_ctx_pinned_internal(ctx, up + 64);
    if (!blob) return ORBHIP_E_HIP;
    layout(arena, D, up);
    {
        PgDev Hh = D;
        size_t up2;
        layout(blob, Hh, up2);
        memset(blob, 0, up);
        memcpy(Hh.est, sim3, sizeof(double) * 8 * (size_t)H.nv);
        memcpy((void *)Hh.meas, H.meas.data(), sizeof(double) * H.meas.size());
        auto cp = [](const int32_t *dst, const std::vector<int32_t> &v) { if (!v.empty()) memcpy((void *)dst, v.data(), sizeof(int32_t) * v.size()); };
        cp(Hh.free_idx, H.free_idx); cp(Hh.free_list, H.free_list); cp(Hh.v0, H.v0); cp(Hh.v1, H.v1);
        cp(Hh.blk_bi, H.blk_bi); cp(Hh.blk_bj, H.blk_bj); cp(Hh.blk_start, H.blk_start); cp(Hh.blk_item, H.blk_item);
        cp(Hh.vb_start, H.vb_start); cp(Hh.vb_item, H.vb_item);
    }
    ORB_HIP_TRY(hipSetDevice(dev));
    ORB_HIP_TRY(hipMemcpyAsync(arena, blob, up, hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));                                          // the blob is reused for the read-backs below
    double *rb = reinterpret_cast<double *>(blob);

    const size_t ldlt_lds = ba_ldlt_lds_bytes(n);
    const size_t rows_lds = sizeof(double) * ((size_t)(LD_NB + 256) * LD_PP + LD_NB * LD_NB + LD_NB + LD_NB + 256);
    const size_t bsub_lds = sizeof(double) * ((size_t)n + 32 * 32 + LD_NB * LD_PP);
    if (!big) { if (orb_lds_optin(reinterpret_cast<const void *>(k_pg_ldlt), dev, ldlt_lds)) return pg_fail(ORBHIP_E_HIP, "LDS opt-in (k_pg_ldlt)"); }
    else if (orb_lds_optin(reinterpret_cast<const void *>(k_pg_big_rows), dev, rows_lds) || orb_lds_optin(reinterpret_cast<const void *>(k_pg_big_backsub), dev, bsub_lds))
        return pg_fail(ORBHIP_E_HIP, "LDS opt-in (k_pg_big_*)");

    const size_t est_bytes = sizeof(double) * 8 * (size_t)H.nv;
    auto chi2 = [&](double lambda, double *out3) -> int {                          // errors at the estimates + the two reductions, read back
        hipLaunchKernelGGL(k_pg_errors, dim3((H.ne + 63) / 64), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, s, D, lambda);
        if (hipGetLastError() != hipSuccess) return pg_fail(ORBHIP_E_HIP, "orbhip_optimize_essential_graph_host: a kernel launch failed");   // any launch since the last read-back
        ORB_HIP_TRY(hipMemcpyAsync(rb, D.result, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        out3[0] = rb[0]; out3[1] = rb[1]; out3[2] = rb[2];
        return ORBHIP_OK;
    };
    auto solve = [&](double lambda) -> int {
        ORB_HIP_TRY(hipMemsetAsync(D.S, 0, sizeof(double) * (size_t)n * n, s));
        hipLaunchKernelGGL(k_pg_fill, dim3(H.nblk), dim3(64), 0, s, D, lambda);
        if (!big) hipLaunchKernelGGL(k_pg_ldlt, dim3(1), dim3(1024), ldlt_lds, s, D);
        else {
            hipLaunchKernelGGL(k_pg_big_init, dim3((n + 255) / 256), dim3(256), 0, s, D);
            for (int p0 = 0; p0 < n; p0 += LD_NB) {
                const int m2 = n - p0 - LD_NB;
                hipLaunchKernelGGL(k_pg_big_diag, dim3(1), dim3(64), 0, s, D, p0);
                if (m2 > 0) {
                    hipLaunchKernelGGL(k_pg_big_rows, dim3((m2 + 255) / 256), dim3(256), rows_lds, s, D, p0);
                    const int nt = (m2 + 63) / 64;
                    hipLaunchKernelGGL(k_pg_big_trail, dim3(nt, nt), dim3(256), 0, s, D, p0);
                }
            }
            hipLaunchKernelGGL(k_pg_big_backsub, dim3(1), dim3(1024), bsub_lds, s, D);
        }
        return ORBHIP_OK;
    };

    PgTimer T(getenv("ORBHIP_PG_PROF") && atoi(getenv("ORBHIP_PG_PROF")) != 0, s);
    g_pg_last_path = big ? 1 : 0;
    if (T.on) g_pg_prof[6] += 1;
    // P5: OptimizationAlgorithmLevenberg::solve per iteration, SparseOptimizer::optimize around it (sparse_optimizer.cpp:355-420)
    double lambda = 0, ni = 2, current_chi = 0, r3[3];
    int nbad = 0, reason = ORBHIP_PG_END_ITERATIONS, iters = 0, trials = 0;
    bool any_solved = false;
    for (int iter = 0; iter < p->iterations; iter++) {
        int rc = chi2(0.0, r3);                                                    // computeActiveErrors + activeRobustChi2
        if (rc) return rc;
        current_chi = r3[0];
        if (iter == 0) S.chi2_initial = current_chi;
        const double ini_chi = current_chi;
        T.start();
        hipLaunchKernelGGL(k_pg_linearize, dim3((H.ne + PG_EPB - 1) / PG_EPB), dim3(256), 0, s, D);       // buildSystem
        T.stop(0); T.start();
        hipLaunchKernelGGL(k_pg_assemble, dim3(H.nblk + H.nf), dim3(64), 0, s, D);
        T.stop(1);
        if (T.on) g_pg_prof[5] += 1;
        if (iter == 0) { lambda = p->lambda_init; ni = 2; nbad = 0; }              // computeLambdaInit with a user value (:171-174)
        double rho = 0;
        int qmax = 0;
        do {
            ORB_HIP_TRY(hipMemcpyAsync(D.est_bk, D.est, est_bytes, hipMemcpyDeviceToDevice, s));           // push
            T.start();
            if ((rc = solve(lambda))) return rc;
            T.stop(2); T.start();
            hipLaunchKernelGGL(k_pg_update, dim3((H.nf + 63) / 64), dim3(64), 0, s, D);
            if ((rc = chi2(lambda, r3))) return rc;
            T.stop(3);
            if (T.on) g_pg_prof[4] += 1;
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
                ORB_HIP_TRY(hipMemcpyAsync(D.est, D.est_bk, est_bytes, hipMemcpyDeviceToDevice, s));       // pop
            }
            if (trace) { double *t = trace + (size_t)trials * ORBHIP_PG_TRACE; t[0] = temp_chi; t[1] = rho; t[2] = used; t[3] = good ? 1.0 : 0.0; }
            qmax++; trials++;
        } while (rho < 0 && qmax < p->max_trials);
        iters++;
        if (qmax == p->max_trials || rho == 0) { reason = (iter == 0 && !any_solved) ? ORBHIP_PG_END_SOLVE_FAILED : ORBHIP_PG_END_TERMINATE; break; }
        if ((ini_chi - current_chi) * 1e3 < ini_chi) nbad++; else nbad = 0;
        if (nbad >= 3) { reason = ORBHIP_PG_END_NBAD; break; }
    }
    if (reason != ORBHIP_PG_END_SOLVE_FAILED) {
        ORB_HIP_TRY(hipMemcpyAsync(rb, D.est, est_bytes, hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        memcpy(sim3, rb, est_bytes);
    }
    S.chi2_final = current_chi; S.lambda = lambda; S.iterations = iters; S.trials = trials; S.end_reason = reason;
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
