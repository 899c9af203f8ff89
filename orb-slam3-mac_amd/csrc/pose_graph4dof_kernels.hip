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
// The dense H + lambda I machinery is that of pose_graph_kernels.hip with 4 unknowns per vertex: its k_pg_fill / _ldlt / _big_* text is
// repeated here on this file's own argument block (no kernel is shared across translation units, see the Makefile), so that file's code
// is untouched.  One LM trial is a short chain of launches; the control flow runs on the host with one 24-byte read-back per trial.
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
#pragma clang fp contract(fast)       // as the other double-precision optimisers
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace {

#define PG4_MAXN 4096
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

struct Pg4Dev {
    int nv, ne, nf, n, nblk;                // vertices, ACTIVE edges, free vertices, unknowns, blocks of the lower block triangle
    double info[6];                         // the diagonal of the edges' information
    double *est, *est_bk;                   // [nv][PG4_VS]
    const int32_t *free_idx, *free_list;    // [nv] -> free index or -1; [nf] -> vertex
    const int32_t *v0, *v1;                 // [ne]
    const double *meas;                     // [ne][12]: dRij row-major, dtij
    double *rows, *chi_e;                   // [ne][PG4_ROW], [ne]
    const int32_t *blk_bi, *blk_bj, *blk_start, *blk_item;       // block (bi >= bj); items: edge << 2 | kind
    const int32_t *vb_start, *vb_item;      // per free vertex; items: edge << 1 | side
    double *Hb, *b, *x;                     // [nblk][16], [n], [n]
    double *S;                              // [n][n]
    double *big_y, *big_d, *big_U;          // [n], [n], [32 * 32]
    int32_t *fail;                          // [1] many-workgroup factorisation: a pivot was zero / non-finite
    double *result;                         // [4] chi2, computeScale, solve ok, max |H(j, j)|
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

__global__ __launch_bounds__(64) void k_pg4_assemble(Pg4Dev G)
{
    const int lane = threadIdx.x;
    if ((int)blockIdx.x < G.nblk) {
        const int blk = blockIdx.x;
        if (lane >= 16) return;
        const int tr = (lane & 3) * 4 + (lane >> 2);
        double acc = 0;
        for (int k = G.blk_start[blk]; k < G.blk_start[blk + 1]; k++) {
            const int it = G.blk_item[k], kind = it & 3;
            const double *row = G.rows + (size_t)(it >> 2) * PG4_ROW;
            acc += kind == 0 ? row[PG4_O_II + lane] : kind == 1 ? row[PG4_O_IJ + lane] : kind == 2 ? row[PG4_O_IJ + tr] : row[PG4_O_JJ + lane];
        }
        G.Hb[(size_t)blk * 16 + lane] = acc;
    } else {
        const int f = blockIdx.x - G.nblk;
        if (f >= G.nf || lane >= 4) return;
        double acc = 0;
        for (int k = G.vb_start[f]; k < G.vb_start[f + 1]; k++) {
            const int it = G.vb_item[k];
            acc += G.rows[(size_t)(it >> 1) * PG4_ROW + ((it & 1) ? PG4_O_BJ : PG4_O_BI) + lane];
        }
        G.b[4 * f + lane] = acc;
    }
}

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

// S (zeroed by the caller) <- the lower triangle of H + lambda I
__global__ __launch_bounds__(64) void k_pg4_fill(Pg4Dev G, double lambda)
{
    const int blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= G.nblk || lane >= 16) return;
    const int bi = G.blk_bi[blk], bj = G.blk_bj[blk], a = lane >> 2, c = lane & 3;
    if (bi == bj && c > a) return;
    G.S[(size_t)(4 * bi + a) * G.n + 4 * bj + c] = G.Hb[(size_t)blk * 16 + lane] + ((bi == bj && a == c) ? lambda : 0.0);
}

__global__ __launch_bounds__(1024) void k_pg4_ldlt(Pg4Dev G)
{
    const bool ok = ldlt_solve_wg(G.S, G.n, G.n, G.b, G.x, G.n);
    if (threadIdx.x == 0) G.result[2] = ok ? 1.0 : 0.0;
}

// ---- n > BA_LDLT_MAXN: the many-workgroup factorisation, as k_pg_big_* (pose_graph_kernels.hip)
__global__ __launch_bounds__(256) void k_pg4_big_init(Pg4Dev G)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < G.n) G.big_y[i] = G.b[i];
    if (i == 0) *G.fail = 0;
}

__global__ __launch_bounds__(64) void k_pg4_big_diag(Pg4Dev G, int p0)
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

__global__ __launch_bounds__(256) void k_pg4_big_rows(Pg4Dev G, int p0)
{
    extern __shared__ double brl4[];                 // P [32 + 256][LD_PP] (rows 0..31 unused), U [32*32], dv [32], yv [32 + 256]
    __shared__ int s_dummy;
    const int tid = threadIdx.x, n = G.n, ld = G.n;
    if (p0 >= n || *G.fail) return;
    const int nb = min(LD_NB, n - p0), m = n - p0;
    const int r = nb + blockIdx.x * 256 + tid;           // row of the panel (relative to p0)
    if (nb + (int)blockIdx.x * 256 >= m) return;
    double *P = brl4, *U = P + (size_t)(LD_NB + 256) * LD_PP, *dv = U + LD_NB * LD_NB, *yv = dv + LD_NB;
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
__global__ __launch_bounds__(256) void k_pg4_big_trail(Pg4Dev G, int p0)
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

__global__ __launch_bounds__(1024) void k_pg4_big_backsub(Pg4Dev G)
{
    extern __shared__ double bbl4[];                 // y [n], red [32*32], P [32][LD_PP]
    const int tid = threadIdx.x, nth = blockDim.x, n = G.n, ld = G.n;
    if (*G.fail) { if (tid == 0) G.result[2] = 0.0; return; }      // x untouched (as the reference on failure)
    double *y = bbl4, *red = y + n, *P = red + 32 * 32;
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

// chi2 = sum of the edges' chi2 and computeScale (levenberg.cpp:187-194): per lane a strided sum in index order, then a binary tree
__global__ __launch_bounds__(256) void k_pg4_reduce(Pg4Dev G, double lambda)
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

thread_local int g_pg4_last_path = -1;      // which factorisation the calling thread's last solved graph took: 0 one workgroup, 1 many
thread_local char g_pg4_msg[320];
#define PG4_FN "orbhip_optimize_essential_graph4dof_host: "
int pg4_fail(int code, const char *fmt, long a = 0, long b = 0, long c = 0)
{
    snprintf(g_pg4_msg, sizeof(g_pg4_msg), fmt, a, b, c);
    orbhip_set_last_error_internal(g_pg4_msg);
    return code;
}

int pg4_check(const orbhip_pose_graph4dof *graphs, int n_graphs, const orbhip_pose_graph4dof_params *p, double *const *state)
{
    if (!(p->iterations >= 1)) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "iterations < 1");
    if (!(p->max_trials >= 1)) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "max_trials < 1");
    if (!std::isfinite(p->lambda_init)) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "lambda_init is not finite");
    if (!(p->lambda_init > 0) && !(std::isfinite(p->tau) && p->tau > 0))
        return pg4_fail(ORBHIP_E_BADARG, PG4_FN "tau is not finite and positive (and lambda_init <= 0 asks for the computed start)");
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(p->info_diag[k])) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "info_diag[%ld] is not finite", k);
    if ((long)p->iterations * p->max_trials > (1L << 24)) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "iterations * max_trials beyond 2^24");
    for (int g = 0; g < n_graphs; g++) {
        const orbhip_pose_graph4dof &G = graphs[g];
        if (G.n_vertices < 0) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: n_vertices < 0", g);
        if (G.n_edges < 0) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: n_edges < 0", g);
        if (G.n_vertices > 0 && !G.fixed) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: fixed is NULL", g);
        if (G.n_vertices > 0 && !state[g]) return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: state_inout is NULL", g);
        if (G.n_edges > 0 && (!G.edge_v0 || !G.edge_v1 || !G.edge_meas))
            return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: edge_v0 / edge_v1 / edge_meas is NULL", g);
        for (int e = 0; e < G.n_edges; e++) {
            if (G.edge_v0[e] < 0 || G.edge_v0[e] >= G.n_vertices)
                return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: edge_v0[%ld] = %ld is outside the vertices", g, e, G.edge_v0[e]);
            if (G.edge_v1[e] < 0 || G.edge_v1[e] >= G.n_vertices)
                return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: edge_v1[%ld] = %ld is outside the vertices", g, e, G.edge_v1[e]);
            if (G.edge_v0[e] == G.edge_v1[e])
                return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: edge_v0[%ld] == edge_v1[%ld]: an edge from a vertex to itself", g, e, e);
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(G.edge_meas[12 * (size_t)e + k]))
                    return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: edge_meas[%ld][%ld] is not finite", g, e, k);
        }
        int nf = 0;
        for (int v = 0; v < G.n_vertices; v++) {
            nf += G.fixed[v] ? 0 : 1;
            for (int k = 0; k < PG4_ABI; k++)
                if (!std::isfinite(state[g][PG4_ABI * (size_t)v + k]))
                    return pg4_fail(ORBHIP_E_BADARG, PG4_FN "graph %ld: state_inout[%ld][%ld] is not finite", g, v, k);
        }
        if (4L * nf > PG4_MAXN)
            return pg4_fail(ORBHIP_E_CAPACITY, PG4_FN "graph %ld: %ld unknowns (%ld free keyframes), at most 4096 (1024): "
                            "a map of this size needs a sparse factorisation; nothing was changed, there is no CPU fallback", g, 4L * nf, nf);
    }
    return ORBHIP_OK;
}

// the host's lists of one graph, built once: free numbering in ABI order, active edges in edge order, per block / per vertex the
// contributions in edge order
struct Pg4Host {
    int nv = 0, ne = 0, nf = 0, n = 0, nblk = 0;
    std::vector<int32_t> free_idx, free_list, v0, v1, blk_bi, blk_bj, blk_start, blk_item, vb_start, vb_item;
    std::vector<double> meas;
};

void pg4_build(const orbhip_pose_graph4dof &G, Pg4Host &H)
{
    H.nv = G.n_vertices;
    H.free_idx.assign(H.nv, -1);
    for (int v = 0; v < H.nv; v++) if (!G.fixed[v]) { H.free_idx[v] = (int32_t)H.free_list.size(); H.free_list.push_back(v); }
    H.nf = (int)H.free_list.size(); H.n = 4 * H.nf;
    for (int e = 0; e < G.n_edges; e++) {
        const int a = G.edge_v0[e], b = G.edge_v1[e];
        if (H.free_idx[a] < 0 && H.free_idx[b] < 0) continue;                // not active (sparse_optimizer.cpp:234)
        H.v0.push_back(a); H.v1.push_back(b);
        for (int k = 0; k < 12; k++) H.meas.push_back(G.edge_meas[12 * (size_t)e + k]);
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
            items[it->second].push_back(e << 2 | (fi > fj ? 1 : 2));         // Ji^T W Jj is block (fi, fj); below the diagonal as it is, else transposed
        }
    }
    H.nblk = (int)items.size();
    H.blk_start.push_back(0);
    for (auto &l : items) { H.blk_item.insert(H.blk_item.end(), l.begin(), l.end()); H.blk_start.push_back((int32_t)H.blk_item.size()); }
    H.vb_start.push_back(0);
    for (auto &l : vb) { H.vb_item.insert(H.vb_item.end(), l.begin(), l.end()); H.vb_start.push_back((int32_t)H.vb_item.size()); }
}

struct Carve4 {
    char *base; size_t off = 0;
    template <class T> T *take(size_t count) { T *p = base ? reinterpret_cast<T *>(base + off) : nullptr; off += align256(count * sizeof(T)); return p; }
};

int pg4_solve_one(orbhip_ctx *ctx, const orbhip_pose_graph4dof &graph, const orbhip_pose_graph4dof_params *p, double *state, orbhip_pose_graph_stats *st,
                  double *trace)
{
    Pg4Host H;
    pg4_build(graph, H);
    orbhip_pose_graph_stats S;
    memset(&S, 0, sizeof(S));
    S.n_free = H.nf; S.n_unknowns = H.n; S.lambda = 0;
    if (H.nf == 0 || H.ne == 0) { if (st) *st = S; return ORBHIP_OK; }
    const int n = H.n;
    const bool force_big = getenv("ORBHIP_PG_FORCE_BIG") && atoi(getenv("ORBHIP_PG_FORCE_BIG")) != 0;       // test-only: the many-workgroup factorisation for every size
    const bool big = n > BA_LDLT_MAXN || force_big;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    const int dev = orbhip_ctx_device_internal(ctx);

    Pg4Dev D;
    memset(&D, 0, sizeof(D));
    D.nv = H.nv; D.ne = H.ne; D.nf = H.nf; D.n = n; D.nblk = H.nblk;
    for (int k = 0; k < 6; k++) D.info[k] = p->info_diag[k];
    // one arena: the uploaded part first (same layout in a host blob), then the work buffers
    auto layout = [&](char *base, Pg4Dev &O, size_t &upload_bytes) {
        Carve4 c{base};
        O.est = c.take<double>(PG4_VS * (size_t)H.nv);
        O.meas = c.take<double>(12 * (size_t)H.ne);
        O.free_idx = c.take<int32_t>(H.nv); O.free_list = c.take<int32_t>(H.nf);
        O.v0 = c.take<int32_t>(H.ne); O.v1 = c.take<int32_t>(H.ne);
        O.blk_bi = c.take<int32_t>(H.nblk); O.blk_bj = c.take<int32_t>(H.nblk); O.blk_start = c.take<int32_t>(H.nblk + 1);
        O.blk_item = c.take<int32_t>(H.blk_item.size());
        O.vb_start = c.take<int32_t>(H.nf + 1); O.vb_item = c.take<int32_t>(H.vb_item.size());
        O.x = c.take<double>(n);                                             // starts at zero (uploaded)
        upload_bytes = c.off;
        O.est_bk = c.take<double>(PG4_VS * (size_t)H.nv);
        O.rows = c.take<double>((size_t)H.ne * PG4_ROW); O.chi_e = c.take<double>(H.ne);
        O.Hb = c.take<double>((size_t)H.nblk * 16); O.b = c.take<double>(n);
        O.S = c.take<double>((size_t)n * n);
        O.big_y = c.take<double>(n); O.big_d = c.take<double>(n); O.big_U = c.take<double>(LD_NB * LD_NB);
        O.fail = c.take<int32_t>(1); O.result = c.take<double>(4);
        return c.off;
    };
    size_t up = 0;
    Pg4Dev dummy = D;
    const size_t total = layout(nullptr, dummy, up);
    const size_t est_bytes = sizeof(double) * PG4_VS * (size_t)H.nv;
    char *arena = (char *)orbhip_ctx_work_internal(ctx, total);
    if (!arena) return ORBHIP_E_HIP;
    char *blob = (char *)orbhip_ctx_pinned_internal(ctx, up + est_bytes + 64);
    if (!blob) return ORBHIP_E_HIP;
    layout(arena, D, up);
    {
        Pg4Dev Hh = D;
        size_t up2;
        layout(blob, Hh, up2);
        memset(blob, 0, up);
        for (int v = 0; v < H.nv; v++) {
            const double *a = state + PG4_ABI * (size_t)v;
            double *d = Hh.est + PG4_VS * (size_t)v;
            for (int k = 0; k < 9; k++) { d[PG4_RWB0 + k] = a[k]; d[PG4_RWB + k] = a[k]; d[PG4_DR + k] = (k % 4 == 0) ? 1.0 : 0.0; d[PG4_RCW + k] = a[12 + k]; d[PG4_RCB + k] = a[24 + k]; }
            for (int k = 0; k < 3; k++) { d[PG4_TWB + k] = a[9 + k]; d[PG4_TCW + k] = a[21 + k]; d[PG4_TCB + k] = a[33 + k]; }
        }
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
    if (!big) { if (orb_lds_optin(reinterpret_cast<const void *>(k_pg4_ldlt), dev, ldlt_lds)) return pg4_fail(ORBHIP_E_HIP, "LDS opt-in (k_pg4_ldlt)"); }
    else if (orb_lds_optin(reinterpret_cast<const void *>(k_pg4_big_rows), dev, rows_lds) || orb_lds_optin(reinterpret_cast<const void *>(k_pg4_big_backsub), dev, bsub_lds))
        return pg4_fail(ORBHIP_E_HIP, "LDS opt-in (k_pg4_big_*)");

    auto chi2 = [&](double lambda, double *out3) -> int {                          // errors at the estimates + the two reductions, read back
        hipLaunchKernelGGL(k_pg4_errors, dim3((H.ne + 63) / 64), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_pg4_reduce, dim3(1), dim3(256), 0, s, D, lambda);
        if (hipGetLastError() != hipSuccess) return pg4_fail(ORBHIP_E_HIP, PG4_FN "a kernel launch failed");   // any launch since the last read-back
        ORB_HIP_TRY(hipMemcpyAsync(rb, D.result, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        ORB_HIP_TRY(hipStreamSynchronize(s));
        out3[0] = rb[0]; out3[1] = rb[1]; out3[2] = rb[2];
        return ORBHIP_OK;
    };
    auto solve = [&](double lambda) -> int {
        ORB_HIP_TRY(hipMemsetAsync(D.S, 0, sizeof(double) * (size_t)n * n, s));
        hipLaunchKernelGGL(k_pg4_fill, dim3(H.nblk), dim3(64), 0, s, D, lambda);
        if (!big) hipLaunchKernelGGL(k_pg4_ldlt, dim3(1), dim3(1024), ldlt_lds, s, D);
        else {
            hipLaunchKernelGGL(k_pg4_big_init, dim3((n + 255) / 256), dim3(256), 0, s, D);
            for (int p0 = 0; p0 < n; p0 += LD_NB) {
                const int m2 = n - p0 - LD_NB;
                hipLaunchKernelGGL(k_pg4_big_diag, dim3(1), dim3(64), 0, s, D, p0);
                if (m2 > 0) {
                    hipLaunchKernelGGL(k_pg4_big_rows, dim3((m2 + 255) / 256), dim3(256), rows_lds, s, D, p0);
                    const int nt = (m2 + 63) / 64;
                    hipLaunchKernelGGL(k_pg4_big_trail, dim3(nt, nt), dim3(256), 0, s, D, p0);
                }
            }
            hipLaunchKernelGGL(k_pg4_big_backsub, dim3(1), dim3(1024), bsub_lds, s, D);
        }
        return ORBHIP_OK;
    };

    g_pg4_last_path = big ? 1 : 0;
    // Q6: OptimizationAlgorithmLevenberg::solve per iteration, SparseOptimizer::optimize around it (sparse_optimizer.cpp:355-420)
    double lambda = 0, ni = 2, current_chi = 0, r3[3];
    int nbad = 0, reason = ORBHIP_PG_END_ITERATIONS, iters = 0, trials = 0;
    bool any_solved = false;
    for (int iter = 0; iter < p->iterations; iter++) {
        int rc = chi2(0.0, r3);                                                    // computeActiveErrors + activeRobustChi2
        if (rc) return rc;
        current_chi = r3[0];
        if (iter == 0) S.chi2_initial = current_chi;
        const double ini_chi = current_chi;
        hipLaunchKernelGGL(k_pg4_linearize, dim3((H.ne + PG4_EPB - 1) / PG4_EPB), dim3(256), 0, s, D);     // buildSystem
        hipLaunchKernelGGL(k_pg4_assemble, dim3(H.nblk + H.nf), dim3(64), 0, s, D);
        if (iter == 0) {                                                           // computeLambdaInit (:171-185)
            if (p->lambda_init > 0) lambda = p->lambda_init;
            else {
                hipLaunchKernelGGL(k_pg4_maxdiag, dim3(1), dim3(256), 0, s, D);
                if (hipGetLastError() != hipSuccess) return pg4_fail(ORBHIP_E_HIP, PG4_FN "a kernel launch failed");
                ORB_HIP_TRY(hipMemcpyAsync(rb, D.result + 3, sizeof(double), hipMemcpyDeviceToHost, s));
                ORB_HIP_TRY(hipStreamSynchronize(s));
                lambda = p->tau * rb[0];
            }
            ni = 2; nbad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            ORB_HIP_TRY(hipMemcpyAsync(D.est_bk, D.est, est_bytes, hipMemcpyDeviceToDevice, s));           // push: the whole state, DR included
            if ((rc = solve(lambda))) return rc;
            hipLaunchKernelGGL(k_pg4_update, dim3((H.nf + 63) / 64), dim3(64), 0, s, D);
            if ((rc = chi2(lambda, r3))) return rc;
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
        for (int f = 0; f < H.nf; f++) {                                           // a fixed vertex keeps its bytes
            const int v = H.free_list[f];
            const double *d = rb + PG4_VS * (size_t)v;
            double *a = state + PG4_ABI * (size_t)v;
            for (int k = 0; k < 9; k++) { a[k] = d[PG4_RWB + k]; a[12 + k] = d[PG4_RCW + k]; }
            for (int k = 0; k < 3; k++) { a[9 + k] = d[PG4_TWB + k]; a[21 + k] = d[PG4_TCW + k]; }
        }
    }
    S.chi2_final = current_chi; S.lambda = lambda; S.iterations = iters; S.trials = trials; S.end_reason = reason;
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
        return pg4_fail(ORBHIP_E_BADARG, PG4_FN "ctx / graphs / params / state_inout is NULL or n_graphs < 0");
    int rc = pg4_check(graphs, n_graphs, params, state_inout);
    if (rc) return rc;
    const size_t stride = (size_t)params->iterations * params->max_trials * ORBHIP_PG_TRACE;
    for (int g = 0; g < n_graphs; g++)
        if ((rc = pg4_solve_one(ctx, graphs[g], params, state_inout[g], stats_out ? stats_out + g : nullptr, trace_out ? trace_out + g * stride : nullptr))) return rc;
    return ORBHIP_OK;
}
