// dense_ldlt_big.h -- the many-workgroup dense LDL^T of systems beyond the single-workgroup solve (n > BA_LDLT_MAXN, ba_ldlt.h): a
// right-looking blocked factorisation in global memory, 32-column panels, ldlt_rows for the per-entry arithmetic (so small and big
// systems factor alike), 64x64 trailing tiles with a 4x4 register tile per thread, then D^-1 and L^T x = y in one workgroup.
// One body per stage; ba_reduced_kernels.hip (k_ba_big_*), pose_graph_kernels.hip (k_pg_big_*) and pose_graph4dof_kernels.hip
// (k_pg4_big_*) keep thin __global__ wrappers that fill a DenseSys from their own argument block, pass the block coordinates and, after
// back-substitution, write the flag where their host code reads it.  No device code is shared across translation units (k_ba_big_* are
// launched from ba_kernels.hip, which also takes the two LDS sizes from here).
//
// Floating-point contraction: the library builds with -ffp-contract=off and the optimisers switch contraction on with a file-scope
// pragma AFTER their includes, so this header sees it off.  The stages have always been compiled contracted (they stood below that
// pragma in the three files); every body that does arithmetic therefore opens with its own `#pragma clang fp contract(fast)`, as
// geom3.h and ba_ldlt.h do, and gives the same bits wherever the #include stands.
#pragma once
#include "wave_dpp.h"
#include "ba_ldlt.h"

struct DenseSys {
    double *S;              // [n][ld] the lower triangle is read and factored in place: L below the diagonal, d on it
    int ld, n;
    const double *rhs;      // [n]
    double *x;              // [n] written by back-substitution only when every pivot was good
    double *y, *d, *U;      // work: [n], [n], [LD_NB * LD_NB] (the diagonal block's unscaled columns for the rows below it)
    int32_t *fail;          // [1] a zero / non-finite pivot was met
};

// dynamic LDS of the rows stage: P [32 + 256][LD_PP] (rows 0..31 unused), U [32*32], dv [32], yv [32 + 256]
static inline size_t dense_big_rows_lds() { return sizeof(double) * ((size_t)(LD_NB + 256) * LD_PP + LD_NB * LD_NB + LD_NB + LD_NB + 256); }
// dynamic LDS of back-substitution: y [y_cap], red [32*32], P [32][LD_PP]; y_cap >= n is what the caller passes to dense_big_backsub
static inline size_t dense_big_bsub_lds(int y_cap) { return sizeof(double) * ((size_t)y_cap + 32 * 32 + LD_NB * LD_PP); }

// 256 threads, (n + 255) / 256 workgroups; bx = the workgroup's index
__device__ __forceinline__ void dense_big_init(const DenseSys &A, int bx)
{
    const int i = bx * 256 + threadIdx.x;
    if (i < A.n) A.y[i] = A.rhs[i];
    if (i == 0) *A.fail = 0;
}

// the diagonal block of the panel at p0: one wave
__device__ __forceinline__ void dense_big_diag(const DenseSys &A, int p0)
{
    __shared__ double P[LD_NB * LD_PP], U[LD_NB * LD_NB], dv[LD_NB], yv[LD_NB];
    __shared__ int s_ok;
    const int lane = threadIdx.x, n = A.n, ld = A.ld;
    if (p0 >= n || *A.fail) return;
    const int nb = min(LD_NB, n - p0);
    double *S = A.S, *y = A.y, *d = A.d;
    if (lane == 0) s_ok = 1;
    if (lane < nb) {
        for (int c = 0; c < nb; c++) P[lane * LD_PP + c] = S[(size_t)(p0 + lane) * ld + p0 + c];
        yv[lane] = y[p0 + lane];
    }
    wave_lds_sync();
    if (lane < nb) ldlt_rows<true>((lds_f64 *)P, (lds_f64 *)U, (lds_f64 *)dv, (lds_f64 *)yv, lane, nb, &s_ok);
    wave_lds_sync();
    if (!s_ok) { if (lane == 0) *A.fail = 1; return; }
    if (lane < nb) {
        for (int c = 0; c <= lane; c++) S[(size_t)(p0 + lane) * ld + p0 + c] = (c == lane) ? dv[c] : P[lane * LD_PP + c];
        d[p0 + lane] = dv[lane]; y[p0 + lane] = yv[lane];
    }
    for (int k = lane; k < LD_NB * LD_NB; k += 64) A.U[k] = U[k];
}

// the rows below the diagonal block: 256 threads, one row each; bx = which 256 rows; lds = dense_big_rows_lds() bytes
__device__ __forceinline__ void dense_big_rows(const DenseSys &A, int p0, int bx, double *lds)
{
    __shared__ int s_dummy;
    const int tid = threadIdx.x, n = A.n, ld = A.ld;
    if (p0 >= n || *A.fail) return;
    const int nb = min(LD_NB, n - p0), m = n - p0;
    const int r = nb + bx * 256 + tid;                   // row of the panel (relative to p0)
    if (nb + bx * 256 >= m) return;
    double *P = lds, *U = P + (size_t)(LD_NB + 256) * LD_PP, *dv = U + LD_NB * LD_NB, *yv = dv + LD_NB;
    double *S = A.S, *y = A.y;
    for (int k = tid; k < LD_NB * LD_NB; k += 256) U[k] = A.U[k];
    if (tid < nb) { dv[tid] = A.d[p0 + tid]; yv[tid] = y[p0 + tid]; }
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

// trailing update S[i][k] -= sum_c L[i][c] d_c L[k][c] for i >= k >= p0 + nb: tile (ti, tk) of the 64x64 tiles of the lower triangle,
// 256 threads, 4x4 per thread
__device__ __forceinline__ void dense_big_trail(const DenseSys &A, int p0, int ti, int tk)
{
#pragma clang fp contract(fast)
    __shared__ double LI[64 * LD_PP], LK[64 * LD_PP], dv[LD_NB];
    const int tid = threadIdx.x, n = A.n, ld = A.ld;
    if (p0 >= n || *A.fail) return;
    const int nb = min(LD_NB, n - p0);
    const int base = p0 + nb, m2 = n - base;
    if (tk > ti || 64 * ti >= m2) return;
    double *S = A.S;
    for (int idx = tid; idx < 64 * LD_NB; idx += 256) {
        const int r = idx >> 5, c = idx & 31;
        const int gi = base + 64 * ti + r, gk = base + 64 * tk + r;
        LI[r * LD_PP + c] = (c < nb && gi < n) ? S[(size_t)gi * ld + p0 + c] : 0.0;
        LK[r * LD_PP + c] = (c < nb && gk < n) ? S[(size_t)gk * ld + p0 + c] : 0.0;
    }
    if (tid < LD_NB) dv[tid] = tid < nb ? A.d[p0 + tid] : 0.0;
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

// y <- D^-1 y, then L^T x = y panel by panel from the bottom: one workgroup of 1024 threads; lds = dense_big_bsub_lds(y_cap) bytes.
// Returns false, x untouched (as the reference on failure), when a pivot failed; the value is block-uniform.
__device__ __forceinline__ bool dense_big_backsub(const DenseSys &A, int y_cap, double *lds)
{
#pragma clang fp contract(fast)
    const int tid = threadIdx.x, nth = blockDim.x, n = A.n, ld = A.ld;
    if (*A.fail) return false;
    double *y = lds, *red = y + y_cap, *P = red + 32 * 32;
    const double *S = A.S, *dval = A.d;
    for (int i = tid; i < n; i += nth) y[i] = A.y[i] / dval[i];
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
    for (int i = tid; i < n; i += nth) A.x[i] = y[i];
    return true;
}
