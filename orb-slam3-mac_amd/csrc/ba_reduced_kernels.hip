// ba_reduced_kernels.hip -- local bundle adjustment, the reduced (pose) system S x = bs (B6 of ba_kernels.hip's table,
// linear_solver_eigen.h:94-125) in its two forms: one workgroup per window with the matrix in LDS (k_ba_ldlt, ba_ldlt.h) and, beyond
// BA_LDLT_MAXN unknowns, the blocked factorisation in global memory by many workgroups (k_ba_big_*, dense_ldlt_big.h).  State and
// kernel argument: ba_batch.h; launch order: ba_kernels.hip.
#include "wave_dpp.h"
#include "ba_ldlt.h"
#include "dense_ldlt_big.h"
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)

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
// single-workgroup kernels, so it is built (k_ba_schur_big / k_ba_schur_rows, ba_schur_kernels.hip) and factored in global memory by
// many workgroups:
//   k_ba_big_diag / _rows / _trail   right-looking blocked LDL^T, 32-column panels: diagonal block (one wave), the rows below
//                       (one row per thread, many workgroups), rank-32 trailing update (64x64 tiles, many workgroups)
//   k_ba_big_backsub    D^-1, L^T x = y
// The stages' bodies are dense_ldlt_big.h's, shared with the pose graphs; the kernels here pick the window by blockIdx, skip an inactive
// one and hand its pointers over.  The arithmetic per entry is the LDS-panel kernel's (same ldlt_rows), so small and big windows factor alike.

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
#ifdef LDLT_PROF
extern "C" int orbhip_debug_ldlt_prof(long long *out8, int reset)      // debug build only (EXTRA=-DLDLT_PROF): cumulative cycles of ldlt_solve_wg's phases
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ldlt_prof), 64) != hipSuccess) return ORBHIP_E_HIP;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_ldlt_prof), z, 64) != hipSuccess) return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
#endif
