// ba_shard_kernels.hip -- local bundle adjustment, the landmark-sharded solve: every rank owns a slice of each graph's
// points, poses are replicated; at four places of a tick the ranks' partial sums meet in BaBatch::xbuf (filled by the caller's
// all-gather) and are reduced in rank order on every rank.  State and kernel argument: ba_batch.h; where the exchanges sit in the tick:
// ba_kernels.hip.
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)

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
