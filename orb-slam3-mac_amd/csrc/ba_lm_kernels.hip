// ba_lm_kernels.hip -- local bundle adjustment, Levenberg-Marquardt control (B7, B8 of ba_kernels.hip's table): the start of an outer
// iteration, the landmark back-substitution with the trial update of every vertex, and the accept / reject decision with the
// two-pass bookkeeping.  State and kernel argument: ba_batch.h; launch order: ba_kernels.hip.
#include "wave_dpp.h"
#include "ba_edges.h"
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)
#include <cfloat>

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
