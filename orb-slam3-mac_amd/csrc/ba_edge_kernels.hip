// ba_edge_kernels.hip -- local bundle adjustment, edge evaluation and assembly (B2 - B5 of ba_kernels.hip's table): residuals and
// robust chi2 of every edge, their per-graph sums, the landmark and pose blocks of the normal equations, max |diag| for the initial
// lambda, and the edge classification between the passes and at the end.  State and kernel argument: ba_batch.h; host side and launch
// order: ba_kernels.hip.
#include "wave_dpp.h"
#include "ba_edges.h"
#include "ba_batch.h"
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)

// (SE3 and edge math, B1 - B3: ba_edges.h; Huber, B4: geom3.h)

// Merge variant, between the passes (Optimizer.cc:6546-6579): chi2 of the last evaluation > gate or depth <= 0 at the
// current estimate => setLevel(1).  Runs at the start of the tick after the pass switch (apply_levels).
__global__ __launch_bounds__(256) void k_ba_levels(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.apply_levels) return;
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int ge = G.edge_off + e;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    const BaCamDev &cam = ba_cam_ref<true>(B, G, B.edge_pose[ge]);      // (mTrl of the edge's own keyframe)
    const double z = edge_depth(cam, pose, X, B.edge_stereo[ge]);
    const double gate = B.edge_stereo[ge] == 1 ? B.gate_s : B.gate_m;
    if ((B.chi2[ge] > gate) || !(z > 0.0)) B.level[ge] = 1;
}

// which: 0 -> evaluate at the CURRENT estimate for graphs that need a (re)build;
//        1 -> evaluate at the TRIAL estimate for every active graph.
// GENERAL = false: every graph of the batch is Pinhole without second-camera edges and without twin edges (the usual local BA)
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_ba_errors(BaBatch B, int which)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || (which == 0 && (!st.need_build || (st.errors_fresh && B.world == 1)))) return;      // after an accepted trial the stored errors ARE the current ones
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int buf = which == 0 ? st.cur : (st.cur ^ 1);
    const int ge = G.edge_off + e;
    if (B.level[ge]) { B.rho0[ge] = 0; return; }      // not an active edge: its stored error / chi2 stay as last computed
    const double *pose = B.poses + ((size_t)buf * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)buf * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    double P[3], er[3];
    const int type = B.edge_stereo[ge], stereo = type == 1;          // 0 mono, 1 stereo, 2 second camera (ToBody)
    const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, B.edge_pose[ge]);
    if (GENERAL && type == 2) tobody_error(cam, pose, X, B.edge_obs + 3 * (size_t)ge, P, er);
    else edge_error<GENERAL>(cam, pose, X, B.edge_obs + 3 * (size_t)ge, stereo, P, er);
    const double chi2 = (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]) * B.edge_is2[ge];
    double r0, r1;
    if (!st.robust) { r0 = chi2; r1 = 1.; }
    else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
    B.err[3 * (size_t)ge] = er[0]; B.err[3 * (size_t)ge + 1] = er[1]; B.err[3 * (size_t)ge + 2] = er[2];
    B.chi2[ge] = chi2;
    B.rho0[ge] = r0;
}
template __global__ void k_ba_errors<true>(BaBatch, int);
template __global__ void k_ba_errors<false>(BaBatch, int);

// Deterministic per-graph sums: chi = sum rho0 over edges (activeRobustChi2, sparse_optimizer.cpp:100-114);
// mode 1 additionally sums computeScale partials (levenberg.cpp:187-194).
__global__ __launch_bounds__(1024) void k_ba_reduce(BaBatch B, int which)
{
    // 1024 threads, four loads in flight per thread, DPP tree per wave, the 16 wave sums added in order: a fixed association (round 1: 256
    // threads walking 78 dependent loads each and an 8-step LDS tree -- 21 us of a single-window LM tick, twice per tick)
    __shared__ double red[16];
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || (which == 0 && (!st.need_build || (st.errors_fresh && B.world == 1)))) return;      // after an accepted trial the stored errors ARE the current ones
    const BaGraphDev &G = B.gd[g];
    auto block_sum = [&](double v) {
        v = wave_sum_f64_dpp(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        double t = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) t += red[w];
        return t;
    };
    {
        const double *r = B.rho0 + G.edge_off;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int e = tid;
        for (; e + 3072 < G.n_edges; e += 4096) { s0 += r[e]; s1 += r[e + 1024]; s2 += r[e + 2048]; s3 += r[e + 3072]; }
        for (; e < G.n_edges; e += 1024) s0 += r[e];
        const double chi = block_sum((s0 + s1) + (s2 + s3));
        if (tid == 0) B.chi[g] = chi;
    }
    if (which == 0 && tid == 0) B.st[g].apply_levels = 0;      // k_ba_levels (earlier in this tick) has consumed it
    if (which == 1) {
        double t = 0;
        for (int l = tid; l < G.n_points; l += 1024) t += B.scale_pt[G.point_off + l];
        if (B.rank == 0) for (int h = tid; h < G.nf; h += 1024) t += B.scale_pose[G.free_off + h];   // replicated: counted once
        const double sc = block_sum(t);
        if (tid == 0) B.scale[g] = sc;
    }
}

// buildSystem, landmark side: 16 lanes per point share its (contiguous) edges -- one edge per lane and trip, so the
// Jacobians of a point's ~10 observations are evaluated side by side and their scattered Hpl writes are in flight
// together; Hll / bl are reduced over the 16 lanes in a fixed (butterfly) order.
// Hll (sym 6), bl, and the edge's Hpl block Wsp[e][6*b + a] = (J_T^T w Omega J_X)[a][b].
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_ba_build_points(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    const int sub = threadIdx.x & 15;
    const int l = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int *ps = B.pt_start + G.ptstart_off;
    if (l >= G.n_points) return;                      // whole 16-lane groups leave together
    const int e0 = ps[l], e1 = ps[l + 1];
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + l) * 3;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // H (6, upper) then b (3)
    for (int e = e0 + sub; e < e1; e += 16) {
        const int ge = G.edge_off + e;
        const int pi = B.edge_pose[ge];
        const int hi = B.hidx[G.pose_off + pi];
        const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + pi) * 7;
        const int type = B.edge_stereo[ge], stereo = type == 1;
        double P[3], R[9], Jx[9], Jt[18];
#pragma unroll
        for (int k = 6; k < 9; k++) Jx[k] = 0;
#pragma unroll
        for (int k = 12; k < 18; k++) Jt[k] = 0;                                     // monocular edge: third row empty
        const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, pi);
        if (GENERAL && type == 2) tobody_jacobians(cam, pose, X, Jx, Jt);
        else {
            quat_rot(pose, X, P);
            P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
            quat_to_R(pose, R);
            edge_jacobians<GENERAL>(cam, P, R, stereo, Jx, Jt);
        }
        const double chi2 = B.chi2[ge];
        double r0, r1;
        if (!st.robust) r1 = 1.;
        else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
        const double w = B.level[ge] ? 0.0 : r1 * B.edge_is2[ge];          // level-1 edge: contributes nothing (its Hpl block is zeroed)
        const double es[3] = {B.err[3 * (size_t)ge], B.err[3 * (size_t)ge + 1], stereo ? B.err[3 * (size_t)ge + 2] : 0.0};
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double j0 = Jx[3 * d], j1 = Jx[3 * d + 1], j2 = Jx[3 * d + 2];
            const double we = -w * es[d];
            acc[6] += j0 * we; acc[7] += j1 * we; acc[8] += j2 * we;
            acc[0] += j0 * w * j0; acc[1] += j0 * w * j1; acc[2] += j0 * w * j2;
            acc[3] += j1 * w * j1; acc[4] += j1 * w * j2; acc[5] += j2 * w * j2;
        }
        if (hi >= 0 && (!GENERAL || !B.edge_dup[ge])) {
            double Wb[18];
#pragma unroll
            for (int bb = 0; bb < 3; bb++)
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    double h = 0;
#pragma unroll
                    for (int d = 0; d < 3; d++) h += Jt[6 * d + a] * w * Jx[3 * d + bb];
                    Wb[6 * bb + a] = h;
                }
            for (int e2 = GENERAL ? B.edge_next[ge] : -1; e2 >= 0; e2 = B.edge_next[G.edge_off + e2]) {      // the same keyframe's other camera (rare)
                const int g2 = G.edge_off + e2;
                const int type2 = B.edge_stereo[g2], st2 = type2 == 1;
                double P2[3], R2[9], Jx2[9], Jt2[18];
                for (int k = 6; k < 9; k++) Jx2[k] = 0;
                for (int k = 12; k < 18; k++) Jt2[k] = 0;
                if (type2 == 2) tobody_jacobians(cam, pose, X, Jx2, Jt2);
                else {
                    quat_rot(pose, X, P2);
                    P2[0] += pose[4]; P2[1] += pose[5]; P2[2] += pose[6];
                    quat_to_R(pose, R2);
                    edge_jacobians(cam, P2, R2, st2, Jx2, Jt2);
                }
                double q0, q1;
                if (!st.robust) q1 = 1.;
                else if (st2) huber(B.chi2[g2], B.delta_s, B.dsqr_s, &q0, &q1); else huber(B.chi2[g2], B.delta_m, B.dsqr_m, &q0, &q1);
                const double w2 = B.level[g2] ? 0.0 : q1 * B.edge_is2[g2];
                for (int bb = 0; bb < 3; bb++)
                    for (int a = 0; a < 6; a++) {
                        double h = 0;
                        for (int d = 0; d < 3; d++) h += Jt2[6 * d + a] * w2 * Jx2[3 * d + bb];
                        Wb[6 * bb + a] += h;
                    }
            }
            // (round 4: parking the blocks of a workgroup's 16 points in LDS and writing the contiguous range out with consecutive lanes on
            // consecutive 16 bytes was SLOWER: 0.55 against 0.42 ms per 256 windows -- two more barriers and the LDS round trip)
            double *wo = B.Wsp + (size_t)B.edge_task[ge] * 18;
#pragma unroll
            for (int k = 0; k < 18; k++) wo[k] = Wb[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        acc[k] = row16_allreduce_f64_dpp(acc[k]);          // the point's 16 lanes = one DPP row
    }
    if (sub == 0) {
        double *Ho = B.Hll + (size_t)(G.point_off + l) * 6, *bo = B.bl + (size_t)(G.point_off + l) * 3;
#pragma unroll
        for (int i = 0; i < 6; i++) Ho[i] = acc[i];
        bo[0] = acc[6]; bo[1] = acc[7]; bo[2] = acc[8];
    }
}
template __global__ void k_ba_build_points<true>(BaBatch);
template __global__ void k_ba_build_points<false>(BaBatch);

// buildSystem, pose side: one wave per free pose over its edges (pose-major list).
template <bool GENERAL>
__global__ __launch_bounds__(64) void k_ba_build_poses(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build) return;
    const BaGraphDev &G = B.gd[g];
    const int h = blockIdx.x;
    if (h >= G.nf) return;
    const int lane = threadIdx.x;
    const int *qs = B.pose_start + G.posestart_off;
    const int *pe = B.pose_edges + G.edge_off;
    double acc[27];
    for (int i = 0; i < 27; i++) acc[i] = 0;
    // every edge of this list has the same pose; the edge's error / chi2 are recomputed from the pose-major copy of its static data
    // (bit-identical to k_ba_errors: same inputs, same code) instead of being gathered from the point-major arrays
    const int pose_i = qs[h] < qs[h + 1] ? B.edge_pose[G.edge_off + pe[qs[h]]] : 0;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + pose_i) * 7;
    const BaCamDev &cam = ba_cam_ref<GENERAL>(B, G, pose_i);
    for (int k = qs[h] + lane; k < qs[h + 1]; k += 64) {
        const size_t gk = (size_t)G.edge_off + k;
        const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.pm_point[gk]) * 3;
        const int type = B.pm_type[gk], stereo = type == 1;
        double P[3], R[9], Jx[9], Jt[18], es[3];
#pragma unroll
        for (int q = 12; q < 18; q++) Jt[q] = 0;                  // monocular edge: third row empty (the loops below run all 3 rows)
        if (GENERAL && type == 2) { tobody_error(cam, pose, X, B.pm_obs + 3 * gk, P, es); tobody_jacobians(cam, pose, X, Jx, Jt); }
        else {
            edge_error<GENERAL>(cam, pose, X, B.pm_obs + 3 * gk, stereo, P, es);
            quat_to_R(pose, R);
            edge_jacobians<GENERAL>(cam, P, R, stereo, Jx, Jt);
        }
        const double is2 = B.pm_is2[gk];
        const double chi2 = (es[0] * es[0] + es[1] * es[1] + es[2] * es[2]) * is2;
        double r0, r1;
        if (!st.robust) r1 = 1.;
        else if (stereo) huber(chi2, B.delta_s, B.dsqr_s, &r0, &r1); else huber(chi2, B.delta_m, B.dsqr_m, &r0, &r1);
        const double w = (B.ex2 && B.level[G.edge_off + pe[k]]) ? 0.0 : r1 * is2;      // levels exist only in the merge variant
#pragma unroll
        for (int d = 0; d < 3; d++) {                             // compile-time indices: acc stays in registers
            const double we = -w * es[d];
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double ja = Jt[6 * d + a];
                acc[21 + a] += ja * we;
#pragma unroll
                for (int bb = a; bb < 6; bb++) acc[idx++] += ja * w * Jt[6 * d + bb];
            }
        }
    }
    for (int i = 0; i < 27; i++) {
        double v = acc[i];
        v = wave_sum_f64_dpp(v);
        acc[i] = v;
    }
    if (lane == 0) {
        double *Hp = B.Hpp + (size_t)(G.free_off + h) * 36;
        int idx = 0;
        for (int a = 0; a < 6; a++)
            for (int bb = a; bb < 6; bb++) { Hp[6 * a + bb] = acc[idx]; Hp[6 * bb + a] = acc[idx]; idx++; }
        for (int a = 0; a < 6; a++) B.bp[(size_t)(G.free_off + h) * 6 + a] = acc[21 + a];
    }
}
template __global__ void k_ba_build_poses<true>(BaBatch);
template __global__ void k_ba_build_poses<false>(BaBatch);

// computeLambdaInit (levenberg.cpp:171-185): max |diag| over pose and landmark blocks
__global__ __launch_bounds__(256) void k_ba_maxdiag(BaBatch B)
{
    __shared__ double red[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const BaState &st = B.st[g];
    if (!st.active || !st.need_build || !st.need_lambda_init) return;
    const BaGraphDev &G = B.gd[g];
    const int *ps = B.pt_start + G.ptstart_off;
    double m = 0;
    if (B.world == 1)                                   // sharded: Hpp is still a partial sum here (k_ba_shard_sum1 finishes the max)
        for (int h = tid; h < G.nf; h += 256)
            for (int a = 0; a < 6; a++) m = fmax(m, fabs(B.Hpp[(size_t)(G.free_off + h) * 36 + 7 * a]));
    for (int l = tid; l < G.n_points; l += 256)
        if (ps[l + 1] > ps[l]) {
            const double *H = B.Hll + (size_t)(G.point_off + l) * 6;
            m = fmax(m, fmax(fabs(H[0]), fmax(fabs(H[3]), fabs(H[5]))));
        }
    red[tid] = m;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (tid < d) red[tid] = fmax(red[tid], red[tid + d]); __syncthreads(); }
    if (tid == 0) B.maxdiag[g] = red[0];
}

// outlier gates, Optimizer.cc:2126-2173: stored chi2 of the last evaluation; depth at the final estimate
__global__ __launch_bounds__(256) void k_ba_finalize(BaBatch B)
{
    const int g = blockIdx.y;
    const BaState &st = B.st[g];
    const BaGraphDev &G = B.gd[g];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n_edges) return;
    const int ge = G.edge_off + e;
    const double *pose = B.poses + ((size_t)st.cur * B.sumP + G.pose_off + B.edge_pose[ge]) * 7;
    const double *X = B.points + ((size_t)st.cur * B.sumL + G.point_off + B.edge_point[ge]) * 3;
    const BaCamDev &cam = ba_cam_ref<true>(B, G, B.edge_pose[ge]);      // (mTrl of the edge's own keyframe)
    const double z = edge_depth(cam, pose, X, B.edge_stereo[ge]);
    const double gate = B.edge_stereo[ge] == 1 ? B.gate_s : B.gate_m;
    const int out = (B.chi2[ge] > gate) || !(z > 0.0);
    B.outlier[ge] = (uint8_t)out;
    if (out) atomicAdd(&B.st[g].n_outliers, 1);
}
