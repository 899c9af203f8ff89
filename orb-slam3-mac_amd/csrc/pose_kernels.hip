// pose_kernels.hip -- pose-only BA on gfx950: Optimizer::PoseOptimization (reference src/Optimizer.cc:854-1168), batched
// over frames.  One free SE3 vertex per frame and a unary edge per observation (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
// / EdgeSE3ProjectXYZOnlyPoseToBody); vertex and edge math are ba_edges.h, shared with the local BA (ba_edge_kernels.hip).
// One 256-thread workgroup per frame; thread t owns
// edges t, t+256, ... (outlier level = one bit per owned edge).  The 6x6 system is tiny, so every thread keeps
// the whole LM state (pose, lambda, ...) in registers and runs the scalar control flow redundantly on the
// block-reduced sums: no broadcasts, two barriers per reduction, fixed summation order (run-to-run identical).
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "ba_edges.h"
#pragma clang fp contract(fast)       // as ba_kernels.hip: the double-precision optimisers are compared to 1e-4, not bit for bit
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

#define PO_THREADS 256
#define PO_NRED 28            // robust chi2 + 21 upper-triangle entries of H + 6 of b
#define PO_KR 4               // edges per thread held in registers (x 256 threads: frames of up to 1024 edges never re-read them)
#define PO_IDX(a, c) ((a) * 6 - (a) * ((a) - 1) / 2 + ((c) - (a)))      // packed upper triangle, a <= c
struct PoArgs {
    const double *Xw, *obs, *inv_s2;
    const int32_t *n;
    int max_edges;
    double fx, fy, cx, cy, bf;
    int cam_model; double kb[4];
    const uint8_t *right;               // [frames][max_edges] 1 = observation in the second camera (may be NULL)
    double Trl[7], fx2, fy2, cx2, cy2, kb2[4]; int cam2_model;
    double *pose;
    uint8_t *outlier;
    int32_t *n_inliers, *stats;
    int stage_cap;                      // edges per frame the four-wave kernel stages in LDS (0: none)
};

#ifdef PO_PROF
__device__ long long g_po_prof[8];            // debug build only (EXTRA=-DPO_PROF): cycles of build walk / 28 block sums / solve + oplus / trial walk / its sum / reclassification, trials
#define PO_T(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const long long t_ = clock64(); g_po_prof[i] += t_ - t_prev; t_prev = t_; } } while (0)
extern "C" int orbhip_debug_po_prof(long long *out8, int reset)
{
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_po_prof), 64) != hipSuccess) return -1;
    if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_po_prof), z, 64) != hipSuccess) return -1; }
    return 0;
}
#else
#define PO_T(i) do { } while (0)
#endif
template <int N, int NT = 256>
__device__ __forceinline__ void po_block_sum(double (&v)[N], double (*red)[PO_NRED])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        v[k] = wave_sum_f64_dpp(v[k]);                    // DPP path: the ~100 block sums per frame were ds_bpermute bound
    }
    if (NT == 64) return;                              // one wave per frame: no LDS, no barrier
    __syncthreads();                                   // previous readers of red are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) red[wv][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {                       // the waves' sums in wave order (a fixed association per NT)
        double s = red[0][k];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) s += red[w][k];
        v[k] = s;
    }
}

// The 28 sums of a build step for the four-wave forms (round 4).  28 wave-level DPP trees of doubles were 3.8 k cycles per step -- 17 % of
// a one-frame call (tools/po_prof_probe.py) -- because every one of them is a chain of 6 dependent (2 x v_mov_dpp + v_add_f64).  Here the
// workgroup transposes through LDS instead: every thread stores its 28 partial sums ([k][8 segments of 32 threads, padded to 33]), thread
// (k, seg) adds the 32 entries of its segment (32 independent LDS reads, a balanced tree), the 8 segment sums of a k meet
// in three DPP steps inside 8 adjacent lanes (quad swaps + half-row mirror: every lane ends with the same bits), one lane per k publishes
// the total and every thread reads the 28 totals back (LDS broadcast).  Two barriers as before; a fixed association (run-to-run identical).
#define PO_RED2_K 265                                  // doubles per k: 8 segments x 33
template <int N>
__device__ __forceinline__ void po_block_sum_lds(double (&v)[N], double *red2, double *tot)
{
    static_assert(N * 8 <= 256, "one (k, segment) task per thread");
    const int tid = threadIdx.x;
    double *mine = red2 + (tid >> 5) * 33 + (tid & 31);
#pragma unroll
    for (int k = 0; k < N; k++) mine[k * PO_RED2_K] = v[k];
    __syncthreads();
    {
        const int k = min(tid >> 3, N - 1), seg = tid & 7;
        const double *p = red2 + k * PO_RED2_K + seg * 33;
        double t[32];
#pragma unroll
        for (int i = 0; i < 32; i++) t[i] = p[i];
        // a balanced tree over the 32 entries (depth 5 instead of a chain of 31 dependent additions: the (k, segment) thread has nothing
        // else to overlap its chain with); the same association in every call, whatever N
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1) {
#pragma unroll
            for (int i = 0; i < w; i++) t[i] = t[2 * i] + t[2 * i + 1];
        }
        double sacc = t[0];
        sacc = oct_allreduce_f64_dpp(sacc);
        if (seg == 0 && (tid >> 3) < N) tot[k] = sacc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = tot[k];
}

// computeError of the two unary edges; returns chi2 = e^T (inv_sigma2 I) e
template <bool GENERAL>
__device__ __forceinline__ double po_edge_chi2(const PoArgs &A, const BaCamDev &cam, const double *pose, const double *X, const double *ob,
                                               double is2, int right, double *P, double *er)
{
    if (GENERAL && right) {                                       // EdgeSE3ProjectXYZOnlyPoseToBody::computeError, OptimizableTypes.h:69-73
        tobody_error(cam, pose, X, ob, P, er);
        return (er[0] * er[0] + er[1] * er[1]) * is2;
    }
    quat_rot(pose, X, P);
    P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
    if (GENERAL && ob[2] < 0 && A.cam_model == 1) {    // OptimizableTypes.h:41-45 with pCamera = KannalaBrandt8: the local BA's monocular edge
        edge_error<true>(cam, pose, X, ob, 0, P, er);
    } else if (ob[2] < 0) {                            // OptimizableTypes.h:41-45, Pinhole.cpp:41-47
        er[0] = ob[0] - (A.fx * P[0] / P[2] + A.cx);
        er[1] = ob[1] - (A.fy * P[1] / P[2] + A.cy);
        er[2] = 0;
    } else {                                           // types_six_dof_expmap.cpp:339-346: float invz, double bf
        const float invz = (float)(1.0 / P[2]);
        const double r0 = P[0] * invz * A.fx + A.cx;
        er[0] = ob[0] - r0;
        er[1] = ob[1] - (P[1] * invz * A.fy + A.cy);
        er[2] = ob[2] - (r0 - A.bf * invz);
    }
    return (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]) * is2;
}

// GENERAL = false: Pinhole camera, no second camera (the common case keeps its registers); true: KannalaBrandt8 and / or
// observations in a second, rigidly attached camera.
// NT threads per frame, KR edges per thread in registers.  <256, 0>: four waves per frame, edges re-read from global memory on every walk
// (frames of more than 2048 edges).  <64, 16>: ONE wave per frame -- up to 1024 edges live in registers (the LM loop walks them ~80
// times per frame: build + trial per iteration, 4 x 10 iterations; every walk was a round of dependent global loads), all sums
// are wave-level DPP trees (no LDS, no barrier), and 1024 frames are one wave per SIMD instead of two rounds of 4-wave workgroups.
template <bool GENERAL, int NT, int KR>
__device__ __forceinline__ void po_body(const PoArgs &A, double (*red)[PO_NRED], double *stage = nullptr, int stage_cap = 0, double *red2 = nullptr, double *tot = nullptr)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = A.n[f];
    const double *Xw = A.Xw + (size_t)f * A.max_edges * 3, *obs = A.obs + (size_t)f * A.max_edges * 3;
    const double *is2 = A.inv_s2 + (size_t)f * A.max_edges;
    uint8_t *outl = A.outlier + (size_t)f * A.max_edges;
    // Optimizer.cc:896; an oversized frame (n > max_edges) is rejected below and must not write past its own row
    for (int e = tid; e < min(n, A.max_edges); e += NT) outl[e] = 0;
    if (n < 3 || n > A.max_edges) {                                             // Optimizer.cc:1040-1041
        if (tid == 0) { A.n_inliers[f] = 0; if (A.stats) { for (int k = 0; k < 4; k++) A.stats[4 * f + k] = 0; } }
        return;
    }
    BaCamDev cam; cam.fx = A.fx; cam.fy = A.fy; cam.cx = A.cx; cam.cy = A.cy; cam.bf = A.bf;
    cam.cam_model = A.cam_model; for (int k = 0; k < 4; k++) cam.kb[k] = A.kb[k];
    for (int k = 0; k < 7; k++) cam.Trl[k] = A.Trl[k];
    cam.fx2 = A.fx2; cam.fy2 = A.fy2; cam.cx2 = A.cx2; cam.cy2 = A.cy2; cam.cam2_model = A.cam2_model; for (int k = 0; k < 4; k++) cam.kb2[k] = A.kb2[k];
    const uint8_t *right = (GENERAL && A.right) ? A.right + (size_t)f * A.max_edges : nullptr;
    if (!GENERAL) cam.cam_model = 0;
    double pose0[7], pose[7], pose_ev[7], x[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 7; k++) pose0[k] = A.pose[7 * f + k];
    quat_norm_rot(pose0);                                                       // SE3Quat ctor
    for (int k = 0; k < 7; k++) { pose[k] = pose0[k]; pose_ev[k] = pose0[k]; }
    const double delta_m = (double)(float)sqrt(5.991), dsqr_m = (double)(float)(delta_m * delta_m);   // Optimizer.cc:887-888
    const double delta_s = (double)(float)sqrt(7.815), dsqr_s = (double)(float)(delta_s * delta_s);
    uint32_t level = 0;                                                          // bit k: edge tid + 256*k is an outlier
    double rX[KR ? KR : 1][3], rO[KR ? KR : 1][3], rW[KR ? KR : 1]; int rR[KR ? KR : 1];
#pragma unroll
    for (int k = 0; k < KR; k++) {
        const int e = min(tid + NT * k, n - 1);
        rX[k][0] = Xw[3 * e]; rX[k][1] = Xw[3 * e + 1]; rX[k][2] = Xw[3 * e + 2];
        rO[k][0] = obs[3 * e]; rO[k][1] = obs[3 * e + 1]; rO[k][2] = obs[3 * e + 2];
        rW[k] = is2[e]; rR[k] = (GENERAL && right) ? right[e] : 0;
    }
    // the multi-wave form keeps the first stage_cap edges in LDS (7 doubles each): the ~80 walks over the edges of a frame are then LDS
    // reads instead of rounds of dependent L2 reads -- what a single frame's latency is made of
    const int stage_lo = NT * KR;                                               // edges below live in registers
    const int n_staged = stage ? min(n, stage_lo + stage_cap) : 0;              // edges [stage_lo, n_staged) live in LDS
    if (stage) {
        for (int e = stage_lo + tid; e < n_staged; e += NT) {
            double *q = stage + 7 * (e - stage_lo);
            q[0] = Xw[3 * e]; q[1] = Xw[3 * e + 1]; q[2] = Xw[3 * e + 2]; q[3] = obs[3 * e]; q[4] = obs[3 * e + 1]; q[5] = obs[3 * e + 2]; q[6] = is2[e];
        }
        __syncthreads();
    }
    // body(k, e, X, ob, w0, rt) for every edge of this thread: the KR register-resident ones, then the tail (LDS stage / global memory)
    auto for_tail_edges = [&](auto body) {
        for (int e = tid + NT * KR, k = KR; e < n; e += NT, k++) {
            if (e < n_staged) { const double *q = stage + 7 * (e - stage_lo); body(k, e, q, q + 3, q[6], (GENERAL && right) ? (int)right[e] : 0); }
            else body(k, e, Xw + 3 * e, obs + 3 * e, is2[e], (GENERAL && right) ? (int)right[e] : 0);
        }
    };
    auto for_edges = [&](auto body) {
#pragma unroll
        for (int k = 0; k < KR; k++) { const int e = tid + NT * k; if (e < n) body(k, e, rX[k], rO[k], rW[k], rR[k]); }
        for_tail_edges(body);
    };
    // Frames whose edges are all monocular Pinhole ones (monocular tracking; Tracking.cc:1934) take a STRAIGHT-LINE form of the two walks
    // over the register-resident edges (round 4): one frame is one wave per SIMD, so a walk is a chain of dependent double-precision
    // latencies (quaternion rotation -> two divisions -> Huber's sqrt / division -> the Jacobian's four divisions), and with a branch per
    // edge (outlier level, mono / stereo, Huber's two cases) the four edges of a thread ran one after the other: 4.0 k cycles per trial walk,
    // 4.1 k per build walk (tools/po_prof_probe.py).  Without branches -- masked by selects -- the scheduler interleaves the four chains.
    // Same expressions in the same order as po_edge_chi2 / huber / edge_jacobians' monocular branches: the same bits.
    bool all_mono = false;
    if (!GENERAL && KR > 0) {
        double ns[1] = {0};
        for (int e = tid; e < n; e += NT) ns[0] += !(obs[3 * e + 2] < 0) ? 1.0 : 0.0;
        po_block_sum<1, NT>(ns, red);
        all_mono = ns[0] == 0.0;
    }
    int robust = 1, nbad = 0, lm_trials = 0, lm_iters = 0, rounds = 0;
#ifdef PO_PROF
    long long t_prev = clock64();
#endif
    for (int it = 0; it < 4; it++) {
        for (int k = 0; k < 7; k++) pose[k] = pose0[k];                          // Optimizer.cc:1053
        double cnt[1] = {0};
        for (int e = tid, k = 0; e < n; e += NT, k++) cnt[0] += !((level >> k) & 1u);
        po_block_sum<1, NT>(cnt, red);
        if (cnt[0] > 0) {
            double lambda = 0, ni = 2;
            int nb = 0, ok = 1;
            for (int iter = 0; iter < 10 && ok; iter++) {                        // SparseOptimizer::optimize(10)
                // ---- computeActiveErrors + activeRobustChi2 + buildSystem at the current estimate (LM:69-87)
                double acc[PO_NRED];
#pragma unroll
                for (int k = 0; k < PO_NRED; k++) acc[k] = 0;
                double R[9];
                quat_to_R(pose, R);
                PO_T(7);
                auto build_edge = [&](int k, int e, const double *Xe, const double *ob, double w0, int rt) {
                    (void)e;
                    if ((level >> k) & 1u) return;
                    const int stereo = !(ob[2] < 0);
                    double P[3], er[3], Jx[9], Jt[18], r0, r1;
#pragma unroll
                    for (int k = 12; k < 18; k++) Jt[k] = 0;                     // monocular edge: third row empty (er[2] == 0)
                    const double chi2 = po_edge_chi2<GENERAL>(A, cam, pose, Xe, ob, w0, rt, P, er);
                    if (robust) huber(chi2, stereo ? delta_s : delta_m, stereo ? dsqr_s : dsqr_m, &r0, &r1);
                    else { r0 = chi2; r1 = 1.; }
                    if (GENERAL && rt) tobody_jacobians(cam, pose, Xe, Jx, Jt);   // OptimizableTypes.cpp:82-106 (the pose block of the binary edge)
                    else edge_jacobians(cam, P, R, stereo, Jx, Jt);
                    const double w = r1 * w0;
                    acc[0] += r0;
                    int h = 1;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
#pragma unroll
                        for (int c = a; c < 6; c++) {
                            double s = 0;
#pragma unroll
                            for (int d = 0; d < 3; d++) s += Jt[6 * d + a] * w * Jt[6 * d + c];
                            acc[h++] += s;
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        double s = 0;
#pragma unroll
                        for (int d = 0; d < 3; d++) s += Jt[6 * d + a] * (-w * er[d]);
                        acc[22 + a] += s;
                    }
                };
                if (!GENERAL && KR > 0 && all_mono) {
#pragma unroll
                    for (int k = 0; k < KR; k++) {
                        const bool act = (tid + NT * k < n) && !((level >> k) & 1u);
                        double P[3], er[2], Jt[12];
                        quat_rot(pose, rX[k], P);
                        P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
                        er[0] = rO[k][0] - (A.fx * P[0] / P[2] + A.cx);                // po_edge_chi2, monocular Pinhole branch
                        er[1] = rO[k][1] - (A.fy * P[1] / P[2] + A.cy);
                        const double chi2 = (er[0] * er[0] + er[1] * er[1] + 0.0 * 0.0) * rW[k];
                        const double sq = sqrt(chi2);
                        const bool quad = !robust || chi2 <= dsqr_m;                   // huber(), selects instead of its two cases
                        const double r0 = quad ? chi2 : 2 * sq * delta_m - dsqr_m, r1 = quad ? 1. : delta_m / sq;
                        {                                                              // edge_jacobians, monocular Pinhole branch
                            const double x = P[0], y = P[1], z = P[2];
                            const double p00 = -(A.fx / z), p02 = A.fx * x / (z * z), p11 = -(A.fy / z), p12 = A.fy * y / (z * z);
                            Jt[0] = p02 * y;            Jt[1] = p00 * z - p02 * x;  Jt[2] = -p00 * y;  Jt[3] = p00; Jt[4] = 0;   Jt[5] = p02;
                            Jt[6] = -p11 * z + p12 * y; Jt[7] = -p12 * x;           Jt[8] = p11 * x;   Jt[9] = 0;   Jt[10] = p11; Jt[11] = p12;
                        }
                        const double w = r1 * rW[k];
                        acc[0] += act ? r0 : 0.0;
                        int h = 1;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
#pragma unroll
                            for (int c = a; c < 6; c++) {
                                double sacc = 0;
                                sacc += Jt[a] * w * Jt[c];
                                sacc += Jt[6 + a] * w * Jt[6 + c];
                                acc[h++] += act ? sacc : 0.0;
                            }
                        }
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            double sacc = 0;
                            sacc += Jt[a] * (-w * er[0]);
                            sacc += Jt[6 + a] * (-w * er[1]);
                            acc[22 + a] += act ? sacc : 0.0;
                        }
                    }
                    for_tail_edges(build_edge);
                } else for_edges(build_edge);
                PO_T(0);
                if (NT == 256 && red2) po_block_sum_lds<PO_NRED>(acc, red2, tot);
                else po_block_sum<PO_NRED, NT>(acc, red);
                PO_T(1);
                for (int k = 0; k < 7; k++) pose_ev[k] = pose[k];
                double current_chi = acc[0];
                const double ini_chi = current_chi;
                // H (symmetric) stays packed as its 21 upper-triangle entries, row-major: Hp[PO_IDX(a, c)], a <= c
                double Hp[21], b[6];
#pragma unroll
                for (int k = 0; k < 21; k++) Hp[k] = acc[1 + k];
#pragma unroll
                for (int a = 0; a < 6; a++) b[a] = acc[22 + a];
                if (iter == 0) {                                                 // computeLambdaInit, LM:171-185 (_tau = 1e-50)
                    double md = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++) md = fmax(fabs(Hp[PO_IDX(a, a)]), md);
                    lambda = 1e-50 * md; ni = 2; nb = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    double pose_bk[7];
                    for (int k = 0; k < 7; k++) pose_bk[k] = pose[k];            // push
                    // LinearSolverDense: LDL^T of H + lambda I; a non-positive pivot fails the solve (x keeps its old value)
                    // Lp[PO_IDX(j, i)] (j <= i) holds L(i, j) below the diagonal and D(j) on it
                    double Lp[21];
#pragma unroll
                    for (int k = 0; k < 21; k++) Lp[k] = Hp[k];
#pragma unroll
                    for (int a = 0; a < 6; a++) Lp[PO_IDX(a, a)] += lambda;
                    bool ok2 = true;
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        double d = Lp[PO_IDX(j, j)];
#pragma unroll
                        for (int k = 0; k < j; k++) d -= Lp[PO_IDX(k, j)] * Lp[PO_IDX(k, j)] * Lp[PO_IDX(k, k)];
                        ok2 = ok2 && (d > 0.0) && isfinite(d);
                        Lp[PO_IDX(j, j)] = d;
#pragma unroll
                        for (int i = j + 1; i < 6; i++) {
                            double sacc = Lp[PO_IDX(j, i)];
#pragma unroll
                            for (int k = 0; k < j; k++) sacc -= Lp[PO_IDX(k, i)] * Lp[PO_IDX(k, j)] * Lp[PO_IDX(k, k)];
                            Lp[PO_IDX(j, i)] = sacc / d;
                        }
                    }
                    if (ok2) {
                        double y[6];
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            double sacc = b[i];
#pragma unroll
                            for (int k = 0; k < i; k++) sacc -= Lp[PO_IDX(k, i)] * y[k];
                            y[i] = sacc;
                        }
#pragma unroll
                        for (int i = 0; i < 6; i++) y[i] /= Lp[PO_IDX(i, i)];
#pragma unroll
                        for (int i = 5; i >= 0; i--) {
                            double sacc = y[i];
#pragma unroll
                            for (int k = i + 1; k < 6; k++) sacc -= Lp[PO_IDX(i, k)] * y[k];
                            y[i] = sacc;
                        }
#pragma unroll
                        for (int i = 0; i < 6; i++) x[i] = y[i];
                    }
                    double pn[7];
                    se3_oplus(x, pose, pn);                                      // update, SO:422-435
                    for (int k = 0; k < 7; k++) pose[k] = pn[k];
                    PO_T(2);
                    double tc[1] = {0};                                          // computeActiveErrors + activeRobustChi2 at the trial
                    auto trial_edge = [&](int k, int e, const double *Xe, const double *ob, double w0, int rt) {
                        (void)e;
                        if ((level >> k) & 1u) return;
                        const int stereo = !(ob[2] < 0);
                        double P[3], er[3], r0, r1;
                        const double chi2 = po_edge_chi2<GENERAL>(A, cam, pose, Xe, ob, w0, rt, P, er);
                        if (robust) huber(chi2, stereo ? delta_s : delta_m, stereo ? dsqr_s : dsqr_m, &r0, &r1);
                        else r0 = chi2;
                        tc[0] += r0;
                    };
                    if (!GENERAL && KR > 0 && all_mono) {
                        double c2[KR ? KR : 1];
                        bool over = false;
#pragma unroll
                        for (int k = 0; k < KR; k++) {
                            const bool act = (tid + NT * k < n) && !((level >> k) & 1u);
                            double P[3];
                            quat_rot(pose, rX[k], P);
                            P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
                            const double e0 = rO[k][0] - (A.fx * P[0] / P[2] + A.cx), e1 = rO[k][1] - (A.fy * P[1] / P[2] + A.cy);
                            c2[k] = (e0 * e0 + e1 * e1 + 0.0 * 0.0) * rW[k];
                            over = over || (act && c2[k] > dsqr_m);
                        }
                        // Huber's square root only where some lane of the wave needs it (after the first round the gross outliers are
                        // at level 1 and almost every trial of the remaining rounds is quadratic throughout): a wave-uniform branch
                        if (robust && __builtin_amdgcn_ballot_w64(over) != 0) {
#pragma unroll
                            for (int k = 0; k < KR; k++) {
                                const bool act = (tid + NT * k < n) && !((level >> k) & 1u);
                                const double r0 = c2[k] <= dsqr_m ? c2[k] : 2 * sqrt(c2[k]) * delta_m - dsqr_m;
                                tc[0] += act ? r0 : 0.0;
                            }
                        } else {
#pragma unroll
                            for (int k = 0; k < KR; k++) tc[0] += ((tid + NT * k < n) && !((level >> k) & 1u)) ? c2[k] : 0.0;
                        }
                        for_tail_edges(trial_edge);
                    } else for_edges(trial_edge);
                    PO_T(3);
                    // (the SAME reduction as the build step's chi2: a trial that does not move the pose must reproduce current_chi bit for
                    // bit -- rho == 0 is how g2o's loop ends at convergence, LM:151-152; with two different summation orders it never did
                    // and every converged iteration burnt trials until lambda overflowed the step: 58 -> 87 trials on the probe frame)
                    if (NT == 256 && red2) po_block_sum_lds<1>(tc, red2, tot);
                    else po_block_sum<1, NT>(tc, red);
                    PO_T(4);
                    for (int k = 0; k < 7; k++) pose_ev[k] = pose[k];
                    double temp_chi = ok2 ? tc[0] : DBL_MAX;
                    rho = current_chi - temp_chi;
                    double scale = 0;                                            // computeScale, LM:187-194
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && isfinite(temp_chi)) {
                        const double t3 = 2 * rho - 1;
                        double alpha = 1. - t3 * t3 * t3;
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha); ni = 2; current_chi = temp_chi;
                    } else {
                        lambda *= ni; ni *= 2;
                        for (int k = 0; k < 7; k++) pose[k] = pose_bk[k];        // pop
                    }
                    qmax++; lm_trials++;
#ifdef PO_PROF
                    if (blockIdx.x == 0 && threadIdx.x == 0) g_po_prof[6]++;
#endif
                } while (rho < 0 && qmax < 100);
                lm_iters++;
                if (qmax == 100 || rho == 0) ok = 0;                             // LM:151-152
                else {
                    if ((ini_chi - current_chi) * 1e3 < ini_chi) nb++; else nb = 0;   // LM:157-166
                    if (nb >= 3) ok = 0;
                }
            }
        }
        // ---- re-classification (Optimizer.cc:1058-1145): inliers keep the error of the last evaluation (possibly a
        // rejected trial), outliers are re-evaluated at the current estimate; the comparison is in float
        double bad[1] = {0};
        for_edges([&](int k, int e, const double *Xe, const double *ob, double w0, int rt) {
            (void)e;
            double P[3], er[3];
            const double chi2d = po_edge_chi2<GENERAL>(A, cam, ((level >> k) & 1u) ? pose : pose_ev, Xe, ob, w0, rt, P, er);
            const float chi2 = (float)chi2d;
            const float gate = ob[2] < 0 ? 5.991f : 7.815f;
            if (chi2 > gate) { level |= 1u << k; bad[0] += 1; } else level &= ~(1u << k);
        });
        po_block_sum<1, NT>(bad, red);
        PO_T(5);
        nbad = (int)bad[0];
        if (it == 2) robust = 0;                                                 // setRobustKernel(0)
        rounds++;
        if (n < 10) break;                                                       // Optimizer.cc:1147-1148
    }
    for (int e = tid, k = 0; e < n; e += NT, k++) outl[e] = (uint8_t)((level >> k) & 1u);
    if (tid == 0) {
        for (int k = 0; k < 7; k++) A.pose[7 * f + k] = pose[k];
        A.n_inliers[f] = n - nbad;
        if (A.stats) { A.stats[4 * f] = rounds; A.stats[4 * f + 1] = lm_iters; A.stats[4 * f + 2] = lm_trials; A.stats[4 * f + 3] = nbad; }
    }
}

template <bool GENERAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pose_opt(PoArgs A)
{
    __shared__ double red[4][PO_NRED];
    __shared__ double red2[PO_NRED * PO_RED2_K], tot[32];
    extern __shared__ double po_stage[];                         // [stage_cap][7] (dynamic: 0 when the launch is a big batch)
    po_body<GENERAL, 256, 0>(A, red, A.stage_cap > 0 ? po_stage : nullptr, A.stage_cap, red2, tot);
}
// Latency form (round 4): what Optimizer::PoseOptimization(Frame*) launches -- ONE frame, i.e. four waves on the whole
// chip.  k_pose_opt above is held at two waves per SIMD (256 VGPRs) for launches that fill the device and spilled there (151 VGPRs /
// 472 B of scratch in the Pinhole instantiation); a launch of up to 256 frames is at most one workgroup per CU = one wave per SIMD, so
// this instantiation takes the whole register file (512 VGPRs), keeps the first 4 edges of every thread (1024 per frame) in registers
// instead of LDS and spills nothing; edges beyond 1024 are staged in LDS as before.
template <bool GENERAL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_pose_opt_lat(PoArgs A)
{
    __shared__ double red[4][PO_NRED];
    __shared__ double red2[PO_NRED * PO_RED2_K], tot[32];
    extern __shared__ double po_stage[];                         // [stage_cap][7]: edges 1024 .. of a frame (index = edge - 1024)
    po_body<GENERAL, 256, PO_KR>(A, red, A.stage_cap > 0 ? po_stage : nullptr, A.stage_cap, red2, tot);
}
template <bool GENERAL>
__global__ __launch_bounds__(64) void k_pose_opt_wave(PoArgs A)
{
    po_body<GENERAL, 64, GENERAL ? 8 : 16>(A, nullptr);          // (the fisheye / second-camera edge code needs the registers: 512 edges resident)
}

extern "C" int orbhip_pose_optimization_device(orbhip_ctx *ctx, const double *d_Xw, const double *d_obs,
                                               const double *d_inv_sigma2, const int32_t *d_n_edges, int frames, int max_edges,
                                               double fx, double fy, double cx, double cy, double bf, const double *kb8_k,
                                               const orbhip_camera2 *cam2, const uint8_t *d_right,
                                               double *d_pose, uint8_t *d_outlier, int32_t *d_n_inliers, int32_t *d_stats)
{
    if (!ctx || !d_Xw || !d_obs || !d_inv_sigma2 || !d_n_edges || frames <= 0 || max_edges <= 0 || max_edges > 8192 ||
        !d_pose || !d_outlier || !d_n_inliers) { orbhip_set_last_error_internal("bad argument"); return ORBHIP_E_BADARG; }
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    PoArgs A;
    A.Xw = d_Xw; A.obs = d_obs; A.inv_s2 = d_inv_sigma2; A.n = d_n_edges; A.max_edges = max_edges;
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.bf = bf; A.pose = d_pose; A.outlier = d_outlier; A.n_inliers = d_n_inliers;
    A.cam_model = kb8_k ? 1 : 0; for (int k = 0; k < 4; k++) A.kb[k] = kb8_k ? kb8_k[k] : 0.0;
    if ((d_right != nullptr) != (cam2 != nullptr)) { orbhip_set_last_error_internal("cam2 and d_right go together"); return ORBHIP_E_BADARG; }
    A.right = d_right;
    for (int k = 0; k < 7; k++) A.Trl[k] = cam2 ? cam2->Trl[k] : (k == 3 ? 1.0 : 0.0);
    A.fx2 = cam2 ? cam2->fx : 0; A.fy2 = cam2 ? cam2->fy : 0; A.cx2 = cam2 ? cam2->cx : 0; A.cy2 = cam2 ? cam2->cy : 0;
    A.cam2_model = cam2 ? cam2->camera_model : 0; for (int k = 0; k < 4; k++) A.kb2[k] = cam2 ? cam2->kb[k] : 0.0;
    A.stats = d_stats; A.stage_cap = 0;
    const bool general = A.cam_model || A.right;
    // one wave per frame is the throughput form (1024 frames: 1.26 ms vs 2.0 ms); four waves per frame have the shorter latency while
    // the frames fit one round of workgroups (1 frame: 0.36 ms vs 0.71 ms, 64 frames: 0.64 vs 1.12 ms)
    const int wave_min_frames = getenv("ORBHIP_POSE_WAVE_MIN_FRAMES") ? atoi(getenv("ORBHIP_POSE_WAVE_MIN_FRAMES")) : 513;
    if (max_edges <= 2048 && frames >= wave_min_frames) {                // outlier bits: 32 per lane
        if (general) hipLaunchKernelGGL(k_pose_opt_wave<true>, dim3(frames), dim3(64), 0, orbhip_ctx_stream_internal(ctx), A);
        else hipLaunchKernelGGL(k_pose_opt_wave<false>, dim3(frames), dim3(64), 0, orbhip_ctx_stream_internal(ctx), A);
    } else {
        // up to one workgroup per CU the edges are staged in LDS (latency form); bigger launches keep the LDS-free one (occupancy)
        static const int stage_env = getenv("ORBHIP_POSE_STAGE_EDGES") ? atoi(getenv("ORBHIP_POSE_STAGE_EDGES")) : 2048;
        static const int lat_env = getenv("ORBHIP_POSE_LAT") ? atoi(getenv("ORBHIP_POSE_LAT")) : 1;       // 0: round 3's kernel for every launch (A/B)
        const bool lat = frames <= 256 && lat_env;               // at most one workgroup per CU: one wave per SIMD, the whole register file
        A.stage_cap = frames <= 256 ? std::max(0, std::min(max_edges, stage_env) - (lat ? PO_THREADS * PO_KR : 0)) : 0;
        const size_t lds = (size_t)A.stage_cap * 7 * sizeof(double);
        const void *fn = lat ? (general ? reinterpret_cast<const void *>(k_pose_opt_lat<true>) : reinterpret_cast<const void *>(k_pose_opt_lat<false>))
                             : (general ? reinterpret_cast<const void *>(k_pose_opt<true>) : reinterpret_cast<const void *>(k_pose_opt<false>));
        if (lds > 0 && orb_lds_optin(fn, orbhip_ctx_device_internal(ctx), lds)) { orbhip_set_last_error_internal("LDS opt-in (k_pose_opt)"); return ORBHIP_E_HIP; }
        if (lat) {
            if (general) hipLaunchKernelGGL(k_pose_opt_lat<true>, dim3(frames), dim3(PO_THREADS), lds, orbhip_ctx_stream_internal(ctx), A);
            else hipLaunchKernelGGL(k_pose_opt_lat<false>, dim3(frames), dim3(PO_THREADS), lds, orbhip_ctx_stream_internal(ctx), A);
        } else if (general) hipLaunchKernelGGL(k_pose_opt<true>, dim3(frames), dim3(PO_THREADS), lds, orbhip_ctx_stream_internal(ctx), A);
        else hipLaunchKernelGGL(k_pose_opt<false>, dim3(frames), dim3(PO_THREADS), lds, orbhip_ctx_stream_internal(ctx), A);
    }
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

