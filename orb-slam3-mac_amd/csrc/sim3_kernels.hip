// sim3_kernels.hip -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3932-4328, the 8-argument overload) on gfx950, batched over
// keyframe pairs: ONE free 7-DoF vertex (VertexSim3Expmap, include/OptimizableTypes.h:146-172) and a pair of unary-in-effect edges per
// correspondence (EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ, :175-215; their point vertices are fixed).
//
//   S1  g2o::Sim3(Vector7d), operator*, inverse, map     Thirdparty/g2o/g2o/types/sim3.h:70-142,144-146,233-236,266-272
//   S2  residuals                                        include/OptimizableTypes.h:183-190,204-211
//   S3  Huber-weighted quadratic form                    g2o/core/base_binary_edge.hpp:55-120, robust_kernel_impl.cpp:65-91
//   S4  LM control                                       g2o/core/optimization_algorithm_levenberg.cpp:61-194 -- the loop of po_body
//                                                        (pose_kernels.hip) restated for 7 unknowns, same order of operations
//   S5  two-pass schedule                                src/Optimizer.cc:4237-4327
//
// One wave per pair.  Lane l owns correspondences l, l + 64, ...; every sum is a wave-level DPP tree (wave_dpp.h) in a fixed association,
// so there is no LDS and no barrier, and every lane holds the whole LM state and runs the scalar control flow redundantly on the reduced
// sums (28 + 7 + 1 doubles per build).  The state of a correspondence (0 active, 1 dropped after pass 1, 2 dropped after pass 2, 3 no
// edge) lives in the caller's flag row: a lane only ever reads back its own bytes.
// The rows arrive with their weights: a row without keypoint in KF2 carries mvInvLevelSigma2[0] (Optimizer.cc:4178 passes
// mnTrackScaleLevel to cv::KeyPoint as the size, the octave read at :4220 stays 0) and the normalised "observation" of :4163-4177.
// Deliberate departure: the Jacobians are analytic (the reference differentiates numerically with a 1e-9 step, base_binary_edge.hpp:
// 136-200); DESIGN 4c has the measured distance between the two.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "geom3.h"
#include "sim3_group.h"
#include "ba_camera.h"
#pragma clang fp contract(fast)       // as ba_kernels.hip: the double-precision optimisers are compared to 1e-9, not bit for bit
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

#define S3_NRED 36            // robust chi2 + 28 upper-triangle entries of H + 7 of b
#define S3_IDX(a, c) ((a) * 7 - (a) * ((a) - 1) / 2 + ((c) - (a)))      // packed upper triangle, a <= c

struct S3Cam { double fx, fy, cx, cy; int model; double kb[4]; };
struct S3Args {
    const double *P1, *P2, *o1, *o2, *w1, *w2;
    const int32_t *n;
    int max_edges;
    S3Cam c1, c2;
    double th2, delta, dsqr;            // Huber delta = (float)sqrt(th2), dsqr = (float)(delta * delta) (robust_kernel_impl.cpp:65-69)
    int fix_scale;
    double *sim3;
    uint8_t *flag;
    int32_t *n_in, *stats, *status;
};

// (quat_rot -- the form Sim3::map uses; g2o::Sim3 normalises nowhere --, quat_to_R, R_to_quat, quat_mul, huber: geom3.h;
// s3_exp, s3_mul, s3_inverse, s3_map -- g2o::Sim3(Vector7d), operator*, inverse, map --: sim3_group.h, the one copy, run alone by
// geom_probe_kernels.hip; k_sim3_opt compiles to the instructions it had with its private copies, profiles/sim3_group_share_streams.txt)
// one edge's computeError: e = obs - cam.project(S.map(X)); returns chi2 = e^T (w I) e
__device__ __forceinline__ double s3_edge(const S3Cam &c, const double *S, const double *X, const double *ob, double w, double *y, double *e)
{
    double uv[2];
    s3_map(S, X, y);
    cam_project(c.fx, c.fy, c.cx, c.cy, c.model, c.kb, y, uv);
    e[0] = ob[0] - uv[0]; e[1] = ob[1] - uv[1];
    return (e[0] * e[0] + e[1] * e[1]) * w;
}
// acc += the edge's share of (robust chi2 | H | b): J [2][7], weight w = rho' * inv_sigma2
__device__ __forceinline__ void s3_accumulate(double (&acc)[S3_NRED], const double *J, double w, const double *e, double r0)
{
    acc[0] += r0;
    int h = 1;
#pragma unroll
    for (int a = 0; a < 7; a++) {
#pragma unroll
        for (int c = a; c < 7; c++) acc[h++] += J[a] * w * J[c] + J[7 + a] * w * J[7 + c];
    }
#pragma unroll
    for (int a = 0; a < 7; a++) acc[29 + a] += J[a] * (-w * e[0]) + J[7 + a] * (-w * e[1]);
}
// J [2][7] = -Jp [2][3] * D [3][7]
__device__ __forceinline__ void s3_chain(const double *Jp, const double (&D)[21], int fix_scale, double *J)
{
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
        for (int c = 0; c < 7; c++) J[7 * r + c] = -(Jp[3 * r] * D[c] + Jp[3 * r + 1] * D[7 + c] + Jp[3 * r + 2] * D[14 + c]);
        if (fix_scale) J[7 * r + 6] = 0;
    }
}

__global__ __launch_bounds__(64) void k_sim3_opt(S3Args A)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = A.n[f];
    const size_t row = (size_t)f * A.max_edges;
    const double *P1 = A.P1 + row * 3, *P2 = A.P2 + row * 3, *o1 = A.o1 + row * 2, *o2 = A.o2 + row * 2, *w1 = A.w1 + row, *w2 = A.w2 + row;
    uint8_t *flag = A.flag + row;
    if (n > A.max_edges || n < 0) {                                      // an oversized (or negative) count: status word, nothing written to its rows
        if (lane == 0) { atomicExch(A.status, ORBHIP_E_CAPACITY); A.n_in[f] = 0; if (A.stats) { for (int k = 0; k < 4; k++) A.stats[4 * f + k] = 0; } }
        return;
    }
    // Optimizer.cc:4082-4088: a correspondence whose P3D2c.z < 0 gets no edges
    double cnt[1] = {0};
    for (int e = lane; e < n; e += 64) { const bool no_edge = P2[3 * e + 2] < 0; flag[e] = no_edge ? 3 : 0; cnt[0] += no_edge ? 0.0 : 1.0; }
    const int ncorr = (int)wave_sum_f64_dpp(cnt[0]);
    double S0[8], S[8], Sev[8], x[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 8; k++) { S0[k] = A.sim3[8 * f + k]; S[k] = S0[k]; Sev[k] = S0[k]; }
    int lm_iters = 0, lm_trials = 0;

    // SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg over the active correspondences (flag 0)
    auto optimize = [&](int iters, int robust) {
        double lambda = 0, ni = 2;
        int nb = 0, ok = 1;
        for (int iter = 0; iter < iters && ok; iter++) {
            // ---- computeActiveErrors + activeRobustChi2 + buildSystem at the current estimate (LM:69-87)
            double acc[S3_NRED];
#pragma unroll
            for (int k = 0; k < S3_NRED; k++) acc[k] = 0;
            double Si[8], Ri[9];
            s3_inverse(S, Si);
            quat_to_R(Si, Ri);
            for (int e = lane; e < n; e += 64) {
                if (flag[e]) continue;
                const double X1[3] = {P1[3 * e], P1[3 * e + 1], P1[3 * e + 2]}, X2[3] = {P2[3 * e], P2[3 * e + 1], P2[3 * e + 2]};
                const double ob1[2] = {o1[2 * e], o1[2 * e + 1]}, ob2[2] = {o2[2 * e], o2[2 * e + 1]};
                double y[3], er[2], Jp[6], J[14], r0, r1;
                {   // EdgeSim3ProjectXYZ: y = S12.map(P2c), dy/d(delta) = [ -[y]x | I | y ]
                    const double chi2 = s3_edge(A.c1, S, X2, ob1, w1[e], y, er);
                    if (robust) huber(chi2, A.delta, A.dsqr, &r0, &r1); else { r0 = chi2; r1 = 1.; }
                    cam_project_jac(A.c1.fx, A.c1.fy, A.c1.model, A.c1.kb, y, Jp);
                    const double D[21] = {0, y[2], -y[1], 1, 0, 0, y[0],
                                          -y[2], 0, y[0], 0, 1, 0, y[1],
                                          y[1], -y[0], 0, 0, 0, 1, y[2]};
                    s3_chain(Jp, D, A.fix_scale, J);
                    s3_accumulate(acc, J, r1 * w1[e], er, r0);
                }
                {   // EdgeInverseSim3ProjectXYZ: y' = S12^-1.map(P1c), dy'/d(delta) = -(1/s) R^T [ -[P1c]x | I | P1c ]
                    const double chi2 = s3_edge(A.c2, Si, X1, ob2, w2[e], y, er);
                    if (robust) huber(chi2, A.delta, A.dsqr, &r0, &r1); else { r0 = chi2; r1 = 1.; }
                    cam_project_jac(A.c2.fx, A.c2.fy, A.c2.model, A.c2.kb, y, Jp);
                    const double M[21] = {0, X1[2], -X1[1], 1, 0, 0, X1[0],
                                          -X1[2], 0, X1[0], 0, 1, 0, X1[1],
                                          X1[1], -X1[0], 0, 0, 0, 1, X1[2]};
                    double D[21];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int c = 0; c < 7; c++) D[7 * r + c] = -Si[7] * (Ri[3 * r] * M[c] + Ri[3 * r + 1] * M[7 + c] + Ri[3 * r + 2] * M[14 + c]);
                    }
                    s3_chain(Jp, D, A.fix_scale, J);
                    s3_accumulate(acc, J, r1 * w2[e], er, r0);
                }
            }
#pragma unroll
            for (int k = 0; k < S3_NRED; k++) acc[k] = wave_sum_f64_dpp(acc[k]);
            for (int k = 0; k < 8; k++) Sev[k] = S[k];
            double current_chi = acc[0];
            const double ini_chi = current_chi;
            double Hp[28], b[7];
#pragma unroll
            for (int k = 0; k < 28; k++) Hp[k] = acc[1 + k];
#pragma unroll
            for (int a = 0; a < 7; a++) b[a] = acc[29 + a];
            if (iter == 0) {                                                     // computeLambdaInit, LM:171-185 (_tau = 1e-50, LM:47)
                double md = 0;
#pragma unroll
                for (int a = 0; a < 7; a++) md = fmax(fabs(Hp[S3_IDX(a, a)]), md);
                lambda = 1e-50 * md; ni = 2; nb = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                double S_bk[8];
                for (int k = 0; k < 8; k++) S_bk[k] = S[k];                      // push
                // LinearSolverDense: LDL^T of H + lambda I; a non-positive pivot fails the solve (x keeps its old value)
                double Lp[28];
#pragma unroll
                for (int k = 0; k < 28; k++) Lp[k] = Hp[k];
#pragma unroll
                for (int a = 0; a < 7; a++) Lp[S3_IDX(a, a)] += lambda;
                bool ok2 = true;
#pragma unroll
                for (int j = 0; j < 7; j++) {
                    double d = Lp[S3_IDX(j, j)];
#pragma unroll
                    for (int k = 0; k < j; k++) d -= Lp[S3_IDX(k, j)] * Lp[S3_IDX(k, j)] * Lp[S3_IDX(k, k)];
                    ok2 = ok2 && (d > 0.0) && isfinite(d);
                    Lp[S3_IDX(j, j)] = d;
#pragma unroll
                    for (int i = j + 1; i < 7; i++) {
                        double sacc = Lp[S3_IDX(j, i)];
#pragma unroll
                        for (int k = 0; k < j; k++) sacc -= Lp[S3_IDX(k, i)] * Lp[S3_IDX(k, j)] * Lp[S3_IDX(k, k)];
                        Lp[S3_IDX(j, i)] = sacc / d;
                    }
                }
                if (ok2) {
                    double y[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        double sacc = b[i];
#pragma unroll
                        for (int k = 0; k < i; k++) sacc -= Lp[S3_IDX(k, i)] * y[k];
                        y[i] = sacc;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) y[i] /= Lp[S3_IDX(i, i)];
#pragma unroll
                    for (int i = 6; i >= 0; i--) {
                        double sacc = y[i];
#pragma unroll
                        for (int k = i + 1; k < 7; k++) sacc -= Lp[S3_IDX(i, k)] * y[k];
                        y[i] = sacc;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) x[i] = y[i];
                }
                if (A.fix_scale) x[6] = 0;                                       // oplusImpl writes through to the solver's x (OptimizableTypes.h:160-163)
                double E[8], Sn[8];
                s3_exp(x, E);                                                    // update: Sim3(update) * estimate
                s3_mul(E, S, Sn);
                for (int k = 0; k < 8; k++) S[k] = Sn[k];
                // ---- computeActiveErrors + activeRobustChi2 at the trial (the SAME reduction as the build step's chi2, see po_body)
                double tc = 0;
                s3_inverse(S, Si);
                for (int e = lane; e < n; e += 64) {
                    if (flag[e]) continue;
                    const double X1[3] = {P1[3 * e], P1[3 * e + 1], P1[3 * e + 2]}, X2[3] = {P2[3 * e], P2[3 * e + 1], P2[3 * e + 2]};
                    const double ob1[2] = {o1[2 * e], o1[2 * e + 1]}, ob2[2] = {o2[2 * e], o2[2 * e + 1]};
                    double y[3], er[2], r0, r1;
                    double chi2 = s3_edge(A.c1, S, X2, ob1, w1[e], y, er);
                    if (robust) huber(chi2, A.delta, A.dsqr, &r0, &r1); else r0 = chi2;
                    tc += r0;
                    chi2 = s3_edge(A.c2, Si, X1, ob2, w2[e], y, er);
                    if (robust) huber(chi2, A.delta, A.dsqr, &r0, &r1); else r0 = chi2;
                    tc += r0;
                }
                tc = wave_sum_f64_dpp(tc);
                for (int k = 0; k < 8; k++) Sev[k] = S[k];
                const double temp_chi = ok2 ? tc : DBL_MAX;
                rho = current_chi - temp_chi;
                double scale = 0;                                                // computeScale, LM:187-194
                for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && isfinite(temp_chi)) {
                    const double t3 = 2 * rho - 1;
                    double alpha = 1. - t3 * t3 * t3;
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha); ni = 2; current_chi = temp_chi;
                } else {
                    lambda *= ni; ni *= 2;
                    for (int k = 0; k < 8; k++) S[k] = S_bk[k];                  // pop
                }
                qmax++; lm_trials++;
            } while (rho < 0 && qmax < 100);                                     // _maxTrialsAfterFailure = 100 (LM:51)
            lm_iters++;
            if (qmax == 100 || rho == 0) ok = 0;                                 // LM:151-152
            else {
                if ((ini_chi - current_chi) * 1e3 < ini_chi) nb++; else nb = 0;  // LM:157-166
                if (nb >= 3) ok = 0;
            }
        }
    };
    // a pair is dropped when either edge's chi2 > th2, evaluated at `at`; returns the number dropped (wave-uniform)
    auto classify = [&](const double *at, uint8_t mark) {
        double Si[8], bad = 0;
        s3_inverse(at, Si);
        for (int e = lane; e < n; e += 64) {
            if (flag[e]) continue;
            const double X1[3] = {P1[3 * e], P1[3 * e + 1], P1[3 * e + 2]}, X2[3] = {P2[3 * e], P2[3 * e + 1], P2[3 * e + 2]};
            const double ob1[2] = {o1[2 * e], o1[2 * e + 1]}, ob2[2] = {o2[2 * e], o2[2 * e + 1]};
            double y[3], er[2];
            const double c12 = s3_edge(A.c1, at, X2, ob1, w1[e], y, er), c21 = s3_edge(A.c2, Si, X1, ob2, w2[e], y, er);
            if (c12 > A.th2 || c21 > A.th2) { flag[e] = mark; bad += 1; }
        }
        return (int)wave_sum_f64_dpp(bad);
    };

    int nbad = 0, nin = 0;
    bool write_sim3 = false;
    if (ncorr > 0) {
        optimize(5, 1);                                                          // Optimizer.cc:4238-4239
        // :4244-4271: NO computeError() here -- the stored errors are those of the LAST LM trial, accepted or not
        nbad = classify(Sev, 1);
        if (ncorr - nbad >= 10) {                                                // :4288-4289
            optimize(nbad > 0 ? 10 : 5, 0);                                      // :4282-4294, survivors without their robust kernel
            nin = ncorr - nbad - classify(S, 2);                                 // :4298-4318, fresh errors at the estimate
            write_sim3 = true;
        }
    }
    if (lane == 0) {
        if (write_sim3) { for (int k = 0; k < 8; k++) A.sim3[8 * f + k] = S[k]; }
        A.n_in[f] = nin;
        if (A.stats) { A.stats[4 * f] = ncorr; A.stats[4 * f + 1] = nbad; A.stats[4 * f + 2] = lm_iters; A.stats[4 * f + 3] = lm_trials; }
    }
}

}  // namespace

extern "C" int orbhip_optimize_sim3_device(orbhip_ctx *ctx, const double *d_P1c, const double *d_P2c, const double *d_obs1, const double *d_obs2,
        const double *d_inv_sigma2_1, const double *d_inv_sigma2_2, const int32_t *d_n, int pairs, int max_edges,
        const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2, double th2, int fix_scale,
        double *d_sim3, uint8_t *d_flag, int32_t *d_n_in, int32_t *d_stats)
{
    if (!ctx || !d_P1c || !d_P2c || !d_obs1 || !d_obs2 || !d_inv_sigma2_1 || !d_inv_sigma2_2 || !d_n || pairs <= 0 || max_edges <= 0 ||
        !cam1 || !cam2 || !(th2 > 0) || !d_sim3 || !d_flag || !d_n_in || (cam1->camera_model != 0 && cam1->camera_model != 1) ||
        (cam2->camera_model != 0 && cam2->camera_model != 1)) {
        orbhip_set_last_error_internal("orbhip_optimize_sim3_device: bad argument");
        return ORBHIP_E_BADARG;
    }
    if (max_edges > 8192) { orbhip_set_last_error_internal("orbhip_optimize_sim3_device: at most 8192 correspondences per pair"); return ORBHIP_E_CAPACITY; }
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    S3Args A;
    A.P1 = d_P1c; A.P2 = d_P2c; A.o1 = d_obs1; A.o2 = d_obs2; A.w1 = d_inv_sigma2_1; A.w2 = d_inv_sigma2_2; A.n = d_n; A.max_edges = max_edges;
    const orbhip_sim3_camera *cs[2] = {cam1, cam2};
    S3Cam *cd[2] = {&A.c1, &A.c2};
    for (int i = 0; i < 2; i++) {
        cd[i]->fx = cs[i]->fx; cd[i]->fy = cs[i]->fy; cd[i]->cx = cs[i]->cx; cd[i]->cy = cs[i]->cy; cd[i]->model = cs[i]->camera_model;
        for (int k = 0; k < 4; k++) cd[i]->kb[k] = cs[i]->kb[k];
    }
    const float delta = sqrtf((float)th2);                                       // Optimizer.cc:3992
    A.th2 = th2; A.delta = (double)delta; A.dsqr = (double)(float)((double)delta * (double)delta);
    A.fix_scale = fix_scale ? 1 : 0;
    A.sim3 = d_sim3; A.flag = d_flag; A.n_in = d_n_in; A.stats = d_stats; A.status = orbhip_ctx_status_internal(ctx);
    hipLaunchKernelGGL(k_sim3_opt, dim3(pairs), dim3(64), 0, orbhip_ctx_stream_internal(ctx), A);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_sim3_opt launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
