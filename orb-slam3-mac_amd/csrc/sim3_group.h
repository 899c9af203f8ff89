// sim3_group.h -- g2o::Sim3 as a group, in double: exponential, logarithm, product, inverse, map (Thirdparty/g2o/g2o/types/sim3.h).  A Sim3 is
// E = (qx qy qz qw tx ty tz s), a tangent vector u = (omega, upsilon, sigma).  The one copy in csrc/: pose_graph_kernels.hip and
// sim3_kernels.hip include it (k_sim3_opt compiles to the instructions it had with its private s3_exp / s3_mul / s3_inverse / s3_map,
// profiles/sim3_group_share_streams.txt), and geom_probe_kernels.hip runs each function alone for tests/test_gpu_geom_probe.py.
// Every body opens with its own contraction pragma, as geom3.h does, so the code is the same wherever the #include stands.
#pragma once
#include <hip/hip_runtime.h>
#include "geom3.h"

// g2o::Sim3(Vector7d) (sim3.h:70-142).  Four branches on |sigma| < 1e-5 and theta < 1e-5; the small-angle ones use R = I + Omega + Omega^2
// (not 1/2 Omega^2), kept.
__device__ __forceinline__ void s3_exp(const double *u, double *E)
{
#pragma clang fp contract(fast)
    const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    double O[9], O2[9], R[9];
    skew_and_square(u, O, O2);
    const double s = exp(sigma), eps = 0.00001;
    double A, B, C, ra = 1, rb = 1;                       // R = I + ra * Omega + rb * Omega^2
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
            ra = sin(theta) / theta; rb = (1 - cos(theta)) / (theta * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            ra = sin(theta) / theta; rb = (1 - cos(theta)) / (theta * theta);
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ra * O[i] + rb * O2[i];
    R_to_quat(R, E);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double t = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) t += (A * O[3 * i + j] + B * O2[3 * i + j] + (i == j ? C : 0.0)) * u[3 + j];
        E[4 + i] = t;
    }
    E[7] = s;
}
// Sim3::operator* (sim3.h:266-272): o = a * b
__device__ __forceinline__ void s3_mul(const double *a, const double *b, double *o)
{
#pragma clang fp contract(fast)
    double rt[3];
    quat_rot(a, b + 4, rt);
    quat_mul(a, b, o);
    o[4] = a[7] * rt[0] + a[4]; o[5] = a[7] * rt[1] + a[5]; o[6] = a[7] * rt[2] + a[6];
    o[7] = a[7] * b[7];
}
// Sim3::inverse (sim3.h:233-236)
__device__ __forceinline__ void s3_inverse(const double *a, double *o)
{
#pragma clang fp contract(fast)
    o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3];
    const double m = -1. / a[7], v[3] = {m * a[4], m * a[5], m * a[6]};
    quat_rot(o, v, o + 4);
    o[7] = 1. / a[7];
}
// Sim3::map (sim3.h:144-146)
__device__ __forceinline__ void s3_map(const double *S, const double *X, double *y)
{
#pragma clang fp contract(fast)
    double r[3];
    quat_rot(S, X, r);
    y[0] = S[7] * r[0] + S[4]; y[1] = S[7] * r[1] + S[5]; y[2] = S[7] * r[2] + S[6];
}
// Sim3::log (sim3.h:148-230).  Four branches on |sigma| < 1e-5 and d > 1 - 1e-5, d = (tr R - 1) / 2; the small-angle omega = 1/2 deltaR(R)
// is kept; upsilon = W.lu().solve(t) is Eigen's PartialPivLU: row pivoting on the largest magnitude of the column.
__device__ __forceinline__ void s3_log(const double *S, double *u)
{
#pragma clang fp contract(fast)
    const double s = S[7], sigma = log(s), eps = 0.00001;
    double R[9];
    quat_to_R(S, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double om[3], A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) { for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i]; A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta = acos(d), theta2 = theta * theta, f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d), f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            const double theta2 = theta * theta, a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    double O[9], O2[9];
    skew_and_square(om, O, O2);
    // rows of [W | t] in registers; every index below is a compile-time constant, the row exchanges are selects
    double w0[4], w1[4], w2[4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        w0[j] = A * O[j] + B * O2[j] + (j == 0 ? C : 0.0);
        w1[j] = A * O[3 + j] + B * O2[3 + j] + (j == 1 ? C : 0.0);
        w2[j] = A * O[6 + j] + B * O2[6 + j] + (j == 2 ? C : 0.0);
    }
    w0[3] = S[4]; w1[3] = S[5]; w2[3] = S[6];
#define S3_SWAP(a, b) do { _Pragma("unroll") for (int j_ = 0; j_ < 4; j_++) { const double t_ = a[j_]; a[j_] = b[j_]; b[j_] = t_; } } while (0)
    {   // column 0: the first row of largest magnitude
        const double a0 = fabs(w0[0]), a1 = fabs(w1[0]), a2 = fabs(w2[0]);
        if (a1 > a0 && a1 >= a2) S3_SWAP(w0, w1);
        else if (a2 > a0 && a2 > a1) S3_SWAP(w0, w2);
    }
    {
        const double l1 = w1[0] / w0[0], l2 = w2[0] / w0[0];
#pragma unroll
        for (int j = 1; j < 4; j++) { w1[j] -= l1 * w0[j]; w2[j] -= l2 * w0[j]; }
    }
    if (fabs(w2[1]) > fabs(w1[1])) S3_SWAP(w1, w2);
#undef S3_SWAP
    {
        const double l2 = w2[1] / w1[1];
        w2[2] -= l2 * w1[2]; w2[3] -= l2 * w1[3];
    }
    const double x2 = w2[3] / w2[2];
    const double x1 = (w1[3] - w1[2] * x2) / w1[1];
    const double x0 = (w0[3] - w0[1] * x1 - w0[2] * x2) / w0[0];
    u[0] = om[0]; u[1] = om[1]; u[2] = om[2]; u[3] = x0; u[4] = x1; u[5] = x2; u[6] = sigma;
}
