// ba_edges.h -- the SE3 vertex and the three visual edge types of the bundle adjustments, shared by the local, global and sharded BA
// (ba_edge_kernels.hip, ba_lm_kernels.hip) and pose_kernels.hip (pose-only BA):
//   B1  SE3Quat exp / oplus / operator*      Thirdparty/g2o/g2o/types/se3quat.h:104-110,223-257
//   B2  residuals                            include/OptimizableTypes.h:99-126, types_six_dof_expmap.cpp:190-197
//   B3  Jacobians                            src/OptimizableTypes.cpp:139-213, types_six_dof_expmap.cpp:228-274
// Every body opens with `#pragma clang fp contract(fast)` (see geom3.h): the edges compile contracted wherever the #include stands.
#pragma once
#include "geom3.h"
#include "ba_camera.h"
#include "ba_graph_lists.h"      // BaCamDev, BaGraphDev: the edge functions below are templates over the calibration object, either of the two

// ------------------------------------------------------------------ SE3 helpers (B1)
// T_new = exp(u) * T  (VertexSE3Expmap::oplusImpl)
__device__ __forceinline__ void se3_oplus(const double *u, const double *pose, double *out)
{
#pragma clang fp contract(fast)
    const double om0 = u[0], om1 = u[1], om2 = u[2];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    double O[9], O2[9], R[9], V[9];
    skew_and_square(u, O, O2);
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i]; V[i] = R[i]; }
    } else {
        double sn, cs;
        sincos(theta, &sn, &cs);                             // one argument reduction for both (the same values sin() and cos() return)
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        const double c = (theta - sn) / (theta * theta * theta);
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double I = (i % 4 == 0 ? 1.0 : 0.0);
            R[i] = I + a * O[i] + b * O2[i];
            V[i] = I + b * O[i] + c * O2[i];
        }
    }
    double qe[4], te[3], rt[3], qn[4];
    R_to_quat(R, qe);
#pragma unroll
    for (int i = 0; i < 3; i++) te[i] = V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
    quat_norm_rot(qe);
    quat_rot(qe, pose + 4, rt);
    quat_mul(qe, pose, qn);
    quat_norm_rot(qn);
    out[0] = qn[0]; out[1] = qn[1]; out[2] = qn[2]; out[3] = qn[3];
    out[4] = te[0] + rt[0]; out[5] = te[1] + rt[1]; out[6] = te[2] + rt[2];
}

// ------------------------------------------------------------------ second camera (EdgeSE3ProjectXYZToBody)
// SE3Quat::operator* (se3quat.h:104-110): o = a * b
__device__ __forceinline__ void se3_mul(const double *a, const double *b, double *o)
{
#pragma clang fp contract(fast)
    double rt[3], q[4];
    quat_rot(a, b + 4, rt);
    quat_mul(a, b, q);
    quat_norm_rot(q);
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
    o[4] = a[4] + rt[0]; o[5] = a[5] + rt[1]; o[6] = a[6] + rt[2];
}
// EdgeSE3ProjectXYZToBody::computeError (OptimizableTypes.h:121-126): obs - cam2.project((mTrl * T_lw).map(X)); P = that point
template <class CAM>
__device__ __forceinline__ void tobody_error(const CAM &g, const double *pose, const double *X, const double *obs, double *P, double *err)
{
#pragma clang fp contract(fast)
    double Trw[7], uv[2];
    se3_mul(g.Trl, pose, Trw);
    quat_rot(Trw, X, P);
    P[0] += Trw[4]; P[1] += Trw[5]; P[2] += Trw[6];
    cam_project(g.fx2, g.fy2, g.cx2, g.cy2, g.cam2_model, g.kb2, P, uv);
    err[0] = obs[0] - uv[0]; err[1] = obs[1] - uv[1]; err[2] = 0;
}
// EdgeSE3ProjectXYZToBody::linearizeOplus (OptimizableTypes.cpp:192-213); rows 2 of Jx / Jt zeroed
template <class CAM>
__device__ __forceinline__ void tobody_jacobians(const CAM &g, const double *pose, const double *X, double *Jx, double *Jt)
{
#pragma clang fp contract(fast)
    double Trw[7], Xl[3], Xr[3], J[6], Rrw[9], Rrl[9], M[6];
    se3_mul(g.Trl, pose, Trw);
    quat_rot(pose, X, Xl); Xl[0] += pose[4]; Xl[1] += pose[5]; Xl[2] += pose[6];
    quat_rot(g.Trl, Xl, Xr); Xr[0] += g.Trl[4]; Xr[1] += g.Trl[5]; Xr[2] += g.Trl[6];
    cam_project_jac(g.fx2, g.fy2, g.cam2_model, g.kb2, Xr, J);
    quat_to_R(Trw, Rrw); quat_to_R(g.Trl, Rrl);
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            Jx[3 * r + c] = -(J[3 * r] * Rrw[c] + J[3 * r + 1] * Rrw[3 + c] + J[3 * r + 2] * Rrw[6 + c]);
            M[3 * r + c] = J[3 * r] * Rrl[c] + J[3 * r + 1] * Rrl[3 + c] + J[3 * r + 2] * Rrl[6 + c];
        }
    const double x = Xl[0], y = Xl[1], z = Xl[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const double m0 = M[3 * r], m1 = M[3 * r + 1], m2 = M[3 * r + 2];
        Jt[6 * r + 0] = -(-m1 * z + m2 * y); Jt[6 * r + 1] = -(m0 * z - m2 * x); Jt[6 * r + 2] = -(-m0 * y + m1 * x);
        Jt[6 * r + 3] = -m0; Jt[6 * r + 4] = -m1; Jt[6 * r + 5] = -m2;
    }
#pragma unroll
    for (int k = 6; k < 9; k++) Jx[k] = 0;
#pragma unroll
    for (int k = 12; k < 18; k++) Jt[k] = 0;
}
// z of the edge's camera-frame point (isDepthPositive of the three edge types)
template <class CAM>
__device__ __forceinline__ double edge_depth(const CAM &g, const double *pose, const double *X, int type)
{
#pragma clang fp contract(fast)
    double P[3];
    if (type == 2) { double Trw[7]; se3_mul(g.Trl, pose, Trw); quat_rot(Trw, X, P); return P[2] + Trw[6]; }
    quat_rot(pose, X, P);
    return P[2] + pose[6];
}

// ------------------------------------------------------------------ edge math (B2, B3)
template <bool KB = true, class CAM = BaCamDev>      // KB = false: Pinhole only (the KannalaBrandt8 branch and its registers compile away)
__device__ __forceinline__ void edge_error(const CAM &g, const double *pose, const double *X, const double *obs,
                                           int stereo, double *P, double *err)
{
#pragma clang fp contract(fast)
    quat_rot(pose, X, P);
    P[0] += pose[4]; P[1] += pose[5]; P[2] += pose[6];
    if (KB && !stereo && g.cam_model == 1) {   // KannalaBrandt8::project, KannalaBrandt8.cpp:52-69; atan2f as the float rounding of the double atan2 (see oracle/ba_oracle.c)
        const double x2y2 = P[0] * P[0] + P[1] * P[1];
        const double theta = (double)(float)atan2((double)sqrtf((float)x2y2), (double)(float)P[2]);
        const double psi = (double)(float)atan2((double)(float)P[1], (double)(float)P[0]);
        const double t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
        const double r = theta + g.kb[0] * t3 + g.kb[1] * t5 + g.kb[2] * t7 + g.kb[3] * t9;
        err[0] = obs[0] - (g.fx * r * cos(psi) + g.cx);
        err[1] = obs[1] - (g.fy * r * sin(psi) + g.cy);
        err[2] = 0;
        return;
    }
    if (!stereo) {
        err[0] = obs[0] - (g.fx * P[0] / P[2] + g.cx);
        err[1] = obs[1] - (g.fy * P[1] / P[2] + g.cy);
        err[2] = 0;
    } else {   // float invz / float bf, types_six_dof_expmap.cpp:190-197
        const float invz = (float)(1.0 / P[2]);
        const float bff = (float)g.bf;
        const double r0 = P[0] * invz * g.fx + g.cx;
        err[0] = obs[0] - r0;
        err[1] = obs[1] - (P[1] * invz * g.fy + g.cy);
        err[2] = obs[2] - (r0 - (double)__fmul_rn(bff, invz));
    }
}

// Jacobians at camera-frame point P with rotation R.  Jx: D x 3, Jt: D x 6 (row-major)
template <bool KB = true, class CAM = BaCamDev>
__device__ __forceinline__ void edge_jacobians(const CAM &g, const double *P, const double *R, int stereo, double *Jx, double *Jt)
{
#pragma clang fp contract(fast)
    const double x = P[0], y = P[1], z = P[2];
    if (KB && !stereo && g.cam_model == 1) {   // KannalaBrandt8::projectJac, KannalaBrandt8.cpp:166-195
        const double x2 = x * x, y2 = y * y, z2 = z * z, r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
        const double theta = atan2(r, z);
        const double t2 = theta * theta, t3 = t2 * theta, t4 = t2 * t2, t5 = t4 * theta, t6 = t2 * t4, t7 = t6 * theta, t8 = t4 * t4, t9 = t8 * theta;
        const double f = theta + t3 * g.kb[0] + t5 * g.kb[1] + t7 * g.kb[2] + t9 * g.kb[3];
        const double fd = 1 + 3 * g.kb[0] * t2 + 5 * g.kb[1] * t4 + 7 * g.kb[2] * t6 + 9 * g.kb[3] * t8;
        const double J00 = g.fx * (fd * z * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
        const double J10 = g.fy * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3);
        const double J01 = g.fx * (fd * z * y * x / (r2 * (r2 + z2)) - f * y * x / r3);
        const double J11 = g.fy * (fd * z * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
        const double J02 = -g.fx * fd * x / (r2 + z2), J12 = -g.fy * fd * y / (r2 + z2);
        for (int c = 0; c < 3; c++) {                // Jx = -projectJac * R  (OptimizableTypes.cpp:139-160)
            Jx[c] = -(J00 * R[c] + J01 * R[3 + c] + J02 * R[6 + c]);
            Jx[3 + c] = -(J10 * R[c] + J11 * R[3 + c] + J12 * R[6 + c]);
        }
        // Jt = -projectJac * [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]
        Jt[0] = -(-J01 * z + J02 * y); Jt[1] = -(J00 * z - J02 * x); Jt[2] = -(-J00 * y + J01 * x); Jt[3] = -J00; Jt[4] = -J01; Jt[5] = -J02;
        Jt[6] = -(-J11 * z + J12 * y); Jt[7] = -(J10 * z - J12 * x); Jt[8] = -(-J10 * y + J11 * x); Jt[9] = -J10; Jt[10] = -J11; Jt[11] = -J12;
        return;
    }
    if (!stereo) {
        const double iz = 1.0 / z;
        const double p00 = -(g.fx / z), p02 = g.fx * x / (z * z), p11 = -(g.fy / z), p12 = g.fy * y / (z * z);
        (void)iz;
        for (int c = 0; c < 3; c++) {
            Jx[c] = p00 * R[c] + p02 * R[6 + c];
            Jx[3 + c] = p11 * R[3 + c] + p12 * R[6 + c];
        }
        // SE3deriv = [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]
        Jt[0] = p02 * y;            Jt[1] = p00 * z - p02 * x;  Jt[2] = -p00 * y;  Jt[3] = p00; Jt[4] = 0;   Jt[5] = p02;
        Jt[6] = -p11 * z + p12 * y; Jt[7] = -p12 * x;           Jt[8] = p11 * x;   Jt[9] = 0;   Jt[10] = p11; Jt[11] = p12;
    } else {
        const double z2 = z * z, fx = g.fx, fy = g.fy, bf = g.bf;
        for (int c = 0; c < 3; c++) {
            Jx[c] = -fx * R[c] / z + fx * x * R[6 + c] / z2;
            Jx[3 + c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z2;
            Jx[6 + c] = Jx[c] - bf * R[6 + c] / z2;
        }
        Jt[0] = x * y / z2 * fx; Jt[1] = -(1 + (x * x / z2)) * fx; Jt[2] = y / z * fx;
        Jt[3] = -1. / z * fx; Jt[4] = 0; Jt[5] = x / z2 * fx;
        Jt[6] = (1 + y * y / z2) * fy; Jt[7] = -x * y / z2 * fy; Jt[8] = -x / z * fy;
        Jt[9] = 0; Jt[10] = -1. / z * fy; Jt[11] = y / z2 * fy;
        Jt[12] = Jt[0] - bf * y / z2; Jt[13] = Jt[1] + bf * x / z2; Jt[14] = Jt[2];
        Jt[15] = Jt[3]; Jt[16] = 0; Jt[17] = Jt[5] - bf / z2;
    }
}
