// iba_edges.h -- the rig's cameras, the visual edges on an ImuCamPose vertex and EdgeInertial, shared by the inertial BA
// (iba_kernels.hip: LocalInertialBA, FullInertialBA) and the inertial pose-only optimisation (pose_inertial_kernels.hip); the inertial
// counterpart of ba_edges.h.  The SO(3) formulas are so3_f64.h's, the state and preintegration layout is imu_layout.h's.
// Every body that computes opens with `#pragma clang fp contract(fast)` (see geom3.h): the edges compile contracted wherever the
// #include stands.  The functions have internal linkage: each includer compiles its own.
//
// Qualifiers: cam_pose and visual_jac are plain __device__ by default (the inliner decides), the rest are force-inlined.  In this form the code of
// k_iba_solve, k_fiba_solve<*> and their out-of-line phases is instruction for instruction what it was when these functions stood in
// iba_kernels.hip (profiles/iba_split_streams.txt).  k_pose_inertial is the one kernel whose code depends on how these two are inlined
// (DESIGN.md 3b): pose_inertial_kernels.hip defines IBA_EDGES_FORCE_INLINE before the #include and gets them force-inlined, the form
// that measured fastest there (profiles/pose_inertial_split_ab.json).
#pragma once
#include "geom3.h"
#include "so3_f64.h"
#include "ba_camera.h"
#include "imu_layout.h"
#include "iba_pack.h"          // IbaWin

// the qualifier of cam_pose and visual_jac, chosen by the includer (see above)
#ifdef IBA_EDGES_FORCE_INLINE
#define IBA_EDGES_HELPER __device__ __forceinline__
#else
#define IBA_EDGES_HELPER __device__
#endif

namespace {
// camera `idx` of the rig: extrinsics w.r.t. the body (G2oTypes.cc:49-52, 57-67) and intrinsics
struct CamView { const double *Rcb, *tcb, *kb; double fx, fy, cx, cy; int model; };
__device__ __forceinline__ CamView cam_view(const IbaWin &W, int idx)
{
    CamView V;
    if (idx == 0) { V.Rcb = W.Rcb; V.tcb = W.tcb; V.kb = W.kb; V.fx = W.fx; V.fy = W.fy; V.cx = W.cx; V.cy = W.cy; V.model = W.cam_model; }
    else { V.Rcb = W.Rcb2; V.tcb = W.tcb2; V.kb = W.kb2; V.fx = W.fx2; V.fy = W.fy2; V.cx = W.cx2; V.cy = W.cy2; V.model = W.cam2_model; }
    return V;
}
// Rcw = Rcb Rbw, tcw = Rcb tbw + tcb for every camera of the keyframe (ImuCamPose::Update, G2oTypes.cc:212-219); c: [2][12]
IBA_EDGES_HELPER void cam_pose(const IbaWin &W, const double *s, double *c)
{
#pragma clang fp contract(fast)
    double Rbw[9], tbw[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rbw[3 * i + j] = s[K_R + 3 * j + i];
    mv3(Rbw, s + K_T, tbw);
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    for (int cam = 0; cam <= W.has_cam2; cam++) {
        const CamView V = cam_view(W, cam);
        double R[9], t[3];
        mm3(V.Rcb, Rbw, R);
        mv3(V.Rcb, tbw, t);
        for (int i = 0; i < 9; i++) c[12 * cam + i] = R[i];
        for (int i = 0; i < 3; i++) c[12 * cam + 9 + i] = t[i] + V.tcb[i];
    }
}

// EdgeMono / EdgeStereo::computeError (G2oTypes.h:350-355, G2oTypes.cc:170-185); type 0 EdgeMono(0), 1 EdgeStereo(0), 2 EdgeMono(1);
// c = the pose of the edge's camera
__device__ __forceinline__ void visual_error(const IbaWin &W, const CamView &V, const double *c, const double *X, const double *obs, int type, double *er, double *Xc)
{
#pragma clang fp contract(fast)
    mv3(c, X, Xc);
    Xc[0] += c[9]; Xc[1] += c[10]; Xc[2] += c[11];
    double uv[2];
    cam_project(V.fx, V.fy, V.cx, V.cy, V.model, V.kb, Xc, uv);
    er[0] = obs[0] - uv[0]; er[1] = obs[1] - uv[1];
    er[2] = type == 1 ? obs[2] - (uv[0] - W.bf * (1 / Xc[2])) : 0.0;
}

// linearizeOplus (G2oTypes.cc:349-373, :397-423): Jx [3][3], Jp [3][6]; row 2 zero when mono
IBA_EDGES_HELPER void visual_jac(const IbaWin &W, const CamView &V, const double *c, const double *Xc, int type, double *Jx, double *Jp)
{
#pragma clang fp contract(fast)
    double pj[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    cam_project_jac(V.fx, V.fy, V.model, V.kb, Xc, pj);
    if (type == 1) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + W.bf * (1.0 / (Xc[2] * Xc[2])); }
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
        for (int j = 0; j < 3; j++) Jx[3 * d + j] = -(pj[3 * d] * c[j] + pj[3 * d + 1] * c[3 + j] + pj[3 * d + 2] * c[6 + j]);
    double Xb[3];
    const double d0[3] = {Xc[0] - V.tcb[0], Xc[1] - V.tcb[1], Xc[2] - V.tcb[2]};
    mtv3(V.Rcb, d0, Xb);
    double PR[9];
    mm3(pj, V.Rcb, PR);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double p0 = PR[3 * d], p1 = PR[3 * d + 1], p2 = PR[3 * d + 2];
        Jp[6 * d + 0] = p1 * -Xb[2] + p2 * Xb[1];            // SE3deriv columns: (0,-z,y) (z,0,-x) (-y,x,0) | I
        Jp[6 * d + 1] = p0 * Xb[2] + p2 * -Xb[0];
        Jp[6 * d + 2] = p0 * -Xb[1] + p1 * Xb[0];
        Jp[6 * d + 3] = p0; Jp[6 * d + 4] = p1; Jp[6 * d + 5] = p2;
    }
}

// EdgeInertial::computeError (+ linearizeOplus into J [9][24] when J != nullptr), G2oTypes.cc:720-800.  The body is inlined where a
// kernel must stay free of calls (a call's frame is scratch); iba_kernels.hip wraps it in the out-of-line form the BA kernels call.
__device__ __forceinline__ void inertial_edge_body(const double *s1, const double *s2, const double *pi, double *err, double *J)
{
#pragma clang fp contract(fast)
    const double dt = pi[P_DT];
    const double g[3] = {0, 0, -IMU_GRAVITY};
    double dbg[3], dba[3], w[3], E[9], dR[9], dV[3], dP[3], t[3];
    for (int i = 0; i < 3; i++) { dbg[i] = s1[K_BG + i] - pi[P_BG + i]; dba[i] = s1[K_BA + i] - pi[P_BA + i]; }
    mv3(pi + P_JRG, dbg, w);
    so3_exp(w, E, 1e-4, false);
    mm3(pi + P_DR, E, dR);
    so3_normalize(dR);
    mv3(pi + P_JVG, dbg, dV); mv3(pi + P_JVA, dba, t);
    for (int i = 0; i < 3; i++) dV[i] = pi[P_DV + i] + dV[i] + t[i];
    mv3(pi + P_JPG, dbg, dP); mv3(pi + P_JPA, dba, t);
    for (int i = 0; i < 3; i++) dP[i] = pi[P_DP + i] + dP[i] + t[i];
    double R12[9], eR[9], er[3], a[3], b[3], va[3], vb[3];
    mtm3(s1 + K_R, s2 + K_R, R12);
    mtm3(dR, R12, eR);
    so3_log(eR, er);
    for (int i = 0; i < 3; i++) {
        a[i] = s2[K_V + i] - s1[K_V + i] - g[i] * dt;
        b[i] = s2[K_T + i] - s1[K_T + i] - s1[K_V + i] * dt - g[i] * dt * dt / 2;
    }
    mtv3(s1 + K_R, a, va); mtv3(s1 + K_R, b, vb);
    for (int i = 0; i < 3; i++) { err[i] = er[i]; err[3 + i] = va[i] - dV[i]; err[6 + i] = vb[i] - dP[i]; }
    if (!J) return;
    for (int i = 0; i < 216; i++) J[i] = 0.0;
    double invJr[9], T[9], S[9];
    so3_inv_right_jac(er, invJr);
#define SETB(r0, c0, M, sgn) for (int i_ = 0; i_ < 3; i_++) for (int j_ = 0; j_ < 3; j_++) J[24 * ((r0) + i_) + (c0) + j_] = (sgn) * (M)[3 * i_ + j_]
    mtm3(s2 + K_R, s1 + K_R, T); mm3(invJr, T, T); SETB(0, 0, T, -1.0);
    so3_skew(va, S); SETB(3, 0, S, 1.0);
    so3_skew(vb, S); SETB(6, 0, S, 1.0);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    SETB(6, 3, I3, -1.0);
    double Rbw1[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rbw1[3 * i + j] = s1[K_R + 3 * j + i];
    SETB(3, 6, Rbw1, -1.0);
    SETB(6, 6, Rbw1, -dt);
    double RJ[9], eRt[9];
    so3_right_jac(w, RJ);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) eRt[3 * i + j] = eR[3 * j + i];
    mm3(invJr, eRt, T); mm3(T, RJ, T); mm3(T, pi + P_JRG, T); SETB(0, 9, T, -1.0);
    SETB(3, 9, pi + P_JVG, -1.0);
    SETB(6, 9, pi + P_JPG, -1.0);
    SETB(3, 12, pi + P_JVA, -1.0);
    SETB(6, 12, pi + P_JPA, -1.0);
    SETB(0, 15, invJr, 1.0);
    SETB(6, 18, R12, 1.0);
    SETB(3, 21, Rbw1, 1.0);
#undef SETB
}
}  // namespace
#undef IBA_EDGES_HELPER
