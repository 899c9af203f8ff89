// geom3.h -- double-precision quaternion / SO3 / 3x3 helpers shared by the optimisers: ba_edges.h (local BA, pose-only BA),
// iba_edges.h (inertial BA in iba_kernels.hip, inertial pose-only in pose_inertial_kernels.hip), so3_f64.h and sim3_kernels.hip.
// Quaternions are (x, y, z, w), matrices row-major, an SE3 is (q, t) in 7 doubles.  Every function is force-inlined device code.
//
// Floating-point contraction: the library builds with -ffp-contract=off (the bit-exact ORB paths) and the optimisers switch it on with
// a file-scope pragma AFTER their includes, so a header sees whatever its includer had set at that line.  These functions have always
// been compiled contracted (a * b + c as one v_fma_f64); each body therefore opens with its own `#pragma clang fp contract(fast)`, as
// ba_ldlt.h does, and compiles the same wherever the #include stands.  No file-scope pragma here: it would leak into the includer.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void quat_to_R(const double *q, double *R)
{
#pragma clang fp contract(fast)
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Eigen's quaternion * vector (no normalisation)
__device__ __forceinline__ void quat_rot(const double *q, const double *v, double *o)
{
#pragma clang fp contract(fast)
    double u0 = q[1] * v[2] - q[2] * v[1], u1 = q[2] * v[0] - q[0] * v[2], u2 = q[0] * v[1] - q[1] * v[0];
    u0 += u0; u1 += u1; u2 += u2;
    o[0] = v[0] + q[3] * u0 + (q[1] * u2 - q[2] * u1);
    o[1] = v[1] + q[3] * u1 + (q[2] * u0 - q[0] * u2);
    o[2] = v[2] + q[3] * u2 + (q[0] * u1 - q[1] * u0);
}
// SE3Quat::normalizeRotation: w >= 0, unit length
__device__ __forceinline__ void quat_norm_rot(double *q)
{
#pragma clang fp contract(fast)
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
// Hamilton product o = a * b; o must not alias a or b
__device__ __forceinline__ void quat_mul(const double *a, const double *b, double *o)
{
#pragma clang fp contract(fast)
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void R_to_quat(const double *R, double *q)
{
#pragma clang fp contract(fast)
    // Eigen::Quaterniond(Matrix3d): trace branch, else the largest diagonal element picks (i,j,k); written out
    // per case so that every index is a compile-time constant
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
        if (i == 0) {          // j = 1, k = 2
            t = sqrt(R[0] - R[4] - R[8] + 1.0);
            q[0] = 0.5 * t; t = 0.5 / t;
            q[3] = (R[7] - R[5]) * t; q[1] = (R[3] + R[1]) * t; q[2] = (R[6] + R[2]) * t;
        } else if (i == 1) {   // j = 2, k = 0
            t = sqrt(R[4] - R[8] - R[0] + 1.0);
            q[1] = 0.5 * t; t = 0.5 / t;
            q[3] = (R[2] - R[6]) * t; q[2] = (R[7] + R[5]) * t; q[0] = (R[1] + R[3]) * t;
        } else {               // j = 0, k = 1
            t = sqrt(R[8] - R[0] - R[4] + 1.0);
            q[2] = 0.5 * t; t = 0.5 / t;
            q[3] = (R[3] - R[1]) * t; q[0] = (R[2] + R[6]) * t; q[1] = (R[5] + R[7]) * t;
        }
    }
}
// O = [w]x and O2 = O O: what the exponential maps of SE3Quat and g2o::Sim3 are built from
__device__ __forceinline__ void skew_and_square(const double *w, double *O, double *O2)
{
#pragma clang fp contract(fast)
    O[0] = 0; O[1] = -w[2]; O[2] = w[1]; O[3] = w[2]; O[4] = 0; O[5] = -w[0]; O[6] = -w[1]; O[7] = w[0]; O[8] = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += O[3 * i + k] * O[3 * k + j];
            O2[3 * i + j] = s;
        }
    }
}

// g2o's RobustKernelHuber (robust_kernel_impl.cpp:65-91) at squared error e: rho(e) and rho'(e); dsqr = delta^2 as the caller rounds it
__device__ __forceinline__ void huber(double e, double delta, double dsqr, double *rho0, double *rho1)
{
#pragma clang fp contract(fast)
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
    else { const double s = sqrt(e); *rho0 = 2 * s * delta - dsqr; *rho1 = delta / s; }
}

// ------------------------------------------------------------------ row-major 3x3 products (C / o may alias an input)
__device__ __forceinline__ void mm3(const double *A, const double *B, double *C)
{
#pragma clang fp contract(fast)
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) t[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = t[i];
}
__device__ __forceinline__ void mtm3(const double *A, const double *B, double *C)     // A^T B
{
#pragma clang fp contract(fast)
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) t[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = t[i];
}
__device__ __forceinline__ void mv3(const double *A, const double *v, double *o)
{
#pragma clang fp contract(fast)
    const double a = A[0] * v[0] + A[1] * v[1] + A[2] * v[2], b = A[3] * v[0] + A[4] * v[1] + A[5] * v[2], c = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
    o[0] = a; o[1] = b; o[2] = c;
}
__device__ __forceinline__ void mtv3(const double *A, const double *v, double *o)     // A^T v
{
#pragma clang fp contract(fast)
    const double a = A[0] * v[0] + A[3] * v[1] + A[6] * v[2], b = A[1] * v[0] + A[4] * v[1] + A[7] * v[2], c = A[2] * v[0] + A[5] * v[1] + A[8] * v[2];
    o[0] = a; o[1] = b; o[2] = c;
}
