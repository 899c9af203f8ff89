// so3_f64.h -- the double-precision SO(3) helpers of the inertial optimisers and the 4-DoF pose graph, the one copy in csrc/: the
// exponential with and without re-orthonormalisation, the logarithm, the right Jacobian and its inverse, as src/G2oTypes.cc:991-1063
// and src/ImuTypes.cc:30-60 state them.  Matrices are row-major.  Includers: inertial_opt_kernels.hip, pose_graph4dof_kernels.hip and
// iba_edges.h (for iba_kernels.hip and pose_inertial_kernels.hip; the BA kernels compile to the same instructions with these as with
// the private copies iba_kernels.hip used to keep, profiles/iba_split_streams.txt).
// Every function is force-inlined (a call's frame would be scratch) and opens with its own contraction pragma, as geom3.h does.
#pragma once
#include <hip/hip_runtime.h>
#include "geom3.h"

__device__ __forceinline__ void so3_skew(const double *w, double *W)
{
    W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
__device__ __forceinline__ void so3_inv3(const double *A, double *I)
{
#pragma clang fp contract(fast)
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c0 + A[1] * c1 + A[2] * c2);
    I[0] = c0 * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = c1 * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = c2 * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
// nearest rotation (IMU::NormalizeRotation, ImuTypes.cc:30-36, takes U V^T of an SVD): two Newton steps of the polar decomposition,
// R <- (R + R^-T) / 2; the argument is a product of rotations, a rounding error away from one, where the iteration converges quadratically
__device__ __forceinline__ void so3_normalize(double *R)
{
#pragma clang fp contract(fast)
#pragma unroll
    for (int it = 0; it < 2; it++) {
        double I[9];
        so3_inv3(R, I);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = 0.5 * (R[3 * i + j] + I[3 * j + i]);
    }
}
__device__ __forceinline__ void so3_rodrigues(const double *w, double a, double b, double *R)     // I + a W + b W W
{
#pragma clang fp contract(fast)
    double W[9], W2[9];
    so3_skew(w, W); mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = a * W[i] + b * W2[i];
    R[0] += 1; R[4] += 1; R[8] += 1;
}
// G2oTypes.cc:991-1008 (eps 1e-5, normalised) / ImuTypes.cc:48-60 (eps 1e-4, not normalised)
__device__ __forceinline__ void so3_exp(const double *w, double *R, double eps, bool normalize)
{
#pragma clang fp contract(fast)
    const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = sqrt(d2);
    if (d < eps) so3_rodrigues(w, 1.0, 0.5, R);
    else so3_rodrigues(w, sin(d) / d, (1.0 - cos(d)) / d2, R);
    if (normalize) so3_normalize(R);
}
__device__ __forceinline__ void so3_log(const double *R, double *w)     // G2oTypes.cc:1009-1023
{
#pragma clang fp contract(fast)
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta), s = sin(theta);
    if (fabs(s) < 1e-5) return;
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}
__device__ __forceinline__ void so3_inv_right_jac(const double *v, double *J)     // G2oTypes.cc:1030-1041
{
#pragma clang fp contract(fast)
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    if (d < 1e-5) {
#pragma unroll
        for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    so3_rodrigues(v, 0.5, 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d)), J);
}
__device__ __forceinline__ void so3_right_jac(const double *v, double *J)         // G2oTypes.cc:1048-1063
{
#pragma clang fp contract(fast)
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    if (d < 1e-5) {
#pragma unroll
        for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    so3_rodrigues(v, -(1.0 - cos(d)) / d2, (d - sin(d)) / (d2 * d), J);
}
