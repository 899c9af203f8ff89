// GeometricCamera::project and unproject in float, op by op in the reference's order, for files compiled with -ffp-contract=off: Pinhole and
// KannalaBrandt8 with the fixed double sequences that stand for atan2f / cosf / sinf (tri_kernels.hip's header comment).
// GeometricCamera::unproject likewise.  Shared by SearchForTriangulation / ComputeStereoFishEyeMatches (tri_kernels.hip), Sim3Solver
// (sim3solver_kernels.hip) and CreateNewMapPoints (newpoints_kernels.hip).
#ifndef ORBHIP_CAM_PROJECT_F32_H
#define ORBHIP_CAM_PROJECT_F32_H
#include <hip/hip_runtime.h>

static __device__ void tri_sincos_signed(double x, double &s_out, double &c_out)
{
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double dk = rint(x * TWO_OVER_PI);
    const int k = (int)dk;
    double r = fma(-dk, PIO2_HI, x);
    r = fma(-dk, PIO2_LO, r);
    const double z = r * r;
    double ps = fma(z, S6, S5); ps = fma(z, ps, S4); ps = fma(z, ps, S3); ps = fma(z, ps, S2); ps = fma(z, ps, S1);
    const double s = fma(r * z, ps, r);
    double pc = fma(z, C6, C5); pc = fma(z, pc, C4); pc = fma(z, pc, C3); pc = fma(z, pc, C2); pc = fma(z, pc, C1);
    const double c = fma(z * z, pc, fma(z, -0.5, 1.0));
    switch (k & 3) {
    case 0: s_out = s; c_out = c; break;
    case 1: s_out = c; c_out = -s; break;
    case 2: s_out = -s; c_out = -c; break;
    default: s_out = -c; c_out = s; break;
    }
}
static __device__ __forceinline__ float tri_atan2f(float y, float x) { return (float)atan2((double)y, (double)x); }

// GeometricCamera::project(cv::Point3f): Pinhole.cpp:34-37, KannalaBrandt8.cpp:28-45
static __device__ void tri_project(int type, const float *p, const float *P, float *uv)
{
    if (type == 0) { uv[0] = p[0] * P[0] / P[2] + p[2]; uv[1] = p[1] * P[1] / P[2] + p[3]; return; }
    const float x2_plus_y2 = P[0] * P[0] + P[1] * P[1];
    const float theta = tri_atan2f(sqrtf(x2_plus_y2), P[2]);
    const float psi = tri_atan2f(P[1], P[0]);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
    double s, c;
    tri_sincos_signed((double)psi, s, c);
    uv[0] = p[0] * r * (float)c + p[2]; uv[1] = p[1] * r * (float)s + p[3];
}
// GeometricCamera::unproject: Pinhole.cpp:57-60, KannalaBrandt8.cpp:103-130
[[maybe_unused]] static __device__ void tri_unproject(int type, const float *p, float u, float v, float *ray)
{
    const float pwx = (u - p[2]) / p[0], pwy = (v - p[3]) / p[1];
    if (type == 0) { ray[0] = pwx; ray[1] = pwy; ray[2] = 1.f; return; }
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-M_PI / 2.f), theta_d), (float)(M_PI / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
#pragma unroll 1
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0_theta2 = p[4] * theta2, k1_theta4 = p[5] * theta4, k2_theta6 = p[6] * theta6, k3_theta8 = p[7] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < 1e-6f) break;
        }
        double s, c;
        tri_sincos_signed((double)theta, s, c);
        scale = (float)(s / c) / theta_d;
    }
    ray[0] = pwx * scale; ray[1] = pwy * scale; ray[2] = 1.f;
}
#endif
