// cam_project_host.h -- GeometricCamera::project(cv::Point3f) (Pinhole.cpp:34-37, KannalaBrandt8.cpp:28-45) in float, op by op in the
// reference's order, with the library's fixed double sequences in place of the platform's atan2f / cosf / sinf: the host twin of
// csrc/cam_project_f32.h, for host members whose results must equal the device's bit for bit (Frame::isInFrustum against
// orbhip_frustum_queries_device).  A pinhole projection is the same arithmetic as GeometricCamera::project; a KannalaBrandt8 one can
// differ from it in the last bits, exactly as the device's does.
#pragma once
#include <cmath>
#include "slam_types.h"

namespace ORB_SLAM3 {
namespace camhost {

inline void sincos_signed(double x, double &s_out, double &c_out)
{
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632679489655800e+00, PIO2_LO = 6.12323399573676603587e-17;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double dk = std::rint(x * TWO_OVER_PI);
    const int k = (int)dk;
    double r = std::fma(-dk, PIO2_HI, x);
    r = std::fma(-dk, PIO2_LO, r);
    const double z = r * r;
    double ps = std::fma(z, S6, S5); ps = std::fma(z, ps, S4); ps = std::fma(z, ps, S3); ps = std::fma(z, ps, S2); ps = std::fma(z, ps, S1);
    const double s = std::fma(r * z, ps, r);
    double pc = std::fma(z, C6, C5); pc = std::fma(z, pc, C4); pc = std::fma(z, pc, C3); pc = std::fma(z, pc, C2); pc = std::fma(z, pc, C1);
    const double c = std::fma(z * z, pc, std::fma(z, -0.5, 1.0));
    switch (k & 3) {
    case 0: s_out = s; c_out = c; break;
    case 1: s_out = c; c_out = -s; break;
    case 2: s_out = -s; c_out = -c; break;
    default: s_out = -c; c_out = s; break;
    }
}
inline float det_atan2f(float y, float x) { return (float)std::atan2((double)y, (double)x); }

inline cv::Point2f project(GeometricCamera *cam, const cv::Point3f &P)
{
    const float fx = cam->getParameter(0), fy = cam->getParameter(1), cx = cam->getParameter(2), cy = cam->getParameter(3);
    if (cam->GetType() == 0) return cv::Point2f(fx * P.x / P.z + cx, fy * P.y / P.z + cy);
    const float x2_plus_y2 = P.x * P.x + P.y * P.y;
    const float theta = det_atan2f(sqrtf(x2_plus_y2), P.z);
    const float psi = det_atan2f(P.y, P.x);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + cam->getParameter(4) * theta3 + cam->getParameter(5) * theta5 + cam->getParameter(6) * theta7 + cam->getParameter(7) * theta9;
    double s, c;
    sincos_signed((double)psi, s, c);
    return cv::Point2f(fx * r * (float)c + cx, fy * r * (float)s + cy);
}

}  // namespace camhost
}  // namespace ORB_SLAM3
