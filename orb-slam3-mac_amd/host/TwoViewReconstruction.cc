// TwoViewReconstruction.cc -- reference src/TwoViewReconstruction.cc:30-127 on the device, and GeometricCamera::ReconstructWithTwoViews
// (src/CameraModels/Pinhole.cpp:105-113, KannalaBrandt8.cpp:202-226) of the stand-in camera of host/slam_types.h.
#include "TwoViewReconstruction.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "hip_context.h"
#include "slam_types.h"

namespace ORB_SLAM3 {

namespace {
// Thirdparty/DBoW2/DUtils/Random.cpp:38-50
bool g_already_seeded = false;
void SeedRandOnce(int seed)
{
    if (!g_already_seeded) { srand(seed); g_already_seeded = true; }
}
int RandomInt(int min, int max)
{
    int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}
}  // namespace

TwoViewReconstruction::TwoViewReconstruction(cv::Mat &K, float sigma, int iterations)
{
    mK = K.clone();
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
}

bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2,
                                        const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D,
                                        std::vector<bool> &vbTriangulated)
{
    // the outputs as a failed call of the reference leaves them (:506-507 R21 / t21 empty; vP3D / vbTriangulated sized vKeys1.size())
    R21 = cv::Mat();
    t21 = cv::Mat();
    vP3D.assign(vKeys1.size(), cv::Point3f());
    vbTriangulated.assign(vKeys1.size(), false);

    // N = mvMatches12.size() (:53-64)
    int N = 0;
    const size_t nm = vMatches12.size() < vKeys1.size() ? vMatches12.size() : vKeys1.size();
    for (size_t i = 0; i < nm; i++)
        if (vMatches12[i] >= 0 && (size_t)vMatches12[i] < vKeys2.size()) N++;

    // Generate sets of 8 points for each RANSAC iteration (:66-96).  Fewer than 8 matches: the reference draws from an empty range
    // (undefined; Tracking never gets there, src/Tracking.cc:1510) -- here no sets and the answer "false".
    mvSets = std::vector<std::vector<size_t>>(mMaxIterations, std::vector<size_t>(8, 0));
    SeedRandOnce(0);
    if (N >= 8) {
        std::vector<size_t> vAllIndices(N), vAvailableIndices;
        for (int i = 0; i < N; i++) vAllIndices[i] = i;
        for (int it = 0; it < mMaxIterations; it++) {
            vAvailableIndices = vAllIndices;
            for (size_t j = 0; j < 8; j++) {
                int randi = RandomInt(0, vAvailableIndices.size() - 1);
                int idx = vAvailableIndices[randi];
                mvSets[it][j] = idx;
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
    }
    if (vKeys1.empty() || mMaxIterations <= 0) return false;

    orbhip_ctx *ctx = hip::ThreadContext();
    if (!ctx) {
        fprintf(stderr, "TwoViewReconstruction::Reconstruct: no usable GPU (there is no CPU fallback), returning false\n");
        return false;
    }
    orbhip_tvr_params prm;
    orbhip_tvr_default_params(&prm);
    prm.sigma = mSigma; prm.iterations = mMaxIterations; prm.draw_sets = 0;
    std::vector<int32_t> sets((size_t)mMaxIterations * 8), m12(vKeys1.size(), -1);
    for (int it = 0; it < mMaxIterations; it++)
        for (int j = 0; j < 8; j++) sets[(size_t)it * 8 + j] = (int32_t)mvSets[it][j];
    for (size_t i = 0; i < nm; i++) m12[i] = vMatches12[i];
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbhip_keypoint), "cv::KeyPoint layout");
    std::vector<float> P3D(vKeys1.size() * 3);
    std::vector<uint8_t> tri(vKeys1.size());
    uint8_t ok = 0;
    float R[9], t[3];
    const int rc = orbhip_two_view_reconstruct_host(ctx, reinterpret_cast<const orbhip_keypoint *>(vKeys1.data()), (int)vKeys1.size(),
                                                    reinterpret_cast<const orbhip_keypoint *>(vKeys2.data()), (int)vKeys2.size(), m12.data(),
                                                    mK.at<float>(0, 0), mK.at<float>(1, 1), mK.at<float>(0, 2), mK.at<float>(1, 2), &prm, sets.data(),
                                                    &ok, R, t, P3D.data(), tri.data(), nullptr);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "TwoViewReconstruction::Reconstruct: orbhip_two_view_reconstruct_host failed: %d (%s)\n", rc, orbhip_last_error());
        return false;
    }
    if (!ok) return false;
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R21.at<float>(i, j) = R[3 * i + j];
        t21.at<float>(i, 0) = t[i];
    }
    for (size_t i = 0; i < vKeys1.size(); i++) {
        vP3D[i] = cv::Point3f(P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
    return true;
}

#ifndef ORBHIP_WITH_ORBSLAM3
// Pinhole::toK / KannalaBrandt8::toK (Pinhole.cpp:116-120, KannalaBrandt8.cpp:229-233)
cv::Mat GeometricCamera::toK()
{
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
    K.at<float>(0, 0) = mvParameters[0]; K.at<float>(1, 1) = mvParameters[1];
    K.at<float>(0, 2) = mvParameters[2]; K.at<float>(1, 2) = mvParameters[3];
    return K;
}

const std::vector<std::vector<size_t>> &GeometricCamera::LastSets() const
{
    static const std::vector<std::vector<size_t>> none;
    return tvr ? tvr->GetSets() : none;
}

namespace {
// cv::fisheye::undistortPoints(pts, pts, K, D, R = I, P = K): per point the Newton inversion of theta_d = theta (1 + k1 theta^2 + ... +
// k4 theta^8) in double (OpenCV modules/calib3d/src/fisheye.cpp), then back through K
void FisheyeUndistort(std::vector<cv::Point2f> &pts, const std::vector<float> &p)
{
    const double fx = p[0], fy = p[1], cx = p[2], cy = p[3], k0 = p[4], k1 = p[5], k2 = p[6], k3 = p[7];
    for (cv::Point2f &pt : pts) {
        const double wx = ((double)pt.x - cx) / fx, wy = ((double)pt.y - cy) / fy;
        double scale = 1.0;
        double theta_d = sqrt(wx * wx + wy * wy);
        theta_d = std::min(std::max(-M_PI / 2., theta_d), M_PI / 2.);
        if (theta_d > 1e-8) {
            double theta = theta_d;
            for (int j = 0; j < 10; j++) {
                const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
                const double k0_theta2 = k0 * theta2, k1_theta4 = k1 * theta4, k2_theta6 = k2 * theta6, k3_theta8 = k3 * theta8;
                const double theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                         (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
                theta = theta - theta_fix;
                if (fabs(theta_fix) < 1e-8) break;
            }
            scale = std::tan(theta) / theta_d;
        }
        pt = cv::Point2f((float)(fx * wx * scale + cx), (float)(fy * wy * scale + cy));
    }
}
}  // namespace

std::vector<cv::Point2f> GeometricCamera::UndistortToPinhole(const std::vector<cv::KeyPoint> &vKeys) const
{
    std::vector<cv::Point2f> vPts(vKeys.size());
    for (size_t i = 0; i < vKeys.size(); i++) vPts[i] = vKeys[i].pt;
    if (mnType != 0) FisheyeUndistort(vPts, mvParameters);
    return vPts;
}

bool GeometricCamera::ReconstructWithTwoViews(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2,
                                              const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D,
                                              std::vector<bool> &vbTriangulated)
{
    if (!tvr) {
        cv::Mat K = this->toK();
        tvr = std::make_shared<TwoViewReconstruction>(K);
    }
    if (mnType == 0) return tvr->Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated);      // Pinhole.cpp:105-113

    // Correct FishEye distortion (KannalaBrandt8.cpp:209-225)
    std::vector<cv::KeyPoint> vKeysUn1 = vKeys1, vKeysUn2 = vKeys2;
    std::vector<cv::Point2f> vPts1 = UndistortToPinhole(vKeys1), vPts2 = UndistortToPinhole(vKeys2);
    for (size_t i = 0; i < vKeys1.size(); i++) vKeysUn1[i].pt = vPts1[i];
    for (size_t i = 0; i < vKeys2.size(); i++) vKeysUn2[i].pt = vPts2[i];
    return tvr->Reconstruct(vKeysUn1, vKeysUn2, vMatches12, R21, t21, vP3D, vbTriangulated);
}
#endif

}  // namespace ORB_SLAM3
