// Optimizer_OptimizeSim3.cc -- int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) with
// the reference's signature (include/Optimizer.h:90, src/Optimizer.cc:3932-4328) around the HIP solver.  LoopClosing calls it between its
// matchers (src/LoopClosing.cc:532, :742).  Host side, in the reference's order: the edge loop of :4007-4233 -- the map-point tests
// (:4025-4074: both points present and not bad), the `i2 < 0 && !bAllPoints` skip (:4076-4080), P3D1c / P3D2c as the float cv::Mat
// products R * Xw + t, the observation of a point without keypoint in KF2 as the NORMALISED (x/z, y/z) of P3D2c at octave 0 (:4161-4181:
// `cv::KeyPoint(cv::Point2f(x, y), pMP2->mnTrackScaleLevel)` passes the level as the keypoint's SIZE, so the octave keeps its default 0
// and :4220 reads mvInvLevelSigma2[0]; kept as written) -- fills flat arrays.  What was g2o (optimize(5) with Huber, the classification on
// the stored chi2, the `< 10` return, optimize(5 or 10) without kernels, the final classification, :4237-4318) runs in ONE device call
// (k_sim3_opt), which also applies the `P3D2c.z < 0` skip of :4082-4086.  Then the NULLs (:4254, :4311), mAcumHessian = 0 (:4297),
// g2oS12 (:4323) and the return value nIn.  The debug drawing (cv::imread / cvtColor / circle / line behind bShowImages = false,
// :4000-4003, :4070, :4116-4130, :4156-4159, :4183-4186, :4199-4213, :4272-4278) is dropped.
#include "Optimizer.h"
#include <cstdio>
#include <tuple>
#include <vector>
#include "cvmath.h"
#include "optimizer_common.h"
#include "host_prof.h"

namespace ORB_SLAM3 {

using namespace optc;

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale, Eigen::Matrix<double, 7, 7> &mAcumHessian, const bool bAllPoints)
{
    hip::HostProf prof("OptimizeSim3");
    // no usable GPU: one message (hip::ThreadContext prints it), nothing touched, no CPU fallback
    orbhip_ctx *ctx = thread_ctx();
    if (!ctx) return 0;

    // Camera poses
    const cvm::M3 R1w = cvm::block3(pKF1->GetRotation()), R2w = cvm::block3(pKF2->GetRotation());
    const cvm::V3 t1w = cvm::vec3(pKF1->GetTranslation()), t2w = cvm::vec3(pKF2->GetTranslation());

    const int N = vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<size_t> vnIndexEdge;
    std::vector<double> P1c, P2c, obs1, obs2, invS1, invS2;
    vnIndexEdge.reserve(N); P1c.reserve((size_t)3 * N); P2c.reserve((size_t)3 * N); obs1.reserve((size_t)2 * N); obs2.reserve((size_t)2 * N);
    invS1.reserve(N); invS2.reserve(N);

    for (int i = 0; i < N; i++) {                              // :4007-4233
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
        if (!(pMP1 && pMP2)) continue;                         // :4052-4074: a match without map point in KF1 gets no edge
        if (pMP1->isBad() || pMP2->isBad()) continue;          // :4046-4050
        const cvm::V3 P3D1c = cvm::mul_add(R1w, cvm::vec3(pMP1->GetWorldPos()), t1w);      // R1w*P3D1w + t1w
        const cvm::V3 P3D2c = cvm::mul_add(R2w, cvm::vec3(pMP2->GetWorldPos()), t2w);
        if (i2 < 0 && !bAllPoints) continue;                   // :4076-4080
        // (:4082-4086, `P3D2c.z < 0: continue`, is applied by the device: the row comes back with flag 3)

        // Set edge x1 = S12*X2
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        obs1.push_back(kpUn1.pt.x); obs1.push_back(kpUn1.pt.y);
        invS1.push_back((double)pKF1->mvInvLevelSigma2[kpUn1.octave]);

        // Set edge x2 = S21*X1
        cv::KeyPoint kpUn2;
        if (i2 >= 0) {
            kpUn2 = pKF2->mvKeysUn[i2];
            obs2.push_back(kpUn2.pt.x); obs2.push_back(kpUn2.pt.y);
        } else {                                               // :4161-4181
            const float invz = 1 / P3D2c(2);
            const float x = P3D2c(0) * invz;
            const float y = P3D2c(1) * invz;
            obs2.push_back(x); obs2.push_back(y);
            // cv::KeyPoint(cv::Point2f(x, y), pMP2->mnTrackScaleLevel): the second argument is the keypoint's size, the octave stays 0
            // (mnTrackScaleLevel may be -1 or unset in the reference; it must never index mvInvLevelSigma2)
            kpUn2 = cv::KeyPoint();
            kpUn2.size = (float)pMP2->mnTrackScaleLevel;
            kpUn2.octave = 0;
        }
        invS2.push_back((double)pKF2->mvInvLevelSigma2[kpUn2.octave]);
        for (int k = 0; k < 3; k++) { P1c.push_back((double)P3D1c(k)); P2c.push_back((double)P3D2c(k)); }
        vnIndexEdge.push_back(i);
    }

    const int n = (int)vnIndexEdge.size();
    orbhip_sim3_camera cam1, cam2;
    camera_fields(pKF1->mpCamera, cam1.fx, cam1.fy, cam1.cx, cam1.cy, cam1.camera_model, cam1.kb);
    camera_fields(pKF2->mpCamera, cam2.fx, cam2.fy, cam2.cx, cam2.cy, cam2.camera_model, cam2.kb);
    double S[8] = {g2oS12.rotation().x(), g2oS12.rotation().y(), g2oS12.rotation().z(), g2oS12.rotation().w(),
                   g2oS12.translation()[0], g2oS12.translation()[1], g2oS12.translation()[2], g2oS12.scale()};
    std::vector<uint8_t> flag(n > 0 ? n : 1, 0);
    int32_t nIn = 0, stats[4] = {0, 0, 0, 0};
    prof.mark();
    const int rc = orbhip_optimize_sim3_host(ctx, P1c.data(), P2c.data(), obs1.data(), obs2.data(), invS1.data(), invS2.data(), n, &cam1, &cam2,
                                             (double)th2, bFixScale ? 1 : 0, S, flag.data(), &nIn, stats);
    prof.mark();
    if (rc != ORBHIP_OK) {
        // the reference has no failure path: leave everything as it is and report no inliers (LoopClosing drops the candidate)
        fprintf(stderr, "OptimizeSim3: HIP solver failed (%d: %s)\n", rc, orbhip_last_error());
        return 0;
    }
    // Check inliers (:4244-4271, :4298-4318): a pair dropped after either pass loses its match
    for (int e = 0; e < n; e++)
        if (flag[e] == 1 || flag[e] == 2) vpMatches1[vnIndexEdge[e]] = static_cast<MapPoint *>(NULL);
    if (stats[0] - stats[1] < 10) return 0;                    // :4288-4289: nCorrespondences - nBad < 10; g2oS12 and mAcumHessian keep their values

    mAcumHessian.setZero();                                    // :4297 (never accumulated, :4316)
    // Recover optimized Sim3 (:4322-4323)
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), [&] { Eigen::Vector3d t; t[0] = S[4]; t[1] = S[5]; t[2] = S[6]; return t; }(), S[7]);
    return nIn;
}

}  // namespace ORB_SLAM3
