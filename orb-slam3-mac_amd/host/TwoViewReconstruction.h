// TwoViewReconstruction.h -- drop-in for the reference's include/TwoViewReconstruction.h: same constructor, same Reconstruct.  The RANSAC
// sets are drawn on the host exactly as the reference draws them (DUtils::Random::SeedRandOnce(0) once per process, then rand());
// everything else -- FindHomography, FindFundamental, ReconstructH / ReconstructF, CheckRT -- is ONE orbhip_two_view_reconstruct_host
// call on the calling thread's device context (host/hip_context.h).  Without a usable GPU Reconstruct prints a message on stderr and
// returns false: there is no CPU fallback.
#pragma once
#include <cstddef>
#include <vector>
#ifdef ORBHIP_WITH_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvlite.h"
#endif

namespace ORB_SLAM3 {

class TwoViewReconstruction {
public:
    // Fix the reference frame
    TwoViewReconstruction(cv::Mat &K, float sigma = 1.0, int iterations = 200);

    // Computes in parallel a fundamental matrix and a homography
    // Selects a model and tries to recover the motion and the structure from motion
    bool Reconstruct(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2, const std::vector<int> &vMatches12,
                     cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

    // mvSets of the latest call (tests read them; the reference keeps them private)
    const std::vector<std::vector<size_t>> &GetSets() const { return mvSets; }

private:
    cv::Mat mK;                                        // Calibration
    float mSigma, mSigma2;                             // Standard Deviation and Variance
    int mMaxIterations;                                // Ransac max iterations
    std::vector<std::vector<size_t>> mvSets;           // Ransac sets
};

}  // namespace ORB_SLAM3
