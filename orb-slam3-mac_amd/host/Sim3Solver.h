// Sim3Solver.h -- the reference's Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) with its public surface, around the HIP solver.
// The constructor gathers on the host as the reference does (:35-124).  The FIRST iterate() / find() draws all mRansacMaxIts sets with
// DUtils::Random::RandomInt's formula on rand() (the reference seeds rand() nowhere for this class, so neither does this one), makes ONE
// orbhip_sim3_solver_host call on the calling thread's context (draw_sets = 0, per-iteration counts requested) and caches the counts, the
// winner and its inlier flags.  Every iterate(n, ...) then replays the reference's loop over the next n cached iterations and returns as
// the reference does: the 4x4 CV_32F mBestT12, or cv::Mat().
// The best-so-far hypothesis of a chunk (what the bConverge overload returns when the chunk improved the best without converging, and
// what GetEstimated* answer in between) is RECOMPUTED ON THE HOST from its set with the kernel's own Horn text (csrc/horn_sim3.h); the
// final winner's R / t / s are the device's.  mBestT12 is [ms12 * mR12 | mt12] by float products, the reference's relation between its
// members (:413-416).
// Deviations: 3 * mRansacMaxIts rand() draws are consumed at once (the reference: 3 per executed iteration); the
// decompositions are a Jacobi iteration in double, not cv::eigen / cv::Rodrigues on floats.
// Without a usable GPU: one message on stderr, bNoMore = true, an empty matrix, nInliers = 0.  There is no CPU fallback.
#ifndef ORBHIP_HOST_SIM3SOLVER_H
#define ORBHIP_HOST_SIM3SOLVER_H
#include <cstdint>
#include <vector>
#include "slam_types.h"

namespace ORB_SLAM3 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true,
               std::vector<KeyFrame *> vpKeyFrameMatchedMP = std::vector<KeyFrame *>());

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, bool &bConverge);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    const std::vector<int32_t> &LastSets() const { return mvSets; }            // the drawn sets [mRansacMaxIts][3] (test plumbing)

protected:
    bool Solve();                                 // the one device call; false without a usable GPU
    void SetBest(int iteration);                  // mBestT12 / mBestRotation / mBestTranslation / mBestScale of a cached iteration

    // KeyFrames and matches
    KeyFrame *mpKF1;
    KeyFrame *mpKF2;

    std::vector<float> mvX3Dc1;                   // [N][3]
    std::vector<float> mvX3Dc2;
    std::vector<MapPoint *> mvpMapPoints1;
    std::vector<MapPoint *> mvpMapPoints2;
    std::vector<MapPoint *> mvpMatches12;
    std::vector<size_t> mvnIndices1;
    std::vector<size_t> mvnMaxError1;
    std::vector<size_t> mvnMaxError2;

    int N;
    int mN1;

    // Current Ransac State
    int mnIterations;
    int mnBestInliers;
    int mnBestIteration;
    cv::Mat mBestT12;
    cv::Mat mBestRotation;
    cv::Mat mBestTranslation;
    float mBestScale;

    // Scale is fixed to 1 in the stereo/RGBD case
    bool mbFixScale;

    // Indices for random selection
    std::vector<size_t> mvAllIndices;

    // RANSAC probability, min inliers, max iterations
    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;

    // Calibration
    cv::Mat mK1;
    cv::Mat mK2;

    GeometricCamera *pCamera1, *pCamera2;

    // the device call's cached answers
    int mnSolved;                                 // 0 not yet, 1 done, -1 failed
    std::vector<int32_t> mvSets, mvCounts;
    std::vector<uint8_t> mvbDeviceInliers;
    int mnDeviceWinner;
    bool mbDeviceConverged;
    float mDeviceR12[9], mDeviceT12[3], mDeviceS12;
};

}  // namespace ORB_SLAM3
#endif
