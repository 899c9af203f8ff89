// MLPnPsolver.h -- the reference's MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp) with its public surface, around the HIP solver.
// The constructor gathers on the host as the reference does (:54-96); the bearings (unproject(pt) / z) are computed on the device.
// The FIRST iterate() draws the sets of all max(mRansacMaxIts, nIterations) iterations it can run with DUtils::Random::RandomInt's formula on
// rand() (the reference seeds rand() nowhere for this class, so neither does this one) and makes ONE orbhip_mlpnp_solver_host call on the
// calling thread's context (draw_sets = 0, first_call_iterations = the number of sets): hypotheses, counts, the scan and the answer come
// from the device.  Refine() is followed AS WRITTEN (:288-342): its computePose fills a local `result` that never reaches mRi / mti, so
// it accepts the current iteration's own hypothesis when that holds more than mRansacMinInliers; iterate() returns that hypothesis.
// It returns as the reference does: the 4x4 CV_32F pose with vbInliers filled through mvKeyPointIndices, or cv::Mat(); bNoMore once the
// budget is spent.
// A LATER iterate() (after such a return, which the caller did not accept) draws the sets of the further iterations and calls again over ALL
// sets with resume_at = the iteration after the last return: the earlier iterations are recomputed to rebuild the best-so-far, they cannot
// return again.  The path is rare (Tracking::Relocalization discards a candidate whose returned pose fails only after bNoMore), so the
// recomputation is accepted.
// Deviations: 6 * max(mRansacMaxIts, nIterations) rand() draws are consumed at once (the reference: 6 per executed
// iteration); Eigen's decompositions are replaced (csrc/mlpnp_core.h), agreement is a tolerance; the N-point solve
// that Refine() computes and discards is not run.
// Without a usable GPU: one message on stderr, bNoMore = true, an empty matrix, nInliers = 0.  There is no CPU fallback.
#ifndef ORBHIP_HOST_MLPNPSOLVER_H
#define ORBHIP_HOST_MLPNPSOLVER_H
#include <cstdint>
#include <vector>
#include "slam_types.h"

namespace ORB_SLAM3 {

class MLPnPsolver {
public:
    MLPnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches);

    ~MLPnPsolver();

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4,
                             float th2 = 5.991);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    // test plumbing, not part of the reference's interface
    const std::vector<int32_t> &LastSets() const { return mvSets; }            // the drawn sets [iterations][6]
    const int32_t *LastStats() const { return mStats; }                        // budget, returning iteration, its count, Refine() calls

private:
    std::vector<MapPoint *> mvpMapPointMatches;

    // 2D points, their sigma2, 3D points (float, [N][2] / [N] / [N][3])
    std::vector<float> mvP2D, mvSigma2, mvP3Dw;

    // Index in Frame
    std::vector<size_t> mvKeyPointIndices;

    // Current Ransac State
    int mnIterations;

    // Number of Correspondences
    int N;

    // Indices for random selection [0 .. N-1]
    std::vector<size_t> mvAllIndices;

    // RANSAC probability, min inliers, max iterations, expected inlier/total ratio, min set, the chi2 threshold
    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;
    float mRansacEpsilon;
    float mRansacTh;
    int mRansacMinSet;

    // what SetRansacParameters was given (the library applies the rules of :229-248 itself)
    int mGivenMinInliers, mGivenMaxIts;
    float mGivenEpsilon;

    GeometricCamera *mpCamera;

    std::vector<int32_t> mvSets;                  // [drawn iterations][6]
    int32_t mStats[4];
};

}  // namespace ORB_SLAM3
#endif
