// MLPnPsolver.cc -- see MLPnPsolver.h.  Line references are to the reference's src/MLPnPsolver.cpp.
#include "MLPnPsolver.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "optimizer_common.h"

namespace ORB_SLAM3 {

using namespace std;

MLPnPsolver::MLPnPsolver(const Frame &F, const vector<MapPoint *> &vpMapPointMatches) :
    mnIterations(0), N(0), mpCamera(F.mpCamera)
{
    mvpMapPointMatches = vpMapPointMatches;
    mvP2D.reserve(2 * F.mvpMapPoints.size());
    mvSigma2.reserve(F.mvpMapPoints.size());
    mvP3Dw.reserve(3 * F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());
    mvAllIndices.reserve(F.mvpMapPoints.size());
    mStats[0] = 0; mStats[1] = -1; mStats[2] = 0; mStats[3] = 0;

    int idx = 0;
    for (size_t i = 0, iend = mvpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];

        if (pMP) {
            if (!pMP->isBad()) {
                if (i >= F.mvKeysUn.size()) continue;
                const cv::KeyPoint &kp = F.mvKeysUn[i];

                mvP2D.push_back(kp.pt.x);
                mvP2D.push_back(kp.pt.y);
                mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);

                // the bearing (:77-80) is computed on the device

                // 3D coordinates
                cv::Mat cv_pos = pMP->GetWorldPos();
                for (int k = 0; k < 3; k++) mvP3Dw.push_back(cv_pos.at<float>(k));

                mvKeyPointIndices.push_back(i);
                mvAllIndices.push_back(idx);

                idx++;
            }
        }
    }

    SetRansacParameters();
}

MLPnPsolver::~MLPnPsolver() {}

void MLPnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;
    mRansacTh = th2;
    mGivenMinInliers = minInliers; mGivenMaxIts = maxIterations; mGivenEpsilon = epsilon;

    N = mvSigma2.size();  // number of correspondences

    // Adjust Parameters according to number of correspondences
    int nMinInliers = N * mRansacEpsilon;
    if (nMinInliers < mRansacMinInliers)
        nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet)
        nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;

    if (mRansacEpsilon < (float)mRansacMinInliers / N)
        mRansacEpsilon = (float)mRansacMinInliers / N;

    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;

    if (mRansacMinInliers == N)
        nIterations = 1;
    else {
        // the reference converts the quotient to int unchecked; beyond the cap (or not a number) it saturates here, as on the device
        const double q = ceil(log(1 - mRansacProb) / log(1 - pow(mRansacEpsilon, 3)));
        nIterations = q < (double)mRansacMaxIts ? (int)q : mRansacMaxIts;
    }

    mRansacMaxIts = max(1, min(nIterations, mRansacMaxIts));

    // mvMaxError (:250-252) = sigma2 * th2 is formed on the device
    mnIterations = 0;
    mvSets.clear();
}

cv::Mat MLPnPsolver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;

    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }

    // the loop's condition (:113): this call may run iterations up to `last`
    const int first = mnIterations;
    const int last = max(mRansacMaxIts, first + max(nIterations, 0));
    // :118-138 for every further iteration at once: RandomInt(0, size - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * size)
    vector<size_t> vAvailableIndices;
    for (int it = (int)(mvSets.size() / 6); it < last; it++) {
        vAvailableIndices = mvAllIndices;
        for (short i = 0; i < mRansacMinSet && i < 6; ++i) {
            const int d = (int)vAvailableIndices.size();
            int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
            mvSets.push_back((int32_t)vAvailableIndices[randi]);
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
    const int K = (int)(mvSets.size() / 6);

    orbhip_ctx *ctx = optc::thread_ctx();      // no usable GPU: hip::ThreadContext has printed the one message
    if (!ctx) {
        bNoMore = true;
        return cv::Mat();
    }
    if (K > 1024 || N > 8192 || mRansacMinSet != 6) {
        fprintf(stderr, "MLPnPsolver: %d correspondences / %d iterations / a minimal set of %d are beyond the HIP solver (8192 / 1024 / 6)\n", N, K, mRansacMinSet);
        bNoMore = true;
        return cv::Mat();
    }
    orbhip_mlpnp_params p;
    orbhip_mlpnp_default_params(&p);
    p.probability = mRansacProb; p.min_inliers = mGivenMinInliers; p.max_iterations = K; p.min_set = 6; p.epsilon = mGivenEpsilon; p.th2 = mRansacTh;
    p.first_call_iterations = K; p.resume_at = first; p.draw_sets = 0;
    orbhip_sim3_camera cam;
    optc::camera_fields(mpCamera, cam.fx, cam.fy, cam.cx, cam.cy, cam.camera_model, cam.kb);
    vector<uint8_t> inl(N > 0 ? N : 1, 0);
    uint8_t outcome = 0;
    float T[12] = {0};
    int32_t nin = 0;
    const int rc = orbhip_mlpnp_solver_host(ctx, mvP3Dw.data(), mvP2D.data(), mvSigma2.data(), N, &cam, &p, mvSets.data(), &outcome, T, &nin,
                                            inl.data(), mStats, nullptr);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "MLPnPsolver: HIP solver failed (%d: %s)\n", rc, orbhip_last_error());
        bNoMore = true;
        return cv::Mat();
    }

    if (outcome == 1)
        mnIterations = mStats[1] + 1;                                            // Refine() accepted: returned at once (:184-194)
    else {
        mnIterations = K;                                                        // :199-213
        bNoMore = true;
        if (outcome == 0) return cv::Mat();
    }
    nInliers = nin;
    vbInliers = vector<bool>(mvpMapPointMatches.size(), false);
    for (int i = 0; i < N; i++) {
        if (inl[i])
            vbInliers[mvKeyPointIndices[i]] = true;
    }
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Tcw.at<float>(i, j) = T[3 * i + j];
        Tcw.at<float>(i, 3) = T[9 + i];
    }
    return Tcw;
}

}  // namespace ORB_SLAM3
