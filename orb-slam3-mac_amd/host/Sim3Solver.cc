// Sim3Solver.cc -- see Sim3Solver.h.  Line references are to the reference's src/Sim3Solver.cc.
#include "Sim3Solver.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include "cvmath.h"
#include "optimizer_common.h"
#include "../csrc/horn_sim3.h"

namespace ORB_SLAM3 {

using namespace std;

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const vector<MapPoint *> &vpMatched12, const bool bFixScale,
                       vector<KeyFrame *> vpKeyFrameMatchedMP) :
    mnIterations(0), mnBestInliers(0), mnBestIteration(-1), mBestScale(0.f), mbFixScale(bFixScale),
    pCamera1(pKF1->mpCamera), pCamera2(pKF2->mpCamera), mnSolved(0), mnDeviceWinner(-1), mbDeviceConverged(false), mDeviceS12(0.f)
{
    // (:40-45) as written: the flag is true when the vector is EMPTY, and only then is pKFm re-read from the vector just filled with pKF2
    bool bDifferentKFs = false;
    if (vpKeyFrameMatchedMP.empty()) {
        bDifferentKFs = true;
        vpKeyFrameMatchedMP = vector<KeyFrame *>(vpMatched12.size(), pKF2);
    }

    mpKF1 = pKF1;
    mpKF2 = pKF2;

    vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();

    mN1 = vpMatched12.size();

    mvpMapPoints1.reserve(mN1);
    mvpMapPoints2.reserve(mN1);
    mvpMatches12 = vpMatched12;
    mvnIndices1.reserve(mN1);
    mvX3Dc1.reserve((size_t)3 * mN1);
    mvX3Dc2.reserve((size_t)3 * mN1);

    const cvm::M3 Rcw1 = cvm::block3(pKF1->GetRotation()), Rcw2 = cvm::block3(pKF2->GetRotation());
    const cvm::V3 tcw1 = cvm::vec3(pKF1->GetTranslation()), tcw2 = cvm::vec3(pKF2->GetTranslation());

    mvAllIndices.reserve(mN1);

    size_t idx = 0;

    KeyFrame *pKFm = pKF2;  // Default variable
    for (int i1 = 0; i1 < mN1; i1++) {
        if (vpMatched12[i1]) {
            MapPoint *pMP1 = vpKeyFrameMP1[i1];
            MapPoint *pMP2 = vpMatched12[i1];

            if (!pMP1)
                continue;

            if (pMP1->isBad() || pMP2->isBad())
                continue;

            if (bDifferentKFs)
                pKFm = vpKeyFrameMatchedMP[i1];

            int indexKF1 = get<0>(pMP1->GetIndexInKeyFrame(pKF1));
            int indexKF2 = get<0>(pMP2->GetIndexInKeyFrame(pKFm));

            if (indexKF1 < 0 || indexKF2 < 0)
                continue;

            const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
            const cv::KeyPoint &kp2 = pKFm->mvKeysUn[indexKF2];

            const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
            const float sigmaSquare2 = pKFm->mvLevelSigma2[kp2.octave];

            mvnMaxError1.push_back(9.210 * sigmaSquare1);                      // std::vector<size_t>: truncated (Sim3Solver.h:78-79)
            mvnMaxError2.push_back(9.210 * sigmaSquare2);

            mvpMapPoints1.push_back(pMP1);
            mvpMapPoints2.push_back(pMP2);
            mvnIndices1.push_back(i1);

            const cvm::V3 X1 = cvm::mul_add(Rcw1, cvm::vec3(pMP1->GetWorldPos()), tcw1);      // Rcw1*X3D1w+tcw1
            const cvm::V3 X2 = cvm::mul_add(Rcw2, cvm::vec3(pMP2->GetWorldPos()), tcw2);
            for (int k = 0; k < 3; k++) { mvX3Dc1.push_back(X1(k)); mvX3Dc2.push_back(X2(k)); }

            mvAllIndices.push_back(idx);
            idx++;
        }
    }

    mK1 = pKF1->mK;
    mK2 = pKF2->mK;

    // FromCameraToImage (:120-121, mvP1im1 / mvP2im2) runs on the device

    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;

    N = mvpMapPoints1.size();  // number of correspondences

    // Adjust Parameters according to number of correspondences
    float epsilon = (float)mRansacMinInliers / N;

    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;

    if (mRansacMinInliers == N)
        nIterations = 1;
    else {
        // the reference converts the quotient to int unchecked; beyond the cap (or not a number) it saturates here, as on the device
        const double q = ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
        nIterations = q < (double)mRansacMaxIts ? (int)q : mRansacMaxIts;
    }

    mRansacMaxIts = max(1, min(nIterations, mRansacMaxIts));

    mnIterations = 0;
    mnSolved = 0;
}

bool Sim3Solver::Solve()
{
    if (mnSolved) return mnSolved > 0;
    mnSolved = -1;
    // :175-189 for every iteration at once: RandomInt(0, size - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * size)
    mvSets.assign((size_t)3 * mRansacMaxIts, -1);
    vector<size_t> vAvailableIndices;
    for (int it = 0; it < mRansacMaxIts && N >= 3; it++) {
        vAvailableIndices = mvAllIndices;
        for (short i = 0; i < 3; ++i) {
            const int d = (int)vAvailableIndices.size();
            int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
            mvSets[3 * it + i] = (int32_t)vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
    orbhip_ctx *ctx = optc::thread_ctx();      // no usable GPU: hip::ThreadContext has printed the one message
    if (!ctx) return false;
    if (mRansacMaxIts > 1024 || N > 8192) {
        fprintf(stderr, "Sim3Solver: %d correspondences / %d iterations exceed the HIP solver's capacity (8192 / 1024)\n", N, mRansacMaxIts);
        return false;
    }
    orbhip_sim3solver_params p;
    orbhip_sim3solver_default_params(&p);
    p.probability = mRansacProb; p.min_inliers = mRansacMinInliers; p.max_iterations = mRansacMaxIts; p.fix_scale = mbFixScale ? 1 : 0; p.draw_sets = 0;
    orbhip_sim3_camera cam1, cam2;
    optc::camera_fields(pCamera1, cam1.fx, cam1.fy, cam1.cx, cam1.cy, cam1.camera_model, cam1.kb);
    optc::camera_fields(pCamera2, cam2.fx, cam2.fy, cam2.cx, cam2.cy, cam2.camera_model, cam2.kb);
    vector<float> max1(N > 0 ? N : 1), max2(N > 0 ? N : 1);
    for (int i = 0; i < N; i++) { max1[i] = (float)mvnMaxError1[i]; max2[i] = (float)mvnMaxError2[i]; }   // err < size_t: the integer as float
    mvCounts.assign(mRansacMaxIts, 0);
    mvbDeviceInliers.assign(N > 0 ? N : 1, 0);
    uint8_t converged = 0;
    int32_t nin = 0, stats[3] = {0, -1, 0};
    const int rc = orbhip_sim3_solver_host(ctx, mvX3Dc1.data(), mvX3Dc2.data(), max1.data(), max2.data(), N, &cam1, &cam2, &p, mvSets.data(), &converged,
                                           mDeviceR12, mDeviceT12, &mDeviceS12, &nin, mvbDeviceInliers.data(), stats, mvCounts.data());
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "Sim3Solver: HIP solver failed (%d: %s)\n", rc, orbhip_last_error());
        return false;
    }
    if (stats[0] > 0 && stats[0] < mRansacMaxIts) mRansacMaxIts = stats[0];     // the device's budget rules (the same formula)
    mbDeviceConverged = converged != 0;
    mnDeviceWinner = stats[1];
    mnSolved = 1;
    return true;
}

void Sim3Solver::SetBest(int it)
{
    float R[9], t[3], s;
    if (it == mnDeviceWinner) {
        for (int k = 0; k < 9; k++) R[k] = mDeviceR12[k];
        for (int k = 0; k < 3; k++) t[k] = mDeviceT12[k];
        s = mDeviceS12;
    } else {                                       // a best-so-far that is not the final winner: recomputed from its set
        float P1[3][3], P2[3][3];
        for (int j = 0; j < 3; j++) {
            const int idx = mvSets[3 * it + j];                              // -1 (N < 3): coincident zeros, NaN as on the device
            for (int c = 0; c < 3; c++) { P1[j][c] = idx >= 0 ? mvX3Dc1[3 * idx + c] : 0.f; P2[j][c] = idx >= 0 ? mvX3Dc2[3 * idx + c] : 0.f; }
        }
        HornSim3f h;
        horn_sim3(P1, P2, mbFixScale, h);
        for (int k = 0; k < 9; k++) R[k] = h.R12[k];
        for (int k = 0; k < 3; k++) t[k] = h.t12[k];
        s = h.s12;
    }
    mBestRotation = cv::Mat(3, 3, CV_32F);
    mBestTranslation = cv::Mat(3, 1, CV_32F);
    mBestT12 = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            mBestRotation.at<float>(i, j) = R[3 * i + j];
            mBestT12.at<float>(i, j) = R[3 * i + j] * s;                        // sR = ms12i*mR12i (:413)
        }
        mBestTranslation.at<float>(i) = t[i];
        mBestT12.at<float>(i, 3) = t[i];
    }
    mBestScale = s;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    bool bConverge;
    cv::Mat T = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
    return bConverge ? T : cv::Mat();                                            // :218: this overload returns nothing short of convergence
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers, bool &bConverge)
{
    bNoMore = false;
    bConverge = false;
    vbInliers = vector<bool>(mN1, false);
    nInliers = 0;

    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (!Solve()) {
        bNoMore = true;
        return cv::Mat();
    }

    int nCurrentIterations = 0;
    int improved = -1;

    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
        const int it = mnIterations;
        nCurrentIterations++;
        mnIterations++;

        const int mnInliersi = mvCounts[it];

        if (mnInliersi >= mnBestInliers) {
            mnBestInliers = mnInliersi;
            mnBestIteration = improved = it;

            if (mnInliersi > mRansacMinInliers) {
                SetBest(it);
                nInliers = mnInliersi;
                // the converging iteration is the device's winner (the same scan); its flags are the winner's
                for (int i = 0; i < N; i++)
                    if (mvbDeviceInliers[i])
                        vbInliers[mvnIndices1[i]] = true;
                bConverge = true;
                return mBestT12;
            }
        }
    }

    if (mnIterations >= mRansacMaxIts)
        bNoMore = true;

    if (improved < 0) return cv::Mat();
    SetBest(improved);
    return mBestT12;
}

cv::Mat Sim3Solver::find(vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    return mBestRotation.clone();
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    return mBestTranslation.clone();
}

float Sim3Solver::GetEstimatedScale()
{
    return mBestScale;
}

}  // namespace ORB_SLAM3
