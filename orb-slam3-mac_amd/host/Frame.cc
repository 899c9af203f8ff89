// Frame.cc -- the Frame member functions of the hot path.  On the device: Frame::ComputeStereoMatches
// (reference src/Frame.cc:802-980, called by the rectified-stereo constructor at :130 right after the two ExtractORB threads, :109-112)
// and Frame::ComputeStereoFishEyeMatches (:1128-1168, called by the stereo-fisheye constructor at :1097 after its two threads, :1056-1059).
// Same signature, same members read and written; the association itself (row bands, descriptor distances, 11 x 11 SAD search on the
// left keypoint's pyramid level of BOTH images, parabola fit, median cut) is orbhip_compute_stereo_matches_* behind the C ABI, on the
// keypoints, descriptors and pyramids the two ORBextractor objects left on the device -- nothing is uploaded and the mvImagePyramid
// copy-back of the reference's host loop (:809, :899, :913, :918) is not needed on this path.
#include <cstdio>
#include "ORBextractor.h"
#include "slam_types.h"
#include "frame_cache.h"
#include "cvmath.h"
#include "cam_project_host.h"

namespace ORB_SLAM3 {

// Frame::UpdatePoseMatrices, isInFrustum and isInFrustumChecks (src/Frame.cc:456-462, :483-572, :1170-1243) are HOST members, written from
// cvmath.h: they answer for a single point (any caller that asks about one) and are the second implementation the device form
// (orbhip_frustum_queries_device, which Tracking::SearchLocalPoints uses for the whole local map) is tested against.  The projection goes
// through cam_project_host.h, the library's float restatement of GeometricCamera::project, not through mpCamera->project: the platform's
// atan2f / cosf / sinf would move a KannalaBrandt8 projection by up to a few hundred ulps from the device's (measured on a 1000-point rig
// scene: 181 points), and a point judged by this member and by the device call must get the same answer.
void Frame::UpdatePoseMatrices()
{
    const cvm::M3 Rcw = cvm::block3(mTcw);
    const cvm::V3 tcw = cvm::col3(mTcw);
    mRcw = cv::Mat(3, 3, CV_32F); mRwc = cv::Mat(3, 3, CV_32F);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { mRcw.at<float>(i, j) = Rcw(i, j); mRwc.at<float>(i, j) = Rcw(j, i); }
    mtcw = cvm::to_mat(tcw);
    mOw = cvm::to_mat(cvm::mul_t(Rcw, tcw, -1.0));                              // -mRcw.t()*mtcw
}

bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit)
{
    if (Nleft == -1) {
        pMP->mbTrackInView = false;
        pMP->mTrackProjX = -1;
        pMP->mTrackProjY = -1;

        const cvm::V3 P = cvm::vec3(pMP->GetWorldPos());

        // Pc = mRcw*P + mtcw (:497): the small-matrix product of cvmath.h; cv::norm in double
        const cvm::V3 Pc = cvm::mul_add(cvm::block3(mRcw), P, cvm::vec3(mtcw));
        const float Pc_dist = cvm::norm(Pc);

        // :501-504 (invz is taken before the sign test, as there)
        const float PcZ = Pc(2);
        const float invz = 1.0f / PcZ;
        if (PcZ < 0.0f)
            return false;

        const cv::Point2f uv = camhost::project(mpCamera, cv::Point3f(Pc(0), Pc(1), Pc(2)));

        if (uv.x < mnMinX || uv.x > mnMaxX)
            return false;
        if (uv.y < mnMinY || uv.y > mnMaxY)
            return false;

        pMP->mTrackProjX = uv.x;
        pMP->mTrackProjY = uv.y;

        // :519-526: the scale-invariance range, written as there (a NaN distance passes)
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        const cvm::V3 PO = cvm::sub(P, cvm::vec3(mOw));
        const float dist = cvm::norm(PO);

        if (dist < minDistance || dist > maxDistance)
            return false;

        // :530-538: Mat::dot in double, divided by the float distance
        const cvm::V3 Pn = cvm::vec3(pMP->GetNormal());

        const float viewCos = cvm::dot(PO, Pn) / dist;

        if (viewCos < viewingCosLimit)
            return false;

        const int nPredictedLevel = pMP->PredictScale(dist, this);

        // :545-559
        pMP->mbTrackInView = true;
        pMP->mTrackProjX = uv.x;
        pMP->mTrackProjXR = uv.x - mbf * invz;

        pMP->mTrackDepth = Pc_dist;

        pMP->mTrackProjY = uv.y;
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;

        return true;
    } else {
        pMP->mbTrackInView = false;
        pMP->mbTrackInViewR = false;
        pMP->mnTrackScaleLevel = -1;
        pMP->mnTrackScaleLevelR = -1;

        pMP->mbTrackInView = isInFrustumChecks(pMP, viewingCosLimit);
        pMP->mbTrackInViewR = isInFrustumChecks(pMP, viewingCosLimit, true);

        return pMP->mbTrackInView || pMP->mbTrackInViewR;
    }
}

bool Frame::isInFrustumChecks(MapPoint *pMP, float viewingCosLimit, bool bRight)
{
    const cvm::V3 P = cvm::vec3(pMP->GetWorldPos());

    cvm::M3 mR;
    cvm::V3 mt, twc;
    if (bRight) {
        const cvm::M3 Rrl = cvm::block3(mTrl);
        const cvm::V3 trl = cvm::col3(mTrl);
        mR = cvm::mul(Rrl, cvm::block3(mRcw));
        mt = cvm::mul_add(Rrl, cvm::vec3(mtcw), trl);
        twc = cvm::mul_add(cvm::block3(mRwc), cvm::col3(mTlr), cvm::vec3(mOw));
    } else {
        mR = cvm::block3(mRcw);
        mt = cvm::vec3(mtcw);
        twc = cvm::vec3(mOw);
    }

    // Pc = mR*P + mt (:1189)
    const cvm::V3 Pc = cvm::mul_add(mR, P, mt);
    const float Pc_dist = cvm::norm(Pc);
    const float PcZ = Pc(2);

    // :1193-1195
    if (PcZ < 0.0f)
        return false;

    // :1197-1205
    cv::Point2f uv;
    if (bRight) uv = camhost::project(mpCamera2, cv::Point3f(Pc(0), Pc(1), Pc(2)));
    else uv = camhost::project(mpCamera, cv::Point3f(Pc(0), Pc(1), Pc(2)));

    if (uv.x < mnMinX || uv.x > mnMaxX)
        return false;
    if (uv.y < mnMinY || uv.y > mnMaxY)
        return false;

    // :1207-1214
    const float maxDistance = pMP->GetMaxDistanceInvariance();
    const float minDistance = pMP->GetMinDistanceInvariance();
    const cvm::V3 PO = cvm::sub(P, twc);
    const float dist = cvm::norm(PO);

    if (dist < minDistance || dist > maxDistance)
        return false;

    // :1216-1222
    const cvm::V3 Pn = cvm::vec3(pMP->GetNormal());

    const float viewCos = cvm::dot(PO, Pn) / dist;

    if (viewCos < viewingCosLimit)
        return false;

    const int nPredictedLevel = pMP->PredictScale(dist, this);

    if (bRight) {
        pMP->mTrackProjXR = uv.x;
        pMP->mTrackProjYR = uv.y;
        pMP->mnTrackScaleLevelR = nPredictedLevel;
        pMP->mTrackViewCosR = viewCos;
        pMP->mTrackDepthR = Pc_dist;
    } else {
        pMP->mTrackProjX = uv.x;
        pMP->mTrackProjY = uv.y;
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        pMP->mTrackDepth = Pc_dist;
    }

    return true;
}

void Frame::ComputeStereoMatches()
{
    mvuRight = std::vector<float>(N, -1.0f);                                  // :804-805
    mvDepth = std::vector<float>(N, -1.0f);
    if (N == 0) return;
    if (!mpORBextractorLeft || !mpORBextractorRight) { fprintf(stderr, "Frame (HIP): ComputeStereoMatches: no extractors\n"); return; }
    orbhip_extractor *eL = mpORBextractorLeft->DeviceExtractor(), *eR = mpORBextractorRight->DeviceExtractor();
    // The kernels read the two extractors' LATEST extractions: this Frame's mvKeys / mDescriptors and mvKeysRight / mDescriptorsRight must be
    // those (they are when the constructor calls this; byte comparison with the extractors' page-locked mirrors, host/frame_cache.h).  The
    // shared locks keep the next operator() of either extractor out until the kernels have finished.
    hip::ResidentFrame rl = hip::FindResidentIn(eL, mvKeys.data(), mDescriptors.ptr<uint8_t>(), N);
    const bool right_empty = mvKeysRight.empty();                             // (a featureless right image: nothing can match)
    hip::ResidentFrame rr = right_empty ? hip::ResidentFrame() : hip::FindResidentIn(eR, mvKeysRight.data(), mDescriptorsRight.ptr<uint8_t>(), (int)mvKeysRight.size());
    if (!rl || !rl.d_kp || (!right_empty && (!rr || !rr.d_kp))) {
        fprintf(stderr, "Frame (HIP): ComputeStereoMatches: the frame's features are not the latest extractions of its two extractors (left %s, right %s)\n",
                rl && rl.d_kp ? "ok" : "no", right_empty || (rr && rr.d_kp) ? "ok" : "no");
        return;
    }
    if (right_empty) return;
    int32_t kept = 0;
    const int rc = orbhip_compute_stereo_matches_host(eL, eR, mb, mbf, mvuRight.data(), mvDepth.data(), N, &kept);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "Frame (HIP): ComputeStereoMatches: %d (%s)\n", rc, orbhip_last_error());
        mvuRight.assign(N, -1.0f); mvDepth.assign(N, -1.0f);
    }
}

void Frame::ComputeStereoFishEyeMatches()
{
    mvLeftToRightMatch = std::vector<int>(Nleft > 0 ? Nleft : 0, -1);           // :1137-1142
    mvRightToLeftMatch = std::vector<int>(Nright > 0 ? Nright : 0, -1);
    mvDepth = std::vector<float>(Nleft > 0 ? Nleft : 0, -1.0f);
    mvuRight = std::vector<float>(Nleft > 0 ? Nleft : 0, -1);
    mvStereo3Dpoints = std::vector<cv::Mat>(Nleft > 0 ? Nleft : 0);
    mnCloseMPs = 0;
    if (Nleft <= 0) return;
    const char *why = nullptr;
    if (!mpORBextractorLeft || !mpORBextractorRight) why = "no extractors";
    else if (!mpCamera || !mpCamera2 || mpCamera->size() < 8 || mpCamera2->size() < 8) why = "no KannalaBrandt8 camera pair";
    else if (mRlr.rows != 3 || mRlr.cols != 3 || mtlr.rows * mtlr.cols != 3 || mvLevelSigma2.empty() || mvLevelSigma2.size() > 16) why = "no rig (mRlr / mtlr / mvLevelSigma2)";
    else if ((int)mvKeys.size() != Nleft || (int)mvKeysRight.size() != Nright) why = "Nleft / Nright are not the keypoint counts";
    if (why) { fprintf(stderr, "Frame (HIP): ComputeStereoFishEyeMatches: %s\n", why); return; }
    orbhip_extractor *eL = mpORBextractorLeft->DeviceExtractor(), *eR = mpORBextractorRight->DeviceExtractor();
    // as in ComputeStereoMatches: the kernels read the two extractors' LATEST extractions, which must be this Frame's features (byte
    // comparison); the shared locks keep the next operator() of either extractor out until the results are back
    hip::ResidentFrame rl = hip::FindResidentIn(eL, mvKeys.data(), mDescriptors.ptr<uint8_t>(), Nleft);
    const bool right_empty = Nright == 0;
    hip::ResidentFrame rr = right_empty ? hip::ResidentFrame() : hip::FindResidentIn(eR, mvKeysRight.data(), mDescriptorsRight.ptr<uint8_t>(), Nright);
    if (!rl || !rl.d_kp || (!right_empty && (!rr || !rr.d_kp))) {
        fprintf(stderr, "Frame (HIP): ComputeStereoFishEyeMatches: the frame's features are not the latest extractions of its two extractors (left %s, right %s)\n",
                rl && rl.d_kp ? "ok" : "no", right_empty || (rr && rr.d_kp) ? "ok" : "no");
        return;
    }
    if (right_empty) return;
    float cam1[8], cam2[8], R[9], t[3];
    for (int k = 0; k < 8; k++) { cam1[k] = mpCamera->getParameter(k); cam2[k] = mpCamera2->getParameter(k); }
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[3 * i + j] = mRlr.at<float>(i, j); t[i] = mtlr.at<float>(i); }
    std::vector<int32_t> l2r(Nleft), r2l(Nright);
    std::vector<float> x3d(3 * (size_t)Nleft);
    int32_t n = 0;
    const int rc = orbhip_compute_stereo_fisheye_matches_host(eL, eR, (int)mpCamera->GetType(), cam1, (int)mpCamera2->GetType(), cam2, R, t,
                                                              mvLevelSigma2.data(), (int)mvLevelSigma2.size(), l2r.data(), mvDepth.data(), x3d.data(),
                                                              Nleft, r2l.data(), Nright, &n);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "Frame (HIP): ComputeStereoFishEyeMatches: %d (%s)\n", rc, orbhip_last_error());
        mvDepth.assign(Nleft, -1.0f);
        return;
    }
    for (int i = 0; i < Nleft; i++) {
        if (l2r[i] < 0) continue;
        mvLeftToRightMatch[i] = l2r[i];                                           // :1161-1164
        cv::Mat p(3, 1, CV_32F);
        p.at<float>(0) = x3d[3 * (size_t)i]; p.at<float>(1) = x3d[3 * (size_t)i + 1]; p.at<float>(2) = x3d[3 * (size_t)i + 2];
        mvStereo3Dpoints[i] = p;
    }
    for (int j = 0; j < Nright; j++) mvRightToLeftMatch[j] = r2l[j];
}

}  // namespace ORB_SLAM3
