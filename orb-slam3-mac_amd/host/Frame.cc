// Frame.cc -- the Frame member functions of the hot path that run on the device: Frame::ComputeStereoMatches
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

namespace ORB_SLAM3 {

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
