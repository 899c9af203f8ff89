// tri_geometry.h -- what ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:969-1210) derives from its two keyframes before the
// candidate walk, in the reference's cv::Mat arithmetic (cvmath.h): the epipole, the relative poses of the camera combinations
// ll / lr / rl / rr and their fundamental matrices -- the orbhip_tri_pair_general record of the device search.  Shared by
// host/ORBmatcher_keyframe.cc and host/LocalMapping_CreateNewMapPoints.cc (which runs the search inside its device chain).
#pragma once
#include <cstring>
#include <vector>
#include "../../include/orbhip.h"
#include "cvmath.h"
#include "slam_types.h"

namespace ORB_SLAM3 {
namespace tri {

inline void flatten(const DBoW2::FeatureVector &fv, std::vector<int32_t> &ids, std::vector<int32_t> &start, std::vector<int32_t> &feat)
{
    start.push_back(0);
    for (const auto &kv : fv) {
        ids.push_back((int32_t)kv.first);
        for (unsigned int i : kv.second) feat.push_back((int32_t)i);
        start.push_back((int32_t)feat.size());
    }
}

inline void camera_params(GeometricCamera *cam, float (&p)[8], int32_t &type)
{
    type = cam->GetType() == cam->CAM_FISHEYE ? 1 : 0;
    for (int i = 0; i < 8; i++) p[i] = i < (int)cam->size() ? cam->getParameter(i) : 0.f;
}
// F12 = K1.t().inv() * t12x * R12 * K2.inv() (Pinhole.cpp:124-127), for the camera pairs whose first camera is a Pinhole and for which the
// caller's F12 does not apply (rig combinations)
inline void fundamental(const float (&c1)[8], const float (&c2)[8], const cvm::M3 &R12, const cvm::V3 &t12, float (&F)[9])
{
    cvm::M3 K1t, K2;
    for (int i = 0; i < 9; i++) K1t.m[i] = K2.m[i] = 0.f;
    K1t(0, 0) = c1[0]; K1t(2, 0) = c1[2]; K1t(1, 1) = c1[1]; K1t(2, 1) = c1[3]; K1t(2, 2) = 1.f;       // K1.t()
    K2(0, 0) = c2[0]; K2(0, 2) = c2[2]; K2(1, 1) = c2[1]; K2(1, 2) = c2[3]; K2(2, 2) = 1.f;
    const cvm::M3 A = cvm::mul(cvm::mul(cvm::mul(cvm::inv3(K1t), cvm::skew(t12)), R12), cvm::inv3(K2));
    for (int i = 0; i < 9; i++) F[i] = A.m[i];
}

// keypoints in descriptor order: mvKeysUn, or mvKeys | mvKeysRight on rig keyframes (:1050-1052, :1084-1086)
inline std::vector<cv::KeyPoint> keys(KeyFrame *pKF)
{
    if (pKF->NLeft == -1) return pKF->mvKeysUn;
    std::vector<cv::KeyPoint> k(pKF->mvKeys.begin(), pKF->mvKeys.begin() + pKF->NLeft);
    k.insert(k.end(), pKF->mvKeysRight.begin(), pKF->mvKeysRight.end());
    return k;
}

// false: exactly one keyframe has a second camera -- the reference reads an empty R12 there (:1131) and nothing can be matched
inline bool fill_pair_general(KeyFrame *pKF1, KeyFrame *pKF2, const cv::Mat &F12, bool bOnlyStereo, bool bCoarse, orbhip_tri_pair_general &g)
{
    memset(&g, 0, sizeof(g));
    // Compute epipole in second image (:978-984)
    const cvm::V3 Cw = cvm::vec3(pKF1->GetCameraCenter());
    const cvm::M3 R2w = cvm::block3(pKF2->GetRotation());
    const cvm::V3 t2w = cvm::vec3(pKF2->GetTranslation());
    const cvm::V3 C2 = cvm::mul_add(R2w, Cw, t2w);
    const cv::Point2f ep = pKF2->mpCamera->project(cvm::to_mat(C2));
    g.ep_x = ep.x; g.ep_y = ep.y;
    const cvm::M3 R1w = cvm::block3(pKF1->GetRotation());
    const cvm::V3 t1w = cvm::vec3(pKF1->GetTranslation());
    auto rel = [](const cvm::M3 &Ra, const cvm::V3 &ta, const cvm::M3 &Rb, const cvm::V3 &tb, float (&R)[9], float (&t)[3]) {
        // R12 = Ra * Rb.t();  t12 = Ra * (-Rb.t() * tb) + ta  -- and for the single-camera pair -Ra*Rb.t()*tb + ta: the same products
        const cvm::M3 Rab = cvm::mul_t(Ra, false, Rb, true);
        const cvm::V3 tmp = cvm::mul_t(Rb, tb, -1.0);
        const cvm::V3 tab = cvm::mul_add(Ra, tmp, ta);
        for (int i = 0; i < 9; i++) R[i] = Rab.m[i];
        for (int i = 0; i < 3; i++) t[i] = tab(i);
    };
    camera_params(pKF1->mpCamera, g.cam1[0], g.cam1_type[0]);
    camera_params(pKF2->mpCamera, g.cam2[0], g.cam2_type[0]);
    const bool rig = pKF1->mpCamera2 && pKF2->mpCamera2;
    if (!pKF1->mpCamera2 && !pKF2->mpCamera2) {                                       // :996-998
        // R12 = R1w*R2w.t(); t12 = -R1w*R2w.t()*t2w + t1w: (-(R1w R2w^T)) is evaluated first, then times t2w plus t1w
        const cvm::M3 R12 = cvm::mul_t(R1w, false, R2w, true);
        const cvm::M3 nR12 = cvm::mul_t(R1w, false, R2w, true, -1.0);
        const cvm::V3 t12 = cvm::mul_add(nR12, t2w, t1w);
        for (int i = 0; i < 9; i++) g.R12[0][i] = R12.m[i];
        for (int i = 0; i < 3; i++) g.t12[0][i] = t12(i);
        for (int i = 0; i < 9; i++) g.F12[0][i] = F12.at<float>(i / 3, i % 3);      // the caller's F12 is the very expression Pinhole::epipolarConstrain evaluates (LocalMapping.cc:1010-1024)
    } else if (rig) {                                                                 // :999-1008
        camera_params(pKF1->mpCamera2, g.cam1[1], g.cam1_type[1]);
        camera_params(pKF2->mpCamera2, g.cam2[1], g.cam2_type[1]);
        const cvm::M3 R1r = cvm::block3(pKF1->GetRightRotation()), R2r = cvm::block3(pKF2->GetRightRotation());
        const cvm::V3 t1r = cvm::vec3(pKF1->GetRightTranslation()), t2r = cvm::vec3(pKF2->GetRightTranslation());
        rel(R1w, t1w, R2w, t2w, g.R12[0], g.t12[0]);                                  // ll
        rel(R1w, t1w, R2r, t2r, g.R12[1], g.t12[1]);                                  // lr
        rel(R1r, t1r, R2w, t2w, g.R12[2], g.t12[2]);                                  // rl
        rel(R1r, t1r, R2r, t2r, g.R12[3], g.t12[3]);                                  // rr
        for (int c = 0; c < 4; c++)
            if (g.cam1_type[c >> 1] == 0) {
                cvm::M3 R; cvm::V3 t;
                for (int i = 0; i < 9; i++) R.m[i] = g.R12[c][i];
                for (int i = 0; i < 3; i++) t(i) = g.t12[c][i];
                fundamental(g.cam1[c >> 1], g.cam2[c & 1], R, t, g.F12[c]);
            }
    } else
        return false;                                                                 // exactly one keyframe with a second camera
    g.nleft1 = pKF1->mpCamera2 ? pKF1->NLeft : -1; g.nleft2 = pKF2->mpCamera2 ? pKF2->NLeft : -1;
    g.only_stereo = bOnlyStereo ? 1 : 0; g.coarse = bCoarse ? 1 : 0;
    return true;
}

}  // namespace tri
}  // namespace ORB_SLAM3
