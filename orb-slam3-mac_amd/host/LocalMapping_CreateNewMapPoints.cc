// LocalMapping_CreateNewMapPoints.cc -- void LocalMapping::CreateNewMapPoints() with the reference's signature (src/LocalMapping.cc:383-726).
// Kept on the host as written: the neighbour selection with the inertial mPrevKF extension (:386-403), the baseline / median-depth skips
// (:437-453), ComputeF12 (:456, :839-856) and bCoarse (:460-462).  The neighbours that survive go to ONE orbhip_create_new_map_points_host
// call: per neighbour SearchForTriangulation and then the per-match loop (:479-707) on the device, the flags AddMapPoint sets (:715-716)
// carried to the next neighbour's search there.  After the call :710-723 are replayed in neighbour order and match-index order
// (vMatchedIndices is vMatches12's non-negative entries in index order, ORBmatcher.cc:1196-1202).
//
// ONE deviation: CheckNewKeyFrames() (:429) is evaluated once per neighbour while the list for the call is built, before any device work;
// the reference evaluates it after the previous neighbour's loop.  A keyframe that arrives during the call is therefore seen one
// CreateNewMapPoints later: the neighbours after it are still triangulated here.
// Without a usable GPU: one message, nothing is created; there is no CPU fallback.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "cvmath.h"
#include "hip_context.h"
#include "slam_types.h"
#include "tri_geometry.h"

using namespace std;

namespace ORB_SLAM3 {

namespace {
static_assert(sizeof(cv::KeyPoint) == sizeof(orbhip_keypoint), "KeyPoint layout");

void rows34(const cv::Mat &T, float *o) { for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) o[4 * i + j] = T.at<float>(i, j); }
void vec3(const cv::Mat &v, float *o) { for (int i = 0; i < 3; i++) o[i] = v.at<float>(i); }

// what the device reads of one keyframe; the vectors own the arrays the record points to
struct KeyFrameArrays {
    vector<cv::KeyPoint> keys;
    vector<uint8_t> has_mp;
    vector<int32_t> nid, ids, start, feat;
    orbhip_newpoints_keyframe rec;
    void fill(KeyFrame *pKF, bool current)
    {
        memset(&rec, 0, sizeof(rec));
        const int n = pKF->N;
        keys = tri::keys(pKF);
        keys.resize(n > 0 ? n : 1);
        has_mp.assign(n > 0 ? n : 1, 0);
        for (int i = 0; i < n; i++) has_mp[i] = pKF->GetMapPoint(i) ? 1 : 0;
        rec.kp = (const orbhip_keypoint *)keys.data();
        rec.kp_raw = pKF->NLeft == -1 && (int)pKF->mvKeys.size() >= n && n > 0 ? (const orbhip_keypoint *)pKF->mvKeys.data() : nullptr;   // UnprojectStereo reads mvKeys
        rec.desc = pKF->mDescriptors.ptr<uint8_t>();
        const bool stereo = n > 0 && (int)pKF->mvuRight.size() >= n && (int)pKF->mvDepth.size() >= n;
        rec.u_right = stereo ? pKF->mvuRight.data() : nullptr; rec.depth = stereo ? pKF->mvDepth.data() : nullptr;
        rec.has_mp = has_mp.data(); rec.n = n;
        if (current) {
            nid.assign(n > 0 ? n : 1, -1);
            for (const auto &kv : pKF->mFeatVec) for (unsigned int i : kv.second) if ((int)i < n) nid[i] = (int32_t)kv.first;
            rec.nid = nid.data();
        } else {
            tri::flatten(pKF->mFeatVec, ids, start, feat);
            rec.node_ids = ids.data(); rec.node_start = start.data(); rec.feat = feat.data(); rec.nnodes = (int32_t)ids.size();
        }
        rec.level_sigma2 = pKF->mvLevelSigma2.data(); rec.scale_factors = pKF->mvScaleFactors.data();
    }
};
}  // namespace

// src/LocalMapping.cc:839-856: K1.t().inv() * t12x * R12 * K2.inv() with toK() = [fx 0 cx; 0 fy cy; 0 0 1] of either camera model
cv::Mat LocalMapping::ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2)
{
    const cvm::M3 R1w = cvm::block3(pKF1->GetRotation()), R2w = cvm::block3(pKF2->GetRotation());
    const cvm::V3 t1w = cvm::vec3(pKF1->GetTranslation()), t2w = cvm::vec3(pKF2->GetTranslation());
    const cvm::M3 R12 = cvm::mul_t(R1w, false, R2w, true);
    const cvm::M3 nR12 = cvm::mul_t(R1w, false, R2w, true, -1.0);
    const cvm::V3 t12 = cvm::mul_add(nR12, t2w, t1w);
    float c1[8], c2[8], F[9];
    int32_t type;
    tri::camera_params(pKF1->mpCamera, c1, type); tri::camera_params(pKF2->mpCamera, c2, type);
    tri::fundamental(c1, c2, R12, t12, F);
    cv::Mat F12(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) F12.at<float>(i / 3, i % 3) = F[i];
    return F12;
}

void LocalMapping::CreateNewMapPoints()
{
    // Retrieve neighbor keyframes in covisibility graph
    int nn = 10;
    // For stereo inertial case
    if(mbMonocular)
        nn=20;
    vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);

    if (mbInertial)
    {
        KeyFrame* pKF = mpCurrentKeyFrame;
        int count=0;
        while(((int)vpNeighKFs.size()<=nn)&&(pKF->mPrevKF)&&(count++<nn))
        {
            vector<KeyFrame*>::iterator it = std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF);
            if(it==vpNeighKFs.end())
                vpNeighKFs.push_back(pKF->mPrevKF);
            pKF = pKF->mPrevKF;
        }
    }

    cv::Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();

    const float ratioFactor = 1.5f*mpCurrentKeyFrame->mfScaleFactor;

    // the neighbours of the device call, in the reference's order, with what :427-463 decides per neighbour on the host
    vector<KeyFrame*> vpCall;
    vector<orbhip_tri_pair_general> vGeom;
    vector<orbhip_newpoints_pair> vPair;
    const bool rig1 = mpCurrentKeyFrame->mpCamera2 != nullptr;
    for(size_t i=0; i<vpNeighKFs.size(); i++)
    {
        if(i>0 && CheckNewKeyFrames())// && (mnMatchesInliers>50))
            break;

        KeyFrame* pKF2 = vpNeighKFs[i];

        // Check first that baseline is not too short
        cv::Mat Ow2 = pKF2->GetCameraCenter();
        const cvm::V3 vBaseline = cvm::sub(cvm::vec3(Ow2), cvm::vec3(Ow1));
        const float baseline = cvm::norm(vBaseline);

        if(!mbMonocular)
        {
            if(baseline<pKF2->mb)
            continue;
        }
        else
        {
            const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
            const float ratioBaselineDepth = baseline/medianDepthKF2;

            if(ratioBaselineDepth<0.01)
                continue;
        }

        // Compute Fundamental Matrix
        cv::Mat F12 = ComputeF12(mpCurrentKeyFrame,pKF2);

        bool bCoarse = mbInertial &&
                ((!mpCurrentKeyFrame->GetMap()->GetIniertialBA2() && mpCurrentKeyFrame->GetMap()->GetIniertialBA1())||
                 mpTracker->mState==Tracking::RECENTLY_LOST);

        orbhip_tri_pair_general g;
        if (!tri::fill_pair_general(mpCurrentKeyFrame, pKF2, F12, false, bCoarse, g))
            continue;       // one rig and one single-camera keyframe: SearchForTriangulation matches nothing there (ORBmatcher.cc:1131)

        orbhip_newpoints_pair P;
        memset(&P, 0, sizeof(P));
        memcpy(P.cam1, g.cam1, sizeof(P.cam1)); memcpy(P.cam2, g.cam2, sizeof(P.cam2));
        memcpy(P.cam1_type, g.cam1_type, sizeof(P.cam1_type)); memcpy(P.cam2_type, g.cam2_type, sizeof(P.cam2_type));
        P.nleft1 = g.nleft1; P.nleft2 = g.nleft2;
        rows34(mpCurrentKeyFrame->GetPose(), P.Tcw1[0]); rows34(pKF2->GetPose(), P.Tcw2[0]);
        rows34(mpCurrentKeyFrame->GetPoseInverse(), P.Twc1); rows34(pKF2->GetPoseInverse(), P.Twc2);
        vec3(Ow1, P.Ow1[0]); vec3(Ow2, P.Ow2[0]);
        if (rig1) {
            rows34(mpCurrentKeyFrame->GetRightPose(), P.Tcw1[1]); rows34(pKF2->GetRightPose(), P.Tcw2[1]);
            vec3(mpCurrentKeyFrame->GetRightCameraCenter(), P.Ow1[1]); vec3(pKF2->GetRightCameraCenter(), P.Ow2[1]);
        }
        P.mb1 = mpCurrentKeyFrame->mb; P.mb2 = pKF2->mb; P.mbf = mpCurrentKeyFrame->mbf;
        P.ratio_factor = ratioFactor;
        P.far_points = mbFarPoints ? 1 : 0; P.th_far_points = mThFarPoints;
        vpCall.push_back(pKF2); vGeom.push_back(g); vPair.push_back(P);
    }
    if (vpCall.empty())
        return;

    orbhip_ctx *ctx = hip::ThreadContext();
    if (!ctx) {
        fprintf(stderr, "LocalMapping::CreateNewMapPoints: no usable GPU (there is no CPU fallback), no map point created\n");
        return;
    }
    const int n1 = mpCurrentKeyFrame->N, K = (int)vpCall.size();
    KeyFrameArrays cur;
    cur.fill(mpCurrentKeyFrame, true);
    vector<KeyFrameArrays> neigh(K);
    vector<orbhip_newpoints_keyframe> recs(K);
    for (int k = 0; k < K; k++) { neigh[k].fill(vpCall[k], false); recs[k] = neigh[k].rec; }
    const size_t rows = (size_t)K * (n1 > 0 ? n1 : 1);
    vector<int32_t> matches12(rows, -1), n_created(K, 0);
    vector<float> x3D(rows * 3, 0.f);
    vector<uint8_t> outcome(rows, 0);
    // th = 0.6f; ORBmatcher matcher(th,false): no orientation check (:405-407; the ratio is not read by SearchForTriangulation)
    const int rc = orbhip_create_new_map_points_host(ctx, &cur.rec, recs.data(), vGeom.data(), vPair.data(), K, (int)mpCurrentKeyFrame->mvScaleFactors.size(),
                                                     0, matches12.data(), x3D.data(), outcome.data(), n_created.data(), nullptr);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "LocalMapping (HIP): CreateNewMapPoints: %d (%s), no map point created\n", rc, orbhip_last_error());
        return;
    }

    // :710-723, per neighbour in order, per match in index order
    for (int k = 0; k < K; k++) {
        KeyFrame* pKF2 = vpCall[k];
        for (int idx1 = 0; idx1 < n1; idx1++) {
            const uint8_t code = outcome[(size_t)k * n1 + idx1];
            if (code < 1 || code > 3)
                continue;
            const int idx2 = matches12[(size_t)k * n1 + idx1];
            cv::Mat x3Dm(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) x3Dm.at<float>(c) = x3D[((size_t)k * n1 + idx1) * 3 + c];

            // Triangulation is succesfull
            MapPoint* pMP = new MapPoint(x3Dm,mpCurrentKeyFrame,mpAtlas->GetCurrentMap());

            pMP->AddObservation(mpCurrentKeyFrame,idx1);
            pMP->AddObservation(pKF2,idx2);

            mpCurrentKeyFrame->AddMapPoint(pMP,idx1);
            pKF2->AddMapPoint(pMP,idx2);

            pMP->ComputeDistinctiveDescriptors();

            pMP->UpdateNormalAndDepth();

            mpAtlas->AddMapPoint(pMP);
            mlpRecentAddedMapPoints.push_back(pMP);
        }
    }
}

}  // namespace ORB_SLAM3
