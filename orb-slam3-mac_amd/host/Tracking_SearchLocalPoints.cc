// Tracking_SearchLocalPoints.cc -- void Tracking::SearchLocalPoints() with the reference's signature (src/Tracking.cc:2358-2430).
// The first loop (:2361-2378: the frame's own map points are marked seen) stays a host pointer walk.  The second loop (:2383-2401:
// Frame::isInFrustum on every local map point) and ORBmatcher::SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, ...) (:2428) are ONE
// orbhip_search_local_points_host(_resident) call: the points are packed once, the frustum kernel builds the matcher's queries on the
// device and the matcher reads them there.  Afterwards the MapPoint fields are written as the reference would have left them (the
// outcome codes of orbhip_track_record say which), IncreaseVisible and mmProjectPoints follow in list order, then the claims.
//
// ONE deviation: the reference runs the matcher only when nToMatch > 0, which it knows after its host loop; here the matcher is queued
// behind the frustum kernel before nToMatch is known.  With nToMatch == 0 it has no queries and claims nothing: mvpMapPoints is untouched
// and mnMatchesLocalPoints stays -1, as if it had not run.
// Without a usable GPU: one message, nothing is changed beyond the first loop; there is no CPU fallback.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ORBmatcher.h"
#include "cvmath.h"
#include "frame_cache.h"
#include "hip_context.h"
#include "slam_types.h"

using namespace std;

namespace ORB_SLAM3 {

namespace {
static_assert(sizeof(cv::KeyPoint) == sizeof(orbhip_keypoint), "KeyPoint layout");
void put3(const cv::Mat &v, float *o) { for (int i = 0; i < 3; i++) o[i] = v.at<float>(i); }
void put9(const cvm::M3 &M, float *o) { for (int i = 0; i < 9; i++) o[i] = M.m[i]; }
void put3(const cvm::V3 &v, float *o) { for (int i = 0; i < 3; i++) o[i] = v(i); }
}  // namespace

void Tracking::SearchLocalPoints()
{
    // Do not search map points already matched
    for(vector<MapPoint*>::iterator vit=mCurrentFrame.mvpMapPoints.begin(), vend=mCurrentFrame.mvpMapPoints.end(); vit!=vend; vit++)
    {
        MapPoint* pMP = *vit;
        if(pMP)
        {
            if(pMP->isBad())
            {
                *vit = static_cast<MapPoint*>(NULL);
            }
            else
            {
                pMP->IncreaseVisible();
                pMP->mnLastFrameSeen = mCurrentFrame.mnId;
                pMP->mbTrackInView = false;
                pMP->mbTrackInViewR = false;
            }
        }
    }
    mnMatchesLocalPoints = -1;
    Frame &F = mCurrentFrame;
    const int np = (int)mvpLocalMapPoints.size();
    if (np == 0) return;

    // th as :2405-2426 choose it (it only matters when something is matched; the record needs it before that is known)
    int th = 1;
    if(mSensor==System::RGBD)
        th=3;
    if(mpAtlas->isImuInitialized())
    {
        if(mpAtlas->GetCurrentMap()->GetIniertialBA2())
            th=2;
        else
            th=3;
    }
    else if(!mpAtlas->isImuInitialized() && (mSensor==System::IMU_MONOCULAR || mSensor==System::IMU_STEREO))
    {
        th=10;
    }
    // If the camera has been relocalised recently, perform a coarser search
    if(mCurrentFrame.mnId<mnLastRelocFrameId+2)
        th=5;
    if(mState==LOST || mState==RECENTLY_LOST) // Lost for less than 1 second
        th=15; // 15

    // the per-frame record: 3 x 3 products done once, in OpenCV's roundings (cvmath.h)
    const bool rig = F.Nleft != -1;
    orbhip_frustum_frame fr;
    memset(&fr, 0, sizeof(fr));
    const cvm::M3 Rcw = cvm::block3(F.mRcw);
    put9(Rcw, fr.Rcw); put3(F.mtcw, fr.tcw); put3(F.mOw, fr.Ow);
    fr.cam_type[0] = (int32_t)F.mpCamera->GetType(); fr.cam_type[1] = -1;
    for (size_t k = 0; k < 8 && k < F.mpCamera->size(); k++) fr.cam[0][k] = F.mpCamera->getParameter((int)k);
    if (rig) {                                                                   // Frame.cc:1176-1180
        const cvm::M3 Rrl = cvm::block3(F.mTrl);
        put9(cvm::mul(Rrl, Rcw), fr.Rrw);
        put3(cvm::mul_add(Rrl, cvm::vec3(F.mtcw), cvm::col3(F.mTrl)), fr.trw);
        put3(cvm::mul_add(cvm::block3(F.mRwc), cvm::col3(F.mTlr), cvm::vec3(F.mOw)), fr.Orw);
        if (F.mpCamera2) {
            fr.cam_type[1] = (int32_t)F.mpCamera2->GetType();
            for (size_t k = 0; k < 8 && k < F.mpCamera2->size(); k++) fr.cam[1][k] = F.mpCamera2->getParameter((int)k);
        }
    }
    fr.rig = rig; fr.mbf = F.mbf;
    fr.nlevels = F.mnScaleLevels;
    if (F.mnScaleLevels < 1 || F.mnScaleLevels > ORBHIP_FRUSTUM_MAX_LEVELS || (int)F.mvScaleFactors.size() < F.mnScaleLevels) {
        fprintf(stderr, "Tracking (HIP): SearchLocalPoints: mnScaleLevels = %d with %zu scale factors (1..32 levels)\n", F.mnScaleLevels, F.mvScaleFactors.size());
        return;
    }
    for (int l = 0; l < F.mnScaleLevels; l++) fr.scale_factors[l] = F.mvScaleFactors[l];
    if (orbhip_predict_scale_thresholds(F.mfLogScaleFactor, F.mnScaleLevels, fr.level_thresholds) != ORBHIP_OK) {
        fprintf(stderr, "Tracking (HIP): SearchLocalPoints: %s\n", orbhip_last_error());
        return;
    }
    fr.th = (float)th; fr.far_points = mpLocalMapper->mbFarPoints; fr.th_far_points = mpLocalMapper->mThFarPoints;
    fr.viewing_cos_limit = 0.5;                                                  // isInFrustum(pMP,0.5), :2392
    fr.n_points = np;

    // the points, packed once
    vector<float> Xw(3 * (size_t)np), normal(3 * (size_t)np), min_dist(np), max_dist(np), track_depth(np);
    vector<uint8_t> flags(np), desc(32 * (size_t)np);
    for (int i = 0; i < np; i++) {
        MapPoint *pMP = mvpLocalMapPoints[i];
        flags[i] = (pMP->Observations() > 0 ? 1 : 0) | ((pMP->mnLastFrameSeen == mCurrentFrame.mnId || pMP->isBad()) ? 2 : 0);   // :2387-2390
        put3(pMP->GetWorldPos(), &Xw[3 * (size_t)i]); put3(pMP->GetNormal(), &normal[3 * (size_t)i]);
        min_dist[i] = pMP->mfMinDistance; max_dist[i] = pMP->mfMaxDistance;      // raw: PredictScale divides mfMaxDistance itself (protected in the reference's
                                                                                 // MapPoint: INTEGRATION.md names the one-line accessors a build against it needs)
        track_depth[i] = pMP->mTrackDepth;
        const cv::Mat d = pMP->GetDescriptor();
        if (d.rows * d.cols >= 32) memcpy(&desc[32 * (size_t)i], d.ptr<uint8_t>(), 32);
    }
    orbhip_local_points pts;
    pts.Xw = Xw.data(); pts.normal = normal.data(); pts.min_dist = min_dist.data(); pts.max_dist = max_dist.data();
    pts.flags = flags.data(); pts.desc = desc.data(); pts.track_depth = track_depth.data(); pts.n = np;

    // the train side as ORBmatcher::SearchByProjection(F, vpMapPoints, ...) hands it over (host/ORBmatcher.cc)
    const int n = F.N;
    vector<int32_t> tm(n > 0 ? n : 1);
    for (int i = 0; i < n; i++) tm[i] = (F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0) ? -2 : -1;
    vector<orbhip_track_record> rec(np);
    vector<int32_t> owner((size_t)np * (rig ? 2 : 1));
    int32_t nToMatch = 0, nq = 0, nmatches = 0;
    orbhip_ctx *ctx = hip::ThreadContext();
    if (!ctx) { fprintf(stderr, "Tracking (HIP): SearchLocalPoints: no device context\n"); return; }
    const float nnratio = 0.8f;                                                  // ORBmatcher matcher(0.8), :2405
    int rc;
    if (!rig) {
        hip::ResidentFrame res = n > 0 ? hip::FindResident(hip::GetDevice(), F.mvKeysUn.data(), F.mDescriptors.ptr<uint8_t>(), n) : hip::ResidentFrame();
        if (res)
            rc = orbhip_search_local_points_host_resident(ctx, &fr, &pts, (const orbhip_keypoint *)F.mvKeysUn.data(), res.d_kp, res.d_desc,
                                                          F.mvuRight.empty() ? nullptr : F.mvuRight.data(), n, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY,
                                                          ORBmatcher::TH_HIGH, nnratio, rec.data(), &nToMatch, owner.data(), &nq, tm.data(), &nmatches);
        else
            rc = orbhip_search_local_points_host(ctx, &fr, &pts, (const orbhip_keypoint *)F.mvKeysUn.data(), F.mDescriptors.ptr<uint8_t>(),
                                                 F.mvuRight.empty() ? nullptr : F.mvuRight.data(), n, -1, nullptr, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY,
                                                 ORBmatcher::TH_HIGH, nnratio, rec.data(), &nToMatch, owner.data(), &nq, tm.data(), &nmatches);
    } else {
        vector<cv::KeyPoint> kp(F.mvKeys.begin(), F.mvKeys.begin() + F.Nleft);
        kp.insert(kp.end(), F.mvKeysRight.begin(), F.mvKeysRight.end());
        vector<int32_t> mirror(kp.size() ? kp.size() : 1, -1);
        for (size_t i = 0; i < F.mvLeftToRightMatch.size() && (int)i < F.Nleft; i++) if (F.mvLeftToRightMatch[i] != -1) mirror[i] = F.mvLeftToRightMatch[i] + F.Nleft;
        for (size_t i = 0; i < F.mvRightToLeftMatch.size() && F.Nleft + i < kp.size(); i++) if (F.mvRightToLeftMatch[i] != -1) mirror[F.Nleft + i] = F.mvRightToLeftMatch[i];
        rc = orbhip_search_local_points_host(ctx, &fr, &pts, (const orbhip_keypoint *)kp.data(), F.mDescriptors.ptr<uint8_t>(), nullptr, n, F.Nleft, mirror.data(),
                                             Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY, ORBmatcher::TH_HIGH, nnratio, rec.data(), &nToMatch,
                                             owner.data(), &nq, tm.data(), &nmatches);
    }
    if (rc != ORBHIP_OK) { fprintf(stderr, "Tracking (HIP): SearchLocalPoints: %d (%s)\n", rc, orbhip_last_error()); return; }

    // Project points in frame and check its visibility: what :2383-2401 leave in the points, in list order
    for (int i = 0; i < np; i++) {
        MapPoint *pMP = mvpLocalMapPoints[i];
        const orbhip_track_record &r = rec[i];
        if (r.code == 1) continue;                                               // :2387-2390
        if (!rig) {                                                              // Frame.cc:487-489, :516-517, :546-555
            pMP->mbTrackInView = r.in_view != 0;
            pMP->mTrackProjX = r.proj_x; pMP->mTrackProjY = r.proj_y;
            if (r.code == 0) { pMP->mTrackProjXR = r.proj_xr; pMP->mTrackDepth = r.depth; pMP->mnTrackScaleLevel = r.level; pMP->mTrackViewCos = r.view_cos; }
        } else {                                                                 // Frame.cc:562-568, :1227-1240
            pMP->mbTrackInView = r.in_view != 0; pMP->mbTrackInViewR = r.in_view_r != 0;
            pMP->mnTrackScaleLevel = r.level; pMP->mnTrackScaleLevelR = r.level_r;
            if (r.code == 0) { pMP->mTrackProjX = r.proj_x; pMP->mTrackProjY = r.proj_y; pMP->mTrackViewCos = r.view_cos; pMP->mTrackDepth = r.depth; }
            if (r.code_r == 0) { pMP->mTrackProjXR = r.proj_xr; pMP->mTrackProjYR = r.proj_yr; pMP->mTrackViewCosR = r.view_cos_r; pMP->mTrackDepthR = r.depth_r; }
        }
        if (r.in_view || r.in_view_r)
            pMP->IncreaseVisible();
        if(pMP->mbTrackInView)
        {
            mCurrentFrame.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
        }
    }

    if(nToMatch>0)
    {
        for (int i = 0; i < n; i++) if (tm[i] >= 0 && tm[i] < nq) F.mvpMapPoints[i] = mvpLocalMapPoints[owner[tm[i]]];   // F.mvpMapPoints[bestIdx]=pMP (ORBmatcher.cc:140-210)
        mnMatchesLocalPoints = nmatches;
    }
}

}  // namespace ORB_SLAM3
