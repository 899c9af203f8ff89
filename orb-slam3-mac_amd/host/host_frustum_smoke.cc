// host_frustum_smoke.cc -- `host_frustum_smoke <mode> <in> <out> [reps]`: Frame::isInFrustum and Tracking::SearchLocalPoints (the class
// members, host/Frame.cc and host/Tracking_SearchLocalPoints.cc) on a stand-in frame and local map from a flat file.  Modes:
//   frustum   ONLY the host member Frame::isInFrustum over the points whose `skip` entry is 0; needs no device
//   track     Tracking::SearchLocalPoints (one device call)
//   today     what a caller had before: the host member in SearchLocalPoints' loop, then ORBmatcher::SearchByProjection(F, vpMapPoints, ...)
// With `reps` the mode runs reps + 1 times on fresh copies of the state and the wall time of every run but the first is printed (ms).
// Input.  Scalars (int): nleft (-1 single camera), cam_type, cam_type2, nlevels, far_points, sensor, imu_init, ba2, frame_id, last_reloc,
// state; floats: Tcw (4x4), Trl, Tlr (3x4 each, rigs), cam, cam2, bounds (minx miny maxx maxy), mbf, scale, log_scale, th_far, limit;
// per point: X, normal (3 floats), min_dist, max_dist, nobs, bad, last_seen, skip, desc (32 bytes), trk_f (mTrackProjX, Y, XR, YR, Depth,
// DepthR, ViewCos, ViewCosR) and trk_i (mnTrackScaleLevel, R, mbTrackInView, R) as an earlier frame left them; the frame: kp (x y
// interleaved, left | right), oct, desc_kp, ur (mvuRight or empty), mirror (frame-wide index of the same point's keypoint in the other
// camera or -1), fmp (per keypoint the index of the local point it holds already, or -1).
// Output: ret (frustum: isInFrustum's value per point, -1 skipped; else mnMatchesLocalPoints), trk_f, trk_i, visible, last_seen_out, fmp
// (per keypoint the index of the local point or -1), proj_id / proj_xy (mmProjectPoints in key order).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "ORBmatcher.h"
#include "flatfile.h"
#include "slam_types.h"

using namespace ORB_SLAM3;

float Frame::mnMinX = 0.f, Frame::mnMaxX = 0.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 0.f;
float Frame::fx = 0.f, Frame::fy = 0.f, Frame::cx = 0.f, Frame::cy = 0.f;

static cv::Mat mat(const std::vector<float> &v, int rows, int cols)
{
    cv::Mat T(rows, cols, CV_32F);
    for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) T.at<float>(i, j) = v[cols * i + j];
    return T;
}

// Tracking::SearchLocalPoints as the reference writes it (src/Tracking.cc:2358-2430) on the host members: the baseline of `today`
static void search_local_points_today(Tracking &T)
{
    Frame &mCurrentFrame = T.mCurrentFrame;
    for (MapPoint *&pMP : mCurrentFrame.mvpMapPoints)
        if (pMP) {
            if (pMP->isBad()) pMP = nullptr;
            else { pMP->IncreaseVisible(); pMP->mnLastFrameSeen = mCurrentFrame.mnId; pMP->mbTrackInView = false; pMP->mbTrackInViewR = false; }
        }
    int nToMatch = 0;
    for (MapPoint *pMP : T.mvpLocalMapPoints) {
        if (pMP->mnLastFrameSeen == mCurrentFrame.mnId) continue;
        if (pMP->isBad()) continue;
        if (mCurrentFrame.isInFrustum(pMP, 0.5)) { pMP->IncreaseVisible(); nToMatch++; }
        if (pMP->mbTrackInView) mCurrentFrame.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
    }
    T.mnMatchesLocalPoints = -1;
    if (nToMatch > 0) {
        ORBmatcher matcher(0.8);
        int th = 1;
        if (T.mSensor == System::RGBD) th = 3;
        if (T.mpAtlas->isImuInitialized()) th = T.mpAtlas->GetCurrentMap()->GetIniertialBA2() ? 2 : 3;
        else if (T.mSensor == System::IMU_MONOCULAR || T.mSensor == System::IMU_STEREO) th = 10;
        if (mCurrentFrame.mnId < T.mnLastRelocFrameId + 2) th = 5;
        if (T.mState == Tracking::LOST || T.mState == Tracking::RECENTLY_LOST) th = 15;
        T.mnMatchesLocalPoints = matcher.SearchByProjection(mCurrentFrame, T.mvpLocalMapPoints, th, T.mpLocalMapper->mbFarPoints, T.mpLocalMapper->mThFarPoints);
    }
}

int main(int argc, char **argv)
{
    if (argc != 4 && argc != 5) { fprintf(stderr, "usage: host_frustum_smoke frustum|track|today <in> <out> [reps]\n"); return 2; }
    const std::string mode = argv[1];
    const int reps = argc == 5 ? atoi(argv[4]) : 0;
    if (mode != "frustum" && mode != "track" && mode != "today") { fprintf(stderr, "frustum: unknown mode %s\n", argv[1]); return 2; }
    FlatFile ff;
    if (!ff.load(argv[2])) { fprintf(stderr, "frustum: cannot read %s\n", argv[2]); return 2; }
    const int nleft = ff.I("nleft")[0];
    const bool rig = nleft != -1;
    GeometricCamera camera(ff.F("cam"), (unsigned)ff.I("cam_type")[0]), camera2(ff.F("cam2"), (unsigned)(rig ? ff.I("cam_type2")[0] : 0));
    const std::vector<float> &b = ff.F("bounds");
    Frame::mnMinX = b[0]; Frame::mnMinY = b[1]; Frame::mnMaxX = b[2]; Frame::mnMaxY = b[3];
    Map map;
    map.mbImuInitialized = ff.I("imu_init")[0] != 0; map.mbIMU_BA2 = ff.I("ba2")[0] != 0;
    Atlas atlas; atlas.mpCurrentMap = &map;
    LocalMapping lm; lm.mbFarPoints = ff.I("far_points")[0] != 0; lm.mThFarPoints = ff.F("th_far")[0];
    Tracking T;
    T.mSensor = ff.I("sensor")[0]; T.mpAtlas = &atlas; T.mpLocalMapper = &lm; T.mnLastRelocFrameId = (unsigned)ff.I("last_reloc")[0];
    T.mState = (Tracking::eTrackingState)ff.I("state")[0];
    Frame &F = T.mCurrentFrame;
    F.mnId = (unsigned long)ff.I("frame_id")[0];
    F.mpCamera = &camera; F.mpCamera2 = rig ? &camera2 : nullptr; F.Nleft = nleft;
    F.mbf = ff.F("mbf")[0];
    F.mnScaleLevels = ff.I("nlevels")[0]; F.mvScaleFactors = ff.F("scale"); F.mfLogScaleFactor = ff.F("log_scale")[0];
    if (rig) { F.mTrl = mat(ff.F("Trl"), 3, 4); F.mTlr = mat(ff.F("Tlr"), 3, 4); }
    F.SetPose(mat(ff.F("Tcw"), 4, 4));
    // the frame's keypoints
    const std::vector<float> &kp = ff.F("kp");
    const int N = (int)kp.size() / 2;
    std::vector<cv::KeyPoint> keys(N);
    for (int i = 0; i < N; i++) { keys[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); keys[i].octave = ff.I("oct")[i]; keys[i].size = 31.f; keys[i].response = 1.f; }
    F.N = N;
    if (!rig) { F.mvKeysUn = keys; F.mvKeys = keys; F.mvuRight = ff.F("ur"); }
    else {
        F.mvKeys.assign(keys.begin(), keys.begin() + nleft); F.mvKeysRight.assign(keys.begin() + nleft, keys.end()); F.Nright = N - nleft;
        const std::vector<int32_t> &mi = ff.I("mirror");
        F.mvLeftToRightMatch.assign(nleft, -1); F.mvRightToLeftMatch.assign(N - nleft, -1);
        for (int i = 0; i < N; i++) if (mi[i] >= 0) { if (i < nleft) F.mvLeftToRightMatch[i] = mi[i] - nleft; else F.mvRightToLeftMatch[i - nleft] = mi[i]; }
    }
    F.mDescriptors = cv::Mat(N > 0 ? N : 1, 32, CV_8U);
    if (N) memcpy(F.mDescriptors.ptr<uint8_t>(), ff.U("desc_kp").data(), 32 * (size_t)N);
    // the local map
    const int np = (int)ff.F("min_dist").size();
    std::vector<std::unique_ptr<MapPoint>> pts;
    const std::vector<float> &X = ff.F("X"), &Nn = ff.F("normal"), &tf = ff.F("trk_f");
    const std::vector<int32_t> &ti = ff.I("trk_i");
    const std::vector<uint8_t> &desc = ff.U("desc");
    auto reset = [&](MapPoint *p, int i) {
        p->mTrackProjX = tf[8 * i]; p->mTrackProjY = tf[8 * i + 1]; p->mTrackProjXR = tf[8 * i + 2]; p->mTrackProjYR = tf[8 * i + 3];
        p->mTrackDepth = tf[8 * i + 4]; p->mTrackDepthR = tf[8 * i + 5]; p->mTrackViewCos = tf[8 * i + 6]; p->mTrackViewCosR = tf[8 * i + 7];
        p->mnTrackScaleLevel = ti[4 * i]; p->mnTrackScaleLevelR = ti[4 * i + 1]; p->mbTrackInView = ti[4 * i + 2] != 0; p->mbTrackInViewR = ti[4 * i + 3] != 0;
        p->mnVisible = 1; p->mnLastFrameSeen = (unsigned long)ff.I("last_seen")[i];
    };
    for (int i = 0; i < np; i++) {
        cv::Mat P(3, 1, CV_32F), n3(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) { P.at<float>(c) = X[3 * i + c]; n3.at<float>(c) = Nn[3 * i + c]; }
        pts.emplace_back(new MapPoint((unsigned long)i, P, &map));
        MapPoint *p = pts.back().get();
        p->mNormalVector = n3; p->mfMinDistance = ff.F("min_dist")[i]; p->mfMaxDistance = ff.F("max_dist")[i];
        p->nObs = ff.I("nobs")[i]; p->mbBad = ff.I("bad")[i] != 0;
        p->mDescriptor = cv::Mat(1, 32, CV_8U);
        memcpy(p->mDescriptor.ptr<uint8_t>(), &desc[32 * (size_t)i], 32);
        reset(p, i);
        T.mvpLocalMapPoints.push_back(p);
    }
    const std::vector<int32_t> &fmp = ff.I("fmp");
    auto reset_frame = [&]() {
        F.mvpMapPoints.assign(N, nullptr);
        for (int k = 0; k < N; k++) if (fmp[k] >= 0) F.mvpMapPoints[k] = pts[fmp[k]].get();
        F.mmProjectPoints.clear();
        for (int i = 0; i < np; i++) reset(pts[i].get(), i);
    };
    std::vector<int32_t> ret;
    const std::vector<int32_t> &skip = ff.I("skip");
    auto run = [&]() {
        if (mode == "frustum") {
            ret.assign(np, -1);
            for (int i = 0; i < np; i++) if (!skip[i]) ret[i] = F.isInFrustum(pts[i].get(), ff.F("limit")[0]) ? 1 : 0;
        } else if (mode == "track") { T.SearchLocalPoints(); ret.assign(1, T.mnMatchesLocalPoints); }
        else { search_local_points_today(T); ret.assign(1, T.mnMatchesLocalPoints); }
    };
    for (int r = 0; r <= reps; r++) {
        reset_frame();
        const auto t0 = std::chrono::steady_clock::now();
        run();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (reps && r > 0) printf("frustum: %s: run %d: %.4f ms\n", mode.c_str(), r, ms);
    }
    FlatWriter w(argv[3]);
    std::vector<float> otf(8 * (size_t)np), pxy;
    std::vector<int32_t> oti(4 * (size_t)np), vis(np), seen(np), ofmp(N), pid;
    std::map<MapPoint *, int> index;
    for (int i = 0; i < np; i++) {
        MapPoint *p = pts[i].get();
        index[p] = i;
        const float f8[8] = {p->mTrackProjX, p->mTrackProjY, p->mTrackProjXR, p->mTrackProjYR, p->mTrackDepth, p->mTrackDepthR, p->mTrackViewCos, p->mTrackViewCosR};
        memcpy(&otf[8 * (size_t)i], f8, sizeof(f8));
        oti[4 * i] = p->mnTrackScaleLevel; oti[4 * i + 1] = p->mnTrackScaleLevelR; oti[4 * i + 2] = p->mbTrackInView; oti[4 * i + 3] = p->mbTrackInViewR;
        vis[i] = p->mnVisible; seen[i] = (int32_t)p->mnLastFrameSeen;
    }
    for (int k = 0; k < N; k++) ofmp[k] = F.mvpMapPoints[k] ? index[F.mvpMapPoints[k]] : -1;
    for (const auto &kv : F.mmProjectPoints) { pid.push_back((int32_t)kv.first); pxy.push_back(kv.second.x); pxy.push_back(kv.second.y); }
    w.ints("ret", ret); w.floats("trk_f", otf); w.ints("trk_i", oti); w.ints("visible", vis); w.ints("last_seen_out", seen); w.ints("fmp", ofmp);
    w.ints("proj_id", pid); w.floats("proj_xy", pxy);
    printf("frustum: %s: %d points, %d keypoints, ret %d\n", mode.c_str(), np, N, ret.empty() ? 0 : ret[0]);
    return 0;
}
