// host_newpoints_smoke.cc -- `host_newpoints_smoke <in> <out> [time]`: LocalMapping::CreateNewMapPoints (the class method,
// host/LocalMapping_CreateNewMapPoints.cc) on stand-in keyframes from a flat file.  Keyframe 0 is mpCurrentKeyFrame, keyframes 1..nkf-1 its
// covisible neighbours in order.  Scalars: nkf, cam_type, nleft (per keyframe; -1 single camera), monocular, inertial, far_points,
// check_true_at (CheckNewKeyFrames turns true at that call; -1 never); floats: cam / cam2 (mvParameters), tlr (mTlr, 4x4, rigs),
// th_far, scale, sigma2, and per keyframe k: Tcw<k> (4x4), mb<k>, kp<k> (the keypoints in descriptor order, x y interleaved), raw<k> (mvKeys
// of a single-camera keyframe), oct<k>, ur<k>, dp<k>, desc<k> (bytes), nid<k> (vocabulary node per feature, -1 none), mp<k> (1: the
// keypoint has a map point already) + mpx<k> (its world position, 3 floats per keypoint).
// Writes: n_created, pos (world positions in mlpRecentAddedMapPoints order), obs (per point: current index, neighbour keyframe, its
// index), atlas_same_order, kfmp<k> (per keypoint: -1 none, -2 the earlier map point, else the position in mlpRecentAddedMapPoints),
// check_calls, desc_updates, normal_updates.  `time`: runs the call 1 + 5 times on fresh copies of the flags and prints the best wall time.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "flatfile.h"
#include "slam_types.h"

using namespace ORB_SLAM3;

static cv::Mat mat44(const std::vector<float> &v)
{
    cv::Mat T(4, 4, CV_32F);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T.at<float>(i, j) = v[4 * i + j];
    return T;
}
static std::string nm(const char *base, int k) { return std::string(base) + std::to_string(k); }

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: host_newpoints_smoke <in> <out> [time]\n"); return 2; }
    const bool time_mode = argc == 4 && std::string(argv[3]) == "time";
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "newpoints: cannot read %s\n", argv[1]); return 2; }
    const int nkf = ff.I("nkf")[0];
    const bool rig = ff.I("nleft")[0] != -1;
    GeometricCamera camera(ff.F("cam"), (unsigned)ff.I("cam_type")[0]), camera2(rig ? ff.F("cam2") : ff.F("cam"), (unsigned)ff.I("cam_type")[0]);
    const std::vector<float> &cam = ff.F("cam");
    Map map;
    Atlas atlas; atlas.mpCurrentMap = &map;
    Tracking tracker;
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<std::unique_ptr<MapPoint>> old_points;
    for (int k = 0; k < nkf; k++) {
        const float mb = ff.F(nm("mb", k).c_str())[0];
        kfs.emplace_back(new KeyFrame(k, &map, cam[0], cam[1], cam[2], cam[3], mb * cam[0], &camera));
        KeyFrame *kf = kfs.back().get();
        kf->SetPose(mat44(ff.F(nm("Tcw", k).c_str())));
        kf->mb = mb;
        kf->mvScaleFactors = ff.F("scale"); kf->mvLevelSigma2 = ff.F("sigma2");
        const std::vector<float> &kp = ff.F(nm("kp", k).c_str()), &raw = ff.F(nm("raw", k).c_str());
        const int n = (int)kp.size() / 2, nleft = ff.I("nleft")[k];
        kf->N = n; kf->NLeft = nleft;
        std::vector<cv::KeyPoint> keys(n), rawk(n);
        for (int i = 0; i < n; i++) {
            keys[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); keys[i].octave = ff.I(nm("oct", k).c_str())[i];
            rawk[i] = keys[i]; rawk[i].pt = cv::Point2f(raw[2 * i], raw[2 * i + 1]);
        }
        if (nleft == -1) { kf->mvKeysUn = keys; kf->mvKeys = rawk; }
        else {
            kf->mpCamera2 = &camera2; kf->mTlr = mat44(ff.F("tlr"));
            kf->mvKeys.assign(keys.begin(), keys.begin() + nleft); kf->mvKeysRight.assign(keys.begin() + nleft, keys.end());
        }
        kf->mvuRight = ff.F(nm("ur", k).c_str()); kf->mvDepth = ff.F(nm("dp", k).c_str());
        const std::vector<uint8_t> &d = ff.U(nm("desc", k).c_str());
        kf->mDescriptors = cv::Mat(n > 0 ? n : 1, 32, CV_8U);
        if (n) memcpy(kf->mDescriptors.ptr<uint8_t>(), d.data(), 32 * (size_t)n);
        const std::vector<int32_t> &nid = ff.I(nm("nid", k).c_str());
        for (int i = 0; i < n; i++) if (nid[i] >= 0) kf->mFeatVec.addFeature((DBoW2::NodeId)nid[i], (unsigned)i);
        kf->mvpMapPoints.assign(n, nullptr);
        const std::vector<int32_t> &mp = ff.I(nm("mp", k).c_str());
        const std::vector<float> &mpx = ff.F(nm("mpx", k).c_str());
        for (int i = 0; i < n; i++)
            if (mp[i]) {
                cv::Mat X(3, 1, CV_32F);
                for (int c = 0; c < 3; c++) X.at<float>(c) = mpx[3 * i + c];
                old_points.emplace_back(new MapPoint(1000000 + old_points.size(), X, &map));
                kf->mvpMapPoints[i] = old_points.back().get();
            }
    }
    for (int k = 1; k < nkf; k++) kfs[0]->mvpOrderedConnectedKeyFrames.push_back(kfs[k].get());
    LocalMapping lm;
    lm.mpCurrentKeyFrame = kfs[0].get();
    lm.mbMonocular = ff.I("monocular")[0] != 0; lm.mbInertial = ff.I("inertial")[0] != 0; lm.mbFarPoints = ff.I("far_points")[0] != 0;
    lm.mThFarPoints = ff.F("th_far")[0];
    lm.mpAtlas = &atlas; lm.mpTracker = &tracker;
    lm.mnCheckTrueAt = ff.I("check_true_at")[0];

    if (time_mode) {
        std::vector<std::vector<MapPoint *>> saved;
        for (auto &kf : kfs) saved.push_back(kf->mvpMapPoints);
        double best = 1e30;
        for (int rep = 0; rep < 6; rep++) {
            for (size_t k = 0; k < kfs.size(); k++) kfs[k]->mvpMapPoints = saved[k];
            lm.mlpRecentAddedMapPoints.clear(); atlas.mvpMapPoints.clear();
            const auto t0 = std::chrono::steady_clock::now();
            lm.CreateNewMapPoints();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rep > 0 && ms < best) best = ms;
        }
        printf("newpoints: time: %d neighbours, %d keypoints in the current keyframe, %zu points created, best of 5: %.3f ms\n", nkf - 1, kfs[0]->N,
               lm.mlpRecentAddedMapPoints.size(), best);
        return 0;
    }
    lm.CreateNewMapPoints();

    FlatWriter w(argv[2]);
    std::vector<float> pos;
    std::vector<int32_t> obs;
    std::map<MapPoint *, int> order;
    int same = lm.mlpRecentAddedMapPoints.size() == atlas.mvpMapPoints.size(), at = 0, desc_updates = 0, normal_updates = 0;
    for (MapPoint *pMP : lm.mlpRecentAddedMapPoints) {
        const cv::Mat X = pMP->GetWorldPos();
        for (int c = 0; c < 3; c++) pos.push_back(X.at<float>(c));
        same = same && atlas.mvpMapPoints[at] == pMP;
        order[pMP] = at++;
        desc_updates += pMP->nDescriptorUpdates; normal_updates += pMP->nNormalUpdates;
        int cur_idx = -1, kf2 = -1, idx2 = -1;
        for (const auto &ob : pMP->GetObservations()) {
            const int idx = std::get<0>(ob.second) != -1 ? std::get<0>(ob.second) : std::get<1>(ob.second);
            if (ob.first == kfs[0].get()) cur_idx = idx;
            else { kf2 = (int)ob.first->mnId; idx2 = idx; }
        }
        obs.push_back(cur_idx); obs.push_back(kf2); obs.push_back(idx2);
        if (pMP->mpRefKF != kfs[0].get() || pMP->GetObservations().size() != 2) same = 0;
    }
    w.one("n_created", (int32_t)lm.mlpRecentAddedMapPoints.size());
    w.floats("pos", pos); w.ints("obs", obs); w.one("atlas_same_order", same);
    for (int k = 0; k < nkf; k++) {
        std::vector<int32_t> v;
        for (MapPoint *pMP : kfs[k]->mvpMapPoints) v.push_back(!pMP ? -1 : order.count(pMP) ? order[pMP] : -2);
        w.ints(nm("kfmp", k).c_str(), v);
    }
    w.one("check_calls", lm.mnCheckCalls); w.one("desc_updates", desc_updates); w.one("normal_updates", normal_updates);
    printf("newpoints: %d neighbours, %zu map points created\n", nkf - 1, lm.mlpRecentAddedMapPoints.size());
    for (MapPoint *pMP : lm.mlpRecentAddedMapPoints) delete pMP;
    return 0;
}
