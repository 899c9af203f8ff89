// host_sim3solver_smoke.cc -- `host_sim3solver_smoke <in> <out>`: Sim3Solver (the class, host/Sim3Solver.cc) on stand-in keyframes from
// a flat file: Tcw1 / Tcw2 (4x4), cam_type (0 Pinhole, 1 KannalaBrandt8) + cam (mvParameters, every keyframe), sigma2 (mvLevelSigma2),
// kp1 / kp2 / kp3 (mvKeysUn, x y interleaved) + oct1 / oct2 / oct3, the map points mp_pos / mp_bad, kf1_mp / kf2_mp / kf3_mp (map point
// index per keypoint, -1 none), matches (vpMatched12 as map point indices, -1 NULL), matched_kf (vpKeyFrameMatchedMP: 2 or 3 per match;
// EMPTY = the constructor's default argument), fix_scale, min_inliers, max_iterations, probability.  `host_sim3solver_smoke <in> <out>
// [loop]` runs LoopClosing's loop (src/LoopClosing.cc:673-684: iterate(20, ...) until bConverge or bNoMore), `... find` one find(); rand()
// is unseeded, as in the reference, so a process draws the sets of srand(1).  Writes the flags, the number of iterate calls, vbInliers,
// nInliers, the returned matrices, GetEstimated* and the sets drawn.  Runs without a GPU too (bNoMore at once, empty matrices).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "Sim3Solver.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

static cv::Mat pose44(const std::vector<float> &v)
{
    cv::Mat T(4, 4, CV_32F);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T.at<float>(i, j) = v[4 * i + j];
    return T;
}
static std::vector<float> flat(const cv::Mat &m)
{
    std::vector<float> v;
    for (int i = 0; i < m.rows; i++) for (int j = 0; j < m.cols; j++) v.push_back(m.at<float>(i, j));
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: host_sim3solver_smoke <in> <out> [loop|find]\n"); return 2; }
    const bool find_mode = argc == 4 && std::string(argv[3]) == "find";
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "sim3solver: cannot read %s\n", argv[1]); return 2; }
    GeometricCamera camera(ff.F("cam"), (unsigned)ff.I("cam_type")[0]);
    Map map;
    const std::vector<float> &cam = ff.F("cam");
    KeyFrame kf1(1, &map, cam[0], cam[1], cam[2], cam[3], 0.f, &camera), kf2(2, &map, cam[0], cam[1], cam[2], cam[3], 0.f, &camera),
             kf3(3, &map, cam[0], cam[1], cam[2], cam[3], 0.f, &camera);
    kf1.SetPose(pose44(ff.F("Tcw1"))); kf2.SetPose(pose44(ff.F("Tcw2"))); kf3.SetPose(pose44(ff.F("Tcw2")));
    kf1.mvLevelSigma2 = kf2.mvLevelSigma2 = kf3.mvLevelSigma2 = ff.F("sigma2");
    const std::vector<float> &mp = ff.F("mp_pos");
    std::vector<std::unique_ptr<MapPoint>> pts;
    for (size_t k = 0; k < mp.size() / 3; k++) {
        cv::Mat X(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) X.at<float>(c) = mp[3 * k + c];
        pts.emplace_back(new MapPoint(k, X, &map));
        pts.back()->mbBad = ff.I("mp_bad")[k] != 0;
    }
    KeyFrame *kfs[3] = {&kf1, &kf2, &kf3};
    const char *kpn[3] = {"kp1", "kp2", "kp3"}, *ocn[3] = {"oct1", "oct2", "oct3"}, *mpn[3] = {"kf1_mp", "kf2_mp", "kf3_mp"};
    for (int s = 0; s < 3; s++) {
        const std::vector<float> &kp = ff.F(kpn[s]);
        const size_t n = kp.size() / 2;
        kfs[s]->mvKeysUn.resize(n); kfs[s]->mvpMapPoints.assign(n, nullptr); kfs[s]->mvuRight.assign(n, -1.f); kfs[s]->N = (int)n;
        for (size_t i = 0; i < n; i++) {
            kfs[s]->mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]);
            kfs[s]->mvKeysUn[i].octave = ff.I(ocn[s])[i];
            const int m = ff.I(mpn[s])[i];
            if (m >= 0) { kfs[s]->mvpMapPoints[i] = pts[m].get(); pts[m]->AddObservation(kfs[s], (int)i, -1); }
        }
    }
    std::vector<MapPoint *> vpMatchedPoints;
    for (int m : ff.I("matches")) vpMatchedPoints.push_back(m >= 0 ? pts[m].get() : nullptr);
    std::vector<KeyFrame *> vpKeyFrameMatchedMP;
    for (int k : ff.I("matched_kf")) vpKeyFrameMatchedMP.push_back(k == 3 ? &kf3 : &kf2);
    const bool bFixedScale = ff.I("fix_scale")[0] != 0;
    const int nBoWInliers = ff.I("min_inliers")[0], maxIts = ff.I("max_iterations")[0];
    const double prob = (double)ff.F("probability")[0];

    FlatWriter w(argv[2]);
    if (!find_mode) {   // src/LoopClosing.cc:673-684
        Sim3Solver solver = Sim3Solver(&kf1, &kf2, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);
        solver.SetRansacParameters(prob, nBoWInliers, maxIts);
        bool bNoMore = false;
        std::vector<bool> vbInliers;
        int nInliers = 0, calls = 0;
        bool bConverge = false;
        cv::Mat mTcm;
        std::vector<int32_t> ret_empty;
        while (!bConverge && !bNoMore) {
            mTcm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
            ret_empty.push_back(mTcm.empty() ? 1 : 0);
            calls++;
        }
        w.one("converged", bConverge); w.one("no_more", bNoMore); w.one("calls", calls); w.one("n_inliers", nInliers);
        w.ints("ret_empty", ret_empty);
        std::vector<int32_t> inl;
        for (bool b : vbInliers) inl.push_back(b ? 1 : 0);
        w.ints("inliers", inl);
        w.floats("T", flat(mTcm));
        w.floats("R", flat(solver.GetEstimatedRotation())); w.floats("t", flat(solver.GetEstimatedTranslation()));
        w.floats("s", std::vector<float>(1, solver.GetEstimatedScale()));
        w.ints("sets", solver.LastSets());
        printf("sim3solver: %zu matches given, loop: converged %d, no more %d after %d calls, %d inliers\n", vpMatchedPoints.size(), (int)bConverge,
               (int)bNoMore, calls, nInliers);
    } else {
        Sim3Solver solver(&kf1, &kf2, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);
        solver.SetRansacParameters(prob, nBoWInliers, maxIts);
        std::vector<bool> vbInliers;
        int nInliers = 0;
        const cv::Mat T = solver.find(vbInliers, nInliers);
        w.one("find_n_inliers", nInliers);
        std::vector<int32_t> inl;
        for (bool b : vbInliers) inl.push_back(b ? 1 : 0);
        w.ints("find_inliers", inl);
        w.floats("find_T", flat(T));
        w.floats("find_R", flat(solver.GetEstimatedRotation())); w.floats("find_t", flat(solver.GetEstimatedTranslation()));
        w.floats("find_s", std::vector<float>(1, solver.GetEstimatedScale()));
        w.ints("find_sets", solver.LastSets());
        printf("sim3solver: find: %s, %d inliers\n", T.empty() ? "empty" : "4x4", nInliers);
    }
    return 0;
}
