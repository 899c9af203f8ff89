// host_sim3_smoke.cc -- `host_sim3_smoke <in> <out>`: Optimizer::OptimizeSim3 (the class method, host/Optimizer_OptimizeSim3.cc) on two
// stand-in keyframes from a flat file: Tcw1 / Tcw2 (4x4), cam_type (0 Pinhole, 1 KannalaBrandt8) + cam (mvParameters, both keyframes),
// inv_sigma2 (mvInvLevelSigma2), kp1 / kp2 (mvKeysUn, x y interleaved) + oct1 / oct2, the map points mp_pos / mp_bad / mp_level
// (mnTrackScaleLevel: -1 or anything else, the method must not index with it), kf1_mp / kf2_mp (map point index per keypoint, -1 none), matches (vpMatches1 as map point indices, -1 NULL),
// sim3 (g2oS12: 8 doubles qx qy qz qw tx ty tz s), th2, fix_scale, all_points.  Writes the return value, which vpMatches1 entries are
// NULL afterwards, g2oS12 and mAcumHessian (filled with 7 before the call).  Runs without a GPU too (the method then answers 0 and
// touches nothing).  `host_sim3_smoke <in> <out> <repeat>` then calls the method `repeat` more times on copies of the inputs and prints
// the median wall time of a call (tools/sim3_probe.py).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "Optimizer.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

static cv::Mat pose44(const std::vector<float> &v)
{
    cv::Mat T(4, 4, CV_32F);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T.at<float>(i, j) = v[4 * i + j];
    return T;
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: host_sim3_smoke <in> <out> [repeat]\n"); return 2; }
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "sim3: cannot read %s\n", argv[1]); return 2; }
    GeometricCamera camera(ff.F("cam"), (unsigned)ff.I("cam_type")[0]);
    Map map;
    const std::vector<float> &cam = ff.F("cam");
    KeyFrame kf1(1, &map, cam[0], cam[1], cam[2], cam[3], 0.f, &camera), kf2(2, &map, cam[0], cam[1], cam[2], cam[3], 0.f, &camera);
    kf1.SetPose(pose44(ff.F("Tcw1"))); kf2.SetPose(pose44(ff.F("Tcw2")));
    kf1.mvInvLevelSigma2 = kf2.mvInvLevelSigma2 = ff.F("inv_sigma2");
    const std::vector<float> &mp = ff.F("mp_pos");
    std::vector<std::unique_ptr<MapPoint>> pts;
    for (size_t k = 0; k < mp.size() / 3; k++) {
        cv::Mat X(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) X.at<float>(c) = mp[3 * k + c];
        pts.emplace_back(new MapPoint(k, X, &map));
        pts.back()->mbBad = ff.I("mp_bad")[k] != 0;
        pts.back()->mnTrackScaleLevel = ff.I("mp_level")[k];
    }
    KeyFrame *kfs[2] = {&kf1, &kf2};
    const char *kpn[2] = {"kp1", "kp2"}, *ocn[2] = {"oct1", "oct2"}, *mpn[2] = {"kf1_mp", "kf2_mp"};
    for (int s = 0; s < 2; s++) {
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
    std::vector<MapPoint *> vpMatches1;
    for (int m : ff.I("matches")) vpMatches1.push_back(m >= 0 ? pts[m].get() : nullptr);
    double S[8];
    memcpy(S, ff.U("sim3").data(), 64);
    Eigen::Vector3d t; t[0] = S[4]; t[1] = S[5]; t[2] = S[6];
    g2o::Sim3 g2oS12(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), t, S[7]);
    Eigen::Matrix<double, 7, 7> mAcumHessian;
    for (int i = 0; i < 7; i++) for (int j = 0; j < 7; j++) mAcumHessian(i, j) = 7.0;

    const std::vector<MapPoint *> vpMatches0 = vpMatches1;
    const g2o::Sim3 g2oS0 = g2oS12;
    const int ret = Optimizer::OptimizeSim3(&kf1, &kf2, vpMatches1, g2oS12, ff.F("th2")[0], ff.I("fix_scale")[0] != 0, mAcumHessian, ff.I("all_points")[0] != 0);
    if (argc == 4) {
        std::vector<double> ms;
        for (int k = 0; k < atoi(argv[3]); k++) {
            std::vector<MapPoint *> vm = vpMatches0;
            g2o::Sim3 S12 = g2oS0;
            Eigen::Matrix<double, 7, 7> H;
            const auto t0 = std::chrono::steady_clock::now();
            Optimizer::OptimizeSim3(&kf1, &kf2, vm, S12, ff.F("th2")[0], ff.I("fix_scale")[0] != 0, H, ff.I("all_points")[0] != 0);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        if (!ms.empty()) printf("sim3: OptimizeSim3 median %.4f ms, min %.4f, max %.4f over %zu calls\n", ms[ms.size() / 2], ms.front(), ms.back(), ms.size());
    }

    FlatWriter w(argv[2]);
    w.one("ret", ret);
    std::vector<int32_t> isnull;
    for (MapPoint *p : vpMatches1) isnull.push_back(p ? 0 : 1);
    w.ints("matches_null", isnull);
    const double So[8] = {g2oS12.rotation().x(), g2oS12.rotation().y(), g2oS12.rotation().z(), g2oS12.rotation().w(),
                          g2oS12.translation()[0], g2oS12.translation()[1], g2oS12.translation()[2], g2oS12.scale()};
    w.rec("sim3", 2, 64, So);
    double H[49];
    for (int i = 0; i < 7; i++) for (int j = 0; j < 7; j++) H[7 * i + j] = mAcumHessian(i, j);
    w.rec("hessian", 2, 49 * 8, H);
    printf("sim3: %zu matches given, OptimizeSim3 returned %d\n", vpMatches1.size(), ret);
    return 0;
}
