// host_mlpnp_smoke.cc -- `host_mlpnp_smoke <in> <out> [calls]`: MLPnPsolver (the class, host/MLPnPsolver.cc) on a stand-in frame from a
// flat file: cam_type (0 Pinhole, 1 KannalaBrandt8) + cam (mvParameters), sigma2 (mvLevelSigma2), kp (mvKeysUn, x y interleaved) + oct,
// the map points mp_pos / mp_bad, matches (vpMapPointMatches as map point indices, -1 NULL; it may be longer than kp), probability,
// min_inliers, max_iterations, epsilon, th2 (SetRansacParameters) and n_iterations (iterate's first argument).  It makes up to `calls`
// (default 1) iterate() calls, as Tracking::Relocalization does (src/Tracking.cc:2697-2698), stopping at bNoMore; rand() is unseeded, as in
// the reference, so a process draws the sets of srand(1).  Per call it writes whether the matrix was empty, bNoMore, nInliers, the 16
// floats, vbInliers and the library's stats; at the end the sets drawn.  Runs without a GPU too (bNoMore at once, an empty matrix).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "MLPnPsolver.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: host_mlpnp_smoke <in> <out> [calls]\n"); return 2; }
    const int max_calls = argc == 4 ? atoi(argv[3]) : 1;
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "mlpnp: cannot read %s\n", argv[1]); return 2; }
    GeometricCamera camera(ff.F("cam"), (unsigned)ff.I("cam_type")[0]);
    Map map;
    Frame mCurrentFrame;
    mCurrentFrame.mpCamera = &camera;
    mCurrentFrame.mvLevelSigma2 = ff.F("sigma2");
    const std::vector<float> &kp = ff.F("kp");
    const size_t n = kp.size() / 2;
    mCurrentFrame.mvKeysUn.resize(n); mCurrentFrame.mvpMapPoints.assign(n, nullptr); mCurrentFrame.N = (int)n;
    for (size_t i = 0; i < n; i++) {
        mCurrentFrame.mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]);
        mCurrentFrame.mvKeysUn[i].octave = ff.I("oct")[i];
    }
    const std::vector<float> &mp = ff.F("mp_pos");
    std::vector<std::unique_ptr<MapPoint>> pts;
    for (size_t k = 0; k < mp.size() / 3; k++) {
        cv::Mat X(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) X.at<float>(c) = mp[3 * k + c];
        pts.emplace_back(new MapPoint(k, X, &map));
        pts.back()->mbBad = ff.I("mp_bad")[k] != 0;
    }
    std::vector<MapPoint *> vpMapPointMatches;
    for (int m : ff.I("matches")) vpMapPointMatches.push_back(m >= 0 ? pts[m].get() : nullptr);

    FlatWriter w(argv[2]);
    MLPnPsolver *pSolver = new MLPnPsolver(mCurrentFrame, vpMapPointMatches);
    pSolver->SetRansacParameters((double)ff.F("probability")[0], ff.I("min_inliers")[0], ff.I("max_iterations")[0], 6, ff.F("epsilon")[0], ff.F("th2")[0]);
    std::vector<int32_t> ret_empty, no_more, n_inliers, inliers, stats;
    std::vector<float> T;
    int calls = 0;
    bool bNoMore = false;
    while (calls < max_calls && !bNoMore) {
        std::vector<bool> vbInliers;
        int nInliers;
        cv::Mat Tcw = pSolver->iterate(ff.I("n_iterations")[0], bNoMore, vbInliers, nInliers);
        calls++;
        ret_empty.push_back(Tcw.empty() ? 1 : 0); no_more.push_back(bNoMore ? 1 : 0); n_inliers.push_back(nInliers);
        for (int i = 0; i < 4 && !Tcw.empty(); i++) for (int j = 0; j < 4; j++) T.push_back(Tcw.at<float>(i, j));
        inliers.push_back((int32_t)vbInliers.size());
        for (bool b : vbInliers) inliers.push_back(b ? 1 : 0);
        for (int k = 0; k < 4; k++) stats.push_back(pSolver->LastStats()[k]);
        printf("mlpnp: call %d: %s, no more %d, %d inliers\n", calls, Tcw.empty() ? "empty" : "4x4", (int)bNoMore, nInliers);
    }
    w.one("calls", calls);
    w.ints("ret_empty", ret_empty); w.ints("no_more", no_more); w.ints("n_inliers", n_inliers); w.ints("inliers", inliers); w.ints("stats", stats);
    w.floats("T", T);
    w.ints("sets", pSolver->LastSets());
    delete pSolver;
    return 0;
}
