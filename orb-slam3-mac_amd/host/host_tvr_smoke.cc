// host_tvr_smoke.cc -- `host_smoke tvr <in> <out>`: GeometricCamera::ReconstructWithTwoViews (-> TwoViewReconstruction::Reconstruct) on one
// frame pair from a flat file: kp1 / kp2 (x, y interleaved), matches (vMatches12), cam_type (0 Pinhole, 1 KannalaBrandt8), cam
// (mvParameters).  Writes the return value, R21 / t21 (empty when the call fails), vP3D, vbTriangulated, their sizes and the RANSAC sets
// the class drew.  Runs without a GPU too (the class then answers false).
#include <cstdio>
#include <vector>
#include "TwoViewReconstruction.h"
#include "flatfile.h"
#include "slam_types.h"

using namespace ORB_SLAM3;

int tvr_smoke(const char *in, const char *out)
{
    FlatFile ff;
    if (!ff.load(in)) { fprintf(stderr, "tvr: cannot read %s\n", in); return 2; }
    const std::vector<float> &k1 = ff.F("kp1"), &k2 = ff.F("kp2"), &cam = ff.F("cam");
    std::vector<cv::KeyPoint> vKeys1(k1.size() / 2), vKeys2(k2.size() / 2);
    for (size_t i = 0; i < vKeys1.size(); i++) vKeys1[i].pt = cv::Point2f(k1[2 * i], k1[2 * i + 1]);
    for (size_t i = 0; i < vKeys2.size(); i++) vKeys2[i].pt = cv::Point2f(k2[2 * i], k2[2 * i + 1]);
    std::vector<int> vMatches12(ff.I("matches").begin(), ff.I("matches").end());
    GeometricCamera camera(cam, (unsigned)ff.I("cam_type")[0]);
    cv::Mat R21, t21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTriangulated;
    const bool ok = camera.ReconstructWithTwoViews(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated);
    FlatWriter w(out);
    w.one("ok", ok ? 1 : 0);
    std::vector<float> R, t, P;
    if (!R21.empty()) for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.push_back(R21.at<float>(i, j));
    if (!t21.empty()) for (int i = 0; i < 3; i++) t.push_back(t21.at<float>(i));
    for (const cv::Point3f &p : vP3D) { P.push_back(p.x); P.push_back(p.y); P.push_back(p.z); }
    std::vector<int32_t> tri(vbTriangulated.begin(), vbTriangulated.end()), sizes = {(int32_t)vP3D.size(), (int32_t)vbTriangulated.size(), (int32_t)vKeys1.size()};
    w.floats("R21", R); w.floats("t21", t); w.floats("P3D", P); w.ints("tri", tri); w.ints("sizes", sizes);
    std::vector<float> un1;
    for (const cv::Point2f &q : camera.UndistortToPinhole(vKeys1)) { un1.push_back(q.x); un1.push_back(q.y); }
    w.floats("un1", un1);
    std::vector<int32_t> sets;
    for (const std::vector<size_t> &s : camera.LastSets()) for (size_t v : s) sets.push_back((int32_t)v);
    w.ints("sets", sets);
    printf("tvr: %zu + %zu keypoints, ok %d\n", vKeys1.size(), vKeys2.size(), ok ? 1 : 0);
    return 0;
}
