// host_essential_graph4dof_smoke.cc -- `host_essential_graph4dof_smoke <in> <out>`: Optimizer::OptimizeEssentialGraph4DoF (the class
// method, host/Optimizer_OptimizeEssentialGraph4DoF.cc) on a stand-in inertial map from a flat file.  Inputs: per keyframe, in the order
// Map::GetAllKeyFrames() returns them: kf_id, kf_bad, kf_parent (index, -1 none; sets the children), kf_prev (index of mPrevKF, -1 none),
// Tcw (4x4); Tcb (4x4, the IMU calibration of every keyframe); max_kf_id, cur, loop (indices); loop edges le_a, le_b (indices, set on
// both ends); covisibility cv_a, cv_b, cv_w (set on both ends; a keyframe's neighbours are ordered by weight, ties in file order);
// LoopConnections lc_a, lc_b; the pose tables sim_kf (indices), sim_c, sim_nc (8 doubles each as bytes: qx qy qz qw tx ty tz s); map
// points mp_pos (3 each), mp_ref (index of the reference keyframe), mp_bad.
// Outputs: Tcw per keyframe, mp_pos, mp_updates (UpdateNormalAndDepth calls), change (the map's change index).
// Runs without a GPU too (the method then prints one message and touches nothing).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "Optimizer.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

static cv::Mat mat(const float *v, int r, int c)
{
    cv::Mat M(r, c, CV_32F);
    for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) M.at<float>(i, j) = v[c * i + j];
    return M;
}
static g2o::Sim3 sim3_of(const uint8_t *bytes)
{
    double e[8];
    memcpy(e, bytes, sizeof(e));
    Eigen::Vector3d t;
    t[0] = e[4]; t[1] = e[5]; t[2] = e[6];
    return g2o::Sim3(Eigen::Quaterniond(e[3], e[0], e[1], e[2]), t, e[7]);
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: host_essential_graph4dof_smoke <in> <out>\n"); return 2; }
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "essential_graph4dof: cannot read %s\n", argv[1]); return 2; }
    const std::vector<int32_t> &id = ff.I("kf_id"), &bad = ff.I("kf_bad"), &par = ff.I("kf_parent"), &prev = ff.I("kf_prev");
    const size_t n = id.size();
    std::vector<float> camp = {500.f, 500.f, 320.f, 240.f};
    GeometricCamera camera(camp, 0u);
    Map map;
    map.mnMaxKFid = (long unsigned int)ff.I("max_kf_id")[0];
    map.mnInitKFid = (long unsigned int)id[0];
    map.mbIsInertial = true;
    const cv::Mat Tcb = mat(&ff.F("Tcb")[0], 4, 4);
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    for (size_t k = 0; k < n; k++) {
        kfs.emplace_back(new KeyFrame((long unsigned int)id[k], &map, camp[0], camp[1], camp[2], camp[3], 40.f, &camera));
        KeyFrame *kf = kfs.back().get();
        kf->SetPose(mat(&ff.F("Tcw")[16 * k], 4, 4));
        kf->mImuCalib.Tcb = Tcb.clone();
        kf->mbBad = bad[k] != 0;
        kf->bImu = true;
        map.mvpKeyFrames.push_back(kf);
    }
    map.nKeyFrames = n;
    for (size_t k = 0; k < n; k++) {
        if (par[k] >= 0) { kfs[k]->mpParent = kfs[par[k]].get(); kfs[par[k]]->mspChildrens.insert(kfs[k].get()); }
        if (prev[k] >= 0) { kfs[k]->mPrevKF = kfs[prev[k]].get(); kfs[prev[k]]->mNextKF = kfs[k].get(); }
    }
    const std::vector<int32_t> &lea = ff.I("le_a"), &leb = ff.I("le_b"), &cva = ff.I("cv_a"), &cvb = ff.I("cv_b"), &cvw = ff.I("cv_w");
    for (size_t e = 0; e < lea.size(); e++) { kfs[lea[e]]->mspLoopEdges.insert(kfs[leb[e]].get()); kfs[leb[e]]->mspLoopEdges.insert(kfs[lea[e]].get()); }
    for (size_t e = 0; e < cva.size(); e++) {
        KeyFrame *a = kfs[cva[e]].get(), *b = kfs[cvb[e]].get();
        a->mConnectedKeyFrameWeights[b] = cvw[e]; b->mConnectedKeyFrameWeights[a] = cvw[e];
        a->mvpOrderedConnectedKeyFrames.push_back(b); b->mvpOrderedConnectedKeyFrames.push_back(a);
    }
    for (auto &kf : kfs) {
        KeyFrame *p = kf.get();
        std::stable_sort(p->mvpOrderedConnectedKeyFrames.begin(), p->mvpOrderedConnectedKeyFrames.end(),
                         [p](KeyFrame *x, KeyFrame *y) { return p->GetWeight(x) > p->GetWeight(y); });
    }
    std::map<KeyFrame *, std::set<KeyFrame *>> LoopConnections;
    const std::vector<int32_t> &lca = ff.I("lc_a"), &lcb = ff.I("lc_b");
    for (size_t e = 0; e < lca.size(); e++) LoopConnections[kfs[lca[e]].get()].insert(kfs[lcb[e]].get());
    LoopClosing::KeyFrameAndPose Corrected, NonCorrected;
    const std::vector<int32_t> &skf = ff.I("sim_kf");
    for (size_t e = 0; e < skf.size(); e++) {
        Corrected[kfs[skf[e]].get()] = sim3_of(&ff.U("sim_c")[64 * e]);
        NonCorrected[kfs[skf[e]].get()] = sim3_of(&ff.U("sim_nc")[64 * e]);
    }
    const std::vector<float> &mpos = ff.F("mp_pos");
    const size_t L = mpos.size() / 3;
    std::vector<std::unique_ptr<MapPoint>> mps;
    for (size_t l = 0; l < L; l++) {
        mps.emplace_back(new MapPoint((long unsigned int)l, mat(&mpos[3 * l], 3, 1), &map));
        MapPoint *mp = mps.back().get();
        mp->mpRefKF = kfs[ff.I("mp_ref")[l]].get();
        mp->mbBad = ff.I("mp_bad")[l] != 0;
        map.mvpMapPoints.push_back(mp);
    }
    Optimizer::OptimizeEssentialGraph4DoF(&map, kfs[ff.I("loop")[0]].get(), kfs[ff.I("cur")[0]].get(), NonCorrected, Corrected, LoopConnections);

    FlatWriter w(argv[2]);
    std::vector<float> Tcw, pos;
    std::vector<int32_t> upd;
    for (size_t k = 0; k < n; k++) { const cv::Mat T = kfs[k]->GetPose(); for (int i = 0; i < 16; i++) Tcw.push_back(T.at<float>(i / 4, i % 4)); }
    for (size_t l = 0; l < L; l++) { const cv::Mat P = mps[l]->GetWorldPos(); for (int i = 0; i < 3; i++) pos.push_back(P.at<float>(i)); upd.push_back(mps[l]->nNormalUpdates); }
    w.floats("Tcw", Tcw); w.floats("mp_pos", pos); w.ints("mp_updates", upd); w.one("change", map.mnMapChange);
    printf("essential_graph4dof: %zu keyframes, %zu points, change index %d\n", n, L, map.mnMapChange);
    return 0;
}
