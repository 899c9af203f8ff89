// Optimizer_OptimizeEssentialGraph.cc -- void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
// LoopConnections, bFixScale) with the reference's signature (include/Optimizer.h:79-82, src/Optimizer.cc:2347-2663) around the HIP
// solver.  LoopClosing::CorrectLoop calls it (src/LoopClosing.cc:1223).  Host side, in the reference's order: the vertices of :2379-2415
// (one per keyframe that is not bad, CorrectedSim3 or Sim3(Rcw, tcw, 1), the map's first keyframe fixed), the LoopConnections edges of
// :2424-2452 (minFeat = 100 and its exception for the (current, loop) pair, measured on vScw), then per keyframe the spanning-tree edge,
// older loop edges, covisibility edges and the mPrevKF edge of :2459-2588 (measured on NonCorrectedSim3 where an endpoint has an entry)
// fill ONE orbhip_pose_graph; what was g2o (optimize(20), :2596-2601) is one call of orbhip_optimize_essential_graph_host; then, under
// mMutexMapUpdate, the map points through orbhip_pose_graph_correct_points_host (:2629-2659, one blob each way; a refusal there leaves
// the map unchanged), SetPose([R | t/s]) and vCorrectedSwc (:2606-2626), UpdateNormalAndDepth, IncreaseChangeIndex (:2662).
// Three deliberate departures: an edge whose endpoint has no vertex (a bad keyframe) is left out with one message (the reference hands
// optimizer.vertex(id) == NULL to HyperGraph::addEdge, which dereferences it); bad keyframes are skipped in the write-back (the reference
// dereferences their NULL vertex at :2613); without a usable GPU, or when the solver refuses the map (more than 585 free keyframes), one
// message and nothing changes.
#include "Optimizer.h"
#include <algorithm>
#include <cstdio>
#include <vector>
#include "optimizer_common.h"

namespace ORB_SLAM3 {

using namespace optc;

namespace {
void put(std::vector<double> &v, const g2o::Sim3 &S)
{
    const double e[8] = {S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(), S.translation()[0], S.translation()[1], S.translation()[2], S.scale()};
    v.insert(v.end(), e, e + 8);
}
g2o::Sim3 get(const double *e)
{
    Eigen::Vector3d t;
    t[0] = e[4]; t[1] = e[5]; t[2] = e[6];
    return g2o::Sim3(Eigen::Quaterniond(e[3], e[0], e[1], e[2]), t, e[7]);
}
}  // namespace

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                       const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections, const bool &bFixScale)
{
    // no usable GPU: one message (hip::ThreadContext prints it), nothing touched, no CPU fallback
    orbhip_ctx *ctx = thread_ctx();
    if (!ctx) return;

    const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();

    long unsigned int nMaxKFid = pMap->GetMaxKFid();
    for (KeyFrame *pKF : vpKFs) nMaxKFid = std::max(nMaxKFid, pKF->mnId);

    std::vector<g2o::Sim3> vScw(nMaxKFid + 1);
    std::vector<int32_t> vertexOf(nMaxKFid + 1, -1);                      // keyframe id -> vertex (the reference's vpVertices)
    const int minFeat = 100;

    // Set KeyFrame vertices (:2379-2415)
    std::vector<uint8_t> fixed;
    std::vector<double> sim3;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) vScw[nIDi] = it->second;
        else {
            Eigen::Matrix<double, 3, 3> Rcw = Converter::toMatrix3d(pKF->GetRotation());
            Eigen::Matrix<double, 3, 1> tcw = Converter::toVector3d(pKF->GetTranslation());
            vScw[nIDi] = g2o::Sim3(Rcw, tcw, 1.0);
        }
        vertexOf[nIDi] = (int32_t)fixed.size();
        fixed.push_back(pKF->mnId == pMap->GetInitKFid() ? 1 : 0);
        put(sim3, vScw[nIDi]);
    }

    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    std::vector<int32_t> v0, v1;
    std::vector<double> meas;
    int nLeftOut = 0;
    auto addEdge = [&](long unsigned int nIDi, long unsigned int nIDj, const g2o::Sim3 &Sji) {     // vertex(0) = i, vertex(1) = j
        if (nIDi > nMaxKFid || nIDj > nMaxKFid || vertexOf[nIDi] < 0 || vertexOf[nIDj] < 0) { nLeftOut++; return; }
        v0.push_back(vertexOf[nIDi]); v1.push_back(vertexOf[nIDj]); put(meas, Sji);
    };
    auto nonCorrected = [&](KeyFrame *pKF) -> g2o::Sim3 {                  // NonCorrectedSim3[pKF] if present, else vScw
        LoopClosing::KeyFrameAndPose::const_iterator it = NonCorrectedSim3.find(pKF);
        if (it != NonCorrectedSim3.end()) return it->second;
        return pKF->mnId <= nMaxKFid ? vScw[pKF->mnId] : g2o::Sim3();
    };

    // Set Loop edges (:2424-2452)
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame*> &spConnections = mit->second;
        const g2o::Sim3 Siw = nIDi <= nMaxKFid ? vScw[nIDi] : g2o::Sim3();
        const g2o::Sim3 Swi = Siw.inverse();
        for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const g2o::Sim3 Sjw = nIDj <= nMaxKFid ? vScw[nIDj] : g2o::Sim3();
            addEdge(nIDi, nIDj, Sjw * Swi);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // Set normal edges (:2459-2588)
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        const long unsigned int nIDi = pKF->mnId;
        const g2o::Sim3 Swi = nonCorrected(pKF).inverse();
        KeyFrame *pParentKF = pKF->GetParent();
        if (pParentKF) addEdge(nIDi, pParentKF->mnId, nonCorrected(pParentKF) * Swi);            // Spanning tree edge
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();                              // Loop edges
        for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame *pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) addEdge(nIDi, pLKF->mnId, nonCorrected(pLKF) * Swi);
        }
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);       // Covisibility graph edges
        for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    addEdge(nIDi, pKFn->mnId, nonCorrected(pKFn) * Swi);
                }
            }
        }
        if (pKF->bImu && pKF->mPrevKF) addEdge(nIDi, pKF->mPrevKF->mnId, nonCorrected(pKF->mPrevKF) * Swi);      // Inertial edges if inertial
    }
    if (nLeftOut) fprintf(stderr, "Optimizer::OptimizeEssentialGraph: %d edges with a bad keyframe at one end left out\n", nLeftOut);

    // Optimize! (:2596-2601)
    orbhip_pose_graph graph;
    graph.n_vertices = (int32_t)fixed.size(); graph.fixed = fixed.data();
    graph.n_edges = (int32_t)v0.size(); graph.edge_v0 = v0.data(); graph.edge_v1 = v1.data(); graph.edge_meas = meas.data();
    orbhip_pose_graph_params params;
    orbhip_pose_graph_default_params(&params);
    params.fix_scale = bFixScale ? 1 : 0;
    std::vector<double> est = sim3;
    double *pest = est.data();
    orbhip_pose_graph_stats stats;
    const int rc = orbhip_optimize_essential_graph_host(ctx, &graph, 1, &params, &pest, &stats, NULL);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "Optimizer::OptimizeEssentialGraph: %s (%d); the map is unchanged, there is no CPU fallback\n", orbhip_last_error(), rc);
        return;
    }

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);          // :2603: everything below runs under it, as in the reference

    // the points' correction on the device: positions as they are now, Scw = vScw, corrected_Swc = estimate^-1 (:2629-2655)
    std::vector<double> Swc;
    for (size_t v = 0; v < fixed.size(); v++) put(Swc, get(&est[8 * v]).inverse());
    std::vector<float> Xw(3 * vpMPs.size(), 0.f), Xout(3 * vpMPs.size(), 0.f);
    std::vector<int32_t> ref(vpMPs.size(), -1);
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        ref[i] = nIDr <= nMaxKFid ? vertexOf[nIDr] : -1;             // no vertex: the reference maps through two default Sim3, the identity
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) Xw[3 * i + k] = P3Dw.at<float>(k);
    }
    const int rc2 = orbhip_pose_graph_correct_points_host(ctx, Xw.data(), ref.data(), (int)vpMPs.size(), sim3.data(), Swc.data(), (int)fixed.size(), Xout.data());
    if (rc2 != ORBHIP_OK) {
        fprintf(stderr, "Optimizer::OptimizeEssentialGraph: %s (%d); the map is unchanged, there is no CPU fallback\n", orbhip_last_error(), rc2);
        return;
    }

    // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1] (:2606-2626)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKFi = vpKFs[i];
        if (pKFi->isBad()) continue;
        const g2o::Sim3 CorrectedSiw = get(&est[8 * (size_t)vertexOf[pKFi->mnId]]);
        Eigen::Matrix3d eigR = CorrectedSiw.rotation().toRotationMatrix();
        Eigen::Vector3d eigt = CorrectedSiw.translation();
        const double s = CorrectedSiw.scale();
        for (int k = 0; k < 3; k++) eigt[k] *= (1. / s);             // [R t/s;0 1]
        pKFi->SetPose(Converter::toCvSE3(eigR, eigt));
    }

    // Correct points (:2629-2659)
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) cvCorrectedP3Dw.at<float>(k) = Xout[3 * i + k];
        pMP->SetWorldPos(cvCorrectedP3Dw);
        pMP->UpdateNormalAndDepth();
    }

    pMap->IncreaseChangeIndex();
}

}  // namespace ORB_SLAM3
