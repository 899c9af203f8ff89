// Optimizer_OptimizeEssentialGraph4DoF.cc -- void Optimizer::OptimizeEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3,
// CorrectedSim3, LoopConnections) with the reference's signature (include/Optimizer.h:84-87, src/Optimizer.cc:8305-8610) around the HIP
// solver.  LoopClosing::CorrectLoop calls it for an inertial map whose IMU is initialised (src/LoopClosing.cc:1218).  Host side, in the
// reference's order: the vertices of :8335-8372 (one per keyframe that is not bad; ImuCamPose(Rwc, twc, pKF) from a CorrectedSim3 entry,
// src/G2oTypes.cc:121-146, else ImuCamPose(pKF), :24-71; the loop keyframe fixed), the LoopConnections edges of :8385-8416 (minFeat = 100
// and its exception for the (current, loop) pair, measured on vScw), then per keyframe the mPrevKF edge, older loop edges and
// covisibility edges of :8420-8557 (measured on NonCorrectedSim3 where an endpoint has an entry; pParentKF is NULL there, so there is no
// spanning-tree edge) fill ONE orbhip_pose_graph4dof; what was g2o (optimize(20), :8560-8562) is one call of
// orbhip_optimize_essential_graph4dof_host with the information diag(1e3, 1e3, 1, 1, 1, 1) of :8378-8381; then, under mMutexMapUpdate,
// the map points through orbhip_pose_graph_correct_points_host with Sim3(R, t, 1) rows (:8585-8608, through the reference keyframe; a
// refusal there leaves the map unchanged), SetPose([R | t]) (:8567-8582), UpdateNormalAndDepth, IncreaseChangeIndex (:8609).
// Three deliberate departures, those of Optimizer_OptimizeEssentialGraph.cc: a bad keyframe has no vertex, and an edge that touches one
// is left out with one message (the reference hands optimizer.vertex(id) == NULL to HyperGraph::addEdge, which dereferences it); bad
// keyframes are skipped in the write-back (the reference dereferences their NULL vertex at :8574); without a usable GPU, or when the
// solver refuses the map (more than 1024 free keyframes), one message and nothing changes.
#include "Optimizer.h"
#include <algorithm>
#include <cstdio>
#include <vector>
#include "optimizer_common.h"

namespace ORB_SLAM3 {

using namespace optc;

namespace {
typedef Eigen::Matrix3d M3;
typedef Eigen::Vector3d V3;
M3 mul(const M3 &A, const M3 &B)
{
    M3 C;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C(i, j) = A(i, 0) * B(0, j) + A(i, 1) * B(1, j) + A(i, 2) * B(2, j);
    return C;
}
V3 mul(const M3 &A, const V3 &v)
{
    V3 o;
    for (int i = 0; i < 3; i++) o[i] = A(i, 0) * v[0] + A(i, 1) * v[1] + A(i, 2) * v[2];
    return o;
}
M3 transpose(const M3 &A)
{
    M3 T;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T(i, j) = A(j, i);
    return T;
}
void put(std::vector<double> &v, const M3 &R) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) v.push_back(R(i, j)); }
void put(std::vector<double> &v, const V3 &t) { for (int i = 0; i < 3; i++) v.push_back(t[i]); }
void put(std::vector<double> &v, const g2o::Sim3 &S)
{
    const double e[8] = {S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(), S.translation()[0], S.translation()[1], S.translation()[2], S.scale()};
    v.insert(v.end(), e, e + 8);
}
}  // namespace

void Optimizer::OptimizeEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                           const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                           const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                           const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections)
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

    // Set KeyFrame vertices (:8335-8372): Rwb twb Rcw tcw Rcb tcb per vertex
    std::vector<uint8_t> fixed;
    std::vector<double> state;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        const V3 tcb = Converter::toVector3d(pKF->mImuCalib.Tcb.rowRange(0, 3).col(3));
        const M3 Rcb = Converter::toMatrix3d(pKF->mImuCalib.Tcb.rowRange(0, 3).colRange(0, 3));
        M3 Rwb, Rcw;
        V3 twb, tcw;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            vScw[nIDi] = it->second;
            const g2o::Sim3 Swc = it->second.inverse();
            const M3 Rwc = Swc.rotation().toRotationMatrix();
            const V3 twc = Swc.translation();
            twb = mul(Rwc, tcb);                                          // ImuCamPose(_Rwc, _twc, pKF)
            for (int k = 0; k < 3; k++) twb[k] += twc[k];
            Rwb = mul(Rwc, Rcb);
            Rcw = transpose(Rwc);
            tcw = mul(Rcw, twc);
            for (int k = 0; k < 3; k++) tcw[k] = -tcw[k];
        } else {
            Rcw = Converter::toMatrix3d(pKF->GetRotation());
            tcw = Converter::toVector3d(pKF->GetTranslation());
            vScw[nIDi] = g2o::Sim3(Rcw, tcw, 1.0);
            twb = Converter::toVector3d(pKF->GetImuPosition());          // ImuCamPose(pKF)
            Rwb = Converter::toMatrix3d(pKF->GetImuRotation());
        }
        vertexOf[nIDi] = (int32_t)fixed.size();
        fixed.push_back(pKF == pLoopKF ? 1 : 0);
        put(state, Rwb); put(state, twb); put(state, Rcw); put(state, tcw); put(state, Rcb); put(state, tcb);
    }

    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    std::vector<int32_t> v0, v1;
    std::vector<double> meas;
    int nLeftOut = 0;
    auto addEdge = [&](long unsigned int nIDi, long unsigned int nIDj, const g2o::Sim3 &Sij) {     // vertex(0) = i, vertex(1) = j; Tij = [R | t] of Sij
        if (nIDi > nMaxKFid || nIDj > nMaxKFid || vertexOf[nIDi] < 0 || vertexOf[nIDj] < 0) { nLeftOut++; return; }
        v0.push_back(vertexOf[nIDi]); v1.push_back(vertexOf[nIDj]);
        put(meas, Sij.rotation().toRotationMatrix()); put(meas, Sij.translation());
    };
    auto nonCorrected = [&](KeyFrame *pKF) -> g2o::Sim3 {                  // NonCorrectedSim3[pKF] if present, else vScw
        LoopClosing::KeyFrameAndPose::const_iterator it = NonCorrectedSim3.find(pKF);
        if (it != NonCorrectedSim3.end()) return it->second;
        return pKF->mnId <= nMaxKFid ? vScw[pKF->mnId] : g2o::Sim3();
    };

    // Set Loop edges (:8385-8416)
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame*> &spConnections = mit->second;
        const g2o::Sim3 Siw = nIDi <= nMaxKFid ? vScw[nIDi] : g2o::Sim3();
        for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const g2o::Sim3 Sjw = nIDj <= nMaxKFid ? vScw[nIDj] : g2o::Sim3();
            addEdge(nIDi, nIDj, Siw * Sjw.inverse());
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // 1. Set normal edges (:8420-8557)
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame *pKF = vpKFs[i];
        const long unsigned int nIDi = pKF->mnId;
        const g2o::Sim3 Siw = nonCorrected(pKF);
        KeyFrame *pParentKF = static_cast<KeyFrame*>(NULL);                                      // 1.1.0: no spanning tree edge (:8438)
        KeyFrame *prevKF = pKF->mPrevKF;                                                         // 1.1.1 Inertial edges
        if (prevKF) addEdge(nIDi, prevKF->mnId, Siw * nonCorrected(prevKF).inverse());
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();                              // 1.2 Loop edges
        for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame *pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) addEdge(nIDi, pLKF->mnId, Siw * nonCorrected(pLKF).inverse());
        }
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);       // 1.3 Covisibility graph edges
        for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame *pKFn = *vit;
            if (pKFn && pKFn != pParentKF && pKFn != prevKF && pKFn != pKF->mNextKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    addEdge(nIDi, pKFn->mnId, Siw * nonCorrected(pKFn).inverse());
                }
            }
        }
    }
    if (nLeftOut) fprintf(stderr, "Optimizer::OptimizeEssentialGraph4DoF: %d edges with a bad keyframe at one end left out\n", nLeftOut);

    // optimizer.optimize(20) (:8560-8562)
    orbhip_pose_graph4dof graph;
    graph.n_vertices = (int32_t)fixed.size(); graph.fixed = fixed.data();
    graph.n_edges = (int32_t)v0.size(); graph.edge_v0 = v0.data(); graph.edge_v1 = v1.data(); graph.edge_meas = meas.data();
    orbhip_pose_graph4dof_params params;
    orbhip_pose_graph4dof_default_params(&params);                         // matLambda of :8378-8381 is the default
    std::vector<double> est = state;
    double *pest = est.data();
    orbhip_pose_graph_stats stats;
    const int rc = orbhip_optimize_essential_graph4dof_host(ctx, &graph, 1, &params, &pest, &stats, NULL);
    if (rc != ORBHIP_OK) {
        fprintf(stderr, "Optimizer::OptimizeEssentialGraph4DoF: %s (%d); the map is unchanged, there is no CPU fallback\n", orbhip_last_error(), rc);
        return;
    }

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);          // :8564: everything below runs under it, as in the reference

    // the optimised [R | t] per vertex, CorrectedSiw = Sim3(Ri, ti, 1) and its inverse (:8573-8578)
    std::vector<M3> vR(fixed.size());
    std::vector<V3> vt(fixed.size());
    std::vector<double> Scw, Swc;
    for (size_t v = 0; v < fixed.size(); v++) {
        const double *e = &est[ORBHIP_PG4_STATE * v];
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) vR[v](i, j) = e[12 + 3 * i + j]; vt[v][i] = e[21 + i]; }
        put(Swc, g2o::Sim3(vR[v], vt[v], 1.).inverse());
    }
    for (size_t i = 0; i < vpKFs.size(); i++) if (!vpKFs[i]->isBad()) put(Scw, vScw[vpKFs[i]->mnId]);      // vertex order

    // the points' correction on the device: positions as they are now, through the reference keyframe (:8585-8606)
    std::vector<float> Xw(3 * vpMPs.size(), 0.f), Xout(3 * vpMPs.size(), 0.f);
    std::vector<int32_t> ref(vpMPs.size(), -1);
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        const long unsigned int nIDr = pMP->GetReferenceKeyFrame()->mnId;
        ref[i] = nIDr <= nMaxKFid ? vertexOf[nIDr] : -1;             // no vertex: the reference maps through two default Sim3, the identity
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) Xw[3 * i + k] = P3Dw.at<float>(k);
    }
    const int rc2 = orbhip_pose_graph_correct_points_host(ctx, Xw.data(), ref.data(), (int)vpMPs.size(), Scw.data(), Swc.data(), (int)fixed.size(), Xout.data());
    if (rc2 != ORBHIP_OK) {
        fprintf(stderr, "Optimizer::OptimizeEssentialGraph4DoF: %s (%d); the map is unchanged, there is no CPU fallback\n", orbhip_last_error(), rc2);
        return;
    }

    // SE3 Pose Recovering (:8567-8582)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKFi = vpKFs[i];
        if (pKFi->isBad()) continue;
        const int32_t v = vertexOf[pKFi->mnId];
        pKFi->SetPose(Converter::toCvSE3(vR[v], vt[v]));
    }

    // Correct points (:8585-8608)
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
