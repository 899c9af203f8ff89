// Optimizer.h -- signature-preserving host mirror of the ORB_SLAM3::Optimizer entry points on the hot path
// (reference include/Optimizer.h:58, :62, :90, :98, :104).  LocalMapping (src/LocalMapping.cc:154) calls it unchanged.
#pragma once
#include <vector>
#include "slam_types.h"

namespace ORB_SLAM3 {

class Optimizer {
public:
    // reference include/Optimizer.h:62, src/Optimizer.cc:854-1168 (Tracking.cc:1775, 1934, 1996, 2002, 2727, 2743)
    int static PoseOptimization(Frame *pFrame);
    // reference include/Optimizer.h:104, src/Optimizer.cc:6255-6911: local BA of the map-merge welding window (LoopClosing::MergeLocal)
    void static LocalBundleAdjustment(KeyFrame *pMainKF, std::vector<KeyFrame *> vpAdjustKF, std::vector<KeyFrame *> vpFixedKF, bool *pbStopFlag);
    // reference include/Optimizer.h:58, src/Optimizer.cc:1699-2344
    void static LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, int &num_fixedKF);
    // reference include/Optimizer.h:98, src/Optimizer.cc:4574-5187 (LocalMapping.cc:131-155 once the IMU is initialised)
    void static LocalInertialBA(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, bool bLarge = false, bool bRecInit = false);
    // reference include/Optimizer.h:90, src/Optimizer.cc:3932-4328 (LoopClosing.cc:532, :742); the overloads at :3734 and :4330 have no callers
    static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale, Eigen::Matrix<double, 7, 7> &mAcumHessian, const bool bAllPoints = false);
    // reference include/Optimizer.h:115-118, src/Optimizer.cc:5303-5908: the inertial-only solve of LocalMapping::InitializeIMU
    // (src/LocalMapping.cc:1306), ScaleRefinement (:1428) and the inertial map merge (src/LoopClosing.cc:2026);
    // host/Optimizer_InertialOptimization.cc
    void static InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale, Eigen::Vector3d &bg, Eigen::Vector3d &ba, bool bMono, Eigen::MatrixXd  &covInertial, bool bFixedVel=false, bool bGauss=false, float priorG = 1e2, float priorA = 1e6);
    void static InertialOptimization(Map *pMap, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG = 1e2, float priorA = 1e6);
    void static InertialOptimization(std::vector<KeyFrame*> vpKFs, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG = 1e2, float priorA = 1e6);
    void static InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale);
    // reference include/Optimizer.h:55, src/Optimizer.cc:420-851: the visual-inertial BA of a whole map -- LocalMapping::InitializeIMU
    // (src/LocalMapping.cc:1347-1353) and the inertial global BA (src/LoopClosing.cc:2439); host/Optimizer_FullInertialBA.cc.  Maps of at
    // most 480 reduced unknowns (52 keyframes with bInit, 32 without); vSingVal and bHess are unread, as in the reference
    void static FullInertialBA(Map *pMap, int its, const bool bFixLocal=false, const unsigned long nLoopKF=0, bool *pbStopFlag=NULL, bool bInit=false, float priorG = 1e2, float priorA=1e6, Eigen::VectorXd *vSingVal = NULL, bool *bHess=NULL);
    // reference include/Optimizer.h:79-82, src/Optimizer.cc:2347-2663: the Sim3 pose graph of a loop closure (src/LoopClosing.cc:1223);
    // host/Optimizer_OptimizeEssentialGraph.cc.  Maps of at most 585 free keyframes
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                       const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections,
                                       const bool &bFixScale);
    // reference include/Optimizer.h:84-87, src/Optimizer.cc:8305-8610: the yaw + translation pose graph of a loop closure on an inertial
    // map whose IMU is initialised (src/LoopClosing.cc:1218); host/Optimizer_OptimizeEssentialGraph4DoF.cc.  Maps of at most 1024 free
    // keyframes
    void static OptimizeEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                           const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                           const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                           const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections);
};

}  // namespace ORB_SLAM3
