// compile_callers_imu_init.cc -- compile-only check of the drop-in claim for the inertial initialisation: the call lines of the
// reference's src/LocalMapping.cc:1306 (LocalMapping::InitializeIMU), :1425-1428 (LocalMapping::ScaleRefinement) and
// src/LoopClosing.cc:2020-2026 (the inertial map merge) against host/Optimizer.h and the Eigen / IMU stand-ins of host/slam_types.h.
// Nothing here runs.  Built by `make lib/compile_callers_imu_init.o` with -Wall -Werror, asserted by tests/test_inertial_opt_abi.py.
#include <vector>
#include "Optimizer.h"

using namespace std;

namespace ORB_SLAM3 {

struct LocalMappingImuState {             // the members of LocalMapping the call lines mention (include/LocalMapping.h:85-88, :171)
    Atlas *mpAtlas;
    Eigen::Matrix3d mRwg;
    Eigen::Vector3d mbg, mba;
    double mScale;
    bool mbMonocular;
    Eigen::MatrixXd infoInertial;
};

// LocalMapping::InitializeIMU, :1301-1306
void local_mapping_initialize_imu(LocalMappingImuState &S, float priorG, float priorA)
{
    Atlas *mpAtlas = S.mpAtlas; Eigen::Matrix3d &mRwg = S.mRwg; Eigen::Vector3d &mbg = S.mbg, &mba = S.mba; double &mScale = S.mScale;
    const bool mbMonocular = S.mbMonocular; Eigen::MatrixXd &infoInertial = S.infoInertial;

    mScale=1.0;

    Optimizer::InertialOptimization(mpAtlas->GetCurrentMap(), mRwg, mScale, mbg, mba, mbMonocular, infoInertial, false, false, priorG, priorA);
}

// LocalMapping::ScaleRefinement, :1425-1428
void local_mapping_scale_refinement(LocalMappingImuState &S)
{
    Atlas *mpAtlas = S.mpAtlas; Eigen::Matrix3d &mRwg = S.mRwg; double &mScale = S.mScale;

    mRwg = Eigen::Matrix3d::Identity();
    mScale=1.0;

    Optimizer::InertialOptimization(mpAtlas->GetCurrentMap(), mRwg, mScale);
}

// LoopClosing::MergeLocal2, :2020-2026
IMU::Bias loop_closing_merge_inertial(Map *pCurrentMap)
{
        Eigen::Vector3d bg, ba;
        bg << 0., 0., 0.;
        ba << 0., 0., 0.;
        Optimizer::InertialOptimization(pCurrentMap,bg,ba);
        IMU::Bias b (ba[0],ba[1],ba[2],bg[0],bg[1],bg[2]);

    return b;
}

// the keyframe-list overload (include/Optimizer.h:117) is not called from those three places; its declaration is held to the same signature
void keyframe_list_overload(vector<KeyFrame*> vpKFs, Eigen::Vector3d &bg, Eigen::Vector3d &ba)
{
    Optimizer::InertialOptimization(vpKFs, bg, ba);
    Optimizer::InertialOptimization(vpKFs, bg, ba, 1e2, 1e6);
}

}  // namespace ORB_SLAM3
