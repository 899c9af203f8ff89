// compile_callers_loop.cc -- compile-only check of the drop-in claim for the Sim3 refinement: the call lines of the reference's
// src/LoopClosing.cc:523-532 (LoopClosing::DetectAndReffineSim3FromLastKF) and :736-742 (LoopClosing::DetectCommonRegionsFromBoW)
// against host/Optimizer.h and the g2o::Sim3 / Eigen / Converter stand-ins of host/slam_types.h.  Nothing here runs.  Built by
// `make lib/compile_callers_loop.o` with -Wall -Werror, asserted by tests/test_sim3_opt_abi.py.
#include <vector>
#include "Optimizer.h"

using namespace std;

namespace ORB_SLAM3 {

struct TrackingSensor { int mSensor; };

struct LoopClosingState {                 // the members of LoopClosing the call lines mention
    KeyFrame *mpCurrentKF;
    TrackingSensor *mpTracker;
    bool mbFixScale;
};

// LoopClosing::DetectAndReffineSim3FromLastKF, :523-532
int loop_closing_refine_from_last_kf(LoopClosingState &S, KeyFrame *pCurrentKF, KeyFrame *pMatchedKF, g2o::Sim3 &gScw, vector<MapPoint*> &vpMatchedMPs)
{
    KeyFrame *mpCurrentKF = S.mpCurrentKF; TrackingSensor *mpTracker = S.mpTracker; const bool mbFixScale = S.mbFixScale;

        cv::Mat mScw = Converter::toCvMat(gScw);
        cv::Mat mTwm = pMatchedKF->GetPoseInverse();
        g2o::Sim3 gSwm(Converter::toMatrix3d(mTwm.rowRange(0, 3).colRange(0, 3)),Converter::toVector3d(mTwm.rowRange(0, 3).col(3)),1.0);
        g2o::Sim3 gScm = gScw * gSwm;
        Eigen::Matrix<double, 7, 7> mHessian7x7;

        bool bFixedScale = mbFixScale;       // TODO CHECK; Solo para el monocular inertial
        if(mpTracker->mSensor==System::IMU_MONOCULAR && !pCurrentKF->GetMap()->GetIniertialBA2())
            bFixedScale=false;
        int numOptMatches = Optimizer::OptimizeSim3(mpCurrentKF, pMatchedKF, vpMatchedMPs, gScm, 10, bFixedScale, mHessian7x7, true);

    (void)mScw;
    return numOptMatches;
}

// LoopClosing::DetectCommonRegionsFromBoW, :736-742
int loop_closing_common_regions_from_bow(LoopClosingState &S, KeyFrame *pKFi, g2o::Sim3 &gScm, vector<MapPoint*> &vpMatchedMP)
{
    KeyFrame *mpCurrentKF = S.mpCurrentKF; TrackingSensor *mpTracker = S.mpTracker; const bool mbFixScale = S.mbFixScale;

                    Eigen::Matrix<double, 7, 7> mHessian7x7;

                    bool bFixedScale = mbFixScale;
                    if(mpTracker->mSensor==System::IMU_MONOCULAR && !mpCurrentKF->GetMap()->GetIniertialBA2())
                        bFixedScale=false;

                    int numOptMatches = Optimizer::OptimizeSim3(mpCurrentKF, pKFi, vpMatchedMP, gScm, 10, mbFixScale, mHessian7x7, true);

    (void)bFixedScale;
    return numOptMatches;
}

}  // namespace ORB_SLAM3
