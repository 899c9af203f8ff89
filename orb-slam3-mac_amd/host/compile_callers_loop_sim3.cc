// compile_callers_loop_sim3.cc -- compile-only check of the drop-in claim for Sim3Solver: the lines of the reference's
// src/LoopClosing.cc:669-684 and :720 (LoopClosing::DetectCommonRegionsFromBoW) against host/Sim3Solver.h and the g2o::Sim3 / Eigen /
// Converter stand-ins of host/slam_types.h.  Nothing here runs.  Built by `make lib/compile_callers_loop_sim3.o` with -Wall -Werror,
// asserted by tests/test_sim3_solver_abi.py.
#include <vector>
#include "Sim3Solver.h"

using namespace std;

namespace ORB_SLAM3 {

struct TrackingSensor { int mSensor; };

struct LoopClosingState {                 // the members of LoopClosing the lines mention
    KeyFrame *mpCurrentKF;
    TrackingSensor *mpTracker;
    bool mbFixScale;
};

// LoopClosing::DetectCommonRegionsFromBoW, :669-684 and :720
g2o::Sim3 loop_closing_geometric_validation(LoopClosingState &S, KeyFrame *pMostBoWMatchesKF, vector<MapPoint*> &vpMatchedPoints,
                                            vector<KeyFrame*> &vpKeyFrameMatchedMP, int nBoWInliers, bool &bConverged)
{
    KeyFrame *mpCurrentKF = S.mpCurrentKF; TrackingSensor *mpTracker = S.mpTracker; const bool mbFixScale = S.mbFixScale;

            bool bFixedScale = mbFixScale;
            if(mpTracker->mSensor==System::IMU_MONOCULAR && !mpCurrentKF->GetMap()->GetIniertialBA2())
                bFixedScale=false;

            Sim3Solver solver = Sim3Solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints, bFixedScale, vpKeyFrameMatchedMP);
            solver.SetRansacParameters(0.99, nBoWInliers, 300); // at least 15 inliers

            bool bNoMore = false;
            vector<bool> vbInliers;
            int nInliers;
            bool bConverge = false;
            cv::Mat mTcm;
            while(!bConverge && !bNoMore)
            {
                mTcm = solver.iterate(20,bNoMore, vbInliers, nInliers, bConverge);
            }

                g2o::Sim3 gScm(Converter::toMatrix3d(solver.GetEstimatedRotation()),Converter::toVector3d(solver.GetEstimatedTranslation()),solver.GetEstimatedScale());

    bConverged = bConverge;
    return gScm;
}

}  // namespace ORB_SLAM3
