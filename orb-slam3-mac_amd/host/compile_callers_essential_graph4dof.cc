// compile_callers_essential_graph4dof.cc -- compile-only check of the drop-in claim for the 4-DoF essential-graph optimisation: the call
// line of the reference's src/LoopClosing.cc:1218 (LoopClosing::CorrectLoop, the branch of an inertial map whose IMU is initialised) with
// the declarations it needs (:1131-1135, :1197) against host/Optimizer.h and the g2o::Sim3 / LoopClosing::KeyFrameAndPose stand-ins of
// host/slam_types.h.  Nothing here runs.  Built by `make lib/compile_callers_essential_graph4dof.o` with -Wall -Werror, asserted by
// tests/test_essential_graph4dof_abi.py.
#include <map>
#include <set>
#include "Optimizer.h"

using namespace std;

namespace ORB_SLAM3 {

struct LoopClosingCorrectLoop4DoFState {   // the members of LoopClosing the call line mentions
    KeyFrame *mpCurrentKF, *mpLoopMatchedKF;
};

// LoopClosing::CorrectLoop, :1215-1219
void loop_closing_correct_loop_4dof(LoopClosingCorrectLoop4DoFState &S, LoopClosing::KeyFrameAndPose &CorrectedSim3, LoopClosing::KeyFrameAndPose &NonCorrectedSim3)
{
    KeyFrame *mpCurrentKF = S.mpCurrentKF, *mpLoopMatchedKF = S.mpLoopMatchedKF;
    Map* pLoopMap = mpCurrentKF->GetMap();
    map<KeyFrame*, set<KeyFrame*> > LoopConnections;

    if(pLoopMap->IsInertial() && pLoopMap->isImuInitialized())
    {
        Optimizer::OptimizeEssentialGraph4DoF(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections);
    }
}

}  // namespace ORB_SLAM3
