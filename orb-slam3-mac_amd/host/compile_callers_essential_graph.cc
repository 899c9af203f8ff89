// compile_callers_essential_graph.cc -- compile-only check of the drop-in claim for the essential-graph optimisation: the call line of the
// reference's src/LoopClosing.cc:1223 (LoopClosing::CorrectLoop, the 7-DoF branch) with the declarations it needs (:1131-1135, :1197)
// against host/Optimizer.h and the g2o::Sim3 / LoopClosing::KeyFrameAndPose stand-ins of host/slam_types.h.  Nothing here runs.  Built by
// `make lib/compile_callers_essential_graph.o` with -Wall -Werror, asserted by tests/test_essential_graph_abi.py.
#include <map>
#include <set>
#include "Optimizer.h"

using namespace std;

namespace ORB_SLAM3 {

struct LoopClosingCorrectLoopState {       // the members of LoopClosing the call line mentions
    KeyFrame *mpCurrentKF, *mpLoopMatchedKF;
    bool mbFixScale;
};

// LoopClosing::CorrectLoop, :1223
void loop_closing_correct_loop(LoopClosingCorrectLoopState &S, LoopClosing::KeyFrameAndPose &CorrectedSim3, LoopClosing::KeyFrameAndPose &NonCorrectedSim3)
{
    KeyFrame *mpCurrentKF = S.mpCurrentKF, *mpLoopMatchedKF = S.mpLoopMatchedKF;
    Map* pLoopMap = mpCurrentKF->GetMap();
    map<KeyFrame*, set<KeyFrame*> > LoopConnections;
    bool bFixedScale = S.mbFixScale;

    if(pLoopMap->IsInertial() && pLoopMap->isImuInitialized())
    {
    }
    else
    {
        Optimizer::OptimizeEssentialGraph(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixedScale);
    }
}

}  // namespace ORB_SLAM3
