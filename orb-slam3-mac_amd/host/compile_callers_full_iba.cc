// compile_callers_full_iba.cc -- compile-only check of the drop-in claim for the full inertial BA: the call lines of the reference's
// src/LocalMapping.cc:1347-1353 (LocalMapping::InitializeIMU) and src/LoopClosing.cc:2439 (LoopClosing::RunGlobalBundleAdjustment)
// against host/Optimizer.h and the stand-ins of host/slam_types.h.  Nothing here runs.  Built by `make lib/compile_callers_full_iba.o`
// with -Wall -Werror, asserted by tests/test_full_iba_abi.py.
#include "Optimizer.h"

using namespace std;

namespace ORB_SLAM3 {

// LocalMapping::InitializeIMU, :1347-1353
void local_mapping_initialize_imu_fiba(Atlas *mpAtlas, bool bFIBA, float priorG, float priorA)
{
    if (bFIBA)
    {
        if (priorA!=0.f)
            Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false, 0, NULL, true, priorG, priorA);
        else
            Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false, 0, NULL, false);
    }
}

struct LoopClosingGbaState {              // the member of LoopClosing the call line mentions (include/LoopClosing.h:206)
    bool mbStopGBA;
};

// LoopClosing::RunGlobalBundleAdjustment, :2434-2439
void loop_closing_run_global_ba(LoopClosingGbaState &S, Map* pActiveMap, unsigned long nLoopKF)
{
    bool &mbStopGBA = S.mbStopGBA;
    const bool bImuInit = pActiveMap->isImuInitialized();

    if(bImuInit)
        Optimizer::FullInertialBA(pActiveMap,7,false,nLoopKF,&mbStopGBA);
}

// the two trailing arguments (include/Optimizer.h:55) are held to the same signature
void all_arguments(Map *pMap, Eigen::VectorXd *vSingVal, bool *bHess)
{
    Optimizer::FullInertialBA(pMap, 7, true, 0, NULL, true, 1e2, 1e6, vSingVal, bHess);
}

}  // namespace ORB_SLAM3
