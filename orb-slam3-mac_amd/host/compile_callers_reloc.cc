// compile_callers_reloc.cc -- compile-only check of the drop-in claim for MLPnPsolver: the lines of the reference's
// src/Tracking.cc:2673-2674 and :2697-2698 (Tracking::Relocalization) against host/MLPnPsolver.h and the stand-ins of host/slam_types.h.
// Nothing here runs.  Built by `make lib/compile_callers_reloc.o` with -Wall -Werror, asserted by tests/test_mlpnp_abi.py.
#include <vector>
#include "MLPnPsolver.h"

using namespace std;

namespace ORB_SLAM3 {

// Tracking::Relocalization, :2673-2674 and :2697-2698
cv::Mat relocalization_solver_lines(Frame &mCurrentFrame, vector<vector<MapPoint*> > &vvpMapPointMatches, vector<MLPnPsolver*> &vpMLPnPsolvers,
                                    int i, bool &bNoMoreOut, vector<bool> &vbInliersOut, int &nInliersOut)
{
                MLPnPsolver* pSolver = new MLPnPsolver(mCurrentFrame,vvpMapPointMatches[i]);
                pSolver->SetRansacParameters(0.99,10,300,6,0.5,5.991);  //This solver needs at least 6 points
                vpMLPnPsolvers[i] = pSolver;
    {
        bool bNoMore = false; vector<bool> vbInliers; int nInliers = 0;            // the caller's locals the two lines mention

            MLPnPsolver* pSolver = vpMLPnPsolvers[i];
            cv::Mat Tcw = pSolver->iterate(5,bNoMore,vbInliers,nInliers);

        bNoMoreOut = bNoMore; vbInliersOut = vbInliers; nInliersOut = nInliers;
        return Tcw;
    }
}

}  // namespace ORB_SLAM3
