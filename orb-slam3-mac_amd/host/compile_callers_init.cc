// compile_callers_init.cc -- compile-only check of the drop-in claim for monocular initialisation: the call lines of the reference's
// src/Tracking.cc:1506-1538 (Tracking::MonocularInitialization from the matcher to the frame poses) against host/ORBmatcher.h,
// host/TwoViewReconstruction.h and the camera stand-in of host/slam_types.h.  Nothing here runs.  Built by
// `make lib/compile_callers_init.o` with -Wall -Werror, asserted by tests/test_two_view_abi.py.
#include <algorithm>
#include <vector>
#include "ORBmatcher.h"
#include "TwoViewReconstruction.h"

using namespace std;

namespace ORB_SLAM3 {

struct TrackingInitState {                // the members of Tracking the call lines mention
    Frame mCurrentFrame, mInitialFrame;
    vector<cv::Point2f> mvbPrevMatched;
    vector<int> mvIniMatches;
    vector<cv::Point3f> mvIniP3D;
    GeometricCamera *mpCamera;
};

// Tracking::MonocularInitialization: the matcher (:1506-1507), the camera model's reconstruction (:1518-1522), the use of its outputs
// (:1524-1538).  The surrounding control flow is not restated -- only the argument types and the call shapes matter.
int tracking_monocular_initialization(TrackingInitState &S)
{
    Frame &mInitialFrame = S.mInitialFrame, &mCurrentFrame = S.mCurrentFrame;
    vector<cv::Point2f> &mvbPrevMatched = S.mvbPrevMatched;
    vector<int> &mvIniMatches = S.mvIniMatches;
    vector<cv::Point3f> &mvIniP3D = S.mvIniP3D;
    GeometricCamera *mpCamera = S.mpCamera;

    ORBmatcher matcher(0.9,true);
    int nmatches = matcher.SearchForInitialization(mInitialFrame,mCurrentFrame,mvbPrevMatched,mvIniMatches,100);     // :1507

    cv::Mat Rcw, tcw;                                                                                                  // :1518-1519
    vector<bool> vbTriangulated;                                                                                       // :1520
    if(mpCamera->ReconstructWithTwoViews(mInitialFrame.mvKeysUn,mCurrentFrame.mvKeysUn,mvIniMatches,Rcw,tcw,mvIniP3D,vbTriangulated))   // :1522
    {
        for(size_t i=0, iend=mvIniMatches.size(); i<iend;i++)                                                          // :1524-1531
            if(mvIniMatches[i]>=0 && !vbTriangulated[i]) { mvIniMatches[i]=-1; nmatches--; }
        mInitialFrame.SetPose(cv::Mat::eye(4,4,CV_32F));                                                               // :1534
        cv::Mat Tcw = cv::Mat::eye(4,4,CV_32F);                                                                        // :1535
        Rcw.copyTo(Tcw.rowRange(0,3).colRange(0,3));                                                                   // :1536
        tcw.copyTo(Tcw.rowRange(0,3).col(3));                                                                          // :1537
        mCurrentFrame.SetPose(Tcw);                                                                                    // :1538
    }
    return nmatches;
}

}  // namespace ORB_SLAM3
