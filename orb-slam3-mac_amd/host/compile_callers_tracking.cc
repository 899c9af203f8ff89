// compile_callers_tracking.cc -- compile-only check of the drop-in claim for Frame::isInFrustum and Tracking::SearchLocalPoints: the
// reference's own lines -- the isInFrustum call of src/Tracking.cc:2392, the matcher call of :2428, and TrackLocalMap's call of the function
// under its own signature (:1981-1982) -- against the Frame / MapPoint / Tracking / Atlas / LocalMapping stand-ins of host/slam_types.h and
// host/ORBmatcher.h.  Nothing here runs.  Built by `make lib/compile_callers_tracking.o` with -Wall -Werror, asserted by
// tests/test_frustum_model.py.
#include <vector>
#include "ORBmatcher.h"
#include "slam_types.h"

using namespace std;

namespace ORB_SLAM3 {

struct TrackingLines : public Tracking {
    void UpdateLocalMap() {}
    // Tracking::TrackLocalMap, :1981-1982
    void TrackLocalMapHead()
    {
    UpdateLocalMap();
    SearchLocalPoints();
    }
    // Tracking::SearchLocalPoints, :2380-2401 and :2405, :2428
    int SearchLocalPointsLines(int th)
    {
    int nToMatch=0;

    for(vector<MapPoint*>::iterator vit=mvpLocalMapPoints.begin(), vend=mvpLocalMapPoints.end(); vit!=vend; vit++)
    {
        MapPoint* pMP = *vit;

        if(pMP->mnLastFrameSeen == mCurrentFrame.mnId)
            continue;
        if(pMP->isBad())
            continue;
        if(mCurrentFrame.isInFrustum(pMP,0.5))
        {
            pMP->IncreaseVisible();
            nToMatch++;
        }
        if(pMP->mbTrackInView)
        {
            mCurrentFrame.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
        }
    }

        ORBmatcher matcher(0.8);
        int matches = matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, mpLocalMapper->mbFarPoints, mpLocalMapper->mThFarPoints);
    return matches + nToMatch;
    }
};

void tracking_lines(TrackingLines &t) { t.TrackLocalMapHead(); t.SearchLocalPointsLines(1); }

}  // namespace ORB_SLAM3
