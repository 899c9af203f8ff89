// Tracking_PreintegrateIMU.cc -- void Tracking::PreintegrateIMU() with the reference's signature (src/Tracking.cc:552-666): the walk
// over mlQueueImuData (:574-606) and the four interpolation cases that turn the frame's IMU points into (acc, angVel, tstep)
// (:609-647) are host code as the reference writes them; every step goes to both chains -- mpImuPreintegratedFromLastKF, which
// continues, and a fresh one from the last frame -- through IMU::Preintegrated::IntegrateNewMeasurement on the host.
// The host path is the measured choice: a frame carries about ten measurements, which the host loop integrates in 9 us
// for both chains, where one two-chain device call takes 53 us; the device call (orbhip_preintegrate_device with d_continue) is for
// callers that keep their records on the device.  No device is touched here.
// The reference's Verbose / cout messages are stderr lines; its unreachable sleep (:598-605: `break` precedes bSleep = true) is left out.
#include <cstdio>
#include <mutex>
#include "ImuTypes.h"
#include "slam_types.h"

using namespace std;

namespace ORB_SLAM3 {

void Tracking::PreintegrateIMU()
{
    if(!mCurrentFrame.mpPrevFrame)
    {
        fprintf(stderr, "non prev frame \n");
        mCurrentFrame.setIntegrated();
        return;
    }

    mvImuFromLastFrame.clear();
    mvImuFromLastFrame.reserve(mlQueueImuData.size());
    if(mlQueueImuData.size() == 0)
    {
        fprintf(stderr, "Not IMU data in mlQueueImuData!!\n");
        mCurrentFrame.setIntegrated();
        return;
    }

    while(true)
    {
        unique_lock<mutex> lock(mMutexImuQueue);
        if(mlQueueImuData.empty())
            break;
        IMU::Point* m = &mlQueueImuData.front();
        if(m->t<mCurrentFrame.mpPrevFrame->mTimeStamp-0.001l)
        {
            mlQueueImuData.pop_front();
        }
        else if(m->t<mCurrentFrame.mTimeStamp-0.001l)
        {
            mvImuFromLastFrame.push_back(*m);
            mlQueueImuData.pop_front();
        }
        else
        {
            mvImuFromLastFrame.push_back(*m);
            break;
        }
    }

    const int n = mvImuFromLastFrame.size()-1;
    IMU::Preintegrated* pImuPreintegratedFromLastFrame = new IMU::Preintegrated(mLastFrame.mImuBias,mCurrentFrame.mImuCalib);

    for(int i=0; i<n; i++)
    {
        float tstep = 0.f;
        cv::Point3f acc, angVel;
        if((i==0) && (i<(n-1)))
        {
            float tab = mvImuFromLastFrame[i+1].t-mvImuFromLastFrame[i].t;
            float tini = mvImuFromLastFrame[i].t-mCurrentFrame.mpPrevFrame->mTimeStamp;
            acc = (mvImuFromLastFrame[i].a+mvImuFromLastFrame[i+1].a-
                    (mvImuFromLastFrame[i+1].a-mvImuFromLastFrame[i].a)*(tini/tab))*0.5f;
            angVel = (mvImuFromLastFrame[i].w+mvImuFromLastFrame[i+1].w-
                    (mvImuFromLastFrame[i+1].w-mvImuFromLastFrame[i].w)*(tini/tab))*0.5f;
            tstep = mvImuFromLastFrame[i+1].t-mCurrentFrame.mpPrevFrame->mTimeStamp;
        }
        else if(i<(n-1))
        {
            acc = (mvImuFromLastFrame[i].a+mvImuFromLastFrame[i+1].a)*0.5f;
            angVel = (mvImuFromLastFrame[i].w+mvImuFromLastFrame[i+1].w)*0.5f;
            tstep = mvImuFromLastFrame[i+1].t-mvImuFromLastFrame[i].t;
        }
        else if((i>0) && (i==(n-1)))
        {
            float tab = mvImuFromLastFrame[i+1].t-mvImuFromLastFrame[i].t;
            float tend = mvImuFromLastFrame[i+1].t-mCurrentFrame.mTimeStamp;
            acc = (mvImuFromLastFrame[i].a+mvImuFromLastFrame[i+1].a-
                    (mvImuFromLastFrame[i+1].a-mvImuFromLastFrame[i].a)*(tend/tab))*0.5f;
            angVel = (mvImuFromLastFrame[i].w+mvImuFromLastFrame[i+1].w-
                    (mvImuFromLastFrame[i+1].w-mvImuFromLastFrame[i].w)*(tend/tab))*0.5f;
            tstep = mCurrentFrame.mTimeStamp-mvImuFromLastFrame[i].t;
        }
        else if((i==0) && (i==(n-1)))
        {
            acc = mvImuFromLastFrame[i].a;
            angVel = mvImuFromLastFrame[i].w;
            tstep = mCurrentFrame.mTimeStamp-mCurrentFrame.mpPrevFrame->mTimeStamp;
        }

        if (!mpImuPreintegratedFromLastKF)
            fprintf(stderr, "mpImuPreintegratedFromLastKF does not exist\n");
        mpImuPreintegratedFromLastKF->IntegrateNewMeasurement(acc,angVel,tstep);
        pImuPreintegratedFromLastFrame->IntegrateNewMeasurement(acc,angVel,tstep);
    }

    mCurrentFrame.mpImuPreintegratedFrame = pImuPreintegratedFromLastFrame;
    mCurrentFrame.mpImuPreintegrated = mpImuPreintegratedFromLastKF;
    mCurrentFrame.mpLastKeyFrame = mpLastKeyFrame;

    if(!mpLastKeyFrame)
    {
        fprintf(stderr, "last KF is empty!\n");
    }
    mCurrentFrame.setIntegrated();
}

}  // namespace ORB_SLAM3
