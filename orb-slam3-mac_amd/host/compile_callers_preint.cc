// compile_callers_preint.cc -- the reference's own call lines of IMU::Preintegrated (src/Tracking.cc:263, :610, :651-656, :763, :1214,
// :1644; src/LocalMapping.cc:1059; src/Optimizer.cc:5474) against host/ImuTypes.h: compile-only, -Werror.  The surrounding state is
// reduced to what the lines name.
#include <cstddef>
#include "ImuTypes.h"
#include "slam_types.h"

using namespace std;
using namespace ORB_SLAM3;

struct FrameImuState {
    IMU::Bias mImuBias;
    IMU::Calib mImuCalib;
    IMU::Preintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
};
struct TrackingImuState {
    IMU::Preintegrated *mpImuPreintegratedFromLastKF = nullptr;
    IMU::Calib *mpImuCalib = nullptr;
    FrameImuState mLastFrame, mCurrentFrame;
};

// Tracking::Tracking, :263
void tracking_constructor(TrackingImuState &S)
{
    IMU::Preintegrated *&mpImuPreintegratedFromLastKF = S.mpImuPreintegratedFromLastKF; IMU::Calib *mpImuCalib = S.mpImuCalib;
        mpImuPreintegratedFromLastKF = new IMU::Preintegrated(IMU::Bias(),*mpImuCalib);
}

// Tracking::PreintegrateIMU, :610, :651-656
void tracking_preintegrate(TrackingImuState &S, cv::Point3f acc, cv::Point3f angVel, float tstep)
{
    IMU::Preintegrated *mpImuPreintegratedFromLastKF = S.mpImuPreintegratedFromLastKF; FrameImuState &mLastFrame = S.mLastFrame, &mCurrentFrame = S.mCurrentFrame;
    IMU::Preintegrated* pImuPreintegratedFromLastFrame = new IMU::Preintegrated(mLastFrame.mImuBias,mCurrentFrame.mImuCalib);
        mpImuPreintegratedFromLastKF->IntegrateNewMeasurement(acc,angVel,tstep);
        pImuPreintegratedFromLastFrame->IntegrateNewMeasurement(acc,angVel,tstep);

    mCurrentFrame.mpImuPreintegratedFrame = pImuPreintegratedFromLastFrame;
    mCurrentFrame.mpImuPreintegrated = mpImuPreintegratedFromLastKF;
}

// Tracking::UpdateFrameIMU (:763), Tracking::Track (:1214), Tracking::CreateNewKeyFrame (:1644)
void tracking_update_frame(FrameImuState *pF, TrackingImuState &S, KeyFrame *pKFcur)
{
    FrameImuState &mCurrentFrame = S.mCurrentFrame; IMU::Preintegrated *&mpImuPreintegratedFromLastKF = S.mpImuPreintegratedFromLastKF;
        pF->mpImuPreintegratedFrame->Reintegrate();
            pF->mpImuPreintegratedFrame = new IMU::Preintegrated(mCurrentFrame.mpImuPreintegratedFrame);
        mpImuPreintegratedFromLastKF = new IMU::Preintegrated(pKFcur->mpImuPreintegrated->GetUpdatedBias(),pKFcur->mImuCalib);
}

// LocalMapping::KeyFrameCulling, :1059
void local_mapping_culling(KeyFrame *pKF)
{
                        pKF->mNextKF->mpImuPreintegrated->MergePrevious(pKF->mpImuPreintegrated);
}

// Optimizer::InertialOptimization, :5471-5474
void optimizer_write_back(KeyFrame *pKFi, const IMU::Bias &b)
{
            pKFi->SetNewBias(b);
            if (pKFi->mpImuPreintegrated)
                pKFi->mpImuPreintegrated->Reintegrate();
}

// the getters the optimisers' edges call (src/G2oTypes.cc:693-715)
void edge_getters(IMU::Preintegrated *pInt, const IMU::Bias &b1)
{
    const cv::Mat dR = pInt->GetDeltaRotation(b1), dV = pInt->GetDeltaVelocity(b1), dP = pInt->GetDeltaPosition(b1);
    const cv::Mat uR = pInt->GetUpdatedDeltaRotation(), uV = pInt->GetUpdatedDeltaVelocity(), uP = pInt->GetUpdatedDeltaPosition();
    const cv::Mat oR = pInt->GetOriginalDeltaRotation(), oV = pInt->GetOriginalDeltaVelocity(), oP = pInt->GetOriginalDeltaPosition();
    const Eigen::Matrix<double,15,15> Info = pInt->GetInformationMatrix();
    const IMU::Bias db = pInt->GetDeltaBias(b1), ob = pInt->GetOriginalBias();
    const cv::Mat dbm = pInt->GetDeltaBias();
    (void)dR; (void)dV; (void)dP; (void)uR; (void)uV; (void)uP; (void)oR; (void)oV; (void)oP; (void)Info; (void)db; (void)ob; (void)dbm;
}
