// ImuTypes.h -- IMU::Point, Bias, Calib, IntegratedRotation and Preintegrated with the reference's members and signatures
// (include/ImuTypes.h:43-270), on this project's cv::Mat / Eigen stand-ins (cvlite.h, eigen_lite.h; slam_types.h includes
// this file).
// IntegrateNewMeasurement is plain float C++ on the host (csrc/preint_core.h, the text the device kernels run); Reintegrate and
// MergePrevious are ONE device call each (orbhip_preintegrate_host).  Two additions do the batching:
//   Preintegrated::ReintegrateBatch(objects)   one device call for all objects;
//   Preintegrated::DeferredReintegration       while one lives on a thread, Reintegrate() on that thread only files the object; the
//                                              scope's end issues them as one batch (Optimizer::InertialOptimization's write-back).
// A Preintegrated without calibration noise (Nga.empty(): the flat-file drivers build such objects by setting fields; the reference
// cannot produce them outside deserialisation) has nothing to integrate with: Reintegrate() counts the call and keeps the fields.
// nReintegrated counts Reintegrate() calls in every case (test plumbing); bu is public here, as the drivers read it.
#pragma once
#include <mutex>
#include <ostream>
#include <vector>
#include "cvlite.h"
#include "eigen_lite.h"

namespace ORB_SLAM3 {
namespace IMU {

const float GRAVITY_VALUE = 9.81;

// IMU measurement (gyro, accelerometer and timestamp)
class Point {
public:
    Point(const float &acc_x, const float &acc_y, const float &acc_z, const float &ang_vel_x, const float &ang_vel_y, const float &ang_vel_z,
          const double &timestamp) : a(acc_x, acc_y, acc_z), w(ang_vel_x, ang_vel_y, ang_vel_z), t(timestamp) {}
    Point(const cv::Point3f Acc, const cv::Point3f Gyro, const double &timestamp) : a(Acc.x, Acc.y, Acc.z), w(Gyro.x, Gyro.y, Gyro.z), t(timestamp) {}
    cv::Point3f a;
    cv::Point3f w;
    double t;
};

// IMU biases (gyro and accelerometer)
class Bias {
public:
    Bias() : bax(0), bay(0), baz(0), bwx(0), bwy(0), bwz(0) {}
    Bias(const float &b_acc_x, const float &b_acc_y, const float &b_acc_z, const float &b_ang_vel_x, const float &b_ang_vel_y, const float &b_ang_vel_z)
        : bax(b_acc_x), bay(b_acc_y), baz(b_acc_z), bwx(b_ang_vel_x), bwy(b_ang_vel_y), bwz(b_ang_vel_z) {}
    void CopyFrom(Bias &b) { bax = b.bax; bay = b.bay; baz = b.baz; bwx = b.bwx; bwy = b.bwy; bwz = b.bwz; }
    friend std::ostream &operator<<(std::ostream &out, const Bias &b)
    {
        const float v[6] = {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz};
        for (int i = 0; i < 6; i++) { if (v[i] > 0) out << " "; out << v[i]; if (i < 5) out << ","; }
        return out;
    }
    float bax, bay, baz;
    float bwx, bwy, bwz;
};

// IMU calibration (Tbc, Tcb, noise)
class Calib {
public:
    Calib(const cv::Mat &Tbc_, const float &ng, const float &na, const float &ngw, const float &naw) { Set(Tbc_, ng, na, ngw, naw); }
    Calib(const Calib &calib) : Tcb(calib.Tcb.clone()), Tbc(calib.Tbc.clone()), Cov(calib.Cov.clone()), CovWalk(calib.CovWalk.clone()) {}
    Calib &operator=(const Calib &calib) { Tcb = calib.Tcb.clone(); Tbc = calib.Tbc.clone(); Cov = calib.Cov.clone(); CovWalk = calib.CovWalk.clone(); return *this; }
    Calib() {}
    void Set(const cv::Mat &Tbc_, const float &ng, const float &na, const float &ngw, const float &naw);
    cv::Mat Tcb;
    cv::Mat Tbc;
    cv::Mat Cov, CovWalk;
};

// Integration of 1 gyro measurement
class IntegratedRotation {
public:
    IntegratedRotation() {}
    IntegratedRotation(const cv::Point3f &angVel, const Bias &imuBias, const float &time);
    float deltaT;     // integration time
    cv::Mat deltaR;   // integrated rotation
    cv::Mat rightJ;   // right jacobian
};

// Preintegration of Imu Measurements
class Preintegrated {
public:
    Preintegrated(const Bias &b_, const Calib &calib);
    Preintegrated(Preintegrated *pImuPre);
    Preintegrated() : dT(0) {}
    ~Preintegrated() {}
    void CopyFrom(Preintegrated *pImuPre);
    void Initialize(const Bias &b_);
    void IntegrateNewMeasurement(const cv::Point3f &acceleration, const cv::Point3f &angVel, const float &dt);
    void Reintegrate()
    {
        nReintegrated++;
        if (Nga.empty()) return;
        if (DeferredReintegration::Active()) { DeferredReintegration::Active()->mvpPending.push_back(this); return; }
        ReintegrateBatch(std::vector<Preintegrated *>(1, this));
    }
    void MergePrevious(Preintegrated *pPrev);
    void SetNewBias(const Bias &bu_)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        bu = bu_;
        if (db.empty()) db = cv::Mat::zeros(6, 1, CV_32F);
        db.at<float>(0) = bu_.bwx - b.bwx; db.at<float>(1) = bu_.bwy - b.bwy; db.at<float>(2) = bu_.bwz - b.bwz;
        db.at<float>(3) = bu_.bax - b.bax; db.at<float>(4) = bu_.bay - b.bay; db.at<float>(5) = bu_.baz - b.baz;
    }
    IMU::Bias GetDeltaBias(const Bias &b_);
    cv::Mat GetDeltaRotation(const Bias &b_);
    cv::Mat GetDeltaVelocity(const Bias &b_);
    cv::Mat GetDeltaPosition(const Bias &b_);
    cv::Mat GetUpdatedDeltaRotation();
    cv::Mat GetUpdatedDeltaVelocity();
    cv::Mat GetUpdatedDeltaPosition();
    cv::Mat GetOriginalDeltaRotation();
    cv::Mat GetOriginalDeltaVelocity();
    cv::Mat GetOriginalDeltaPosition();
    Eigen::Matrix<double, 15, 15> GetInformationMatrix();
    cv::Mat GetDeltaBias();
    Bias GetOriginalBias();
    Bias GetUpdatedBias();

    // every object re-integrated from its own measurements at its updated bias, as Reintegrate() would, in ONE device call; objects
    // without calibration noise are left alone.  -> the ORBHIP_* code of the call (nothing is changed unless it is ORBHIP_OK)
    static int ReintegrateBatch(const std::vector<Preintegrated *> &vpPre);
    // collects this thread's Reintegrate() calls while it lives and issues them as one batch when it ends
    class DeferredReintegration {
    public:
        DeferredReintegration() : mpOuter(Active()) { Active() = this; }
        ~DeferredReintegration() { Active() = mpOuter; if (!mvpPending.empty()) ReintegrateBatch(mvpPending); }
        DeferredReintegration(const DeferredReintegration &) = delete;
        DeferredReintegration &operator=(const DeferredReintegration &) = delete;
        static DeferredReintegration *&Active() { static thread_local DeferredReintegration *p = nullptr; return p; }
        std::vector<Preintegrated *> mvpPending;
    private:
        DeferredReintegration *mpOuter;
    };
    static int nDeviceCalls;        // device calls issued by Reintegrate / ReintegrateBatch / MergePrevious so far (test plumbing)
    size_t NumMeasurements() const { return mvMeasurements.size(); }
    void GetMeasurement(size_t i, float *m7) const          // (ax, ay, az, wx, wy, wz, dt) as IntegrateNewMeasurement took it (test plumbing)
    {
        const integrable &m = mvMeasurements[i];
        m7[0] = m.a.x; m7[1] = m.a.y; m7[2] = m.a.z; m7[3] = m.w.x; m7[4] = m.w.y; m7[5] = m.w.z; m7[6] = m.t;
    }

public:
    float dT;
    cv::Mat C;
    cv::Mat Info;
    cv::Mat Nga, NgaWalk;

    // Values for the original bias (when integration was computed)
    Bias b;
    cv::Mat dR, dV, dP;
    cv::Mat JRg, JVg, JVa, JPg, JPa;
    cv::Mat avgA;
    cv::Mat avgW;

    // Updated bias
    Bias bu;
    int nReintegrated = 0;

private:
    // Dif between original and updated bias
    // This is used to compute the updated values of the preintegration
    cv::Mat db;

    struct integrable {
        integrable(const cv::Point3f &a_, const cv::Point3f &w_, const float &t_) : a(a_), w(w_), t(t_) {}
        cv::Point3f a;
        cv::Point3f w;
        float t;
    };

    std::vector<integrable> mvMeasurements;

    std::mutex mMutex;
};

// Lie Algebra Functions
cv::Mat ExpSO3(const float &x, const float &y, const float &z);
cv::Mat ExpSO3(const cv::Mat &v);
cv::Mat LogSO3(const cv::Mat &R);
cv::Mat RightJacobianSO3(const float &x, const float &y, const float &z);
cv::Mat RightJacobianSO3(const cv::Mat &v);
cv::Mat InverseRightJacobianSO3(const float &x, const float &y, const float &z);
cv::Mat InverseRightJacobianSO3(const cv::Mat &v);
cv::Mat Skew(const cv::Mat &v);
cv::Mat NormalizeRotation(const cv::Mat &R);

}  // namespace IMU
}  // namespace ORB_SLAM3
