// host_preint_smoke.cc -- `host_preint_smoke <in> <out>`: IMU::Preintegrated (host/ImuTypes.cc) on chains from a flat file.
// Inputs: mode, noise (ng, na, ngw, naw: IMU::Calib::Set), meas_off [n + 1], meas [total][7] (ax, ay, az, wx, wy, wz, dt), bias [n][6]
// and bias_new [n][6] (gyro 3, accelerometer 3).  Every chain becomes Preintegrated(bias, calib) and takes its measurements through
// IntegrateNewMeasurement (host arithmetic): outputs host_*.  Then, by mode:
//   0  SetNewBias(bias_new) and Reintegrate() on every object (one device call each)
//   1  SetNewBias(bias_new) and ONE Preintegrated::ReintegrateBatch over all objects (with `dup`: every object listed twice)
//   2  chains in pairs: object 2k+1 ->MergePrevious(object 2k) (the outputs keep all objects)
//   3  the objects hang on a chain of stand-in keyframes (keyframe k + 1 carries object k; identity poses, zero velocities, kf_bias
//      [n + 1][6]) and Optimizer::InertialOptimization(map, bg, ba, priorG, priorA) runs: outputs bg / ba (raw doubles) too
// Outputs after that: dev_* (dT, dR, dV, dP, JRg, JVg, JVa, JPg, JPa, avg, C, b per object), reint (Reintegrate() calls), nmeas,
// device_calls.  mode -1 stops after the host loop and needs no GPU; mode -2 does the same and times the host loop on this thread
// (reps [1] repetitions -> host_us: the shortest repetition, all chains, in microseconds).
// mode -3: Tracking::PreintegrateIMU (host/Tracking_PreintegrateIMU.cc, no GPU).  Inputs: imu [k][6] (ax, ay, az, wx, wy, wz), imu_t
// [k] and t_prev, t_cur (raw doubles; t_prev absent = no previous frame), bias [1][6] (the last frame's), kf_pre [1] (measurements
// meas[0 : kf_pre] the keyframe chain holds already).  Outputs: steps [m][7] (what the frame's chain took), kf_n, frame_n, queue_left,
// from_last_frame, integrated, and the fields of both chains (host_*: the keyframe chain, then the frame chain).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "Optimizer.h"
#include "ImuTypes.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

static void dump(FlatWriter &out, const char *prefix, const std::vector<std::unique_ptr<IMU::Preintegrated>> &v)
{
    const char *names[] = {"dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "avgA", "avgW", "C"};
    std::vector<float> dT, b;
    std::vector<std::vector<float>> f(11);
    for (const auto &p : v) {
        const cv::Mat *m[] = {&p->dR, &p->dV, &p->dP, &p->JRg, &p->JVg, &p->JVa, &p->JPg, &p->JPa, &p->avgA, &p->avgW, &p->C};
        dT.push_back(p->dT);
        for (int k = 0; k < 11; k++)
            for (int r = 0; r < m[k]->rows; r++) for (int c = 0; c < m[k]->cols; c++) f[k].push_back(m[k]->at<float>(r, c));
        const float bb[6] = {p->b.bwx, p->b.bwy, p->b.bwz, p->b.bax, p->b.bay, p->b.baz};
        b.insert(b.end(), bb, bb + 6);
    }
    out.floats((std::string(prefix) + "dT").c_str(), dT);
    for (int k = 0; k < 11; k++) out.floats((std::string(prefix) + names[k]).c_str(), f[k]);
    out.floats((std::string(prefix) + "b").c_str(), b);
}

static int tracking_mode(const FlatFile &ff, const char *path)
{
    const std::vector<float> &noise = ff.F("noise"), &imu = ff.F("imu"), &bias = ff.F("bias"), &meas = ff.F("meas");
    const size_t k = imu.size() / 6;
    std::vector<double> ts(k);
    if (k) memcpy(ts.data(), ff.U("imu_t").data(), 8 * k);
    IMU::Calib calib(cv::Mat::eye(4, 4, CV_32F), noise[0], noise[1], noise[2], noise[3]);
    Tracking tr;
    Frame prev;
    for (size_t i = 0; i < k; i++) tr.mlQueueImuData.push_back(IMU::Point(imu[6 * i], imu[6 * i + 1], imu[6 * i + 2], imu[6 * i + 3], imu[6 * i + 4], imu[6 * i + 5], ts[i]));
    memcpy(&tr.mCurrentFrame.mTimeStamp, ff.U("t_cur").data(), 8);
    if (ff.has("t_prev")) { memcpy(&prev.mTimeStamp, ff.U("t_prev").data(), 8); tr.mCurrentFrame.mpPrevFrame = &prev; }
    tr.mCurrentFrame.mImuCalib = calib;
    tr.mLastFrame.mImuBias = IMU::Bias(bias[3], bias[4], bias[5], bias[0], bias[1], bias[2]);
    std::vector<std::unique_ptr<IMU::Preintegrated>> pre;
    pre.emplace_back(new IMU::Preintegrated(tr.mLastFrame.mImuBias, calib));
    for (int i = 0; i < ff.I("kf_pre")[0]; i++) pre[0]->IntegrateNewMeasurement(cv::Point3f(meas[7 * i], meas[7 * i + 1], meas[7 * i + 2]), cv::Point3f(meas[7 * i + 3], meas[7 * i + 4], meas[7 * i + 5]), meas[7 * i + 6]);
    tr.mpImuPreintegratedFromLastKF = pre[0].get();
    tr.PreintegrateIMU();
    FlatWriter out(path);
    if (!out.fp) return 2;
    std::vector<float> steps;
    if (tr.mCurrentFrame.mpImuPreintegratedFrame) {
        pre.emplace_back(tr.mCurrentFrame.mpImuPreintegratedFrame);
        for (size_t i = 0; i < pre[1]->NumMeasurements(); i++) { float m[7]; pre[1]->GetMeasurement(i, m); steps.insert(steps.end(), m, m + 7); }
        out.one("frame_n", (int32_t)pre[1]->NumMeasurements());
    }
    out.floats("steps", steps);
    out.one("kf_n", (int32_t)pre[0]->NumMeasurements());
    out.one("queue_left", (int32_t)tr.mlQueueImuData.size());
    out.one("from_last_frame", (int32_t)tr.mvImuFromLastFrame.size());
    out.one("integrated", tr.mCurrentFrame.mbImuPreintegrated ? 1 : 0);
    out.one("kf_is_current", tr.mCurrentFrame.mpImuPreintegrated == pre[0].get() ? 1 : 0);
    dump(out, "host_", pre);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: host_preint_smoke <in> <out>\n"); return 2; }
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "preint: cannot read %s\n", argv[1]); return 2; }
    const int mode = ff.I("mode")[0];
    if (mode == -3) return tracking_mode(ff, argv[2]);
    const std::vector<int32_t> &off = ff.I("meas_off");
    const std::vector<float> &meas = ff.F("meas"), &bias = ff.F("bias"), &bias_new = ff.F("bias_new"), &noise = ff.F("noise");
    const size_t n = off.size() - 1;
    IMU::Calib calib(cv::Mat::eye(4, 4, CV_32F), noise[0], noise[1], noise[2], noise[3]);
    std::vector<std::unique_ptr<IMU::Preintegrated>> pre;
    double best_us = 0;
    for (int rep = 0, reps = mode == -2 ? ff.I("reps")[0] : 1; rep < reps; rep++) {
        pre.clear();
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t k = 0; k < n; k++) {
            const float *b = &bias[6 * k];
            pre.emplace_back(new IMU::Preintegrated(IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]), calib));
            for (int i = off[k]; i < off[k + 1]; i++) {
                const float *m = &meas[7 * (size_t)i];
                pre.back()->IntegrateNewMeasurement(cv::Point3f(m[0], m[1], m[2]), cv::Point3f(m[3], m[4], m[5]), m[6]);
            }
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (rep == 0 || us < best_us) best_us = us;
    }
    FlatWriter out(argv[2]);
    if (!out.fp) { fprintf(stderr, "preint: cannot write %s\n", argv[2]); return 2; }
    out.floats("host_us", std::vector<float>(1, (float)best_us));
    dump(out, "host_", pre);
    std::vector<float> cal(calib.Cov.ptr<float>(0), calib.Cov.ptr<float>(0) + 36);
    cal.insert(cal.end(), calib.CovWalk.ptr<float>(0), calib.CovWalk.ptr<float>(0) + 36);
    out.floats("calib", cal);
    if (mode < 0) return 0;

    auto new_bias = [&](size_t k) { const float *b = &bias_new[6 * k]; return IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]); };
    if (mode == 0) {
        for (size_t k = 0; k < n; k++) { pre[k]->SetNewBias(new_bias(k)); pre[k]->Reintegrate(); }
    } else if (mode == 1) {
        std::vector<IMU::Preintegrated *> v;
        for (size_t k = 0; k < n; k++) { pre[k]->SetNewBias(new_bias(k)); v.push_back(pre[k].get()); }
        if (ff.has("dup")) for (size_t k = 0; k < n; k++) v.push_back(pre[k].get());      // every object listed twice
        if (IMU::Preintegrated::ReintegrateBatch(v) != 0) return 1;
    } else if (mode == 2) {
        for (size_t k = 0; k + 1 < n; k += 2) pre[k + 1]->MergePrevious(pre[k].get());
    } else if (mode == 3) {
        const std::vector<float> &kb = ff.F("kf_bias"), &prior = ff.F("prior");
        std::vector<float> camp = {500.f, 500.f, 320.f, 240.f};
        GeometricCamera camera(camp, 0u);
        Map map;
        map.mnMaxKFid = (long unsigned int)n;
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        for (size_t k = 0; k <= n; k++) {
            kfs.emplace_back(new KeyFrame(k, &map, 500.f, 500.f, 320.f, 240.f, 0.f, &camera));
            KeyFrame *kf = kfs.back().get();
            kf->SetPose(cv::Mat::eye(4, 4, CV_32F));
            kf->mImuCalib = calib;
            kf->SetVelocity(cv::Mat::zeros(3, 1, CV_32F));
            kf->bImu = true;
            const float *b = &kb[6 * k];
            kf->mImuBias = IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]);
            if (k > 0) { kf->mpImuPreintegrated = pre[k - 1].get(); kf->mPrevKF = kfs[k - 1].get(); kfs[k - 1]->mNextKF = kf; }
            map.mvpKeyFrames.push_back(kf);
        }
        map.nKeyFrames = n + 1;
        Eigen::Vector3d bg, ba;
        Optimizer::InertialOptimization(&map, bg, ba, prior[0], prior[1]);
        out.rec("bg", 2, 24, &bg[0]); out.rec("ba", 2, 24, &ba[0]);
    }
    dump(out, "dev_", pre);
    std::vector<int32_t> reint, nmeas;
    for (const auto &p : pre) { reint.push_back(p->nReintegrated); nmeas.push_back((int32_t)p->NumMeasurements()); }
    out.ints("reint", reint); out.ints("nmeas", nmeas);
    out.one("device_calls", IMU::Preintegrated::nDeviceCalls);
    return 0;
}
