// host_inertial_opt_smoke.cc -- `host_inertial_opt_smoke <in> <out>`: Optimizer::InertialOptimization (the class methods,
// host/Optimizer_InertialOptimization.cc) on stand-in keyframes from a flat file.  Inputs: overload (0..3 = (a)..(d)), mono, fixed_vel,
// prior (priorG, priorA), max_kf_id; per keyframe, in the order Map::GetAllKeyFrames() returns them: kf_id, kf_prev (index of mPrevKF,
// -1 none), kf_bad, Tcw (4x4), vel (3), bias (gyro 3, accelerometer 3), has_preint and the preintegration pre_dT, pre_dR, pre_dV, pre_dP,
// pre_JRg, pre_JVg, pre_JVa, pre_JPg, pre_JPa, pre_b (gyro 3, accelerometer 3), pre_C (15x15); Tcb (4x4); list (overload 2: the
// keyframe indices of the vector argument); Rwg, scale, bg, ba as raw doubles.  Outputs: Rwg, scale, bg, ba (raw doubles), every
// keyframe's velocity and bias, pre_bu (the preintegration's SetNewBias argument), reint (Reintegrate() calls), and what the test needs
// to feed the C ABI the same numbers: Rwb, twb (GetImuRotation / GetImuPosition) and info (the edge information, raw doubles).
// Runs without a GPU too (the methods then print one message and touch nothing).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "Optimizer.h"
#include "optimizer_common.h"
#include "flatfile.h"

using namespace ORB_SLAM3;

static cv::Mat mat(const float *v, int r, int c)
{
    cv::Mat M(r, c, CV_32F);
    for (int i = 0; i < r; i++) for (int j = 0; j < c; j++) M.at<float>(i, j) = v[c * i + j];
    return M;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: host_inertial_opt_smoke <in> <out>\n"); return 2; }
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "inertial_opt: cannot read %s\n", argv[1]); return 2; }
    const int overload = ff.I("overload")[0];
    const std::vector<int32_t> &id = ff.I("kf_id"), &prev = ff.I("kf_prev"), &bad = ff.I("kf_bad"), &hasp = ff.I("has_preint");
    const size_t n = id.size();
    std::vector<float> camp = {500.f, 500.f, 320.f, 240.f};
    GeometricCamera camera(camp, 0u);
    Map map;
    map.mnMaxKFid = (long unsigned int)ff.I("max_kf_id")[0];
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<std::unique_ptr<IMU::Preintegrated>> pre;
    const cv::Mat Tcb = mat(ff.F("Tcb").data(), 4, 4);
    for (size_t k = 0; k < n; k++) {
        kfs.emplace_back(new KeyFrame((long unsigned int)id[k], &map, camp[0], camp[1], camp[2], camp[3], 0.f, &camera));
        KeyFrame *kf = kfs.back().get();
        kf->SetPose(mat(&ff.F("Tcw")[16 * k], 4, 4));
        kf->mImuCalib.Tcb = Tcb.clone();
        kf->bImu = true;
        kf->mbBad = bad[k] != 0;
        kf->SetVelocity(mat(&ff.F("vel")[3 * k], 3, 1));
        const float *b = &ff.F("bias")[6 * k];
        kf->mImuBias = IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]);
        pre.emplace_back(nullptr);
        if (hasp[k]) {
            pre.back().reset(new IMU::Preintegrated());
            IMU::Preintegrated *p = pre.back().get();
            p->dT = ff.F("pre_dT")[k];
            p->dR = mat(&ff.F("pre_dR")[9 * k], 3, 3); p->dV = mat(&ff.F("pre_dV")[3 * k], 3, 1); p->dP = mat(&ff.F("pre_dP")[3 * k], 3, 1);
            p->JRg = mat(&ff.F("pre_JRg")[9 * k], 3, 3); p->JVg = mat(&ff.F("pre_JVg")[9 * k], 3, 3); p->JVa = mat(&ff.F("pre_JVa")[9 * k], 3, 3);
            p->JPg = mat(&ff.F("pre_JPg")[9 * k], 3, 3); p->JPa = mat(&ff.F("pre_JPa")[9 * k], 3, 3);
            const float *pb = &ff.F("pre_b")[6 * k];
            p->b = IMU::Bias(pb[3], pb[4], pb[5], pb[0], pb[1], pb[2]);
            p->bu = p->b;
            p->C = mat(&ff.F("pre_C")[225 * k], 15, 15);
            kf->mpImuPreintegrated = p;
        }
        map.mvpKeyFrames.push_back(kf);
    }
    map.nKeyFrames = n;
    for (size_t k = 0; k < n; k++) if (prev[k] >= 0) { kfs[k]->mPrevKF = kfs[prev[k]].get(); kfs[prev[k]]->mNextKF = kfs[k].get(); }

    Eigen::Matrix3d Rwg; Eigen::Vector3d bg, ba; double scale;
    memcpy(&Rwg(0, 0), ff.U("Rwg").data(), 72); memcpy(&scale, ff.U("scale").data(), 8);
    memcpy(&bg[0], ff.U("bg").data(), 24); memcpy(&ba[0], ff.U("ba").data(), 24);
    Eigen::MatrixXd covInertial(9, 9);
    const float priorG = ff.F("prior")[0], priorA = ff.F("prior")[1];
    if (overload == 0) Optimizer::InertialOptimization(&map, Rwg, scale, bg, ba, ff.I("mono")[0] != 0, covInertial, ff.I("fixed_vel")[0] != 0, false, priorG, priorA);
    else if (overload == 1) Optimizer::InertialOptimization(&map, bg, ba, priorG, priorA);
    else if (overload == 2) {
        std::vector<KeyFrame *> v;
        for (int i : ff.I("list")) v.push_back(kfs[i].get());
        Optimizer::InertialOptimization(v, bg, ba, priorG, priorA);
    } else Optimizer::InertialOptimization(&map, Rwg, scale);

    FlatWriter w(argv[2]);
    w.rec("Rwg", 2, 72, &Rwg(0, 0)); w.rec("scale", 2, 8, &scale); w.rec("bg", 2, 24, &bg[0]); w.rec("ba", 2, 24, &ba[0]);
    std::vector<float> vel, bias, bu, Rwb, twb;
    std::vector<int32_t> reint;
    std::vector<double> info(81 * n, 0.0);
    for (size_t k = 0; k < n; k++) {
        KeyFrame *kf = kfs[k].get();
        const cv::Mat V = kf->GetVelocity(), R = kf->GetImuRotation(), t = kf->GetImuPosition();
        for (int r = 0; r < 3; r++) { vel.push_back(V.at<float>(r)); twb.push_back(t.at<float>(r)); }
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rwb.push_back(R.at<float>(r, c));
        const IMU::Bias b = kf->GetImuBias();
        const float bb[6] = {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz};
        bias.insert(bias.end(), bb, bb + 6);
        IMU::Preintegrated *p = kf->mpImuPreintegrated;
        const float pu[6] = {p ? p->bu.bwx : 0.f, p ? p->bu.bwy : 0.f, p ? p->bu.bwz : 0.f, p ? p->bu.bax : 0.f, p ? p->bu.bay : 0.f, p ? p->bu.baz : 0.f};
        bu.insert(bu.end(), pu, pu + 6);
        reint.push_back(p ? p->nReintegrated : 0);
        if (p) optc::inertial_information(p->C, &info[81 * k]);
    }
    w.floats("vel", vel); w.floats("bias", bias); w.floats("pre_bu", bu); w.ints("reint", reint);
    w.floats("Rwb", Rwb); w.floats("twb", twb);
    w.rec("info", 2, (int32_t)(info.size() * 8), info.data());
    printf("inertial_opt: overload %d on %zu keyframes done, scale %.9g\n", overload, n, scale);
    return 0;
}
