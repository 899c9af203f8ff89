// host_full_iba_smoke.cc -- `host_full_iba_smoke <in> <out>`: Optimizer::FullInertialBA (the class method,
// host/Optimizer_FullInertialBA.cc) on stand-in keyframes and map points from a flat file.  Inputs: its, fix_local, loop_id, b_init,
// stop, prior (priorG, priorA), max_kf_id; cam (fx, fy, cx, cy, bf), inv_sigma2 (per octave), Tcb (4x4); per keyframe, in the order
// Map::GetAllKeyFrames() returns them: kf_id, kf_prev (index of mPrevKF, -1 none), kf_bad, kf_imu, kf_local, kf_fixedfor
// (mnBALocalForKF, mnBAFixedForKF), Tcw (4x4), vel (3), bias (gyro 3, accelerometer 3), has_preint and pre_dT, pre_dR, pre_dV, pre_dP,
// pre_JRg, pre_JVg, pre_JVa, pre_JPg, pre_JPa, pre_b (gyro 3, accelerometer 3), pre_C (15x15); the keypoints of all keyframes
// key_off (n + 1), key_x, key_y, key_ur, key_oct; the map points mp_pos (3 each); the observations ob_mp, ob_kf, ob_idx.
// Outputs per keyframe: Tcw, vel, bias, TcwGBA (zeros when unset), velGBA, biasGBA, kf_gba (mnBAGlobalForKF), pre_bu; per point: mp_pos,
// mp_gba_pos, mp_gba, mp_updates (UpdateNormalAndDepth calls); change (the map's change index); and what the test needs to feed the
// C ABI the same numbers: Rwb, twb before the call and info (the edge information, raw doubles).
// Runs without a GPU too (the method then prints one message and touches nothing).
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
static void push(std::vector<float> &v, const cv::Mat &M, int n) { for (int i = 0; i < n; i++) v.push_back(M.empty() ? 0.f : M.at<float>(i / M.cols, i % M.cols)); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: host_full_iba_smoke <in> <out>\n"); return 2; }
    FlatFile ff;
    if (!ff.load(argv[1])) { fprintf(stderr, "full_iba: cannot read %s\n", argv[1]); return 2; }
    const std::vector<int32_t> &id = ff.I("kf_id"), &prev = ff.I("kf_prev"), &bad = ff.I("kf_bad"), &hasp = ff.I("has_preint"), &kimu = ff.I("kf_imu");
    const std::vector<int32_t> &koff = ff.I("key_off"), &koct = ff.I("key_oct");
    const size_t n = id.size();
    const std::vector<float> &cam = ff.F("cam");
    std::vector<float> camp(cam.begin(), cam.begin() + 4);
    GeometricCamera camera(camp, 0u);
    Map map;
    map.mnMaxKFid = (long unsigned int)ff.I("max_kf_id")[0];
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<std::unique_ptr<IMU::Preintegrated>> pre;
    const cv::Mat Tcb = mat(ff.F("Tcb").data(), 4, 4);
    for (size_t k = 0; k < n; k++) {
        kfs.emplace_back(new KeyFrame((long unsigned int)id[k], &map, camp[0], camp[1], camp[2], camp[3], cam[4], &camera));
        KeyFrame *kf = kfs.back().get();
        kf->SetPose(mat(&ff.F("Tcw")[16 * k], 4, 4));
        kf->mImuCalib.Tcb = Tcb.clone();
        kf->bImu = kimu[k] != 0;
        kf->mbBad = bad[k] != 0;
        kf->mnBALocalForKF = (long unsigned int)ff.I("kf_local")[k]; kf->mnBAFixedForKF = (long unsigned int)ff.I("kf_fixedfor")[k];
        kf->SetVelocity(mat(&ff.F("vel")[3 * k], 3, 1));
        const float *b = &ff.F("bias")[6 * k];
        kf->mImuBias = IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]);
        kf->mvInvLevelSigma2 = ff.F("inv_sigma2");
        for (int q = koff[k]; q < koff[k + 1]; q++) {
            cv::KeyPoint kp; kp.pt.x = ff.F("key_x")[q]; kp.pt.y = ff.F("key_y")[q]; kp.octave = koct[q];
            kf->mvKeysUn.push_back(kp); kf->mvuRight.push_back(ff.F("key_ur")[q]);
        }
        kf->mvpMapPoints.assign(kf->mvKeysUn.size(), nullptr);
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
    const std::vector<float> &mpos = ff.F("mp_pos");
    const size_t L = mpos.size() / 3;
    std::vector<std::unique_ptr<MapPoint>> mps;
    for (size_t l = 0; l < L; l++) { mps.emplace_back(new MapPoint((long unsigned int)l, mat(&mpos[3 * l], 3, 1), &map)); map.mvpMapPoints.push_back(mps.back().get()); }
    const std::vector<int32_t> &omp = ff.I("ob_mp"), &okf = ff.I("ob_kf"), &oidx = ff.I("ob_idx");
    for (size_t o = 0; o < omp.size(); o++) mps[omp[o]]->AddObservation(kfs[okf[o]].get(), oidx[o], -1);

    // what the C ABI gets from the class: body poses before the call, edge information
    std::vector<float> Rwb, twb;
    std::vector<double> info(81 * n, 0.0);
    for (size_t k = 0; k < n; k++) {
        push(Rwb, kfs[k]->GetImuRotation(), 9); push(twb, kfs[k]->GetImuPosition(), 3);
        if (kfs[k]->mpImuPreintegrated) optc::inertial_information(kfs[k]->mpImuPreintegrated->C, &info[81 * k]);
    }
    bool stop = ff.I("stop")[0] != 0;
    const float priorG = ff.F("prior")[0], priorA = ff.F("prior")[1];
    Optimizer::FullInertialBA(&map, ff.I("its")[0], ff.I("fix_local")[0] != 0, (unsigned long)ff.I("loop_id")[0], ff.I("stop")[0] < 0 ? NULL : &stop,
                              ff.I("b_init")[0] != 0, priorG, priorA);

    FlatWriter w(argv[2]);
    std::vector<float> Tcw, vel, bias, TcwG, velG, biasG, bu, pos, posG;
    std::vector<int32_t> kgba, mgba, mupd;
    for (size_t k = 0; k < n; k++) {
        KeyFrame *kf = kfs[k].get();
        push(Tcw, kf->GetPose(), 16); push(vel, kf->GetVelocity(), 3); push(TcwG, kf->mTcwGBA, 16); push(velG, kf->mVwbGBA, 3);
        const IMU::Bias b = kf->GetImuBias(), g = kf->mBiasGBA;
        const float bb[6] = {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz}, gg[6] = {g.bwx, g.bwy, g.bwz, g.bax, g.bay, g.baz};
        bias.insert(bias.end(), bb, bb + 6); biasG.insert(biasG.end(), gg, gg + 6);
        IMU::Preintegrated *p = kf->mpImuPreintegrated;
        const float pu[6] = {p ? p->bu.bwx : 0.f, p ? p->bu.bwy : 0.f, p ? p->bu.bwz : 0.f, p ? p->bu.bax : 0.f, p ? p->bu.bay : 0.f, p ? p->bu.baz : 0.f};
        bu.insert(bu.end(), pu, pu + 6);
        kgba.push_back((int32_t)kf->mnBAGlobalForKF);
    }
    for (size_t l = 0; l < L; l++) {
        push(pos, mps[l]->GetWorldPos(), 3); push(posG, mps[l]->mPosGBA, 3);
        mgba.push_back((int32_t)mps[l]->mnBAGlobalForKF); mupd.push_back(mps[l]->nNormalUpdates);
    }
    w.floats("Tcw", Tcw); w.floats("vel", vel); w.floats("bias", bias); w.floats("TcwGBA", TcwG); w.floats("velGBA", velG); w.floats("biasGBA", biasG);
    w.floats("pre_bu", bu); w.ints("kf_gba", kgba); w.floats("mp_pos", pos); w.floats("mp_gba_pos", posG); w.ints("mp_gba", mgba); w.ints("mp_updates", mupd);
    w.one("change", map.mnMapChange);
    w.floats("Rwb", Rwb); w.floats("twb", twb);
    w.rec("info", 2, (int32_t)(info.size() * 8), info.data());
    printf("full_iba: %zu keyframes, %zu points, change index %d\n", n, L, map.mnMapChange);
    return 0;
}
