// Optimizer_FullInertialBA.cc -- Optimizer::FullInertialBA(Map*, int its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA, ...)
// with the reference's signature (include/Optimizer.h:55) around the HIP solver.  The host parts of the reference function stay host
// code, restated in the reference's order (src/Optimizer.cc:420-851): the keyframe vertices with the mnId > maxKFid skip and bFixLocal
// (:446-500), the IMU links with SetNewBias(mPrevKF->GetImuBias()) (:503-608), the map points with their mono / stereo / right-camera
// edges and the bAllFixed removal (:636-756), the stop flag (:758-760), the write-back (:767-850).  What was the g2o block is flat
// packing plus ONE call of orbhip_full_inertial_ba_solve_batch.  The edge information comes from mpImuPreintegrated->C through
// optc::inertial_information (no 1e-2 scaling here); the random-walk informations (:581-598) are 3x3 inverses rounded to float.
// With bInit the shared biases start from pIncKF, the last keyframe admitted (:453, :486-490).
// A map beyond the solver's 480 reduced unknowns, or no usable GPU: one message on stderr, the map untouched; no CPU fallback.
// The stop flag is read once before the solve and not while it runs: g2o would stop after the current iteration, but
// LoopClosing::RunGlobalBundleAdjustment discards the result of a stopped global BA anyway.
#include "Optimizer.h"
#include <cmath>
#include <cstdio>
#include <map>
#include "hip_context.h"
#include "optimizer_common.h"
#include "../../include/orbhip.h"

namespace ORB_SLAM3 {

namespace {
void put3x3(double *dst, const cv::Mat &m) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) dst[3 * r + c] = (double)m.at<float>(r, c); }
void put3(double *dst, const cv::Mat &m) { for (int r = 0; r < 3; r++) dst[r] = (double)m.at<float>(r); }
void inv3_block(const cv::Mat &C, int o, double *out9)           // C.rowRange(o, o+3).colRange(o, o+3).inv(DECOMP_SVD), read back as float
{
    double A[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) A[3 * r + c] = (double)C.at<float>(o + r, o + c);
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c0 + A[1] * c1 + A[2] * c2);
    out9[0] = c0 * id; out9[1] = (A[2] * A[7] - A[1] * A[8]) * id; out9[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    out9[3] = c1 * id; out9[4] = (A[0] * A[8] - A[2] * A[6]) * id; out9[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    out9[6] = c2 * id; out9[7] = (A[1] * A[6] - A[0] * A[7]) * id; out9[8] = (A[0] * A[4] - A[1] * A[3]) * id;
    for (int i = 0; i < 9; i++) out9[i] = (double)(float)out9[i];
}
}  // namespace

void Optimizer::FullInertialBA(Map *pMap, int its, const bool bFixLocal, const unsigned long nLoopId, bool *pbStopFlag, bool bInit, float priorG, float priorA,
                               Eigen::VectorXd *vSingVal, bool *bHess)
{
    (void)vSingVal; (void)bHess;                                               // unread in the reference too
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();

    // ---- keyframe vertices (:446-500)
    int nNonFixed = 0;
    KeyFrame *pIncKF = nullptr;
    std::vector<KeyFrame *> vKF;
    std::map<KeyFrame *, int> kfIndex;
    std::vector<uint8_t> fixed, imu;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKFi = vpKFs[i];
        if (pKFi->mnId > maxKFid) continue;
        pIncKF = pKFi;
        bool bFixed = false;
        if (bFixLocal) {
            bFixed = (pKFi->mnBALocalForKF >= (maxKFid - 1)) || (pKFi->mnBAFixedForKF >= (maxKFid - 1));
            if (!bFixed) nNonFixed++;
        }
        kfIndex[pKFi] = (int)vKF.size();
        vKF.push_back(pKFi); fixed.push_back(bFixed ? 1 : 0); imu.push_back(pKFi->bImu ? 1 : 0);
    }
    if (bFixLocal && nNonFixed < 3) return;                                    // :496-500
    const int nKF = (int)vKF.size();
    if (nKF == 0) return;
    std::vector<double> kf((size_t)ORBHIP_IBA_KF * nKF, 0.0);
    for (int i = 0; i < nKF; i++) {
        KeyFrame *pKFi = vKF[i];
        double *s = &kf[(size_t)ORBHIP_IBA_KF * i];
        put3x3(s, pKFi->GetImuRotation()); put3(s + 9, pKFi->GetImuPosition());
        if (pKFi->bImu) { put3(s + 12, pKFi->GetVelocity()); put3(s + 15, pKFi->GetGyroBias()); put3(s + 18, pKFi->GetAccBias()); }
    }
    double shared[6] = {0, 0, 0, 0, 0, 0};
    if (bInit) { put3(shared, pIncKF->GetGyroBias()); put3(shared + 3, pIncKF->GetAccBias()); }      // VertexGyroBias(pIncKF), VertexAccBias(pIncKF)

    KeyFrame *pKF0 = vKF[0];                                                   // ImuCamPose(KeyFrame*): every keyframe of a map shares the rig
    orbhip_iba_window w = {};
    w.n_kf = nKF; w.kf_fixed = fixed.data(); w.kf_imu = imu.data();
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) w.Rcb[3 * r + c] = (double)pKF0->mImuCalib.Tcb.at<float>(r, c); w.tcb[r] = (double)pKF0->mImuCalib.Tcb.at<float>(r, 3); }
    w.fx = pKF0->mpCamera->getParameter(0); w.fy = pKF0->mpCamera->getParameter(1); w.cx = pKF0->mpCamera->getParameter(2); w.cy = pKF0->mpCamera->getParameter(3);
    w.bf = pKF0->mbf;
    w.camera_model = pKF0->mpCamera->GetType() == pKF0->mpCamera->CAM_FISHEYE ? 1 : 0;
    for (int i = 0; i < 4; i++) w.kb[i] = w.camera_model ? (double)pKF0->mpCamera->getParameter(4 + i) : 0.0;
    if (pKF0->mpCamera2) {
        GeometricCamera *c2 = pKF0->mpCamera2;
        w.has_cam2 = 1;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) w.Trl[4 * r + c] = (double)pKF0->mTrl.at<float>(r, c);
        w.fx2 = c2->getParameter(0); w.fy2 = c2->getParameter(1); w.cx2 = c2->getParameter(2); w.cy2 = c2->getParameter(3);
        w.camera2_model = c2->GetType() == c2->CAM_FISHEYE ? 1 : 0;
        for (int i = 0; i < 4; i++) w.kb2[i] = w.camera2_model ? (double)c2->getParameter(4 + i) : 0.0;
    }

    // ---- IMU links (:503-608)
    std::vector<int32_t> in1, in2;
    std::vector<double> preint, info, infog, infoa;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKFi = vpKFs[i];
        if (!pKFi->mPrevKF) continue;                                          // "NOT INERTIAL LINK TO PREVIOUS FRAME!"
        if (pKFi->mnId > maxKFid) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        if (!(pKFi->bImu && pKFi->mPrevKF->bImu)) continue;
        if (!pKFi->mpImuPreintegrated) continue;
        pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());
        auto it1 = kfIndex.find(pKFi->mPrevKF), it2 = kfIndex.find(pKFi);
        if (it1 == kfIndex.end() || it2 == kfIndex.end()) continue;           // optimizer.vertex() == NULL: "Error", :545-560
        IMU::Preintegrated *pInt = pKFi->mpImuPreintegrated;
        in1.push_back(it1->second); in2.push_back(it2->second);
        const size_t o = preint.size();
        preint.resize(o + ORBHIP_IBA_PREINT);
        double *p = &preint[o];
        p[0] = (double)pInt->dT;
        put3x3(p + 1, pInt->dR); put3(p + 10, pInt->dV); put3(p + 13, pInt->dP);
        put3x3(p + 16, pInt->JRg); put3x3(p + 25, pInt->JVg); put3x3(p + 34, pInt->JVa); put3x3(p + 43, pInt->JPg); put3x3(p + 52, pInt->JPa);
        p[61] = pInt->b.bwx; p[62] = pInt->b.bwy; p[63] = pInt->b.bwz; p[64] = pInt->b.bax; p[65] = pInt->b.bay; p[66] = pInt->b.baz;
        double I9[81];
        optc::inertial_information(pInt->C, I9);
        info.insert(info.end(), I9, I9 + 81);
        if (!bInit) {
            double G[9], A[9];
            inv3_block(pInt->C, 9, G); inv3_block(pInt->C, 12, A);
            infog.insert(infog.end(), G, G + 9); infoa.insert(infoa.end(), A, A + 9);
        }
    }
    w.n_inertial = (int32_t)in1.size(); w.in_kf1 = in1.data(); w.in_kf2 = in2.data(); w.in_preint = preint.data(); w.in_info = info.data();
    w.in_info_g = bInit ? nullptr : infog.data(); w.in_info_a = bInit ? nullptr : infoa.data(); w.in_robust = nullptr;

    // ---- map points and their edges (:636-756)
    std::vector<bool> vbNotIncludedMP(vpMPs.size(), false);
    std::vector<double> points(3 * vpMPs.size() + 3, 0.0);
    std::vector<int32_t> eKF, ePoint;
    std::vector<double> obs, invS2;
    std::vector<uint8_t> stereo;
    for (size_t l = 0; l < vpMPs.size(); l++) {
        MapPoint *pMP = vpMPs[l];
        const cv::Mat Xw = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) points[3 * l + k] = (double)Xw.at<float>(k);
        const std::map<KeyFrame *, std::tuple<int, int>> observations = pMP->GetObservations();
        bool bAllFixed = true;
        for (auto &ob : observations) {
            KeyFrame *pKFi = ob.first;
            if (pKFi->mnId > maxKFid) continue;
            if (pKFi->isBad()) continue;
            auto it = kfIndex.find(pKFi);
            if (it == kfIndex.end()) continue;
            const int leftIndex = std::get<0>(ob.second);
            cv::KeyPoint kpUn;
            if (leftIndex != -1) {                                             // monocular (:664) or stereo (:690) observation
                kpUn = pKFi->mvKeysUn[leftIndex];
                const float ur = pKFi->mvuRight[leftIndex];
                if (!fixed[it->second]) bAllFixed = false;
                eKF.push_back(it->second); ePoint.push_back((int32_t)l);
                obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(ur);
                stereo.push_back(ur < 0 ? 0 : 1);
                invS2.push_back((double)pKFi->mvInvLevelSigma2[kpUn.octave]);
            }
            if (pKFi->mpCamera2) {                                             // monocular right observation (:718-747)
                int rightIndex = std::get<1>(ob.second);
                if (rightIndex != -1 && rightIndex < (int)pKFi->mvKeysRight.size()) {
                    rightIndex -= pKFi->NLeft;
                    kpUn = pKFi->mvKeysRight[rightIndex];
                    if (!fixed[it->second]) bAllFixed = false;
                    eKF.push_back(it->second); ePoint.push_back((int32_t)l);
                    obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(-1.0);
                    stereo.push_back(2);
                    invS2.push_back((double)pKFi->mvInvLevelSigma2[kpUn.octave]);
                }
            }
        }
        if (bAllFixed) vbNotIncludedMP[l] = true;                              // removeVertex(vPoint): the solver drops such a point's edges itself
    }
    w.n_points = (int32_t)vpMPs.size(); w.n_edges = (int32_t)eKF.size(); w.edge_kf = eKF.data(); w.edge_point = ePoint.data(); w.edge_obs = obs.data();
    w.edge_stereo = stereo.data(); w.edge_inv_sigma2 = invS2.data(); w.edge_close = nullptr;

    if (pbStopFlag)                                                            // :758-760
        if (*pbStopFlag) return;

    orbhip_ctx *ctx = hip::ThreadContext();
    if (!ctx) return;                                                          // one message from hip::ThreadContext ("no device context ... no CPU fallback")
    orbhip_fiba_params prm;
    orbhip_fiba_default_params(&prm, its, bInit ? 1 : 0, (double)priorG, (double)priorA);
    double *pk = kf.data(), *px = points.data();
    orbhip_fiba_stats st;
    const int rc = orbhip_full_inertial_ba_solve_batch(ctx, &w, 1, &prm, nullptr, &pk, &px, shared, &st);
    if (rc != ORBHIP_OK) { fprintf(stderr, "orbhip FullInertialBA: %d (%s); the map is left as it is (no CPU fallback)\n", rc, orbhip_last_error()); return; }

    // ---- recover optimized data (:767-850)
    for (int i = 0; i < nKF; i++) {
        KeyFrame *pKFi = vKF[i];
        const double *s = &kf[(size_t)ORBHIP_IBA_KF * i];
        cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);                              // Rcw[0] = Rcb Rwb^T, tcw[0] = -Rcw twb + tcb
        for (int r = 0; r < 3; r++) {
            double t = w.tcb[r];
            for (int c = 0; c < 3; c++) {
                double a = 0;
                for (int k = 0; k < 3; k++) a += w.Rcb[3 * r + k] * s[3 * c + k];
                Tcw.at<float>(r, c) = (float)a;
                t -= a * s[9 + c];
            }
            Tcw.at<float>(r, 3) = (float)t;
        }
        if (nLoopId == 0) pKFi->SetPose(Tcw);
        else { pKFi->mTcwGBA = Tcw; pKFi->mnBAGlobalForKF = nLoopId; }
        if (pKFi->bImu) {
            cv::Mat V(3, 1, CV_32F);
            for (int k = 0; k < 3; k++) V.at<float>(k) = (float)s[12 + k];
            if (nLoopId == 0) pKFi->SetVelocity(V);
            else pKFi->mVwbGBA = V;
            const double *vb = bInit ? shared : s + 15;                        // gyro 3, accelerometer 3
            const IMU::Bias b((float)vb[3], (float)vb[4], (float)vb[5], (float)vb[0], (float)vb[1], (float)vb[2]);
            if (nLoopId == 0) pKFi->SetNewBias(b);
            else pKFi->mBiasGBA = b;
        }
    }
    for (size_t l = 0; l < vpMPs.size(); l++) {
        if (vbNotIncludedMP[l]) continue;
        MapPoint *pMP = vpMPs[l];
        cv::Mat X(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) X.at<float>(k) = (float)points[3 * l + k];
        if (nLoopId == 0) { pMP->SetWorldPos(X); pMP->UpdateNormalAndDepth(); }
        else { pMP->mPosGBA = X; pMP->mnBAGlobalForKF = nLoopId; }
    }
    pMap->IncreaseChangeIndex();
}

}  // namespace ORB_SLAM3
