// Optimizer_InertialOptimization.cc -- the four overloads of Optimizer::InertialOptimization with the reference's signatures
// (include/Optimizer.h:115-118) around the HIP solver.  What stays host code, in the reference's order (src/Optimizer.cc): the walk over
// GetAllKeyFrames() (or the list) with its filters -- mnId > maxKFid (:5330, :5396), isBad() and a previous keyframe beyond maxKFid
// (:5398) -- SetNewBias of every used preintegration to its previous keyframe's bias (:5401; not in (d); applied once the solve has
// succeeded) -- and the write-back of
// :5440-5480: scale, biases, Rwg, every keyframe's velocity and SetNewBias(b), Reintegrate() where the gyro bias moved by more than
// 0.01.  What was the g2o block is flat packing plus ONE call of orbhip_inertial_optimization_host.
// The device call wants the keyframes in chain order: the walk follows the mPrevKF links, chain heads in mnId order.  A keyframe whose
// previous keyframe already has a successor among the used ones (a fork; the reference's graph would hold both edges) is reported
// and starts a chain of its own without that edge.  covInertial is never written (as in the reference); bGauss is unused there too.
// Without a device context: one message (hip::ThreadContext prints "no device context ... no CPU fallback"), every argument and
// keyframe stays as it was.
#include "Optimizer.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include "optimizer_common.h"

namespace ORB_SLAM3 {

namespace {

void put3x3(double *dst, const cv::Mat &m) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) dst[3 * r + c] = (double)m.at<float>(r, c); }
void put3(double *dst, const cv::Mat &m) { for (int r = 0; r < 3; r++) dst[r] = (double)m.at<float>(r); }

struct Packed {
    std::vector<KeyFrame *> order;           // chain order
    std::vector<double> kf, preint, info;
    std::vector<uint8_t> link;
};

// vertices: every keyframe of vpKFs with mnId <= maxKFid; edges as :5392-5432.  Changes nothing.
void pack(const std::vector<KeyFrame *> &vpKFs, long unsigned int maxKFid, Packed &P)
{
    std::map<KeyFrame *, int> vertex;        // optimizer.vertex(id) != NULL
    for (KeyFrame *pKFi : vpKFs)
        if (pKFi->mnId <= maxKFid) vertex[pKFi] = 1;
    std::map<KeyFrame *, KeyFrame *> next;   // previous keyframe -> the keyframe whose edge starts there
    std::map<KeyFrame *, bool> has_edge;     // the keyframe carries an edge to its previous one
    for (KeyFrame *pKFi : vpKFs) {
        if (!(pKFi->mPrevKF && pKFi->mnId <= maxKFid)) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        if (!vertex.count(pKFi->mPrevKF) || !pKFi->mpImuPreintegrated) { fprintf(stderr, "Optimizer::InertialOptimization: Error, no vertex / preintegration for the edge into keyframe %lu\n", pKFi->mnId); continue; }
        if (next.count(pKFi->mPrevKF)) { fprintf(stderr, "Optimizer::InertialOptimization: keyframe %lu has two successors, the edge into %lu is left out\n", pKFi->mPrevKF->mnId, pKFi->mnId); continue; }
        next[pKFi->mPrevKF] = pKFi;
        has_edge[pKFi] = true;
    }
    std::vector<KeyFrame *> heads;
    for (auto &v : vertex) if (!has_edge.count(v.first)) heads.push_back(v.first);
    std::sort(heads.begin(), heads.end(), [](KeyFrame *a, KeyFrame *b) { return a->mnId < b->mnId; });
    for (KeyFrame *h : heads)
        for (KeyFrame *k = h; k; k = next.count(k) ? next[k] : nullptr) { P.order.push_back(k); P.link.push_back(k == h ? 0 : 1); }
    const size_t n = P.order.size();
    P.kf.assign(n * ORBHIP_IBA_KF, 0.0); P.preint.assign(n * ORBHIP_IBA_PREINT, 0.0); P.info.assign(n * 81, 0.0);
    for (size_t i = 0; i < n; i++) {
        KeyFrame *pKFi = P.order[i];
        double *s = &P.kf[i * ORBHIP_IBA_KF];
        put3x3(s, pKFi->GetImuRotation()); put3(s + 9, pKFi->GetImuPosition());              // VertexPose(KeyFrame*), fixed
        put3(s + 12, pKFi->GetVelocity());                                                    // VertexVelocity(KeyFrame*)
        put3(s + 15, pKFi->GetGyroBias()); put3(s + 18, pKFi->GetAccBias());
        if (!P.link[i]) continue;
        IMU::Preintegrated *pInt = pKFi->mpImuPreintegrated;
        double *p = &P.preint[i * ORBHIP_IBA_PREINT];
        p[0] = (double)pInt->dT;
        put3x3(p + 1, pInt->dR); put3(p + 10, pInt->dV); put3(p + 13, pInt->dP);
        put3x3(p + 16, pInt->JRg); put3x3(p + 25, pInt->JVg); put3x3(p + 34, pInt->JVa); put3x3(p + 43, pInt->JPg); put3x3(p + 52, pInt->JPa);
        p[61] = pInt->b.bwx; p[62] = pInt->b.bwy; p[63] = pInt->b.bwz; p[64] = pInt->b.bax; p[65] = pInt->b.bay; p[66] = pInt->b.baz;
        optc::inertial_information(pInt->C, &P.info[i * 81]);
    }
}

// -> false: nothing was solved (no context, no keyframe, or the call failed) and nothing may be written back
bool solve(const std::vector<KeyFrame *> &vpKFs, long unsigned int maxKFid, int overload, bool mono, bool fixed_vel, float priorG, float priorA,
           double *glob, Packed &P)
{
    if (vpKFs.empty()) return false;
    orbhip_ctx *ctx = optc::thread_ctx();
    if (!ctx) return false;                                  // one message from hip::ThreadContext; no CPU fallback
    pack(vpKFs, maxKFid, P);
    KeyFrame *front = vpKFs.front();                         // VertexGyroBias(vpKFs.front()), VertexAccBias(vpKFs.front()) in every overload
    put3(glob + 10, front->GetGyroBias()); put3(glob + 13, front->GetAccBias());
    orbhip_inertial_opt_params prm;
    orbhip_inertial_opt_default_params(&prm, overload, mono ? 1 : 0, fixed_vel ? 1 : 0, priorG, priorA);
    const int rc = orbhip_inertial_optimization_host(ctx, &prm, (int)P.order.size(), P.kf.data(), P.link.data(), P.preint.data(), P.info.data(),
                                                     glob, nullptr, nullptr);
    if (rc != ORBHIP_OK) { fprintf(stderr, "Optimizer::InertialOptimization: device solve failed: %d (%s)\n", rc, orbhip_last_error()); return false; }
    // :5401, once the solve has succeeded (a failed call leaves everything as it was): every used preintegration takes its previous
    // keyframe's bias; (d) does not do this
    if (overload != 3)
        for (size_t i = 0; i < P.order.size(); i++)
            if (P.link[i]) P.order[i]->mpImuPreintegrated->SetNewBias(P.order[i]->mPrevKF->GetImuBias());
    return true;
}

// :5442-5480 (and the same lines of (b), (c)): velocity, SetNewBias(b), Reintegrate() where the gyro bias moved by more than 0.01
void write_back(const std::vector<KeyFrame *> &vpKFs, long unsigned int maxKFid, const Packed &P, const double *glob)
{
    const IMU::Bias b((float)glob[13], (float)glob[14], (float)glob[15], (float)glob[10], (float)glob[11], (float)glob[12]);
    const float cvbg[3] = {(float)glob[10], (float)glob[11], (float)glob[12]};
    std::map<KeyFrame *, size_t> row;
    for (size_t i = 0; i < P.order.size(); i++) row[P.order[i]] = i;
    IMU::Preintegrated::DeferredReintegration batch;         // the loop's Reintegrate() calls leave as ONE device call when it ends
    for (KeyFrame *pKFi : vpKFs) {
        if (pKFi->mnId > maxKFid) continue;
        const double *s = &P.kf[row[pKFi] * ORBHIP_IBA_KF];
        cv::Mat Vw(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) Vw.at<float>(r) = (float)s[12 + r];
        pKFi->SetVelocity(Vw);
        const cv::Mat g = pKFi->GetGyroBias();
        double d2 = 0;                                       // cv::norm of the float difference, accumulated in double
        for (int r = 0; r < 3; r++) { const float d = g.at<float>(r) - cvbg[r]; d2 += (double)d * (double)d; }
        if (std::sqrt(d2) > 0.01) {
            pKFi->SetNewBias(b);
            if (pKFi->mpImuPreintegrated) pKFi->mpImuPreintegrated->Reintegrate();
        } else
            pKFi->SetNewBias(b);
    }
}

}  // namespace

void Optimizer::InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale, Eigen::Vector3d &bg, Eigen::Vector3d &ba, bool bMono, Eigen::MatrixXd &covInertial, bool bFixedVel, bool bGauss, float priorG, float priorA)
{
    (void)covInertial; (void)bGauss;
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    double glob[ORBHIP_IO_GLOBAL];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) glob[3 * r + c] = Rwg(r, c);
    glob[9] = scale;
    Packed P;
    if (!solve(vpKFs, maxKFid, 0, bMono, bFixedVel, priorG, priorA, glob, P)) return;
    scale = glob[9];
    for (int r = 0; r < 3; r++) { bg[r] = glob[10 + r]; ba[r] = glob[13 + r]; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rwg(r, c) = glob[3 * r + c];
    write_back(vpKFs, maxKFid, P, glob);
}

void Optimizer::InertialOptimization(Map *pMap, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA)
{
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    double glob[ORBHIP_IO_GLOBAL] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0};       // VertexGDir(Identity), VertexScale(1.0), both fixed
    Packed P;
    if (!solve(vpKFs, maxKFid, 1, false, false, priorG, priorA, glob, P)) return;
    for (int r = 0; r < 3; r++) { bg[r] = glob[10 + r]; ba[r] = glob[13 + r]; }
    write_back(vpKFs, maxKFid, P, glob);
}

void Optimizer::InertialOptimization(std::vector<KeyFrame*> vpKFs, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA)
{
    if (vpKFs.empty()) return;
    const long unsigned int maxKFid = vpKFs[0]->GetMap()->GetMaxKFid();
    double glob[ORBHIP_IO_GLOBAL] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0};
    Packed P;
    if (!solve(vpKFs, maxKFid, 2, false, false, priorG, priorA, glob, P)) return;
    for (int r = 0; r < 3; r++) { bg[r] = glob[10 + r]; ba[r] = glob[13 + r]; }
    write_back(vpKFs, maxKFid, P, glob);
}

void Optimizer::InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale)
{
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    double glob[ORBHIP_IO_GLOBAL];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) glob[3 * r + c] = Rwg(r, c);
    glob[9] = scale;
    Packed P;
    if (!solve(vpKFs, maxKFid, 3, false, false, 0.f, 0.f, glob, P)) return;
    scale = glob[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rwg(r, c) = glob[3 * r + c];
}

}  // namespace ORB_SLAM3
