// ImuTypes.cc -- the IMU types of host/ImuTypes.h (src/ImuTypes.cc).  IntegrateNewMeasurement runs csrc/preint_core.h on the host, one
// step per call; Reintegrate / ReintegrateBatch / MergePrevious pack bias and measurement lists and make ONE orbhip_preintegrate_host
// call.  Without a usable GPU those three leave the object as it was (one message from hip::ThreadContext); there is no CPU fallback.
#include "ImuTypes.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include "hip_context.h"
#include "optimizer_common.h"
#include "../csrc/preint_core.h"
#include "../../include/orbhip.h"

namespace ORB_SLAM3 {
namespace IMU {

const float eps = 1e-4;
int Preintegrated::nDeviceCalls = 0;

namespace {

cv::Mat mat3(const float *m) { cv::Mat M(3, 3, CV_32F); for (int i = 0; i < 9; i++) M.at<float>(i / 3, i % 3) = m[i]; return M; }
cv::Mat vec3(const float *v) { cv::Mat M(3, 1, CV_32F); for (int i = 0; i < 3; i++) M.at<float>(i) = v[i]; return M; }
void get3x3(const cv::Mat &M, float *m) { for (int i = 0; i < 9; i++) m[i] = M.at<float>(i / 3, i % 3); }
void get3(const cv::Mat &M, float *v) { for (int i = 0; i < 3; i++) v[i] = M.at<float>(i); }
void skew3(float x, float y, float z, float *W) { const float w[9] = {0, -z, y, z, 0, -x, -y, x, 0}; for (int i = 0; i < 9; i++) W[i] = w[i]; }
// I + a W + b W W
cv::Mat rodrigues(float x, float y, float z, float a, float b)
{
    float W[9], W2[9], R[9];
    skew3(x, y, z, W); preint_mm3(W, W, W2);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.f : 0.f) + W[i] * a + W2[i] * b;
    return mat3(R);
}
void mul33v(const cv::Mat &M, const float *v, float *o) { for (int i = 0; i < 3; i++) o[i] = M.at<float>(i, 0) * v[0] + M.at<float>(i, 1) * v[1] + M.at<float>(i, 2) * v[2]; }

// the object's cv::Mat fields <-> the flat state of preint_core.h
void to_state(const Preintegrated &P, PreintState &S)
{
    S.dT = P.dT;
    get3x3(P.dR, S.dR); get3(P.dV, S.dV); get3(P.dP, S.dP); get3(P.avgA, S.avgA); get3(P.avgW, S.avgW);
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) {
            S.Jg[j][i] = P.JRg.at<float>(i, j); S.Jg[j][3 + i] = P.JVg.at<float>(i, j); S.Jg[j][6 + i] = P.JPg.at<float>(i, j);
            S.Ja[j][i] = 0.f; S.Ja[j][3 + i] = P.JVa.at<float>(i, j); S.Ja[j][6 + i] = P.JPa.at<float>(i, j);
        }
    for (int c = 0; c < 9; c++) for (int r = 0; r < 9; r++) S.C[c][r] = P.C.at<float>(c, r);
}
void from_state(const PreintState &S, Preintegrated &P)
{
    P.dT = S.dT;
    P.dR = mat3(S.dR); P.dV = vec3(S.dV); P.dP = vec3(S.dP); P.avgA = vec3(S.avgA); P.avgW = vec3(S.avgW);
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) {
            P.JRg.at<float>(i, j) = S.Jg[j][i]; P.JVg.at<float>(i, j) = S.Jg[j][3 + i]; P.JPg.at<float>(i, j) = S.Jg[j][6 + i];
            P.JVa.at<float>(i, j) = S.Ja[j][3 + i]; P.JPa.at<float>(i, j) = S.Ja[j][6 + i];
        }
    for (int c = 0; c < 9; c++) for (int r = 0; r < 9; r++) P.C.at<float>(c, r) = S.C[c][r];
}
void mat66(const cv::Mat &M, float *o) { for (int i = 0; i < 36; i++) o[i] = M.at<float>(i / 6, i % 6); }

// one device record (ORBHIP_IBA_PREINT doubles, 225 + 6 floats) into the object's fields
void from_record(const double *r, const float *cov, const float *avg, Preintegrated &P)
{
    float m[9];
    auto m3 = [&](int o) { for (int i = 0; i < 9; i++) m[i] = (float)r[o + i]; return mat3(m); };
    auto v3 = [&](int o) { for (int i = 0; i < 3; i++) m[i] = (float)r[o + i]; return vec3(m); };
    P.dT = (float)r[0];
    P.dR = m3(1); P.dV = v3(10); P.dP = v3(13); P.JRg = m3(16); P.JVg = m3(25); P.JVa = m3(34); P.JPg = m3(43); P.JPa = m3(52);
    P.avgA = vec3(avg); P.avgW = vec3(avg + 3);
    P.C = cv::Mat(15, 15, CV_32F);
    for (int i = 0; i < 225; i++) P.C.at<float>(i / 15, i % 15) = cov[i];
    P.Info = cv::Mat();
}

}  // namespace

cv::Mat NormalizeRotation(const cv::Mat &R) { float m[9]; get3x3(R, m); preint_normalize(m); return mat3(m); }
cv::Mat Skew(const cv::Mat &v) { float W[9]; skew3(v.at<float>(0), v.at<float>(1), v.at<float>(2), W); return mat3(W); }
cv::Mat ExpSO3(const float &x, const float &y, const float &z)
{
    const float d2 = x * x + y * y + z * z, d = std::sqrt(d2);
    if (d < eps) return rodrigues(x, y, z, 1.f, 0.5f);
    return rodrigues(x, y, z, std::sin(d) / d, (1.0f - std::cos(d)) / d2);
}
cv::Mat ExpSO3(const cv::Mat &v) { return ExpSO3(v.at<float>(0), v.at<float>(1), v.at<float>(2)); }
cv::Mat LogSO3(const cv::Mat &R)
{
    const float tr = R.at<float>(0, 0) + R.at<float>(1, 1) + R.at<float>(2, 2);
    float w[3] = {(R.at<float>(2, 1) - R.at<float>(1, 2)) / 2, (R.at<float>(0, 2) - R.at<float>(2, 0)) / 2, (R.at<float>(1, 0) - R.at<float>(0, 1)) / 2};
    const float costheta = (tr - 1.0f) * 0.5f;
    if (costheta > 1 || costheta < -1) return vec3(w);
    const float theta = std::acos(costheta), s = std::sin(theta);
    if (std::fabs(s) < eps) return vec3(w);
    for (float &c : w) c = theta * c / s;
    return vec3(w);
}
cv::Mat RightJacobianSO3(const float &x, const float &y, const float &z)
{
    const float d2 = x * x + y * y + z * z, d = std::sqrt(d2);
    if (d < eps) return cv::Mat::eye(3, 3, CV_32F);
    return rodrigues(x, y, z, -(1.0f - std::cos(d)) / d2, (d - std::sin(d)) / (d2 * d));
}
cv::Mat RightJacobianSO3(const cv::Mat &v) { return RightJacobianSO3(v.at<float>(0), v.at<float>(1), v.at<float>(2)); }
cv::Mat InverseRightJacobianSO3(const float &x, const float &y, const float &z)
{
    const float d2 = x * x + y * y + z * z, d = std::sqrt(d2);
    if (d < eps) return cv::Mat::eye(3, 3, CV_32F);
    return rodrigues(x, y, z, 0.5f, 1.0f / d2 - (1.0f + std::cos(d)) / (2.0f * d * std::sin(d)));
}
cv::Mat InverseRightJacobianSO3(const cv::Mat &v) { return InverseRightJacobianSO3(v.at<float>(0), v.at<float>(1), v.at<float>(2)); }

IntegratedRotation::IntegratedRotation(const cv::Point3f &angVel, const Bias &imuBias, const float &time) : deltaT(time)
{
    const float bg[3] = {imuBias.bwx, imuBias.bwy, imuBias.bwz}, ba[3] = {0, 0, 0}, m[7] = {0, 0, 0, angVel.x, angVel.y, angVel.z, time};
    PreintMeas M;
    preint_measure(bg, ba, m, M);
    deltaR = mat3(M.E);
    rightJ = RightJacobianSO3(M.accW[0] * time, M.accW[1] * time, M.accW[2] * time);
}

void Calib::Set(const cv::Mat &Tbc_, const float &ng, const float &na, const float &ngw, const float &naw)
{
    Tbc = Tbc_.clone();
    Tcb = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) {
        float t = 0;
        for (int j = 0; j < 3; j++) { Tcb.at<float>(i, j) = Tbc.at<float>(j, i); t += Tbc.at<float>(j, i) * Tbc.at<float>(j, 3); }
        Tcb.at<float>(i, 3) = -t;
    }
    Cov = cv::Mat::eye(6, 6, CV_32F);
    CovWalk = cv::Mat::eye(6, 6, CV_32F);
    const float ng2 = ng * ng, na2 = na * na, ngw2 = ngw * ngw, naw2 = naw * naw;
    for (int i = 0; i < 3; i++) {
        Cov.at<float>(i, i) = ng2; Cov.at<float>(3 + i, 3 + i) = na2;
        CovWalk.at<float>(i, i) = ngw2; CovWalk.at<float>(3 + i, 3 + i) = naw2;
    }
}

Preintegrated::Preintegrated(const Bias &b_, const Calib &calib)
{
    Nga = calib.Cov.clone();
    NgaWalk = calib.CovWalk.clone();
    Initialize(b_);
}

// Copy constructor
Preintegrated::Preintegrated(Preintegrated *pImuPre)
    : dT(pImuPre->dT), C(pImuPre->C.clone()), Info(pImuPre->Info.clone()), Nga(pImuPre->Nga.clone()), NgaWalk(pImuPre->NgaWalk.clone()),
      b(pImuPre->b), dR(pImuPre->dR.clone()), dV(pImuPre->dV.clone()), dP(pImuPre->dP.clone()), JRg(pImuPre->JRg.clone()),
      JVg(pImuPre->JVg.clone()), JVa(pImuPre->JVa.clone()), JPg(pImuPre->JPg.clone()), JPa(pImuPre->JPa.clone()), avgA(pImuPre->avgA.clone()),
      avgW(pImuPre->avgW.clone()), bu(pImuPre->bu), db(pImuPre->db.clone()), mvMeasurements(pImuPre->mvMeasurements)
{
}

void Preintegrated::CopyFrom(Preintegrated *pImuPre)
{
    dT = pImuPre->dT;
    C = pImuPre->C.clone(); Info = pImuPre->Info.clone(); Nga = pImuPre->Nga.clone(); NgaWalk = pImuPre->NgaWalk.clone();
    b.CopyFrom(pImuPre->b);
    dR = pImuPre->dR.clone(); dV = pImuPre->dV.clone(); dP = pImuPre->dP.clone();
    JRg = pImuPre->JRg.clone(); JVg = pImuPre->JVg.clone(); JVa = pImuPre->JVa.clone(); JPg = pImuPre->JPg.clone(); JPa = pImuPre->JPa.clone();
    avgA = pImuPre->avgA.clone(); avgW = pImuPre->avgW.clone();
    bu.CopyFrom(pImuPre->bu);
    db = pImuPre->db.clone();
    mvMeasurements = pImuPre->mvMeasurements;
}

void Preintegrated::Initialize(const Bias &b_)
{
    dR = cv::Mat::eye(3, 3, CV_32F);
    dV = cv::Mat::zeros(3, 1, CV_32F);
    dP = cv::Mat::zeros(3, 1, CV_32F);
    JRg = cv::Mat::zeros(3, 3, CV_32F);
    JVg = cv::Mat::zeros(3, 3, CV_32F);
    JVa = cv::Mat::zeros(3, 3, CV_32F);
    JPg = cv::Mat::zeros(3, 3, CV_32F);
    JPa = cv::Mat::zeros(3, 3, CV_32F);
    C = cv::Mat::zeros(15, 15, CV_32F);
    Info = cv::Mat();
    db = cv::Mat::zeros(6, 1, CV_32F);
    b = b_;
    bu = b_;
    avgA = cv::Mat::zeros(3, 1, CV_32F);
    avgW = cv::Mat::zeros(3, 1, CV_32F);
    dT = 0.0f;
    mvMeasurements.clear();
}

void Preintegrated::IntegrateNewMeasurement(const cv::Point3f &acceleration, const cv::Point3f &angVel, const float &dt)
{
    mvMeasurements.push_back(integrable(acceleration, angVel, dt));
    const float bg[3] = {b.bwx, b.bwy, b.bwz}, ba[3] = {b.bax, b.bay, b.baz};
    const float m[7] = {acceleration.x, acceleration.y, acceleration.z, angVel.x, angVel.y, angVel.z, dt};
    float nga[36];
    mat66(Nga, nga);
    PreintState S;
    to_state(*this, S);
    preint_step(S, bg, ba, m, nga);
    from_state(S, *this);
    for (int i = 9; i < 15; i++) for (int j = 9; j < 15; j++) C.at<float>(i, j) = C.at<float>(i, j) + NgaWalk.at<float>(i - 9, j - 9);
}

int Preintegrated::ReintegrateBatch(const std::vector<Preintegrated *> &vpPre)
{
    std::vector<Preintegrated *> v;
    for (Preintegrated *p : vpPre)                                                      // an object listed twice is integrated once
        if (p && !p->Nga.empty() && std::find(v.begin(), v.end(), p) == v.end()) v.push_back(p);
    if (v.empty()) return ORBHIP_OK;
    orbhip_ctx *ctx = hip::ThreadContext();
    if (!ctx) return ORBHIP_E_NODEVICE;
    // one call has one Nga / NgaWalk: objects are grouped by their noise (one group in every configuration the reference ships)
    std::vector<char> done(v.size(), 0);
    for (size_t g = 0; g < v.size(); g++) {
        if (done[g]) continue;
        orbhip_preint_params prm;
        orbhip_preint_default_params(&prm, 0.f, 0.f, 0.f, 0.f);
        prm.want_info = 0;
        mat66(v[g]->Nga, prm.nga); mat66(v[g]->NgaWalk, prm.nga_walk);
        std::vector<size_t> grp;
        for (size_t i = g; i < v.size(); i++) {
            if (done[i]) continue;
            float a[36], w[36];
            mat66(v[i]->Nga, a); mat66(v[i]->NgaWalk, w);
            bool same = true;
            for (int k = 0; k < 36; k++) same = same && a[k] == prm.nga[k] && w[k] == prm.nga_walk[k];
            if (same) { grp.push_back(i); done[i] = 1; }
        }
        std::vector<int32_t> off(1, 0);
        std::vector<float> meas;
        std::vector<double> rec(grp.size() * ORBHIP_IBA_PREINT, 0.0);
        for (size_t k = 0; k < grp.size(); k++) {                                       // packed under the object's lock, which is then released
            Preintegrated *p = v[grp[k]];
            std::unique_lock<std::mutex> lock(p->mMutex);
            for (const integrable &m : p->mvMeasurements) { const float r[7] = {m.a.x, m.a.y, m.a.z, m.w.x, m.w.y, m.w.z, m.t}; meas.insert(meas.end(), r, r + 7); }
            off.push_back((int32_t)(meas.size() / 7));
            double *r = &rec[k * ORBHIP_IBA_PREINT];                                     // Initialize(bu)
            r[61] = p->bu.bwx; r[62] = p->bu.bwy; r[63] = p->bu.bwz; r[64] = p->bu.bax; r[65] = p->bu.bay; r[66] = p->bu.baz;
        }
        std::vector<float> cov(grp.size() * 225, 0.f), avg(grp.size() * 6, 0.f);
        nDeviceCalls++;
        const int rc = orbhip_preintegrate_host(ctx, &prm, (int)grp.size(), off.data(), meas.data(), nullptr, rec.data(), cov.data(), avg.data(),
                                                nullptr, nullptr, nullptr);
        if (rc != ORBHIP_OK) { fprintf(stderr, "IMU::Preintegrated: device preintegration failed: %d (%s)\n", rc, orbhip_last_error()); return rc; }
        for (size_t k = 0; k < grp.size(); k++) {
            Preintegrated *p = v[grp[k]];
            std::unique_lock<std::mutex> lock(p->mMutex);
            const double *r = &rec[k * ORBHIP_IBA_PREINT];
            from_record(r, &cov[k * 225], &avg[k * 6], *p);
            p->b = Bias((float)r[64], (float)r[65], (float)r[66], (float)r[61], (float)r[62], (float)r[63]);      // the bias that was integrated at
            p->db = cv::Mat::zeros(6, 1, CV_32F);                                        // bu - b: zero unless SetNewBias ran meanwhile
            p->db.at<float>(0) = p->bu.bwx - p->b.bwx; p->db.at<float>(1) = p->bu.bwy - p->b.bwy; p->db.at<float>(2) = p->bu.bwz - p->b.bwz;
            p->db.at<float>(3) = p->bu.bax - p->b.bax; p->db.at<float>(4) = p->bu.bay - p->b.bay; p->db.at<float>(5) = p->bu.baz - p->b.baz;
        }
    }
    return ORBHIP_OK;
}

void Preintegrated::MergePrevious(Preintegrated *pPrev)
{
    if (pPrev == this) return;
    {
        std::unique_lock<std::mutex> lock1(mMutex);
        std::unique_lock<std::mutex> lock2(pPrev->mMutex);
        std::vector<integrable> all = pPrev->mvMeasurements;
        all.insert(all.end(), mvMeasurements.begin(), mvMeasurements.end());
        mvMeasurements.swap(all);
    }
    if (Nga.empty()) return;
    // Initialize(bav) with bav = bu, then both lists in order: what one re-integration of the joined list at bu computes
    ReintegrateBatch(std::vector<Preintegrated *>(1, this));
}

IMU::Bias Preintegrated::GetDeltaBias(const Bias &b_)
{
    std::unique_lock<std::mutex> lock(mMutex);
    return IMU::Bias(b_.bax - b.bax, b_.bay - b.bay, b_.baz - b.baz, b_.bwx - b.bwx, b_.bwy - b.bwy, b_.bwz - b.bwz);
}

namespace {
cv::Mat corrected_rotation(const cv::Mat &dR, const cv::Mat &JRg, const float *dbg)
{
    float w[3], a[9], e[9], r[9];
    mul33v(JRg, dbg, w);
    get3x3(dR, a); get3x3(ExpSO3(w[0], w[1], w[2]), e);
    preint_mm3(a, e, r);
    preint_normalize(r);
    return mat3(r);
}
cv::Mat corrected_vector(const cv::Mat &d, const cv::Mat &Jg, const cv::Mat &Ja, const float *dbg, const float *dba)
{
    float g[3], a[3], o[3];
    mul33v(Jg, dbg, g); mul33v(Ja, dba, a);
    for (int i = 0; i < 3; i++) o[i] = d.at<float>(i) + g[i] + a[i];
    return vec3(o);
}
}  // namespace

cv::Mat Preintegrated::GetDeltaRotation(const Bias &b_)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const float dbg[3] = {b_.bwx - b.bwx, b_.bwy - b.bwy, b_.bwz - b.bwz};
    return corrected_rotation(dR, JRg, dbg);
}
cv::Mat Preintegrated::GetDeltaVelocity(const Bias &b_)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const float dbg[3] = {b_.bwx - b.bwx, b_.bwy - b.bwy, b_.bwz - b.bwz}, dba[3] = {b_.bax - b.bax, b_.bay - b.bay, b_.baz - b.baz};
    return corrected_vector(dV, JVg, JVa, dbg, dba);
}
cv::Mat Preintegrated::GetDeltaPosition(const Bias &b_)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const float dbg[3] = {b_.bwx - b.bwx, b_.bwy - b.bwy, b_.bwz - b.bwz}, dba[3] = {b_.bax - b.bax, b_.bay - b.bay, b_.baz - b.baz};
    return corrected_vector(dP, JPg, JPa, dbg, dba);
}
cv::Mat Preintegrated::GetUpdatedDeltaRotation()
{
    std::unique_lock<std::mutex> lock(mMutex);
    return corrected_rotation(dR, JRg, db.ptr<float>(0));
}
cv::Mat Preintegrated::GetUpdatedDeltaVelocity()
{
    std::unique_lock<std::mutex> lock(mMutex);
    return corrected_vector(dV, JVg, JVa, db.ptr<float>(0), db.ptr<float>(3));
}
cv::Mat Preintegrated::GetUpdatedDeltaPosition()
{
    std::unique_lock<std::mutex> lock(mMutex);
    return corrected_vector(dP, JPg, JPa, db.ptr<float>(0), db.ptr<float>(3));
}
cv::Mat Preintegrated::GetOriginalDeltaRotation() { std::unique_lock<std::mutex> lock(mMutex); return dR.clone(); }
cv::Mat Preintegrated::GetOriginalDeltaVelocity() { std::unique_lock<std::mutex> lock(mMutex); return dV.clone(); }
cv::Mat Preintegrated::GetOriginalDeltaPosition() { std::unique_lock<std::mutex> lock(mMutex); return dP.clone(); }
Bias Preintegrated::GetOriginalBias() { std::unique_lock<std::mutex> lock(mMutex); return b; }
Bias Preintegrated::GetUpdatedBias() { std::unique_lock<std::mutex> lock(mMutex); return bu; }
cv::Mat Preintegrated::GetDeltaBias() { std::unique_lock<std::mutex> lock(mMutex); return db.clone(); }

// Info(0:9, 0:9) = C(0:9, 0:9).inv(DECOMP_SVD) as the optimisers here compute it (optc::inertial_information, in double, rounded to
// the float Info the reference keeps), the walk diagonal 1 / C(i, i)
Eigen::Matrix<double, 15, 15> Preintegrated::GetInformationMatrix()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (Info.empty()) {
        Info = cv::Mat::zeros(15, 15, CV_32F);
        double info[81];
        optc::inertial_information(C, info);
        for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) Info.at<float>(i, j) = (float)info[9 * i + j];
        for (int i = 9; i < 15; i++) Info.at<float>(i, i) = 1.0f / C.at<float>(i, i);
    }
    Eigen::Matrix<double, 15, 15> EI;
    for (int i = 0; i < 15; i++) for (int j = 0; j < 15; j++) EI(i, j) = Info.at<float>(i, j);
    return EI;
}

}  // namespace IMU
}  // namespace ORB_SLAM3
