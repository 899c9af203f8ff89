// slam_types.h -- minimal stand-ins for the reference's Frame / KeyFrame / MapPoint / Map / GeometricCamera, exposing ONLY the
// members and accessors that the hot-path callers' code touches (reference include/Frame.h, KeyFrame.h, MapPoint.h, Map.h,
// CameraModels/GeometricCamera.h -- same names, same types, same meaning), so that host/Optimizer_LocalBA.cc and
// host/ORBmatcher.cc compile and run in this image (no OpenCV, no Eigen, no reference build).  In a real integration define
// ORBHIP_WITH_ORBSLAM3 and the reference's own headers are included instead; nothing in the shims depends on anything that is
// not in the reference's classes.  These are plain containers: the pointer graph, not its maintenance (covisibility updates,
// culling ...), which stays the caller's.
#pragma once
#ifdef ORBHIP_WITH_ORBSLAM3
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"
#include "CameraModels/GeometricCamera.h"
#else
#include <algorithm>
#include <cmath>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>
#include <vector>
#include "cvlite.h"
#include "eigen_lite.h"
#include "ImuTypes.h"       // include/ImuTypes.h: IMU::Point, Bias, Calib, Preintegrated (host/ImuTypes.cc)

namespace ORB_SLAM3 {

class KeyFrame;
class Map;
class TwoViewReconstruction;
}  // namespace ORB_SLAM3

// Thirdparty/DBoW2/DBoW2/FeatureVector.h:25-56: vocabulary node -> indices of the features below it
namespace DBoW2 {
typedef unsigned int NodeId;
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {
public:
    void addFeature(NodeId id, unsigned int i_feature) { (*this)[id].push_back(i_feature); }
};
}  // namespace DBoW2

// The smallest part of g2o::Sim3 that Optimizer::OptimizeSim3 and its two call sites (src/LoopClosing.cc:523-532, :736-742) touch,
// written from the interface (Thirdparty/g2o/g2o/types/sim3.h): the Sim3 group law only (below; the Eigen part is eigen_lite.h).
// Thirdparty/DBoW2/DBoW2/BowVector.h:52-110: word id -> value, ascending (what KeyFrameDatabase walks); TemplatedVocabulary.h as far as
// KeyFrameDatabase's constructor needs it (size())
namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
}  // namespace DBoW2
namespace ORB_SLAM3 {
class ORBVocabulary {
public:
    explicit ORBVocabulary(unsigned int nWords = 0) : mnWords(nWords) {}
    unsigned int size() const { return mnWords; }
private:
    unsigned int mnWords;
};
}  // namespace ORB_SLAM3


namespace g2o {
class Sim3 {
public:
    Sim3() : s(1.) {}
    Sim3(const Eigen::Quaterniond &r_, const Eigen::Vector3d &t_, double s_) : r(r_), t(t_), s(s_) {}
    Sim3(const Eigen::Matrix3d &R, const Eigen::Vector3d &t_, double s_) : r(Eigen::Quaterniond(R)), t(t_), s(s_) {}
    Eigen::Vector3d map(const Eigen::Vector3d &xyz) const
    {
        const Eigen::Vector3d a = r * xyz;
        Eigen::Vector3d o;
        for (int i = 0; i < 3; i++) o[i] = s * a[i] + t[i];
        return o;
    }
    Sim3 inverse() const
    {
        Eigen::Vector3d m;
        for (int i = 0; i < 3; i++) m[i] = (-1. / s) * t[i];
        return Sim3(r.conjugate(), r.conjugate() * m, 1. / s);
    }
    Sim3 operator*(const Sim3 &other) const
    {
        Sim3 ret;
        ret.r = r * other.r;
        const Eigen::Vector3d a = r * other.t;
        for (int i = 0; i < 3; i++) ret.t[i] = s * a[i] + t[i];
        ret.s = s * other.s;
        return ret;
    }
    const Eigen::Vector3d &translation() const { return t; }
    Eigen::Vector3d &translation() { return t; }
    const Eigen::Quaterniond &rotation() const { return r; }
    Eigen::Quaterniond &rotation() { return r; }
    const double &scale() const { return s; }
    double &scale() { return s; }
private:
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s;
};
}  // namespace g2o

namespace ORB_SLAM3 {

// include/Converter.h: the three conversions the Sim3 call sites use (src/Converter.cc:52-58, 117-123, 133-142)
class Converter {
public:
    static Eigen::Matrix<double, 3, 1> toVector3d(const cv::Mat &cvVector)
    {
        Eigen::Matrix<double, 3, 1> v;
        for (int i = 0; i < 3; i++) v[i] = cvVector.at<float>(i);
        return v;
    }
    static Eigen::Matrix<double, 3, 3> toMatrix3d(const cv::Mat &cvMat3)
    {
        Eigen::Matrix<double, 3, 3> M;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M(i, j) = cvMat3.at<float>(i, j);
        return M;
    }
    static cv::Mat toCvSE3(const Eigen::Matrix<double, 3, 3> &R, const Eigen::Matrix<double, 3, 1> &t)      // src/Converter.cc:85-102
    {
        cv::Mat m = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m.at<float>(i, j) = (float)R(i, j); m.at<float>(i, 3) = (float)t(i); }
        return m;
    }
    static cv::Mat toCvMat(const Eigen::Matrix<double, 3, 1> &v)    // src/Converter.cc:76-83
    {
        cv::Mat m(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) m.at<float>(i) = (float)v(i);
        return m;
    }
    static cv::Mat toCvMat(const g2o::Sim3 &Sim3)                   // toCvSE3(s * R, t)
    {
        const Eigen::Matrix3d R = Sim3.rotation().toRotationMatrix();
        cv::Mat m = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) m.at<float>(i, j) = (float)(Sim3.scale() * R(i, j)); m.at<float>(i, 3) = (float)Sim3.translation()[i]; }
        return m;
    }
};


// include/CameraModels/GeometricCamera.h:36-104 (type tag + parameter vector; project(cv::Mat) as Pinhole.cpp:34-39 /
// KannalaBrandt8.cpp:52-69 compute it, in float)
class GeometricCamera {
public:
    GeometricCamera(const std::vector<float> &p, unsigned int type) : mvParameters(p), mnType(type) {}
    float getParameter(const int i) { return mvParameters[i]; }
    size_t size() { return mvParameters.size(); }
    unsigned int GetType() { return mnType; }
    const unsigned int CAM_PINHOLE = 0;
    const unsigned int CAM_FISHEYE = 1;
    cv::Point2f project(const cv::Mat &m3D)
    {
        const float *p = m3D.ptr<float>();
        const float x = m3D.cols == 1 ? m3D.at<float>(0) : p[0], y = m3D.cols == 1 ? m3D.at<float>(1) : p[1], z = m3D.cols == 1 ? m3D.at<float>(2) : p[2];
        return project(cv::Point3f(x, y, z));
    }
    cv::Point2f project(const cv::Point3f &p3D)
    {
        const float x = p3D.x, y = p3D.y, z = p3D.z;
        if (mnType == 0) return cv::Point2f(mvParameters[0] * x / z + mvParameters[2], mvParameters[1] * y / z + mvParameters[3]);
        const float x2_plus_y2 = x * x + y * y;
        const float theta = atan2f(sqrtf(x2_plus_y2), z), psi = atan2f(y, x);
        const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
        const float r = theta + mvParameters[4] * theta3 + mvParameters[5] * theta5 + mvParameters[6] * theta7 + mvParameters[7] * theta9;
        return cv::Point2f(mvParameters[0] * r * cosf(psi) + mvParameters[2], mvParameters[1] * r * sinf(psi) + mvParameters[3]);
    }
    // Pinhole.cpp:105-120 / KannalaBrandt8.cpp:202-233 (defined in host/TwoViewReconstruction.cc): the pinhole camera passes the keys
    // through, the fisheye camera first undistorts both key sets to the pinhole K; `tvr` is created on the first call as there
    bool ReconstructWithTwoViews(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2, const std::vector<int> &vMatches12,
                                 cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);
    cv::Mat toK();
    std::vector<cv::Point2f> UndistortToPinhole(const std::vector<cv::KeyPoint> &vKeys) const;   // the fisheye correction of KannalaBrandt8.cpp:209-225
    const std::vector<std::vector<size_t>> &LastSets() const;          // the RANSAC sets of the latest call (test plumbing, host_smoke tvr)
protected:
    std::vector<float> mvParameters;
    unsigned int mnType;
    std::shared_ptr<TwoViewReconstruction> tvr;
};

// include/MapPoint.h (the members Optimizer.cc:1699-2344 and ORBmatcher.cc:48-218, 1965-2181 read or write)
class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &Pos, Map *pMap) : mnId(id), mnBALocalForKF(0), mTrackProjX(0), mTrackProjY(0),
        mTrackDepth(0), mTrackDepthR(0), mTrackProjXR(0), mTrackProjYR(0), mbTrackInView(false), mbTrackInViewR(false),
        mnTrackScaleLevel(0), mnTrackScaleLevelR(-1), mTrackViewCos(1), mTrackViewCosR(1), mWorldPos(Pos.clone()), mpMap(pMap),
        mbBad(false), nObs(0), nNormalUpdates(0), mfMinDistance(0), mfMaxDistance(0), mNormalVector(cv::Mat::zeros(3, 1, CV_32F)), mpReplaced(nullptr) {}
    // MapPoint(Pos, pRefKF, pMap) (src/MapPoint.cc:44-68): what LocalMapping::CreateNewMapPoints constructs; ids count up from nNextId
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : MapPoint(nNextId++, Pos, pMap) { mpRefKF = pRefKF; }
    static inline long unsigned int nNextId = 0;                      // include/MapPoint.h:133 (defined in MapPoint.cc:27 there)
    KeyFrame *mpRefKF = nullptr;
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }             // src/MapPoint.cc:109-113
    // what LoopClosing::CorrectLoop leaves for Optimizer::OptimizeEssentialGraph (include/MapPoint.h:143-144, src/LoopClosing.cc:1171-1173)
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    void ComputeDistinctiveDescriptors() { nDescriptorUpdates++; }    // MapPoint.cc:304-380 is orbhip_distinctive_descriptors_device's; the stand-in counts the calls
    int nDescriptorUpdates = 0;
    // MapPoint.cc:116-127: SetWorldPos takes the class-wide mGlobalMutex (what Optimizer::PoseOptimization holds while it snapshots the
    // positions, Optimizer.cc:895) and then the point's own mMutexPos; GetWorldPos the latter only
    void SetWorldPos(const cv::Mat &Pos) { std::unique_lock<std::mutex> lock2(mGlobalMutex); std::unique_lock<std::mutex> lock(mMutexPos); mWorldPos = Pos.clone(); }
    cv::Mat GetWorldPos() { std::unique_lock<std::mutex> lock(mMutexPos); return mWorldPos.clone(); }
    static inline std::mutex mGlobalMutex;                            // include/MapPoint.h:226 (defined in MapPoint.cc:28 there)
    std::map<KeyFrame *, std::tuple<int, int>> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    // stand-in helper of the test programs (not a reference method): both indices of an observation at once
    void AddObservation(KeyFrame *pKF, int idxLeft, int idxRight) { mObservations[pKF] = std::make_tuple(idxLeft, idxRight); nObs += (idxLeft != -1) + (idxRight != -1); }
    inline void AddObservation(KeyFrame *pKF, int idx);               // src/MapPoint.cc:114-139 (defined below KeyFrame)
    std::tuple<int, int> GetIndexInKeyFrame(KeyFrame *pKF)             // MapPoint.cc:412-419
    {
        auto it = mObservations.find(pKF);
        return it != mObservations.end() ? it->second : std::tuple<int, int>(-1, -1);
    }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }          // MapPoint.cc:421-425
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }                   // MapPoint.cc:502-506
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }                   // MapPoint.cc:508-512
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    template <class T> int PredictScale(const float &currentDist, T *pKF)               // MapPoint.cc:514-546 (KeyFrame* and Frame* overloads)
    {
        const float ratio = mfMaxDistance / currentDist;
        int nScale = std::ceil(std::log(ratio) / pKF->mfLogScaleFactor);
        if (nScale < 0) nScale = 0;
        else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
        return nScale;
    }
    // MapPoint.cc:233-300 moves the observations over and flags this point bad; the stand-in records the decision (the tests compare it)
    void Replace(MapPoint *pMP) { if (pMP != this) { mpReplaced = pMP; mbBad = true; } }
    MapPoint *GetReplaced() { return mpReplaced; }
    inline void EraseObservation(KeyFrame *pKF);                      // src/MapPoint.cc:168-201 (defined below KeyFrame)
    bool isBad() { return mbBad; }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    void UpdateNormalAndDepth() { nNormalUpdates++; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }               // MapPoint.cc:312-316
    int mnVisible = 1;                                                // MapPoint.cc:33, :42
    long unsigned int mnLastFrameSeen = 0;                            // include/MapPoint.h:201 (Tracking::SearchLocalPoints)
    Map *GetMap() { return mpMap; }
    long unsigned int mnId;
    long unsigned int mnBALocalForKF;
    long unsigned int mnBALocalForMerge = 0;
    // what a global BA leaves for LoopClosing::RunGlobalBundleAdjustment to propagate (include/MapPoint.h:146-147)
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF = 0;
    // Tracking's per-frame projection record (Frame::isInFrustum fills it; ORBmatcher.cc:57-79 reads it)
    float mTrackProjX, mTrackProjY, mTrackDepth, mTrackDepthR, mTrackProjXR, mTrackProjYR;
    bool mbTrackInView, mbTrackInViewR;
    int mnTrackScaleLevel, mnTrackScaleLevelR;
    float mTrackViewCos, mTrackViewCosR;
    cv::Mat mDescriptor;
    // stand-in state
    cv::Mat mWorldPos;
    std::mutex mMutexPos;
    std::map<KeyFrame *, std::tuple<int, int>> mObservations;
    Map *mpMap;
    bool mbBad;
    int nObs, nNormalUpdates;
    float mfMinDistance, mfMaxDistance;
    cv::Mat mNormalVector;
    MapPoint *mpReplaced;
};

// include/KeyFrame.h
class KeyFrame {
public:
    KeyFrame(long unsigned int id, Map *pMap, float fx_, float fy_, float cx_, float cy_, float mbf_, GeometricCamera *cam)
        : mnId(id), mnBALocalForKF(0), mnBAFixedForKF(0), fx(fx_), fy(fy_), cx(cx_), cy(cy_), mbf(mbf_), mpCamera(cam), mpCamera2(nullptr),
          NLeft(-1), mPrevKF(nullptr), mNextKF(nullptr), bImu(false), mpImuPreintegrated(nullptr), mpMap(pMap), mbBad(false) {}
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); }
    cv::Mat GetPose() { return Tcw.clone(); }
    // src/KeyFrame.cc:131-160, 1176-1262: pose parts in the reference's float cv::Mat arithmetic (products accumulated in double,
    // one rounding per element, as cv::gemm does for CV_32F)
    cv::Mat GetRotation() { cv::Mat R(3, 3, CV_32F); for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.at<float>(i, j) = Tcw.at<float>(i, j); return R; }
    cv::Mat GetTranslation() { cv::Mat t(3, 1, CV_32F); for (int i = 0; i < 3; i++) t.at<float>(i) = Tcw.at<float>(i, 3); return t; }
    cv::Mat GetCameraCenter()                               // Ow = -Rwc * tcw (KeyFrame.cc:113-118, SetPose)
    {
        cv::Mat o(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)Tcw.at<float>(k, i) * (double)Tcw.at<float>(k, 3);
            o.at<float>(i) = (float)(-1.0 * a);
        }
        return o;
    }
    cv::Mat GetPoseInverse()                                // Twc = [Rwc | Ow] (KeyFrame.cc:113-126, SetPose)
    {
        cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
        const cv::Mat Ow = GetCameraCenter();
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.at<float>(i, j) = Tcw.at<float>(j, i); T.at<float>(i, 3) = Ow.at<float>(i); }
        return T;
    }
    cv::Mat GetRightRotation()                              // Rrw = Rrl * Rlw, Rrl = mTlr.R^T (KeyFrame.cc:1243-1251)
    {
        cv::Mat R(3, 3, CV_32F);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)mTlr.at<float>(k, i) * (double)Tcw.at<float>(k, j);
            R.at<float>(i, j) = (float)a;
        }
        return R;
    }
    cv::Mat GetRightTranslation()                           // trw = Rrl * tlw + trl, trl = -Rrl * tlr (KeyFrame.cc:1253-1262)
    {
        float trl[3];
        for (int i = 0; i < 3; i++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)mTlr.at<float>(k, i) * (double)mTlr.at<float>(k, 3);
            trl[i] = (float)(-1.0 * a);
        }
        cv::Mat t(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)mTlr.at<float>(k, i) * (double)Tcw.at<float>(k, 3);
            t.at<float>(i) = (float)(a + (double)trl[i]);
        }
        return t;
    }
    cv::Mat GetRightPose()                                  // Trw = [Rrw | trw], 3x4 (KeyFrame.cc:1176-1192: the same products)
    {
        const cv::Mat R = GetRightRotation(), t = GetRightTranslation();
        cv::Mat T(3, 4, CV_32F);
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.at<float>(i, j) = R.at<float>(i, j); T.at<float>(i, 3) = t.at<float>(i); }
        return T;
    }
    cv::Mat GetRightCameraCenter()                          // twr = Rwl * tlr + twl (KeyFrame.cc:1232-1241)
    {
        const cv::Mat Ow = GetCameraCenter();
        cv::Mat t(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)Tcw.at<float>(k, i) * (double)mTlr.at<float>(k, 3);
            t.at<float>(i) = (float)(a + (double)Ow.at<float>(i));
        }
        return t;
    }
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }    // KeyFrame.cc:816-819
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    std::set<MapPoint *> GetMapPoints()                     // KeyFrame.cc:600-613
    {
        std::set<MapPoint *> s;
        for (size_t i = 0, iend = mvpMapPoints.size(); i < iend; i++) {
            if (!mvpMapPoints[i]) continue;
            MapPoint *pMP = mvpMapPoints[i];
            if (!pMP->isBad()) s.insert(pMP);
        }
        return s;
    }
    // src/KeyFrame.cc:161-172: Owb = Rwc tcb + Ow, Rwb = Rwc Rcb (float cv::Mat arithmetic)
    cv::Mat GetImuPosition()
    {
        cv::Mat o(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) {
            float a = 0;                                  // Ow = -Rwc tcw
            for (int k = 0; k < 3; k++) a += Tcw.at<float>(k, i) * (mImuCalib.Tcb.at<float>(k, 3) - Tcw.at<float>(k, 3));
            o.at<float>(i) = a;
        }
        return o;
    }
    cv::Mat GetImuRotation()
    {
        cv::Mat R(3, 3, CV_32F);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
            float a = 0;
            for (int k = 0; k < 3; k++) a += Tcw.at<float>(k, i) * mImuCalib.Tcb.at<float>(k, j);
            R.at<float>(i, j) = a;
        }
        return R;
    }
    cv::Mat GetVelocity() { return Vw.clone(); }
    void SetVelocity(const cv::Mat &Vw_) { Vw = Vw_.clone(); }
    void SetNewBias(const IMU::Bias &b) { mImuBias = b; if (mpImuPreintegrated) mpImuPreintegrated->SetNewBias(b); }     // KeyFrame.cc:871-877
    IMU::Bias GetImuBias() { return mImuBias; }
    cv::Mat GetGyroBias() { cv::Mat m(3, 1, CV_32F); m.at<float>(0) = mImuBias.bwx; m.at<float>(1) = mImuBias.bwy; m.at<float>(2) = mImuBias.bwz; return m; }
    cv::Mat GetAccBias() { cv::Mat m(3, 1, CV_32F); m.at<float>(0) = mImuBias.bax; m.at<float>(1) = mImuBias.bay; m.at<float>(2) = mImuBias.baz; return m; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)         // KeyFrame.cc:251-259
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    float ComputeSceneMedianDepth(const int q)                                 // KeyFrame.cc:839-869 (Mat::dot in double, + zcw, narrowed)
    {
        std::vector<float> vDepths;
        vDepths.reserve(N);
        for (int i = 0; i < N; i++)
            if (mvpMapPoints[i]) {
                const cv::Mat x3Dw = mvpMapPoints[i]->GetWorldPos();
                double d = 0;
                for (int k = 0; k < 3; k++) d += (double)Tcw.at<float>(2, k) * (double)x3Dw.at<float>(k);
                vDepths.push_back((float)(d + Tcw.at<float>(2, 3)));
            }
        std::sort(vDepths.begin(), vDepths.end());
        return vDepths[(vDepths.size() - 1) / q];
    }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    void EraseMapPointMatch(MapPoint *pMP) { for (auto &p : mvpMapPoints) if (p == pMP) p = nullptr; }
    bool isBad() { return mbBad; }
    Map *GetMap() { return mpMap; }
    std::set<KeyFrame *> GetConnectedKeyFrames()            // KeyFrame.cc:218-225: every key of mConnectedKeyFrameWeights
    {
        std::set<KeyFrame *> s;
        for (auto &kv : mConnectedKeyFrameWeights) s.insert(kv.first);
        return s;
    }
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;    // include/KeyFrame.h:497
    // the spanning tree, the loop edges and the covisibility graph as Optimizer::OptimizeEssentialGraph reads them (src/KeyFrame.cc:
    // 261-296, 298-306, 520-548, 550-560); the stand-in's state is filled by the test programs
    KeyFrame *GetParent() { return mpParent; }
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(KeyFrame *pKF) { auto it = mConnectedKeyFrameWeights.find(pKF); return it != mConnectedKeyFrameWeights.end() ? it->second : 0; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w)    // the ordered neighbours of weight >= w, in their order
    {
        std::vector<KeyFrame *> v;
        for (KeyFrame *pKF : mvpOrderedConnectedKeyFrames) if (GetWeight(pKF) >= w) v.push_back(pKF);
        return v;
    }
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens, mspLoopEdges;
    DBoW2::BowVector mBowVec;                               // include/KeyFrame.h:393
    // Variables used by KeyFrameDatabase (include/KeyFrame.h:331-340)
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0.f;
    long unsigned int mnPlaceRecognitionQuery = 0;
    int mnPlaceRecognitionWords = 0;
    float mPlaceRecognitionScore = 0.f;
    long unsigned int mnId;
    long unsigned int mnBALocalForKF, mnBAFixedForKF;
    long unsigned int mnBALocalForMerge = 0;
    // what a global BA leaves for LoopClosing::RunGlobalBundleAdjustment to propagate (include/KeyFrame.h:343-349)
    cv::Mat mTcwGBA, mVwbGBA;
    IMU::Bias mBiasGBA;
    long unsigned int mnBAGlobalForKF = 0;
    const float fx, fy, cx, cy, mbf;
    cv::Mat mK;                                             // include/KeyFrame.h:383 (Sim3Solver copies it, nothing reads it)
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<float> mvInvLevelSigma2;
    GeometricCamera *mpCamera, *mpCamera2;
    cv::Mat mTrl;
    std::vector<cv::KeyPoint> mvKeysRight;
    int NLeft;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    // inertial members (include/KeyFrame.h:405-470)
    KeyFrame *mPrevKF, *mNextKF;
    bool bImu;
    IMU::Preintegrated *mpImuPreintegrated;
    IMU::Calib mImuCalib;
    // members the keyframe-side matchers read (include/KeyFrame.h:360-400)
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    int mnScaleLevels = 8;
    float mfLogScaleFactor = std::log(1.2f);
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    cv::Mat mTlr;
    // members LocalMapping::CreateNewMapPoints reads (include/KeyFrame.h:357, 388, 394)
    float mb = 0.f;
    std::vector<float> mvDepth;
    float mfScaleFactor = 1.2f;
    // stand-in state
    cv::Mat Tcw, Vw;
    IMU::Bias mImuBias;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<MapPoint *> mvpMapPoints;
    Map *mpMap;
    bool mbBad;
};

// src/MapPoint.cc:114-139
inline void MapPoint::AddObservation(KeyFrame *pKF, int idx)
{
    std::tuple<int, int> indexes = mObservations.count(pKF) ? mObservations[pKF] : std::tuple<int, int>(-1, -1);
    if (pKF->NLeft != -1 && idx >= pKF->NLeft) std::get<1>(indexes) = idx;
    else std::get<0>(indexes) = idx;
    mObservations[pKF] = indexes;
    if (!pKF->mpCamera2 && pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
}

// src/MapPoint.cc:168-201 (SetBadFlag reduced to the flag)
inline void MapPoint::EraseObservation(KeyFrame *pKF)
{
    auto it = mObservations.find(pKF);
    if (it == mObservations.end()) return;
    const int leftIndex = std::get<0>(it->second), rightIndex = std::get<1>(it->second);
    if (leftIndex != -1) {
        if (!pKF->mpCamera2 && pKF->mvuRight[leftIndex] >= 0) nObs -= 2;
        else nObs--;
    }
    if (rightIndex != -1) nObs--;
    mObservations.erase(it);
    if (nObs <= 2) mbBad = true;
}

// include/Map.h
class Map {
public:
    Map() : mnInitKFid(0), mbIsInertial(false), mnMapChange(0), nKeyFrames(0) {}
    long unsigned int KeyFramesInMap() { return nKeyFrames; }
    long unsigned int GetInitKFid() { return mnInitKFid; }
    long unsigned int GetMaxKFid() { return mnMaxKFid; }               // src/Map.cc:165-169
    std::vector<KeyFrame *> GetAllKeyFrames() { return mvpKeyFrames; } // src/Map.cc:135-139 (there a copy of a pointer-ordered set)
    std::vector<MapPoint *> GetAllMapPoints() { return mvpMapPoints; } // src/Map.cc:141-145
    long unsigned int mnMaxKFid = 0;                                   // stand-in state
    std::vector<KeyFrame *> mvpKeyFrames;
    std::vector<MapPoint *> mvpMapPoints;
    bool IsInertial() { return mbIsInertial; }
    bool IsBad() { return mbBad; }                                     // src/Map.cc:284-287
    void SetBad() { mbBad = true; }                                    // src/Map.cc:278-282
    bool mbBad = false;
    void IncreaseChangeIndex() { mnMapChange++; }
    bool GetIniertialBA2() { return mbIMU_BA2; }                       // src/Map.cc:360-364
    bool GetIniertialBA1() { return mbIMU_BA1; }                       // src/Map.cc:354-358
    bool mbIMU_BA1 = false;
    bool isImuInitialized() { return mbImuInitialized; }               // src/Map.cc:92-96
    bool mbImuInitialized = false;
    std::mutex mMutexMapUpdate;
    long unsigned int mnInitKFid;
    bool mbIsInertial;
    int mnMapChange;
    long unsigned int nKeyFrames;
    bool mbIMU_BA2 = false;
};

// include/LoopClosing.h:50-51: the pose tables CorrectLoop hands to Optimizer::OptimizeEssentialGraph (there with Eigen's aligned allocator)
class LoopClosing {
public:
    typedef std::map<KeyFrame *, g2o::Sim3, std::less<KeyFrame *>> KeyFrameAndPose;
};

// include/Atlas.h, include/Tracking.h: what LocalMapping::CreateNewMapPoints touches of them
class Atlas {
public:
    Map *GetCurrentMap() { return mpCurrentMap; }
    bool isImuInitialized() { return mpCurrentMap->isImuInitialized(); }   // src/Atlas.cc:256-260
    void AddMapPoint(MapPoint *pMP) { mvpMapPoints.push_back(pMP); }    // src/Atlas.cc:93-97 -> Map::AddMapPoint
    Map *mpCurrentMap = nullptr;
    std::vector<MapPoint *> mvpMapPoints;                             // stand-in state: in order of insertion
};
class Tracking;                                                       // (below Frame: it holds mCurrentFrame)

// include/LocalMapping.h: the members the lines of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:383-726) touch
class LocalMapping {
public:
    // Triangulate new map points from the current keyframe and its covisible neighbours.  src/LocalMapping.cc:383-726
    // (host/LocalMapping_CreateNewMapPoints.cc)
    void CreateNewMapPoints();
    bool CheckNewKeyFrames()                                            // LocalMapping.cc:286-290; mnCheckTrueAt: test plumbing, true from that call on
    {
        std::unique_lock<std::mutex> lock(mMutexNewKFs);
        mnCheckCalls++;
        return !mlNewKeyFrames.empty() || (mnCheckTrueAt > 0 && mnCheckCalls >= mnCheckTrueAt);
    }
    cv::Mat ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2);             // LocalMapping.cc:839-856 (host/LocalMapping_CreateNewMapPoints.cc)
    KeyFrame *mpCurrentKeyFrame = nullptr;
    bool mbMonocular = false, mbInertial = false, mbFarPoints = false;
    float mThFarPoints = 0.f;
    Atlas *mpAtlas = nullptr;
    Tracking *mpTracker = nullptr;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    std::list<KeyFrame *> mlNewKeyFrames;
    std::mutex mMutexNewKFs;
    int mnCheckCalls = 0, mnCheckTrueAt = -1;
};

// include/Frame.h (the members ORBmatcher.cc:48-218, 710-825, 1965-2181 read or write)
class ORBextractor;
class Frame {
public:
    Frame() : mbf(0), mb(0), N(0), mpORBextractorLeft(nullptr), mpORBextractorRight(nullptr), mpCamera(nullptr), mpCamera2(nullptr), Nleft(-1), Nright(-1),
              mnScaleLevels(8), mfLogScaleFactor(std::log(1.2f)) {}
    float mbf, mb;
    int N;
    // include/Frame.h:92-97, :127-129, :208-209, :265-274: what Tracking::PreintegrateIMU reads and sets
    double mTimeStamp = 0;
    Frame *mpPrevFrame = nullptr;
    KeyFrame *mpLastKeyFrame = nullptr;
    IMU::Bias mImuBias;
    IMU::Calib mImuCalib;
    IMU::Preintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
    bool mbImuPreintegrated = false;
    void setIntegrated() { mbImuPreintegrated = true; }                 // src/Frame.cc:1068-1072 (there under *mpMutexImu)
    // rectified stereo (include/Frame.h:153,239-248,296): the two extractors, the right image's features, and what ComputeStereoMatches fills
    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    cv::Mat mDescriptorsRight;
    std::vector<float> mvDepth;
    // Search a match for each keypoint in the left image to a keypoint in the right image.  If there is a match, depth is computed and the
    // right coordinate associated to the left keypoint is stored.  include/Frame.h:98-99, src/Frame.cc:802-980  (host/Frame.cc)
    void ComputeStereoMatches();
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    std::vector<bool> mvbOutlier;
    DBoW2::FeatureVector mFeatVec;
    DBoW2::BowVector mBowVec;                             // include/Frame.h:254
    cv::Mat mTcw;
    std::vector<float> mvScaleFactors;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    GeometricCamera *mpCamera, *mpCamera2;
    int Nleft, Nright;
    std::vector<int> mvLeftToRightMatch, mvRightToLeftMatch;
    cv::Mat mTrl;
    int mnScaleLevels;
    float mfLogScaleFactor;
    std::vector<float> mvInvLevelSigma2;
    static float fx, fy, cx, cy;                          // include/Frame.h:212-217 (static calibration)
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); UpdatePoseMatrices(); }     // src/Frame.cc:419-423
    // Computes rotation, translation and camera center matrices from the camera pose.  src/Frame.cc:456-462 (host/Frame.cc)
    void UpdatePoseMatrices();
    cv::Mat mRcw, mtcw, mRwc, mOw;                        // include/Frame.h:131-132, :268-269
    // Check if a MapPoint is in the frustum of the camera and fill variables of the MapPoint to be used by the tracking.
    // include/Frame.h:103-105, :304, src/Frame.cc:483-572, :1170-1243 (host/Frame.cc): the single-point host form of what
    // orbhip_frustum_queries_device does for the whole local map
    bool isInFrustum(MapPoint *pMP, float viewingCosLimit);
    bool isInFrustumChecks(MapPoint *pMP, float viewingCosLimit, bool bRight = false);
    std::map<long unsigned int, cv::Point2f> mmProjectPoints;   // include/Frame.h:243
    long unsigned int mnId = 0;                           // include/Frame.h:221
    // stereo fisheye (include/Frame.h:188, 232, 282-297): the lapping split of both sides, the rig, what ComputeStereoFishEyeMatches fills
    // Search a match for each keypoint of the left image's lapping area among the right one's (2-NN + ratio test), triangulate it with the
    // rig and keep it if the point is in front of both cameras and reprojects well.  include/Frame.h:302, src/Frame.cc:1128-1168 (host/Frame.cc)
    void ComputeStereoFishEyeMatches();
    int monoLeft = -1, monoRight = -1;
    std::vector<cv::Mat> mvStereo3Dpoints;
    cv::Mat mTlr, mRlr, mtlr;
    std::vector<float> mvLevelSigma2;
    int mnCloseMPs = 0;
};

// include/System.h:85-91
class System {
public:
    enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2, IMU_MONOCULAR = 3, IMU_STEREO = 4 };
};

// include/Tracking.h: the members Tracking::SearchLocalPoints (src/Tracking.cc:2358-2430) touches, and the state LocalMapping reads
class Tracking {
public:
    enum eTrackingState { SYSTEM_NOT_READY = -1, NO_IMAGES_YET = 0, NOT_INITIALIZED = 1, OK = 2, RECENTLY_LOST = 3, LOST = 4, OK_KLT = 5 };   // include/Tracking.h:103-111
    eTrackingState mState = NO_IMAGES_YET;
    // Project the local map points into the current frame and search matches for the ones in its frustum.  src/Tracking.cc:2358-2430
    // (host/Tracking_SearchLocalPoints.cc).  mnMatchesLocalPoints: what SearchByProjection returned (the reference drops it), -1 = not run
    void SearchLocalPoints();
    // Preintegrate the IMU measurements between the previous and the current frame.  src/Tracking.cc:552-666
    // (host/Tracking_PreintegrateIMU.cc)
    void PreintegrateIMU();
    std::list<IMU::Point> mlQueueImuData;                 // include/Tracking.h:192-199
    std::vector<IMU::Point> mvImuFromLastFrame;
    std::mutex mMutexImuQueue;
    IMU::Preintegrated *mpImuPreintegratedFromLastKF = nullptr;
    KeyFrame *mpLastKeyFrame = nullptr;                   // :235
    Frame mLastFrame;                                     // :237
    int mSensor = System::MONOCULAR;                      // include/Tracking.h:115
    Frame mCurrentFrame;                                  // :118
    std::vector<MapPoint *> mvpLocalMapPoints;            // :248
    LocalMapping *mpLocalMapper = nullptr;                // :230
    Atlas *mpAtlas = nullptr;                             // :260
    unsigned int mnLastRelocFrameId = 0;                  // :288
    int mnMatchesLocalPoints = -1;
};

}  // namespace ORB_SLAM3
#endif
