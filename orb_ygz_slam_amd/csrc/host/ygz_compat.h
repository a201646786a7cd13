// ygz_compat.h -- the types the three class shells are written against (product code, host side).
//
// Built inside the reference tree (-DYGZF_WITH_REFERENCE_HEADERS) this header simply pulls the
// reference's own Common.h / Frame.h / MapPoint.h / KeyFrame.h (OpenCV cv::Mat / cv::KeyPoint, Sophus SE3f, Eigen) and defines the
// few adapters below on top of them; it is included by the shells' .cc files only (Frame.h itself includes ORBextractor.h).
// Built stand-alone (this repository: no OpenCV / Eigen / Sophus installed) it provides a
// minimal stand-in for exactly the slice of those types the hot-path signatures touch, layout-compatible where layout
// matters (cv::KeyPoint = 7 x 4 bytes, continuous 8-bit Mats), so that the shells compile and are testable here.
#ifndef YGZF_COMPAT_H
#define YGZF_COMPAT_H

#ifdef YGZF_WITH_REFERENCE_HEADERS
#include "Common.h"     // reference include/Common.h: OpenCV, Eigen, Sophus, glog, typedefs (SE3f, Vector3f, ...)
#include "Frame.h"
#include "MapPoint.h"
#include "KeyFrame.h"
namespace ygz_compat {   // SE3f / Vector3f / Matrix3f are the global names include/Common.h brings in (using Sophus::SE3f, Eigen::...)
inline void se3_to7(const SE3f &T, float o[7]) {
    const Eigen::Quaternionf q = T.unit_quaternion();
    o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w();
    o[4] = T.translation()[0]; o[5] = T.translation()[1]; o[6] = T.translation()[2];
}
inline SE3f se3_from7(const float i[7]) {
    return SE3f(Eigen::Quaternionf(i[3], i[0], i[1], i[2]), Vector3f(i[4], i[5], i[6]));
}
inline void se3_to_Rt(const SE3f &T, float R[9], float t[3]) {
    const Matrix3f M = T.rotationMatrix();
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[3 * r + c] = M(r, c);
    for (int r = 0; r < 3; r++) t[r] = T.translation()[r];
}
inline void world_pos(ygz::MapPoint *mp, float o[3]) { const Vector3f p = mp->GetWorldPos(); o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
// how many cv::Mat headers share m's buffer (0: no buffer of its own / external data): the level pool of ORBextractor::ComputePyramid hands a
// buffer out again only when nobody but the pool refers to it
inline int mat_refcount(const cv::Mat &m) {
#if defined(YGZ_MINI_CV)
    return m.use_count();
#elif defined(CV_MAJOR_VERSION) && CV_MAJOR_VERSION >= 3
    return m.u ? (int) m.u->refcount : 0;
#else
    return m.refcount ? *m.refcount : 0;
#endif
}
}  // namespace ygz_compat
#else  // ---------------------------------------------------------------------------------------------- stand-alone shim
#include <algorithm>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#define CV_8U 0
#define CV_8UC1 0
#define CV_32F 5
#define CV_16UC1 2    // the types of cv::initUndistortRectifyMap's fixed-point maps (ORBextractor::SetUndistortMaps)
#define CV_16SC2 11

#include <set>
namespace cv {
struct Point2f { float x, y; };
struct KeyPoint {  // bit-compatible with cv::KeyPoint
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;
    unsigned char *data = nullptr;
    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(int r, int c, int type, void *ext, size_t st = 0) : rows(r), cols(c), step(st ? st : (size_t) c * esz(type)), data((unsigned char *) ext), type_(type) {}
    void create(int r, int c, int type) {
        if (r == rows && c == cols && type == type_ && data && hold_ && step == (size_t) c * esz(type)) return;
        rows = r; cols = c; type_ = type; step = (size_t) c * esz(type);
        hold_.reset(new unsigned char[(size_t) r * step + 16], std::default_delete<unsigned char[]>());
        data = hold_.get();
    }
    void release() { hold_.reset(); data = nullptr; rows = cols = 0; step = 0; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    bool isContinuous() const { return step == (size_t) cols * esz(type_); }
    int type() const { return type_; }
    template <typename T> T *ptr(int r = 0) { return (T *) (data + (size_t) r * step); }
    template <typename T> const T *ptr(int r = 0) const { return (const T *) (data + (size_t) r * step); }
    unsigned char *ptr(int r = 0) { return data + (size_t) r * step; }
    const unsigned char *ptr(int r = 0) const { return data + (size_t) r * step; }
    Mat row(int r) const { Mat m(1, cols, type_, (void *) (data + (size_t) r * step), step); m.hold_ = hold_; return m; }
    int refcount() const { return hold_ ? (int) hold_.use_count() : 0; }   // (stand-in for cv::Mat::u->refcount)
    Mat clone() const {
        Mat m(rows, cols, type_);
        for (int r = 0; r < rows; r++) std::memcpy(m.ptr(r), ptr(r), (size_t) cols * esz(type_));
        return m;
    }
private:
    static size_t esz(int type) { return type == CV_32F || type == CV_16SC2 ? 4 : type == CV_16UC1 ? 2 : 1; }
    int type_ = CV_8U;
    std::shared_ptr<unsigned char> hold_;
};
class _InputArray {
public:
    _InputArray(const Mat &m) : m_(&m) {}
    Mat getMat() const { return *m_; }
    bool empty() const { return m_->empty(); }
private:
    const Mat *m_;
};
class _OutputArray {
public:
    _OutputArray(Mat &m) : m_(&m) {}
    void create(int r, int c, int type) const { m_->create(r, c, type); }
    void release() const { m_->release(); }
    Mat getMat() const { return *m_; }
private:
    Mat *m_;
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;
}  // namespace cv

namespace DBoW2 {
typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;   // node id -> feature indices (DBoW2/FeatureVector.h)
class BowVector : public std::map<unsigned int, double> {};                // word id -> value (DBoW2/BowVector.h)
}

namespace ygz {
struct Vector3f { float v[3]; float &operator[](int i) { return v[i]; } const float &operator[](int i) const { return v[i]; } };
struct Matrix3f { float m[9]; float &operator()(int r, int c) { return m[3 * r + c]; } const float &operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vector2f { float v[2]; float &operator[](int i) { return v[i]; } const float &operator[](int i) const { return v[i]; } };
class KeyFrame;
struct SE3f {  // Sophus::SE3f storage: unit quaternion (x,y,z,w) + translation
    float q[4] = {0, 0, 0, 1};
    float t[3] = {0, 0, 0};
};
class Frame;
class ORBextractor;
class Map;
class MapPoint {  // the accessors the hot path calls (reference include/MapPoint.h)
public:
    MapPoint() = default;
    inline MapPoint(const Vector3f &Pos, KeyFrame *pRefKF, Map *pMap);   // src/MapPoint.cc:32-39 (LocalMapping::CreateNewMapPoints)
    KeyFrame *mpRefKF = nullptr;
    Map *mpMap = nullptr;
    inline void UpdateNormalAndDepth();                                   // :291-331
    Vector3f mWorldPos{};
    cv::Mat mDescriptor;
    int nObs = 1;
    bool mbBad = false;
    // set by Frame::isInFrustum (src/Frame.cc:413-419)
    bool mbTrackInView = false;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 0;
    int mnTrackScaleLevel = 0;
    Vector3f GetWorldPos() const { return mWorldPos; }
    cv::Mat GetDescriptor() const { return mDescriptor.clone(); }
    int Observations() const { return nObs; }
    bool isBad() const { return mbBad; }
    // scale-invariance range (src/MapPoint.cc:325-373)
    float mfMinDistance = 0, mfMaxDistance = 0;
    float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
    inline int PredictScale(const float &currentDist, Frame *pF);
    std::map<KeyFrame *, size_t> mObservations;
    std::map<KeyFrame *, size_t> GetObservations() const { return mObservations; }
    // read and written by ORBmatcher::Fuse(KeyFrame*, MapPoints, th) (src/ORBmatcher.cc:748-886); bodies below KeyFrame
    long unsigned int mnId = 0;
    Vector3f mNormalVector{};
    int mnVisible = 1, mnFound = 1;
    MapPoint *mpReplaced = nullptr;
    Vector3f GetNormal() const { return mNormalVector; }                                        // src/MapPoint.cc:74-77
    MapPoint *GetReplaced() const { return mpReplaced; }
    bool IsInKeyFrame(KeyFrame *pKF) const { return mObservations.count(pKF) != 0; }           // :286-289
    int GetIndexInKeyFrame(KeyFrame *pKF) const {                                              // :278-284 (SearchBySim3)
        const std::map<KeyFrame *, size_t>::const_iterator it = mObservations.find(pKF);
        return it == mObservations.end() ? -1 : (int) it->second;
    }
    void IncreaseVisible(int n) { mnVisible += n; }                                             // :196-199
    void IncreaseFound(int n) { mnFound += n; }                                                 // :201-204
    inline void AddObservation(KeyFrame *pKF, size_t idx);
    inline void Replace(MapPoint *pMP);
    inline void ComputeDistinctiveDescriptors();
    inline int PredictScale(const float &currentDist, KeyFrame *pKF);
    static inline std::mutex mGlobalMutex;   // include/MapPoint.h:134: held while Optimizer::PoseOptimization reads the points (src/Optimizer.cc:1694)
};
class Frame {  // the members the hot path reads/writes (reference include/Frame.h)
public:
    static float fx, fy, cx, cy, invfx, invfy, mnMinX, mnMaxX, mnMinY, mnMaxY;
    float mb = 0, mbf = 0;
    int N = 0;
    cv::Mat mImGray, mImRight;
    std::vector<cv::Mat> mvImagePyramid;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvScaleFactors, mvInvScaleFactors;
    SE3f mTcw;
    float mfLogScaleFactor = 0;
    int mnScaleLevels = 0;
    DBoW2::FeatureVector mFeatVec;
    long unsigned int mnId = 0;
    ORBextractor *mpORBextractorLeft = nullptr;   // the extractor whose ComputePyramid built mvImagePyramid (include/Frame.h:220)
    DBoW2::BowVector mBowVec;                     // read by KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:180-284)
    // read and written by Optimizer::PoseOptimization (src/Optimizer.cc:1656-1842)
    std::vector<float> mvInvLevelSigma2;
    std::vector<float> mvLevelSigma2;             // read by PnPsolver's constructor (src/PnPsolver.cc:81)
    void SetPose(const SE3f &Tcw) { mTcw = Tcw; }   // (the reference also refreshes mRcw / mtcw / mOw: src/Frame.cc:338-346)
};
inline int MapPoint::PredictScale(const float &currentDist, Frame *pF) {  // src/MapPoint.cc:359-373
    float ratio = mfMaxDistance / currentDist;
    int nScale = (int) std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
    return nScale;
}
class KeyFrame {  // the members SearchByProjection(Cur, KF, ...) reads (reference include/KeyFrame.h)
public:
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<MapPoint *> GetMapPointMatches() const { return mvpMapPoints; }
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    // read by FindDirectProjection (src/ORBmatcher.cc:1574-1602)
    long unsigned int mnId = 0;
    std::vector<cv::Mat> mvImagePyramid;
    SE3f mPose;
    SE3f GetPose() const { return mPose; }
    // read by SearchForTriangulation (src/ORBmatcher.cc:596-741)
    int N = 0;
    std::vector<float> mvuRight, mvScaleFactors, mvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    MapPoint *GetMapPoint(const size_t &i) const { return mvpMapPoints[i]; }
    Matrix3f mRcw{};
    Vector3f mtcw{}, mOw{};
    Matrix3f GetRotation() const { return mRcw; }
    Vector3f GetTranslation() const { return mtcw; }
    Vector3f GetCameraCenter() const { return mOw; }
    // read by LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:978-1217; include/KeyFrame.h:289-345)
    float mb = 0, invfx = 0, invfy = 0, mfScaleFactor = 0;
    std::vector<float> mvDepth;
    SE3f Twc;
    SE3f GetPoseInverse() const { return Twc; }
    float ComputeSceneMedianDepth(const int q) const {                                          // src/KeyFrame.cc:830-857
        std::vector<float> vDepths;
        for (int i = 0; i < N; i++)
            if (mvpMapPoints[i]) {
                const Vector3f x = mvpMapPoints[i]->GetWorldPos();
                vDepths.push_back((mRcw(2, 0) * x[0] + mRcw(2, 1) * x[1]) + mRcw(2, 2) * x[2] + mtcw[2]);
            }
        std::sort(vDepths.begin(), vDepths.end());
        return vDepths[(vDepths.size() - 1) / q];
    }
    // read and written by ORBmatcher::Fuse(KeyFrame*, MapPoints, th) (src/ORBmatcher.cc:748-886; include/KeyFrame.h:289-317)
    float mbf = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::vector<float> mvInvLevelSigma2;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    bool mbBad = false;
    bool isBad() const { return mbBad; }
    std::set<MapPoint *> GetMapPoints() const {                                                 // src/KeyFrame.cc:449-460 (Fuse(pKF, Scw, ..))
        std::set<MapPoint *> s;
        for (MapPoint *pMP : mvpMapPoints)
            if (pMP && !pMP->isBad()) s.insert(pMP);
        return s;
    }
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }   // src/KeyFrame.cc:811-813
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }             // :428-431
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(nullptr); }   // :433-436
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }    // :445-447
    // read and written by KeyFrameDatabase (src/KeyFrameDatabase.cc:36-284; include/KeyFrame.h:276-281) and LoopClosing::DetectLoop (src/LoopClosing.cc:123-136)
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    std::set<KeyFrame *> mspConnected;                       // (the keys of mConnectedKeyFrameWeights)
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> GetConnectedKeyFrames() const { return mspConnected; }                               // src/KeyFrame.cc:381-388
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() const { return mvpOrderedConnectedKeyFrames; }      // :390-393
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) const {                                // :395-402
        if ((int) mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
};
class Map {  // include/Map.h: what CreateNewMapPoints touches
public:
    std::set<MapPoint *> mspMapPoints;
    long unsigned int nNextPointId = 0;   // (MapPoint::nNextId in the reference)
    void AddMapPoint(MapPoint *pMP) { mspMapPoints.insert(pMP); }
};
inline MapPoint::MapPoint(const Vector3f &Pos, KeyFrame *pRefKF, Map *pMap) : mpRefKF(pRefKF), mpMap(pMap), mWorldPos(Pos), nObs(0) {
    mnId = pMap ? pMap->nNextPointId++ : 0;
}
inline void MapPoint::UpdateNormalAndDepth() {  // src/MapPoint.cc:291-331
    if (mbBad || mObservations.empty()) return;
    float normal[3] = {0, 0, 0};
    int n = 0;
    for (std::map<KeyFrame *, size_t>::iterator mit = mObservations.begin(), mend = mObservations.end(); mit != mend; mit++) {
        const Vector3f Owi = mit->first->GetCameraCenter();
        float d[3] = {mWorldPos[0] - Owi[0], mWorldPos[1] - Owi[1], mWorldPos[2] - Owi[2]};
        const float nrm = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        for (int a = 0; a < 3; a++) normal[a] = normal[a] + d[a] / nrm;
        n++;
    }
    const Vector3f Or = mpRefKF->GetCameraCenter();
    const float PC[3] = {mWorldPos[0] - Or[0], mWorldPos[1] - Or[1], mWorldPos[2] - Or[2]};
    const float dist = std::sqrt((PC[0] * PC[0] + PC[1] * PC[1]) + PC[2] * PC[2]);
    const int level = mpRefKF->mvKeys[mObservations[mpRefKF]].octave;
    const float levelScaleFactor = mpRefKF->mvScaleFactors[level];
    const int nLevels = mpRefKF->mnScaleLevels;
    mfMaxDistance = dist * levelScaleFactor;
    mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors[nLevels - 1];
    for (int a = 0; a < 3; a++) mNormalVector[a] = normal[a] / n;
}
inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx) {  // src/MapPoint.cc:84-94
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
}
inline void MapPoint::Replace(MapPoint *pMP) {  // src/MapPoint.cc:155-188 (the stand-in has no Map: mpMap->EraseMapPoint(this) is left out)
    if (pMP->mnId == this->mnId) return;
    std::map<KeyFrame *, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pMP;
    for (std::map<KeyFrame *, size_t>::iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
        KeyFrame *pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
    pMP->IncreaseFound(nfound);
    pMP->IncreaseVisible(nvisible);
    pMP->ComputeDistinctiveDescriptors();
}
inline void MapPoint::ComputeDistinctiveDescriptors() {  // src/MapPoint.cc:211-271: the observed descriptor of least median distance
    if (mbBad || mObservations.empty()) return;
    std::vector<const unsigned char *> vDescriptors;
    for (std::map<KeyFrame *, size_t>::iterator mit = mObservations.begin(), mend = mObservations.end(); mit != mend; mit++)
        if (!mit->first->isBad()) vDescriptors.push_back(mit->first->mDescriptors.ptr(mit->second));
    if (vDescriptors.empty()) return;
    const size_t N = vDescriptors.size();
    std::vector<float> Distances(N * N);
    for (size_t i = 0; i < N; i++) {
        Distances[i * N + i] = 0;
        for (size_t j = i + 1; j < N; j++) {
            int distij = 0;   // ORBmatcher::DescriptorDistance
            for (int b = 0; b < 32; b++) distij += __builtin_popcount((unsigned) (vDescriptors[i][b] ^ vDescriptors[j][b]));
            Distances[i * N + j] = (float) distij;
            Distances[j * N + i] = (float) distij;
        }
    }
    int BestMedian = 0x7fffffff;
    int BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t) (0.5 * (N - 1))];
        if (median < BestMedian) {
            BestMedian = median;
            BestIdx = (int) i;
        }
    }
    cv::Mat best(1, 32, CV_8U);   // vDescriptors[BestIdx].clone()
    std::memcpy(best.ptr(0), vDescriptors[BestIdx], 32);
    mDescriptor = best;
}
inline int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) {  // src/MapPoint.cc:343-357
    float ratio = mfMaxDistance / currentDist;
    int nScale = (int) std::ceil(std::log(ratio) / pKF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
    return nScale;
}
}  // namespace ygz

namespace ygz_compat {
inline int mat_refcount(const cv::Mat &m) { return m.refcount(); }
inline void se3_to7(const ygz::SE3f &T, float o[7]) { std::memcpy(o, T.q, 16); std::memcpy(o + 4, T.t, 12); }
inline ygz::SE3f se3_from7(const float i[7]) { ygz::SE3f T; std::memcpy(T.q, i, 16); std::memcpy(T.t, i + 4, 12); return T; }
inline void se3_to_Rt(const ygz::SE3f &T, float R[9], float t[3]) {  // Eigen Quaternion::toRotationMatrix
    const float *q = T.q;
    const float tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const float txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const float tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
    t[0] = T.t[0]; t[1] = T.t[1]; t[2] = T.t[2];
}
inline void world_pos(ygz::MapPoint *mp, float o[3]) { const ygz::Vector3f p = mp->GetWorldPos(); o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
}  // namespace ygz_compat
#endif
#endif
