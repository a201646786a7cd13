// LocalMappingTriangulate.cc -- ygz::TriangulatePairsDevice and ygz::CreateNewMapPointsBatch (LocalMappingTriangulate.h): the neighbour loop of
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1009-1216) over libygzf (product code, host side).  The searches go through
// ORBmatcher::SearchForTriangulation, the per-pair body of :1060-1194 through one ygzf_triangulate_pairs call for all neighbours -- or, below the
// host threshold, through the same text (csrc/tri_math.h) on the calling thread --, and the map updates of :1197-1214 run in the reference's order
// (TriangulateApply.h).  Compiled beside ORBmatcher.cc, ORBextractor.cc and ygzf_pool.cc; LocalMapping.cc stays the reference's.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "ORBmatcher.h"
#include "ygz_compat.h"
#ifdef YGZF_WITH_REFERENCE_HEADERS
#include "Map.h"
#endif

#include <cmath>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "../../../include/ygzf.h"
#include "../tri_math.h"
#include "LocalMappingTriangulate.h"
#include "TriangulateApply.h"
#include "ygzf_pool.h"

namespace {
int tri_min_from_env() {
    const char *e = std::getenv("YGZF_TRI_DEVICE_MIN");
    if (!e || !*e) return 64;   // profiles/triangulate_rate.txt: the device call and the host thread meet near 50 pairs
    char *end = nullptr;
    const long v = std::strtol(e, &end, 10);
    if (end == e || v < 0 || v > (1 << 30)) return 64;
    return (int) v;
}
}  // namespace
int ygzf_host_tri_device_min = tri_min_from_env();

namespace ygz {

namespace {

// cos(2 * atan2(mb / 2, mvDepth[i])) per feature, once per keyframe.  The reference's expression (:1090, :1092) with `using namespace std` in
// force and float operands: std::atan2(float, float) and std::cos(float).
std::mutex gCosMutex;
std::unordered_map<KeyFrame *, std::vector<float>> gCosStereo;

const float *cos_stereo_of(KeyFrame *pKF) {
    std::lock_guard<std::mutex> lock(gCosMutex);
    std::vector<float> &v = gCosStereo[pKF];
    if (v.size() != pKF->mvDepth.size()) {
        v.resize(pKF->mvDepth.size());
        for (size_t i = 0; i < v.size(); i++) v[i] = std::cos(2 * std::atan2(pKF->mb / 2, pKF->mvDepth[i]));
    }
    return v.data();   // (the map's nodes do not move when others are added)
}

bool stereo_arrays(KeyFrame *pKF) { return pKF->N > 0 && (int) pKF->mvuRight.size() == pKF->N && (int) pKF->mvDepth.size() == pKF->N; }

bool pack(KeyFrame *pKF, ygzf_tri_kf &k, const char *who) {
    if (pKF->mvScaleFactors.empty() || pKF->mvLevelSigma2.size() != pKF->mvScaleFactors.size()) {
        ygzf_host::report_failure(who, "keyframe without scale tables");
        return false;
    }
    k.view.n = pKF->N;
    k.view.keys = (const ygzf_kp *) pKF->mvKeys.data();
    k.view.desc = nullptr;
    const bool st = stereo_arrays(pKF);
    k.view.u_right = st ? pKF->mvuRight.data() : nullptr;
    k.view.scale_factors = pKF->mvScaleFactors.data();
    k.view.nlevels = (int) pKF->mvScaleFactors.size();
    k.cam = ygzf_camera{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mb, pKF->mbf, 0.f, 0.f, 0.f, 0.f};
    k.invfx = pKF->invfx;
    k.invfy = pKF->invfy;
    k.level_sigma2 = pKF->mvLevelSigma2.data();
    k.depth = st ? pKF->mvDepth.data() : nullptr;
    k.cos_stereo = st ? cos_stereo_of(pKF) : nullptr;
    const Matrix3f R = pKF->GetRotation();
    const Vector3f t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) k.Rcw[3 * r + c] = R(r, c);
        k.tcw[r] = t[r];
        k.Ow[r] = O[r];
    }
    float T7[7];
    ygz_compat::se3_to7(pKF->GetPoseInverse(), T7);   // Twc as the keyframe holds it: quaternion x y z w, translation
    for (int i = 0; i < 4; i++) k.Twc_q[i] = T7[i];
    for (int i = 0; i < 3; i++) k.Twc_t[i] = T7[4 + i];
    return true;
}

// ---- the host path: csrc/tri_math.h on the calling thread, over the records the device call would take --------------------------------
ygzf::tri::Kf kf_of(const ygzf_tri_kf &k) {
    ygzf::tri::Kf o;
    o.fx = k.cam.fx; o.fy = k.cam.fy; o.cx = k.cam.cx; o.cy = k.cam.cy; o.invfx = k.invfx; o.invfy = k.invfy; o.mbf = k.cam.mbf;
    for (int i = 0; i < 9; i++) o.Rcw[i] = k.Rcw[i];
    for (int i = 0; i < 3; i++) { o.tcw[i] = k.tcw[i]; o.Ow[i] = k.Ow[i]; o.t[i] = k.Twc_t[i]; }
    for (int i = 0; i < 4; i++) o.q[i] = k.Twc_q[i];
    return o;
}
bool feature_of(const ygzf_tri_kf &k, int idx, ygzf::tri::Feat &f) {   // the gather of tri_kernels.hip's tri_feature, with the C call's checks
    if (idx < 0 || idx >= k.view.n) return false;
    const ygzf_kp &kp = k.view.keys[idx];
    if (kp.octave < 0 || kp.octave >= k.view.nlevels) return false;
    f.x = kp.x; f.y = kp.y;
    f.uR = k.view.u_right ? k.view.u_right[idx] : -1.f;
    const bool stereo = f.uR >= 0.f;
    f.depth = stereo ? k.depth[idx] : -1.f;
    f.cosStereo = stereo ? k.cos_stereo[idx] : 0.f;
    f.sigma2 = k.level_sigma2[kp.octave];
    f.scale = k.view.scale_factors[kp.octave];
    return true;
}
bool triangulate_on_host(const ygzf_tri_kf &k1, float ratio, const std::vector<ygzf_tri_problem> &prob, const std::vector<float *> &x3d,
                         const std::vector<uint8_t *> &status, const char *who) {
    const ygzf::tri::Kf K1 = kf_of(k1);
    for (size_t j = 0; j < prob.size(); j++) {
        const ygzf::tri::Kf K2 = kf_of(prob[j].kf2);
        for (int i = 0; i < prob[j].n_pairs; i++) {
            ygzf::tri::Feat f1, f2;
            if (!feature_of(k1, prob[j].idx1[i], f1) || !feature_of(prob[j].kf2, prob[j].idx2[i], f2)) {
                ygzf_host::report_failure(who, "feature index or keypoint octave out of range");
                return false;
            }
            status[j][i] = ygzf::tri::triangulate_pair(K1, K2, f1, f2, ratio, x3d[j] + 3 * (size_t) i, nullptr);
        }
    }
    return true;
}

typedef std::vector<std::pair<size_t, size_t>> Pairs;

// every pair of every listed neighbour: one device call, or the host text below the threshold
bool triangulate(KeyFrame *pKF1, const std::vector<KeyFrame *> &kfs, const std::vector<Pairs> &pairs, float ratio, std::vector<std::vector<float>> &x3d,
                 std::vector<std::vector<uint8_t>> &status, const char *who) {
    const size_t B = kfs.size();
    ygzf_tri_kf k1;
    if (!pack(pKF1, k1, who)) return false;
    std::vector<ygzf_tri_problem> prob(B);
    std::vector<std::vector<int>> i1(B), i2(B);
    std::vector<float *> xp(B);
    std::vector<uint8_t *> sp(B);
    long long total = 0;
    for (size_t j = 0; j < B; j++) {
        if (!pack(kfs[j], prob[j].kf2, who)) return false;
        const size_t n = pairs[j].size();
        i1[j].resize(n);
        i2[j].resize(n);
        for (size_t i = 0; i < n; i++) { i1[j][i] = (int) pairs[j][i].first; i2[j][i] = (int) pairs[j][i].second; }
        x3d[j].assign(3 * n, 0.f);
        status[j].assign(n, 0);
        prob[j].n_pairs = (int) n;
        prob[j].idx1 = i1[j].data();
        prob[j].idx2 = i2[j].data();
        xp[j] = x3d[j].data();
        sp[j] = status[j].data();
        total += (long long) n;
    }
    if (total == 0) return true;
    if (total < (long long) ygzf_host_tri_device_min) return triangulate_on_host(k1, ratio, prob, xp, sp, who);
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return false;
    const int rc = ygzf_triangulate_pairs(lease.get(), &k1, ratio, (int) B, prob.data(), xp.data(), sp.data());
    if (rc != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
        return false;
    }
    return true;
}

}  // namespace

bool TriangulatePairsDevice(KeyFrame *pKF1, KeyFrame *pKF2, const Pairs &vMatchedIndices, float ratioFactor, std::vector<float> &x3D,
                            std::vector<uint8_t> &status) {
    std::vector<std::vector<float>> x(1);
    std::vector<std::vector<uint8_t>> s(1);
    if (!triangulate(pKF1, std::vector<KeyFrame *>{pKF2}, std::vector<Pairs>{vMatchedIndices}, ratioFactor, x, s, "ygz::TriangulatePairsDevice")) return false;
    x3D.swap(x[0]);
    status.swap(s[0]);
    return true;
}

int CreateNewMapPointsBatch(KeyFrame *pCurrentKeyFrame, const std::vector<KeyFrame *> &vpNeighKFs, Map *pMap, std::list<MapPoint *> &lpRecentAddedMapPoints,
                            bool bMonocular, const std::function<Matrix3f(KeyFrame *&, KeyFrame *&)> &computeF12,
                            const std::function<bool()> &checkNewKeyFrames) {
    const char *who = "ygz::CreateNewMapPointsBatch";
    KeyFrame *cur = pCurrentKeyFrame;
    ORBmatcher matcher(0.6, false);                              // :986
    const float ratioFactor = 1.5f * cur->mfScaleFactor;         // :1003
    const Vector3f Ow1 = cur->GetCameraCenter();
    auto gate = [&](KeyFrame *pKF2) {                            // :1016-1035
        const Vector3f Ow2 = pKF2->GetCameraCenter();
        const float b[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
        const float baseline = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        if (!bMonocular) return !(baseline < pKF2->mb);
        const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        return !(ratioBaselineDepth < 0.01);
    };
    // The searches all run before the first map update, so what the matcher reads of the two keyframes' slots IS the snapshot: the arrays
    // triangulate_apply hands over say the same and are not needed here.
    auto search = [&](KeyFrame *pKF2, const std::vector<uint8_t> &, const std::vector<uint8_t> &, Pairs &out) {
        Matrix3f F12 = computeF12(cur, pKF2);                    // :1038
        matcher.SearchForTriangulation(cur, pKF2, F12, out, false);   // :1042
        return true;
    };
    auto query = [&](const std::vector<KeyFrame *> &kfs, const std::vector<Pairs> &pairs, std::vector<std::vector<uint8_t>> &accepted,
                     std::vector<std::vector<float>> &x3d) {
        std::vector<std::vector<uint8_t>> status(kfs.size());
        if (!triangulate(cur, kfs, pairs, ratioFactor, x3d, status, who)) return false;
        for (size_t j = 0; j < kfs.size(); j++)
            for (size_t i = 0; i < status[j].size(); i++) accepted[j][i] = (status[j][i] & ygzf::tri::kStatusMask) == ygzf::tri::kAccepted;
        return true;
    };
    auto create = [&](KeyFrame *pKF2, size_t idx1, size_t idx2, const float *x) {   // :1197-1214
        Vector3f x3D;
        x3D[0] = x[0]; x3D[1] = x[1]; x3D[2] = x[2];
        MapPoint *pMP = new MapPoint(x3D, cur, pMap);
        pMP->AddObservation(cur, idx1);
        pMP->AddObservation(pKF2, idx2);
        cur->AddMapPoint(pMP, idx1);
        pKF2->AddMapPoint(pMP, idx2);
        pMP->ComputeDistinctiveDescriptors();
        pMP->UpdateNormalAndDepth();
        pMap->AddMapPoint(pMP);
        lpRecentAddedMapPoints.push_back(pMP);
    };
    const ygzf_host::TriangulateApplyResult r = ygzf_host::triangulate_apply<KeyFrame, MapPoint>(cur, vpNeighKFs, gate, search, query, create, checkNewKeyFrames);
    return r.ok ? r.nnew : 0;
}

void TriangulateForget(KeyFrame *pKF) {
    std::lock_guard<std::mutex> lock(gCosMutex);
    gCosStereo.erase(pKF);
}

}  // namespace ygz
