// ORBmatcherFuse.cc -- ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) over libygzf (product code, host side), and ygz::FuseBatch,
// the forward pass of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1259-1269: every point of the new keyframe fused into each target
// in turn) as one batch.  The candidate search runs on the device (ygzf_fuse_candidates); the map updates of src/ORBmatcher.cc:868-883 run
// here in the reference's order (FuseApply.h says why that is exact).
// Kept apart from ORBmatcher.cc: inside the reference tree this file supplies the strong Fuse beside the weakened ORBmatcher.o
// (link recipe), while ORBmatcher.cc keeps the member set the boundary build pins.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "ORBmatcher.h"
#include "ygz_compat.h"

#include <cstring>
#include <vector>

#include "../../../include/ygzf.h"
#include "FuseApply.h"
#include "ORBmatcherFuse.h"
#include "ygzf_pool.h"

namespace ygz {

namespace {
// MapPoint::mfMaxDistance (PredictScale's numerator) is private in the reference's MapPoint.h: read through an explicit instantiation, whose
// arguments access checking does not apply to (as host/TrackingBatched.cc does)
template <typename Tag, typename Tag::type M>
struct FuseMemberOf {
    friend typename Tag::type member_ptr(Tag) { return M; }
};
struct FuseMaxDistanceTag {
    typedef float MapPoint::*type;
    friend type member_ptr(FuseMaxDistanceTag);
};
template struct FuseMemberOf<FuseMaxDistanceTag, &MapPoint::mfMaxDistance>;
inline float max_distance(MapPoint *mp) { return mp->*member_ptr(FuseMaxDistanceTag()); }

// the device query of FuseApply.h: one ygzf_fuse_candidates call for kfs x pts
struct DeviceQuery {
    ygzf_ctx *c;
    float th;
    const char *who;
    bool operator()(const std::vector<KeyFrame *> &kfs, const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi,
                    std::vector<int> &bd) const {
        const size_t K = kfs.size(), P = pts.size();
        if (K == 0 || P == 0) return true;
        std::vector<ygzf_fuse_kf> kv(K);
        std::vector<std::vector<uint8_t>> hold(K);
        for (size_t k = 0; k < K; k++) {
            KeyFrame *pKF = kfs[k];
            ygzf_fuse_kf &f = kv[k];
            std::memset(&f, 0, sizeof f);
            const int n = pKF->N;
            f.view.n = n;
            f.view.keys = (const ygzf_kp *) pKF->mvKeys.data();
            const cv::Mat &D = pKF->mDescriptors;
            if (n > 0 && !(D.isContinuous() && D.cols == 32)) {
                hold[k].resize((size_t) n * 32);
                for (int i = 0; i < n; i++) std::memcpy(&hold[k][(size_t) i * 32], D.ptr<uint8_t>(i), 32);
                f.view.desc = hold[k].data();
            } else {
                f.view.desc = n > 0 ? D.ptr<uint8_t>(0) : nullptr;
            }
            f.view.u_right = (int) pKF->mvuRight.size() == n ? pKF->mvuRight.data() : nullptr;
            f.view.scale_factors = pKF->mvScaleFactors.data();
            f.view.nlevels = pKF->mnScaleLevels;
            if ((int) pKF->mvScaleFactors.size() < pKF->mnScaleLevels || (int) pKF->mvInvLevelSigma2.size() < pKF->mnScaleLevels) {
                ygzf_host::report_failure(who, "keyframe scale tables shorter than mnScaleLevels");
                return false;
            }
            f.cam.fx = pKF->fx; f.cam.fy = pKF->fy; f.cam.cx = pKF->cx; f.cam.cy = pKF->cy; f.cam.mbf = pKF->mbf;
            f.cam.min_x = (float) pKF->mnMinX; f.cam.min_y = (float) pKF->mnMinY; f.cam.max_x = (float) pKF->mnMaxX; f.cam.max_y = (float) pKF->mnMaxY;
            f.inv_level_sigma2 = pKF->mvInvLevelSigma2.data();
            const Matrix3f R = pKF->GetRotation();
            const Vector3f t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
            for (int r = 0; r < 3; r++) {
                for (int cc = 0; cc < 3; cc++) f.Rcw[3 * r + cc] = R(r, cc);
                f.tcw[r] = t[r];
                f.Ow[r] = O[r];
            }
            f.log_scale_factor = pKF->mfLogScaleFactor;
        }
        std::vector<float> world(3 * P, 0.f), normal(3 * P, 0.f), maxInv(P, 0.f), minInv(P, 0.f), maxDist(P, 1.f);
        std::vector<uint8_t> desc(32 * P, 0);
        for (size_t i = 0; i < P; i++) {
            MapPoint *mp = pts[i];
            if (!mp) continue;   // (every row skips it)
            ygz_compat::world_pos(mp, &world[3 * i]);
            const Vector3f nrm = mp->GetNormal();
            for (int r = 0; r < 3; r++) normal[3 * i + r] = nrm[r];
            maxInv[i] = mp->GetMaxDistanceInvariance();
            minInv[i] = mp->GetMinDistanceInvariance();
            maxDist[i] = max_distance(mp);
            const cv::Mat d = mp->GetDescriptor();
            if (!d.empty()) std::memcpy(&desc[32 * i], d.ptr<uint8_t>(0), 32);
        }
        ygzf_fuse_points fp = {world.data(), normal.data(), maxInv.data(), minInv.data(), maxDist.data(), desc.data()};
        const int rc = ygzf_fuse_candidates(c, (int) K, kv.data(), (int) P, &fp, skip.data(), th, bi.data(), bd.data());
        if (rc != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(c));
            return false;
        }
        return true;
    }
};

int fuse_targets(const std::vector<KeyFrame *> &targets, const std::vector<MapPoint *> &points, float th, const char *who) {
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return 0;
    const ygzf_host::FuseApplyResult r = ygzf_host::fuse_apply(targets, points, ORBmatcher::TH_LOW, DeviceQuery{lease.get(), th, who});
    int n = 0;   // (after a failure: what the targets applied before it fused; 0 when the first query failed)
    for (int k : r.nFused) n += k;
    return n;
}
}  // namespace

// src/ORBmatcher.cc:748-886
int ORBmatcher::Fuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMapPoints, const float th) {
    return fuse_targets(std::vector<KeyFrame *>{pKF}, vpMapPoints, th, "ygz::ORBmatcher::Fuse");
}

// `for (pKFi : targets) matcher.Fuse(pKFi, points, th)` as one batch (src/LocalMapping.cc:1259-1269); returns the summed nFused of the targets
// applied (ORBmatcherFuse.h: what a device failure leaves).
int FuseBatch(const std::vector<KeyFrame *> &targets, const std::vector<MapPoint *> &points, float th) {
    return fuse_targets(targets, points, th, "ygz::FuseBatch");
}

}  // namespace ygz
