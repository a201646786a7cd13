// MatcherPack.h -- what ORBmatcherFuse.cc and ORBmatcherLoop.cc share (product code, host side, internal): reading MapPoint::mfMaxDistance, and
// packing a KeyFrame / a MapPoint list into the plain arrays of ygzf_fuse_kf / ygzf_fuse_points.  Include after ORBmatcher.h and ygz_compat.h,
// from one .cc per use (everything here has internal linkage).
#ifndef YGZF_MATCHER_PACK_H
#define YGZF_MATCHER_PACK_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/ygzf.h"
#include "ygzf_pool.h"

namespace ygz {
namespace {
// MapPoint::mfMaxDistance (PredictScale's numerator) is private in the reference's MapPoint.h: read through an explicit instantiation, whose
// arguments access checking does not apply to (as host/TrackingBatched.cc does)
template <typename Tag, typename Tag::type M>
struct PackMemberOf {
    friend typename Tag::type member_ptr(Tag) { return M; }
};
struct PackMaxDistanceTag {
    typedef float MapPoint::*type;
    friend type member_ptr(PackMaxDistanceTag);
};
template struct PackMemberOf<PackMaxDistanceTag, &MapPoint::mfMaxDistance>;
inline float max_distance(MapPoint *mp) { return mp->*member_ptr(PackMaxDistanceTag()); }

// the rows of an N x 32 descriptor matrix as one block: the Mat's own buffer when it is continuous, a packed copy in `hold` otherwise
inline const uint8_t *desc_rows(const cv::Mat &D, int n, std::vector<uint8_t> &hold) {
    if (n <= 0) return nullptr;
    if (D.isContinuous() && D.cols == 32) return D.ptr<uint8_t>(0);
    hold.resize((size_t) n * 32);
    for (int i = 0; i < n; i++) std::memcpy(&hold[(size_t) i * 32], D.ptr<uint8_t>(i), 32);
    return hold.data();
}

// A keyframe's keys, descriptors (copied into `hold` when the cv::Mat is not 32 contiguous bytes per row), mvuRight, scale tables, mvInvLevelSigma2,
// image bounds and mfLogScaleFactor; fx fy cx cy mbf from `cam` (SearchBySim3 projects both directions with pKF1's).  The pose is the caller's.
inline bool pack_keyframe(KeyFrame *pKF, const KeyFrame *cam, ygzf_fuse_kf &f, std::vector<uint8_t> &hold, const char *who) {
    std::memset(&f, 0, sizeof f);
    const int n = pKF->N;
    f.view.n = n;
    f.view.keys = (const ygzf_kp *) pKF->mvKeys.data();
    f.view.desc = desc_rows(pKF->mDescriptors, n, hold);
    f.view.u_right = (int) pKF->mvuRight.size() == n ? pKF->mvuRight.data() : nullptr;
    f.view.scale_factors = pKF->mvScaleFactors.data();
    f.view.nlevels = pKF->mnScaleLevels;
    if ((int) pKF->mvScaleFactors.size() < pKF->mnScaleLevels || (int) pKF->mvInvLevelSigma2.size() < pKF->mnScaleLevels) {
        ygzf_host::report_failure(who, "keyframe scale tables shorter than mnScaleLevels");
        return false;
    }
    f.cam.fx = cam->fx; f.cam.fy = cam->fy; f.cam.cx = cam->cx; f.cam.cy = cam->cy; f.cam.mbf = cam->mbf;
    f.cam.min_x = (float) pKF->mnMinX; f.cam.min_y = (float) pKF->mnMinY; f.cam.max_x = (float) pKF->mnMaxX; f.cam.max_y = (float) pKF->mnMaxY;
    f.inv_level_sigma2 = pKF->mvInvLevelSigma2.data();
    f.log_scale_factor = pKF->mfLogScaleFactor;
    return true;
}

// ... the same without a pose, for the resident store (KeyFrameStore.h: ygzf_kf_put)
inline bool pack_keyframe_static(KeyFrame *pKF, ygzf_kf_static &rec, std::vector<uint8_t> &hold, const char *who) {
    ygzf_fuse_kf f;
    if (!pack_keyframe(pKF, pKF, f, hold, who)) return false;
    rec.view = f.view;
    rec.cam = f.cam;
    rec.inv_level_sigma2 = f.inv_level_sigma2;
    rec.log_scale_factor = f.log_scale_factor;
    return true;
}

// GetWorldPos, GetNormal, the distance limits, mfMaxDistance and GetDescriptor of pts[first ..]; entries that are null or have skip[i - first] != 0
// are not read (they stay zero: the device skips them by the same mask)
struct PointArrays {
    std::vector<float> world, normal, maxInv, minInv, maxDist;
    std::vector<uint8_t> desc;
    ygzf_fuse_points view;
    PointArrays(const std::vector<MapPoint *> &pts, size_t first, const uint8_t *skip) {
        const size_t P = pts.size() - first;
        world.assign(3 * P, 0.f); normal.assign(3 * P, 0.f); maxInv.assign(P, 0.f); minInv.assign(P, 0.f); maxDist.assign(P, 1.f);
        desc.assign(32 * P, 0);
        for (size_t i = 0; i < P; i++) {
            MapPoint *mp = pts[first + i];
            if (!mp || (skip && skip[i])) continue;
            ygz_compat::world_pos(mp, &world[3 * i]);
            const Vector3f nrm = mp->GetNormal();
            for (int r = 0; r < 3; r++) normal[3 * i + r] = nrm[r];
            maxInv[i] = mp->GetMaxDistanceInvariance();
            minInv[i] = mp->GetMinDistanceInvariance();
            maxDist[i] = max_distance(mp);
            const cv::Mat d = mp->GetDescriptor();
            if (!d.empty()) std::memcpy(&desc[32 * i], d.ptr<uint8_t>(0), 32);
        }
        view = ygzf_fuse_points{world.data(), normal.data(), maxInv.data(), minInv.data(), maxDist.data(), desc.data()};
    }
};
}  // namespace
}  // namespace ygz
#endif
