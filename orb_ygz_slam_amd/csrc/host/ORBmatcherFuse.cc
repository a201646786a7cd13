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
#include "KeyFrameStore.h"
#include "MatcherPack.h"
#include "ORBmatcherFuse.h"
#include "ygzf_pool.h"

namespace ygz {

namespace {
// the device query of FuseApply.h: one ygzf_fuse_candidates call for kfs x pts
struct DeviceQuery {
    ygzf_ctx *c;
    float th;
    const char *who;
    bool operator()(const std::vector<KeyFrame *> &kfs, const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi,
                    std::vector<int> &bd) const {
        const size_t K = kfs.size(), P = pts.size();
        if (K == 0 || P == 0) return true;
        if (KeyFrameDeviceStore::sResident) return resident(kfs, pts, skip, bi, bd);
        std::vector<ygzf_fuse_kf> kv(K);
        std::vector<std::vector<uint8_t>> hold(K);
        for (size_t k = 0; k < K; k++) {
            KeyFrame *pKF = kfs[k];
            ygzf_fuse_kf &f = kv[k];
            if (!pack_keyframe(pKF, pKF, f, hold[k], who)) return false;
            const Matrix3f R = pKF->GetRotation();
            const Vector3f t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
            for (int r = 0; r < 3; r++) {
                for (int cc = 0; cc < 3; cc++) f.Rcw[3 * r + cc] = R(r, cc);
                f.tcw[r] = t[r];
                f.Ow[r] = O[r];
            }
        }
        const PointArrays pa(pts, 0, nullptr);   // (a null entry stays zero: every row skips it)
        const ygzf_fuse_points &fp = pa.view;
        const int rc = ygzf_fuse_candidates(c, (int) K, kv.data(), (int) P, &fp, skip.data(), th, bi.data(), bd.data());
        if (rc != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(c));
            return false;
        }
        return true;
    }
    // the same query against the store's resident copies (KeyFrameStore.h): each keyframe is put when it is met first, the poses are read now
    bool resident(const std::vector<KeyFrame *> &kfs, const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi,
                  std::vector<int> &bd) const {
        KeyFrameDeviceStore::Guard g(KeyFrameDeviceStore::instance(ORBextractor::sDevice));
        ygzf_ctx *sc = g.ctx(who);
        if (!sc) return false;
        std::vector<ygzf_kf_ref> refs(kfs.size());
        for (size_t k = 0; k < kfs.size(); k++) {
            KeyFrame *pKF = kfs[k];
            if (!g.resident(pKF, pKF->mnId, pKF->N, [&](ygzf_kf_static &rec, std::vector<uint8_t> &hold) { return pack_keyframe_static(pKF, rec, hold, who); }, who))
                return false;
            ygzf_kf_ref &f = refs[k];
            f.key = KeyFrameDeviceStore::key(pKF);
            const Matrix3f R = pKF->GetRotation();
            const Vector3f t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
            for (int r = 0; r < 3; r++) {
                for (int cc = 0; cc < 3; cc++) f.Rcw[3 * r + cc] = R(r, cc);
                f.tcw[r] = t[r];
                f.Ow[r] = O[r];
            }
        }
        const PointArrays pa(pts, 0, nullptr);
        g.count_query();
        const int rc = ygzf_fuse_candidates_resident(sc, (int) refs.size(), refs.data(), (int) pts.size(), &pa.view, skip.data(), th, bi.data(), bd.data());
        if (rc != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(sc));
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
