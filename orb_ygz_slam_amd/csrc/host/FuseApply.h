// FuseApply.h -- the exact sequential result of `for (k : targets) ORBmatcher::Fuse(targets[k], points, th)` (src/ORBmatcher.cc:748-886;
// LocalMapping::SearchInNeighbors, src/LocalMapping.cc:1259-1269) from candidates computed in batches (product code, host side, header only,
// no libygzf dependency: the device call hides behind `query`).
//
// Why batching is exact.  Fuse's candidate search (projection -> bestIdx, bestDist; :764-868) reads only what the loop never changes --
// the point's position, normal, distance limits and descriptor, the keyframe's pose, keys, grid and tables -- with one exception: a
// MapPoint::Replace survivor gets a new descriptor (ComputeDistinctiveDescriptors, src/MapPoint.cc:185).  Within one target a survivor is never
// searched again (pMPinKF is in that keyframe; a pMP survivor now observes it), and a point that is in a keyframe stays so or turns bad
// (Replace moves observations only away from points it makes bad).  So: every (distinct target, point) pair is searched from one snapshot,
// pairs already excluded at snapshot time are skipped, and the map updates of :868-883 run here in the reference's order with its live
// checks (isBad, IsInKeyFrame, GetMapPoint, Observations).  Listed points that survived a Replace are searched again before the next target
// step, against the targets still to come.
//
//   query(kfs, pts, skip, bestIdx, bestDist) -> bool: the candidate search of every (kfs[r], pts[i]) pair with skip[r * P + i] == 0
//   (bestIdx -1 / bestDist 256 where none), rows = kfs; false = failure (nothing more is applied).
#ifndef YGZF_FUSE_APPLY_H
#define YGZF_FUSE_APPLY_H

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace ygzf_host {

struct FuseApplyResult {
    bool ok = true;
    std::vector<int> nFused;        // per target: Fuse's return value
    long long requeried = 0;        // (survivor, remaining target) pairs searched again
};

// thLow = ORBmatcher::TH_LOW (50).  requery = false leaves survivors' stale candidates in place (tests: shows the hazard it guards against).
template <class KeyFrameT, class MapPointT, class Query>
FuseApplyResult fuse_apply(const std::vector<KeyFrameT *> &targets, const std::vector<MapPointT *> &points, int thLow, Query &&query,
                           bool requery = true) {
    FuseApplyResult res;
    const size_t T = targets.size(), P = points.size();
    res.nFused.assign(T, 0);
    if (T == 0 || P == 0) return res;
    // distinct targets: a keyframe listed twice is searched once
    std::vector<KeyFrameT *> rows;
    std::vector<int> rowOf(T, -1);
    {
        std::unordered_map<KeyFrameT *, int> seen;
        for (size_t t = 0; t < T; t++) {
            if (!targets[t]) continue;
            auto it = seen.find(targets[t]);
            if (it == seen.end()) it = seen.emplace(targets[t], (int) rows.size()).first, rows.push_back(targets[t]);
            rowOf[t] = it->second;
        }
    }
    const size_t R = rows.size();
    // snapshot: pairs the reference's :770 test already excludes (bad points stay bad; an observation of a good point is never removed)
    auto excluded = [](MapPointT *p, KeyFrameT *kf) { return !p || p->isBad() || p->IsInKeyFrame(kf); };
    std::vector<uint8_t> skip(R * P);
    for (size_t r = 0; r < R; r++)
        for (size_t i = 0; i < P; i++) skip[r * P + i] = excluded(points[i], rows[r]) ? 1 : 0;
    std::vector<int> bestIdx(R * P, -1), bestDist(R * P, 256);
    if (R > 0 && !query(rows, points, skip, bestIdx, bestDist)) {
        res.ok = false;
        return res;
    }
    std::unordered_set<MapPointT *> listed(points.begin(), points.end());
    std::unordered_set<MapPointT *> changed;   // listed points whose descriptor a Replace recomputed since their candidates were searched
    for (size_t t = 0; t < T; t++) {
        if (rowOf[t] < 0) continue;
        if (requery && !changed.empty()) {
            // the changed points against the distinct targets still to come, in one query
            std::vector<int> rrows;
            {
                std::vector<uint8_t> want(R, 0);
                for (size_t u = t; u < T; u++)
                    if (rowOf[u] >= 0 && !want[rowOf[u]]) want[rowOf[u]] = 1, rrows.push_back(rowOf[u]);
            }
            std::vector<MapPointT *> qp;   // in list order, each once
            for (size_t i = 0; i < P; i++)
                if (changed.erase(points[i])) qp.push_back(points[i]);
            std::vector<KeyFrameT *> qk;
            for (int r : rrows) qk.push_back(rows[r]);
            std::vector<uint8_t> qs(qk.size() * qp.size());
            for (size_t a = 0; a < qk.size(); a++)
                for (size_t b = 0; b < qp.size(); b++) qs[a * qp.size() + b] = excluded(qp[b], qk[a]) ? 1 : 0;
            std::vector<int> qi(qs.size(), -1), qd(qs.size(), 256);
            if (!query(qk, qp, qs, qi, qd)) {
                res.ok = false;
                return res;
            }
            res.requeried += (long long) qs.size();
            std::unordered_map<MapPointT *, size_t> col;
            for (size_t b = 0; b < qp.size(); b++) col[qp[b]] = b;
            for (size_t a = 0; a < qk.size(); a++)
                for (size_t i = 0; i < P; i++) {
                    auto it = col.find(points[i]);
                    if (it == col.end()) continue;
                    const size_t o = (size_t) rrows[a] * P + i, q = a * qp.size() + it->second;
                    bestIdx[o] = qi[q];
                    bestDist[o] = qd[q];
                    skip[o] = qs[q];
                }
        }
        KeyFrameT *pKF = targets[t];
        const size_t r = (size_t) rowOf[t];
        int nFused = 0;
        for (size_t i = 0; i < P; i++) {   // src/ORBmatcher.cc:764-883, the map updates in list order
            MapPointT *pMP = points[i];
            if (!pMP || skip[r * P + i]) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            const int bd = bestDist[r * P + i], bi = bestIdx[r * P + i];
            if (bd > thLow) continue;
            MapPointT *pMPinKF = pKF->GetMapPoint(bi);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    MapPointT *survivor;
                    if (pMPinKF->Observations() > pMP->Observations()) {
                        pMP->Replace(pMPinKF);
                        survivor = pMPinKF;
                    } else {
                        pMPinKF->Replace(pMP);
                        survivor = pMP;
                    }
                    if (listed.count(survivor)) changed.insert(survivor);
                }
            } else {
                pMP->AddObservation(pKF, bi);
                pKF->AddMapPoint(pMP, bi);
            }
            nFused++;
        }
        res.nFused[t] = nFused;
    }
    return res;
}

}  // namespace ygzf_host
#endif
