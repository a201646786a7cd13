// LoopApply.h -- the exact sequential results of two LoopClosing searches from candidates computed in batches (product code, host side, header
// only, no libygzf dependency: the device calls hide behind `query`, as in FuseApply.h).
//
// 1. search_and_fuse_apply: LoopClosing::SearchAndFuse (src/LoopClosing.cc:546-569),
//        for (pKF, Scw) in CorrectedPosesMap:  Fuse(pKF, Scw, loopPoints, th, vpReplace);  for i: if (vpReplace[i]) vpReplace[i]->Replace(loopPoints[i]);
//    with the candidate search of every (keyframe, loop point) pair taken from ONE snapshot.
//    Why that is exact.  The candidate search of src/ORBmatcher.cc:918-987 reads the point's position, normal, distance limits and descriptor
//    and the keyframe's corrected pose, keys, grid and tables.  Nothing in the loop writes any of these except MapPoint::Replace, which
//    recomputes the SURVIVOR's descriptor (ComputeDistinctiveDescriptors, src/MapPoint.cc:185) -- and the survivor of `pRep->Replace(
//    loopPoints[i])` is always a listed point.  Everything else the loop reads is read here, live, in the reference's order: the isBad test and
//    the spAlreadyFound set of :904 / :915 (taken from the keyframe when its turn starts, as the reference takes it, and NOT refreshed inside
//    the turn), GetMapPoint(bestIdx) and the isBad of what it returns (:991-994; an AddMapPoint of :997 earlier in the same turn is seen by a
//    later point that lands on the same key), then the Replace pass of :562-567 over the whole list.  Inside one turn no descriptor changes
//    (Fuse itself replaces nothing), so a turn only ever uses candidates that are current when it starts: before each turn the listed
//    points whose descriptor a Replace has recomputed since their last search are searched again against the keyframes still to come
//    (counted in `requeried`).  A pair the snapshot left out (bad, or already in the keyframe) is never wanted later: a bad point stays bad and
//    a good point only ever gains keyframes (Replace moves observations away from the point it makes bad only); an assert holds that.
//
//      query(rows, pts, skip, bestIdx, bestDist) -> bool: the candidate search of every (keyframe rows[r] of `kfs`, pts[i]) pair with
//      skip[r * P + i] == 0 (bestIdx -1 / bestDist 256 where none); false = failure (nothing more is applied).
//
// 2. search_by_projection_apply: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:265-373).  Its inner loop
//    passes over keys with vpMatched[idx] set (:348), and :366 sets one per match: a point's result depends on the points before it, through
//    that mask alone (no map is written, no descriptor changes, spAlreadyFound is the entry snapshot of :281).
//    Why the candidate lists are exact.  Every point is searched once against the ENTRY mask for its nBest least (distance, list position)
//    keys with distance <= TH_LOW.  The mask only grows, so the keys free when the point's turn comes are a subset of those free at entry, in
//    the same order: the first listed candidate that is still free is the least free key, i.e. the reference's bestIdx (a best key beyond
//    TH_LOW matches nothing in the reference either).  A list that is not full and has no free entry left means no free key within TH_LOW:
//    no match.  A FULL list without a free entry says nothing: the walk stops there and that point and all after it are searched again
//    against the live mask (counted in `requeries`); the point then settles with its first candidate, so the walk always advances.
//
//      query(first, skip, keyMatched, nBest, candIdx, candDist) -> bool: for the points first .. P-1 (skip[i - first] != 0: not searched) the
//      nBest least candidates among keys with keyMatched[idx] == 0, (P - first) x nBest, ascending, padded with -1 / 256.
#ifndef YGZF_LOOP_APPLY_H
#define YGZF_LOOP_APPLY_H

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <set>
#include <unordered_set>
#include <vector>

namespace ygzf_host {

struct SearchAndFuseResult {
    bool ok = true;
    std::vector<int> nFused;        // per keyframe: Fuse's return value
    long long replaced = 0;         // Replace calls of :565
    long long requeried = 0;        // (point, remaining keyframe) pairs searched again
};

// thLow = ORBmatcher::TH_LOW (50).  requery = false leaves survivors' stale candidates in place (tests: shows the hazard it guards against).
template <class KeyFrameT, class MapPointT, class Query>
SearchAndFuseResult search_and_fuse_apply(const std::vector<KeyFrameT *> &kfs, const std::vector<MapPointT *> &points, int thLow, Query &&query,
                                          bool requery = true) {
    SearchAndFuseResult res;
    const size_t K = kfs.size(), P = points.size();
    res.nFused.assign(K, 0);
    if (K == 0 || P == 0) return res;
    auto excluded = [](MapPointT *p, const std::set<MapPointT *> &inKf) { return p->isBad() || inKf.count(p) != 0; };
    std::vector<uint8_t> skip(K * P);
    std::vector<int> all(K);
    for (size_t k = 0; k < K; k++) {
        all[k] = (int) k;
        const std::set<MapPointT *> inKf = kfs[k]->GetMapPoints();
        for (size_t i = 0; i < P; i++) skip[k * P + i] = excluded(points[i], inKf) ? 1 : 0;
    }
    std::vector<int> bestIdx(K * P, -1), bestDist(K * P, 256);
    if (!query(all, points, skip, bestIdx, bestDist)) {
        res.ok = false;
        return res;
    }
    std::unordered_set<MapPointT *> changed;   // listed points whose descriptor a Replace recomputed since their candidates were searched
    for (size_t k = 0; k < K; k++) {
        KeyFrameT *pKF = kfs[k];
        const std::set<MapPointT *> spAlreadyFound = pKF->GetMapPoints();   // :904, when this keyframe's turn starts
        if (requery) {
            std::vector<MapPointT *> qp;   // in list order, each once
            {
                std::unordered_set<MapPointT *> seen;
                for (size_t i = 0; i < P; i++) {
                    if (changed.count(points[i]) && seen.insert(points[i]).second) qp.push_back(points[i]);
                }
            }
            changed.clear();
            if (!qp.empty()) {
                std::vector<int> rows;
                for (size_t r = k; r < K; r++) rows.push_back((int) r);
                const size_t Q = qp.size();
                std::vector<uint8_t> qs(rows.size() * Q);
                for (size_t a = 0; a < rows.size(); a++) {
                    const std::set<MapPointT *> inKf = a == 0 ? spAlreadyFound : kfs[rows[a]]->GetMapPoints();
                    for (size_t b = 0; b < Q; b++) qs[a * Q + b] = excluded(qp[b], inKf) ? 1 : 0;
                }
                std::vector<int> qi(qs.size(), -1), qd(qs.size(), 256);
                if (!query(rows, qp, qs, qi, qd)) {
                    res.ok = false;
                    return res;
                }
                res.requeried += (long long) qs.size();
                for (size_t b = 0; b < Q; b++)
                    for (size_t i = 0; i < P; i++) {
                        if (points[i] != qp[b]) continue;
                        for (size_t a = 0; a < rows.size(); a++) {
                            const size_t o = (size_t) rows[a] * P + i, q = a * Q + b;
                            bestIdx[o] = qi[q];
                            bestDist[o] = qd[q];
                            skip[o] = qs[q];
                        }
                    }
            }
        }
        std::vector<MapPointT *> vpReplacePoint(P, nullptr);
        int nFused = 0;
        for (size_t i = 0; i < P; i++) {   // src/ORBmatcher.cc:911-1001, the updates in list order
            MapPointT *pMP = points[i];
            if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;   // :915
            assert(!skip[k * P + i]);                                  // no pair without a candidate is ever wanted (header comment)
            if (skip[k * P + i]) continue;
            const int bd = bestDist[k * P + i], bi = bestIdx[k * P + i];
            if (bd > thLow) continue;
            MapPointT *pMPinKF = pKF->GetMapPoint(bi);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
            } else {
                pMP->AddObservation(pKF, bi);
                pKF->AddMapPoint(pMP, bi);
            }
            nFused++;
        }
        res.nFused[k] = nFused;
        for (size_t i = 0; i < P; i++) {   // src/LoopClosing.cc:562-567
            MapPointT *pRep = vpReplacePoint[i];
            if (!pRep) continue;
            pRep->Replace(points[i]);
            res.replaced++;
            changed.insert(points[i]);
        }
    }
    return res;
}

struct ProjectionApplyResult {
    bool ok = true;
    int nmatches = 0;               // the member's return value
    long long conflicts = 0;        // points whose best key at entry had been taken by an earlier point
    long long requeries = 0;        // searches repeated from a point on, its candidate list exhausted
};

// vpMatched: one slot per key of the keyframe, in / out as the member's.  thLow = ORBmatcher::TH_LOW; nBest = 4 in the shell.
template <class MapPointT, class Query>
ProjectionApplyResult search_by_projection_apply(const std::vector<MapPointT *> &points, std::vector<MapPointT *> &vpMatched, int nBest, Query &&query) {
    ProjectionApplyResult res;
    const size_t P = points.size();
    if (P == 0) return res;
    std::set<MapPointT *> spAlreadyFound(vpMatched.begin(), vpMatched.end());   // :281-282
    spAlreadyFound.erase(static_cast<MapPointT *>(nullptr));
    std::vector<uint8_t> mask(vpMatched.size());
    std::vector<int> ci, cd;
    size_t first = 0;
    bool have = false;
    for (size_t i = 0; i < P;) {
        if (!have) {
            for (size_t j = 0; j < vpMatched.size(); j++) mask[j] = vpMatched[j] ? 1 : 0;
            std::vector<uint8_t> skip(P - i);
            for (size_t j = i; j < P; j++) skip[j - i] = (points[j]->isBad() || spAlreadyFound.count(points[j])) ? 1 : 0;   // :291
            ci.assign((P - i) * (size_t) nBest, -1);
            cd.assign((P - i) * (size_t) nBest, 256);
            if (!query(i, skip, mask, nBest, ci, cd)) {
                res.ok = false;
                return res;
            }
            if (i > 0) res.requeries++;
            first = i;
            have = true;
        }
        const int *c = &ci[(i - first) * (size_t) nBest];
        int pick = -1, n = 0;
        for (; n < nBest && c[n] >= 0; n++)
            if (!vpMatched[(size_t) c[n]]) { pick = c[n]; break; }
        if (pick < 0 && n == nBest) {   // a full list, every key of it taken since: search again from here with the live mask
            res.conflicts++;
            have = false;
            continue;
        }
        if (n > 0) res.conflicts++;     // (its best key at entry went to an earlier point)
        if (pick >= 0) {
            vpMatched[(size_t) pick] = points[i];   // :365-368
            res.nmatches++;
        }
        i++;
    }
    return res;
}

}  // namespace ygzf_host
#endif
