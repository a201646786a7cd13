// TriangulateApply.h -- the exact sequential result of the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1009-1216) from
// searches and triangulations computed in one batch (product code, host side, header only, no libygzf dependency: the device calls hide behind
// `search` and `query`).
//
// Why batching is exact.
//   - CreateNewMapPoints builds `ORBmatcher matcher(0.6, false)` (:986): the orientation check is off, so no match depends on a histogram of
//     the others.
//   - SearchForTriangulation never sets vbMatched2 (src/ORBmatcher.cc:654-706).  The match of KF1 feature idx1 against neighbour j therefore
//     depends only on whether KF1 holds a MapPoint in slot idx1 (:638), on which slots of neighbour j hold one, and on data nobody changes
//     (keys, descriptors, the vocabulary's nodes, F12 from the two poses).
//   - Iteration j adds MapPoints only to the current keyframe and to ITS OWN neighbour (:1202-1203), and the neighbours of a covisibility
//     list are distinct: neighbour j's slots are at iteration j what they were before the loop.
//   - The baseline gate (:1016-1035), ComputeSceneMedianDepth(2) of the monocular case included, reads poses and the neighbour's own points'
//     positions: nothing an earlier iteration wrote.
// So the search of every neighbour against ONE snapshot of the slots differs from the reference's search at iteration j in exactly one way: it
// still matches the KF1 features that received a point from a neighbour before j, which the reference skips at :638.  Dropping those pairs in
// the replay gives the reference's list; every other pair is the same pair, its triangulation depends on nothing but the pair, and the map
// updates of :1197-1214 run here in the reference's order: neighbours in list order, pairs in ascending idx1 (:731-736).
//
// Two more rules of the reference carry over as they are:
//   - two pairs of one neighbour may name the same idx2; the reference creates both points and the second AddMapPoint overwrites the slot.
//     The replay makes the same two calls;
//   - CheckNewKeyFrames() (:1010) is polled before each neighbour after the first -- before its baseline gate -- and the loop ends there.  The
//     searches and triangulations of the neighbours behind that point were done for nothing; nothing of them is applied.
//
// The callables:
//   gate(kf2) -> bool                       the neighbour passes the baseline gate
//   search(kf2, hasMp1, hasMp2, pairs)      SearchForTriangulation(cur, kf2, F12, pairs, false) against the snapshot: hasMp1[i] != 0 <=> cur holds
//       -> bool                             a MapPoint in slot i, hasMp2 likewise for kf2; pairs in ascending idx1.  false = failure
//   query(kfs, pairs, accepted, x3d)        the per-pair body (:1060-1194) of every pair of every searched neighbour in ONE call: accepted[j][i]
//       -> bool                             != 0 <=> pair i of kfs[j] passed every gate, x3d[j][3 i ..] its point.  false = failure
//   create(kf2, idx1, idx2, x3d)            :1197-1214 for one accepted pair
//   poll() -> bool                          CheckNewKeyFrames()
#ifndef YGZF_TRIANGULATE_APPLY_H
#define YGZF_TRIANGULATE_APPLY_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ygzf_host {

struct TriangulateApplyResult {
    bool ok = true;
    int nnew = 0;                   // the reference's nnew
    int stoppedAt = -1;             // the neighbour before which CheckNewKeyFrames() ended the loop; -1: the loop ran out
    long long searchedPairs = 0;    // pairs the snapshot searches returned
    long long dropped = 0;          // pairs whose idx1 an earlier neighbour had filled: the ones the reference never sees
    std::vector<int> created;       // per neighbour
};

// KeyFrameT: int N; MapPointT *GetMapPoint(size_t).  drop = false applies the pairs of filled slots all the same (tests: shows the hazard the
// drop rule guards against).
template <class KeyFrameT, class MapPointT, class Gate, class Search, class Query, class Create, class Poll>
TriangulateApplyResult triangulate_apply(KeyFrameT *cur, const std::vector<KeyFrameT *> &neighbours, Gate &&gate, Search &&search, Query &&query,
                                         Create &&create, Poll &&poll, bool drop = true) {
    typedef std::vector<std::pair<size_t, size_t>> Pairs;
    TriangulateApplyResult res;
    const size_t M = neighbours.size();
    res.created.assign(M, 0);
    if (!cur || M == 0) return res;
    // 1. the snapshot
    auto slots = [](KeyFrameT *kf) {
        std::vector<uint8_t> has((size_t) kf->N);
        for (size_t i = 0; i < has.size(); i++) has[i] = kf->GetMapPoint(i) ? 1 : 0;
        return has;
    };
    const std::vector<uint8_t> hasMp1 = slots(cur);
    // 2. the searches of the neighbours that pass the gate, against it
    std::vector<int> rowOf(M, -1);
    std::vector<KeyFrameT *> rows;
    std::vector<Pairs> pairs;
    for (size_t j = 0; j < M; j++) {
        KeyFrameT *kf2 = neighbours[j];
        if (!kf2 || !gate(kf2)) continue;
        Pairs p;
        if (!search(kf2, hasMp1, slots(kf2), p)) {
            res.ok = false;
            return res;
        }
        res.searchedPairs += (long long) p.size();
        rowOf[j] = (int) rows.size();
        rows.push_back(kf2);
        pairs.push_back(std::move(p));
    }
    // 3. every pair in one query
    std::vector<std::vector<uint8_t>> accepted(rows.size());
    std::vector<std::vector<float>> x3d(rows.size());
    for (size_t r = 0; r < rows.size(); r++) {
        accepted[r].assign(pairs[r].size(), 0);
        x3d[r].assign(3 * pairs[r].size(), 0.f);
    }
    if (!rows.empty() && !query(rows, pairs, accepted, x3d)) {
        res.ok = false;
        return res;
    }
    // 4. the replay, in neighbour order
    for (size_t j = 0; j < M; j++) {
        if (j > 0 && poll()) {
            res.stoppedAt = (int) j;
            return res;
        }
        if (rowOf[j] < 0) continue;
        const size_t r = (size_t) rowOf[j];
        for (size_t i = 0; i < pairs[r].size(); i++) {
            const size_t idx1 = pairs[r][i].first, idx2 = pairs[r][i].second;
            if (!hasMp1[idx1] && cur->GetMapPoint(idx1)) {   // filled by an earlier neighbour (one neighbour names an idx1 once)
                res.dropped++;
                if (drop) continue;
            }
            if (!accepted[r][i]) continue;
            create(rows[r], idx1, idx2, &x3d[r][3 * i]);
            res.created[j]++;
            res.nnew++;
        }
    }
    return res;
}

}  // namespace ygzf_host
#endif
