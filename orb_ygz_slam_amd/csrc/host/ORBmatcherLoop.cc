// ORBmatcherLoop.cc -- the four matcher searches LoopClosing calls, over libygzf (product code, host side):
//   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)                     src/ORBmatcher.cc:480-595    ygzf_search_by_bow_kf
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)            src/ORBmatcher.cc:888-1004   ygzf_fuse_sim3_candidates
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)   :265-373                     ygzf_search_by_projection_sim3
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) :1006-1216                  ygzf_search_by_sim3
// and ygz::SearchAndFuseBatch / ygz::SearchByBoWBatch, the loops of LoopClosing::SearchAndFuse and LoopClosing::ComputeSim3 as one batch each
// (ORBmatcherLoop.h).  The candidate searches run on the device; everything that reads or writes the map runs here in the reference's order
// (LoopApply.h says why that is exact); the Scw / Sim3 algebra and the FeatureVector merge-join stay on the host (ORBmatcherLoop.h).
// Kept apart from ORBmatcher.cc, like ORBmatcherFuse.cc: inside the reference tree this file supplies these four strong members beside the
// weakened ORBmatcher.o (link recipe), while ORBmatcher.cc keeps the member set the boundary build pins.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "ORBmatcher.h"
#include "ygz_compat.h"

#include <cstring>
#include <vector>

#include "../../../include/ygzf.h"
#include "KeyFrameStore.h"
#include "LoopApply.h"
#include "MatcherPack.h"
#include "ORBmatcherLoop.h"
#include "ygzf_pool.h"

namespace ygz {

namespace {
struct Pose { float R[9], t[3], Ow[3]; };

// pack_keyframe (MatcherPack.h) with a decomposed pose
bool pack_kf(KeyFrame *pKF, const KeyFrame *cam, const Pose *pose, ygzf_fuse_kf &f, std::vector<uint8_t> &hold, const char *who) {
    if (!pack_keyframe(pKF, cam, f, hold, who)) return false;
    if (pose) {
        std::memcpy(f.Rcw, pose->R, 36);
        std::memcpy(f.tcw, pose->t, 12);
        std::memcpy(f.Ow, pose->Ow, 12);
    }
    return true;
}

// LoopApply.h's query for Fuse(.., Scw, ..): one ygzf_fuse_sim3_candidates call for the keyframes rows[] x pts
struct FuseScwQuery {
    ygzf_ctx *c;
    const std::vector<KeyFrame *> &kfs;
    const std::vector<Pose> &poses;
    float th;
    const char *who;
    bool operator()(const std::vector<int> &rows, const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi,
                    std::vector<int> &bd) const {
        const size_t K = rows.size(), P = pts.size();
        if (K == 0 || P == 0) return true;
        const PointArrays pa(pts, 0, nullptr);
        if (KeyFrameDeviceStore::sResident) {   // against the store's resident copies (KeyFrameStore.h); the decomposed Scw travels with the call
            KeyFrameDeviceStore::Guard g(KeyFrameDeviceStore::instance(ORBextractor::sDevice));
            ygzf_ctx *sc = g.ctx(who);
            if (!sc) return false;
            std::vector<ygzf_kf_ref> refs(K);
            for (size_t k = 0; k < K; k++) {
                KeyFrame *pKF = kfs[rows[k]];
                if (!g.resident(pKF, pKF->mnId, pKF->N, [&](ygzf_kf_static &rec, std::vector<uint8_t> &hold) { return pack_keyframe_static(pKF, rec, hold, who); }, who))
                    return false;
                refs[k].key = KeyFrameDeviceStore::key(pKF);
                std::memcpy(refs[k].Rcw, poses[rows[k]].R, 36);
                std::memcpy(refs[k].tcw, poses[rows[k]].t, 12);
                std::memcpy(refs[k].Ow, poses[rows[k]].Ow, 12);
            }
            g.count_query();
            const int rc = ygzf_fuse_sim3_candidates_resident(sc, (int) K, refs.data(), (int) P, &pa.view, skip.data(), th, bi.data(), bd.data());
            if (rc != YGZF_OK) {
                ygzf_host::report_failure(who, ygzf_last_error(sc));
                return false;
            }
            return true;
        }
        std::vector<ygzf_fuse_kf> kv(K);
        std::vector<std::vector<uint8_t>> hold(K);
        for (size_t k = 0; k < K; k++)
            if (!pack_kf(kfs[rows[k]], kfs[rows[k]], &poses[rows[k]], kv[k], hold[k], who)) return false;
        const int rc = ygzf_fuse_sim3_candidates(c, (int) K, kv.data(), (int) P, &pa.view, skip.data(), th, bi.data(), bd.data());
        if (rc != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(c));
            return false;
        }
        return true;
    }
};

int search_and_fuse(const std::vector<KeyFrame *> &kfs, const std::vector<Pose> &poses, const std::vector<MapPoint *> &points, float th, const char *who) {
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return 0;
    const ygzf_host::SearchAndFuseResult r =
        ygzf_host::search_and_fuse_apply(kfs, points, ORBmatcher::TH_LOW, FuseScwQuery{lease.get(), kfs, poses, th, who});
    int n = 0;
    for (int k : r.nFused) n += k;
    return n;
}

// SearchByBoW(pKF1, pKF2) for one pKF1 against `cands` as one ygzf_search_by_bow_kf call: per candidate the FeatureVector merge-join of
// src/ORBmatcher.cc:507-575 (equal node ids, lower_bound on a miss) and the "MapPoint exists and is not bad" masks of :512-516 / :527-533 run
// here; the per-node brute force, the vbMatched2 chain and the rotation histogram run on the device.  out[k] comes back with one slot per
// KF1 key, all NULL on failure (reported, returns false).
bool search_by_bow_kf(KeyFrame *pKF1, const std::vector<KeyFrame *> &cands, float nnratio, bool checkOri, std::vector<std::vector<MapPoint *>> &out,
                      std::vector<int> &nm, const char *who) {
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();   // one snapshot for the batch
    const size_t K = cands.size(), N1 = vpMapPoints1.size();
    out.assign(K, std::vector<MapPoint *>(N1, static_cast<MapPoint *>(nullptr)));
    nm.assign(K, 0);
    if (K == 0 || N1 == 0) return true;
    if ((int) N1 != pKF1->N) {
        ygzf_host::report_failure(who, "GetMapPointMatches does not have one slot per key");
        return false;
    }
    std::vector<uint8_t> valid1(N1), hold1;
    for (size_t i = 0; i < N1; i++) valid1[i] = vpMapPoints1[i] && !vpMapPoints1[i]->isBad();
    struct Side {
        std::vector<MapPoint *> mps;
        std::vector<uint8_t> valid, hold;
        std::vector<int> off1, idx1, off2, idx2;
    };
    std::vector<Side> side(K);
    std::vector<ygzf_bow_kf_candidate> q(K);
    const DBoW2::FeatureVector &vFeatVec1 = pKF1->mFeatVec;
    for (size_t k = 0; k < K; k++) {
        KeyFrame *pKF2 = cands[k];
        Side &S = side[k];
        S.mps = pKF2->GetMapPointMatches();
        const size_t N2 = S.mps.size();
        if ((int) N2 != pKF2->N) {
            ygzf_host::report_failure(who, "GetMapPointMatches does not have one slot per key");
            return false;
        }
        S.valid.resize(N2);
        for (size_t i = 0; i < N2; i++) S.valid[i] = S.mps[i] && !S.mps[i]->isBad();
        const DBoW2::FeatureVector &vFeatVec2 = pKF2->mFeatVec;
        S.off1.push_back(0);
        S.off2.push_back(0);
        DBoW2::FeatureVector::const_iterator f1it = vFeatVec1.begin(), f2it = vFeatVec2.begin();
        const DBoW2::FeatureVector::const_iterator f1end = vFeatVec1.end(), f2end = vFeatVec2.end();
        while (f1it != f1end && f2it != f2end) {
            if (f1it->first == f2it->first) {
                S.idx1.insert(S.idx1.end(), f1it->second.begin(), f1it->second.end());
                S.idx2.insert(S.idx2.end(), f2it->second.begin(), f2it->second.end());
                S.off1.push_back((int) S.idx1.size());
                S.off2.push_back((int) S.idx2.size());
                f1it++;
                f2it++;
            } else if (f1it->first < f2it->first) {
                f1it = vFeatVec1.lower_bound(f2it->first);
            } else {
                f2it = vFeatVec2.lower_bound(f1it->first);
            }
        }
        ygzf_bow_kf_candidate &Q = q[k];
        Q.n = (int) N2;
        Q.keys = (const ygzf_kp *) pKF2->mvKeys.data();
        Q.desc = desc_rows(pKF2->mDescriptors, (int) N2, S.hold);
        Q.valid = S.valid.data();
        Q.n_nodes = (int) S.off1.size() - 1;
        Q.off1 = S.off1.data(); Q.idx1 = S.idx1.data(); Q.off2 = S.off2.data(); Q.idx2 = S.idx2.data();
    }
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return false;
    std::vector<int> match12(K * N1 + 1);
    const int rc = ygzf_search_by_bow_kf(lease.get(), (int) N1, (const ygzf_kp *) pKF1->mvKeys.data(), desc_rows(pKF1->mDescriptors, (int) N1, hold1),
                                         valid1.data(), (int) K, q.data(), nnratio, checkOri, match12.data(), nm.data());
    if (rc != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
        nm.assign(K, 0);
        return false;
    }
    for (size_t k = 0; k < K; k++)
        for (size_t i = 0; i < N1; i++)
            if (match12[k * N1 + i] >= 0) out[k][i] = side[k].mps[match12[k * N1 + i]];   // :550
    return true;
}
}  // namespace

int SearchByBoWBatch(KeyFrame *pKF1, const std::vector<KeyFrame *> &candidates, float nnratio, bool checkOrientation,
                     std::vector<std::vector<MapPoint *>> &vvpMatches12, std::vector<int> &nmatches) {
    search_by_bow_kf(pKF1, candidates, nnratio, checkOrientation, vvpMatches12, nmatches, "ygz::SearchByBoWBatch");
    int enough = 0;
    for (int n : nmatches) enough += n >= 20;   // src/LoopClosing.cc:251
    return enough;
}

// src/ORBmatcher.cc:480-595: a batch of one
int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12) {
    std::vector<std::vector<MapPoint *>> out;
    std::vector<int> nm;
    search_by_bow_kf(pKF1, std::vector<KeyFrame *>{pKF2}, mfNNratio, mbCheckOrientation, out, nm, "ygz::ORBmatcher::SearchByBoW(KF, KF)");
    vpMatches12.swap(out[0]);
    return nm[0];
}

int SearchAndFuseBatch(const std::vector<std::pair<KeyFrame *, cv::Mat>> &poses, const std::vector<MapPoint *> &loopPoints, float th) {
    std::vector<KeyFrame *> kfs;
    std::vector<Pose> dec(poses.size());
    for (size_t k = 0; k < poses.size(); k++) {
        kfs.push_back(poses[k].first);
        loop::decompose_scw(poses[k].second, dec[k].R, dec[k].t, dec[k].Ow);
    }
    return search_and_fuse(kfs, dec, loopPoints, th, "ygz::SearchAndFuseBatch");
}

bool SearchAndFuseCandidates(const std::vector<std::pair<KeyFrame *, cv::Mat>> &poses, const std::vector<MapPoint *> &points,
                             const std::vector<uint8_t> &skip, float th, std::vector<int> &bestIdx, std::vector<int> &bestDist) {
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return false;
    std::vector<KeyFrame *> kfs;
    std::vector<Pose> dec(poses.size());
    std::vector<int> rows;
    for (size_t k = 0; k < poses.size(); k++) {
        kfs.push_back(poses[k].first);
        rows.push_back((int) k);
        loop::decompose_scw(poses[k].second, dec[k].R, dec[k].t, dec[k].Ow);
    }
    bestIdx.assign(poses.size() * points.size(), -1);
    bestDist.assign(poses.size() * points.size(), 256);
    return FuseScwQuery{lease.get(), kfs, dec, th, "ygz::SearchAndFuseCandidates"}(rows, points, skip, bestIdx, bestDist);
}

// src/ORBmatcher.cc:888-1004.  One keyframe of the batch without the Replace pass: vpReplacePoint comes back for the caller's own :562-567.
int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, float th, std::vector<MapPoint *> &vpReplacePoint) {
    const char *who = "ygz::ORBmatcher::Fuse(Scw)";
    const size_t P = vpPoints.size();
    if (P == 0) return 0;
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return 0;
    std::vector<Pose> pose(1);
    loop::decompose_scw(Scw, pose[0].R, pose[0].t, pose[0].Ow);
    const std::vector<KeyFrame *> kfs{pKF};
    const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();   // :904
    std::vector<uint8_t> skip(P);
    for (size_t i = 0; i < P; i++) skip[i] = (vpPoints[i]->isBad() || spAlreadyFound.count(vpPoints[i])) ? 1 : 0;   // :915
    std::vector<int> bi(P, -1), bd(P, 256);
    if (!FuseScwQuery{lease.get(), kfs, pose, th, who}(std::vector<int>{0}, vpPoints, skip, bi, bd)) return 0;
    int nFused = 0;
    for (size_t i = 0; i < P; i++) {   // :989-1000; no descriptor changes inside this member, so the one snapshot is current throughout
        if (skip[i] || bd[i] > TH_LOW) continue;
        MapPoint *pMP = vpPoints[i];
        MapPoint *pMPinKF = pKF->GetMapPoint(bi[i]);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
        } else {
            pMP->AddObservation(pKF, bi[i]);
            pKF->AddMapPoint(pMP, bi[i]);
        }
        nFused++;
    }
    return nFused;
}

// src/ORBmatcher.cc:265-373
int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, std::vector<MapPoint *> &vpMatched, int th) {
    const char *who = "ygz::ORBmatcher::SearchByProjection(KF, Scw)";
    if (vpPoints.empty()) return 0;
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return 0;
    Pose pose;
    loop::decompose_scw(Scw, pose.R, pose.t, pose.Ow);
    ygzf_fuse_kf kf;
    std::vector<uint8_t> hold;
    if (!pack_kf(pKF, pKF, &pose, kf, hold, who)) return 0;
    ygzf_ctx *c = lease.get();
    auto query = [&](size_t first, const std::vector<uint8_t> &skip, const std::vector<uint8_t> &mask, int nBest, std::vector<int> &ci,
                     std::vector<int> &cd) {
        const PointArrays pa(vpPoints, first, skip.data());
        const int rc = ygzf_search_by_projection_sim3(c, &kf, (int) (vpPoints.size() - first), &pa.view, skip.data(), mask.data(), (float) th, nBest,
                                                      TH_LOW, ci.data(), cd.data());
        if (rc != YGZF_OK) ygzf_host::report_failure(who, ygzf_last_error(c));
        return rc == YGZF_OK;
    };
    // 4 candidates per point: the device finds them in 4 passes over the point's window (keys, mask and Hamming distances read again each
    // pass), so this member does up to 4 times the search work of one pass to spare the rare second query.  Neither cost has been measured;
    // a per-lane top-k in one pass is the alternative if this member ever matters.
    return ygzf_host::search_by_projection_apply(vpPoints, vpMatched, 4, query).nmatches;
}

// src/ORBmatcher.cc:1006-1216
int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, const float &s12, const cv::Mat &R12,
                             const cv::Mat &t12, const float th) {
    const char *who = "ygz::ORBmatcher::SearchBySim3";
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return 0;
    ygzf_sim3_transforms T;
    {
        const Matrix3f R1 = pKF1->GetRotation(), R2 = pKF2->GetRotation();
        const Vector3f t1 = pKF1->GetTranslation(), t2 = pKF2->GetTranslation();
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) { T.R1w[3 * r + k] = R1(r, k); T.R2w[3 * r + k] = R2(r, k); }
            T.t1w[r] = t1[r];
            T.t2w[r] = t2[r];
        }
        loop::sim3_transforms(s12, R12, t12, T.sR12, T.t12, T.sR21, T.t21);
    }
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int) vpMapPoints1.size(), N2 = (int) vpMapPoints2.size();
    std::vector<uint8_t> skip1(N1, 0), skip2(N2, 0);   // vbAlreadyMatched1 / 2 (:1032-1043) joined with the tests of :1052-1056 / :1128-1132
    for (int i = 0; i < N1; i++) {
        MapPoint *pMP = vpMatches12[i];
        if (pMP) {
            skip1[i] = 1;
            const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
            if (idx2 >= 0 && idx2 < N2) skip2[idx2] = 1;
        }
    }
    for (int i = 0; i < N1; i++)
        if (!vpMapPoints1[i] || vpMapPoints1[i]->isBad()) skip1[i] = 1;
    for (int i = 0; i < N2; i++)
        if (!vpMapPoints2[i] || vpMapPoints2[i]->isBad()) skip2[i] = 1;
    ygzf_fuse_kf k1, k2;
    std::vector<uint8_t> h1, h2;
    if (N1 != pKF1->N || N2 != pKF2->N) {
        ygzf_host::report_failure(who, "GetMapPointMatches does not have one slot per key");
        return 0;
    }
    if (!pack_kf(pKF1, pKF1, nullptr, k1, h1, who) || !pack_kf(pKF2, pKF1, nullptr, k2, h2, who)) return 0;   // pKF1's fx fy cx cy for both (:1008-1011)
    const PointArrays p1(vpMapPoints1, 0, skip1.data()), p2(vpMapPoints2, 0, skip2.data());
    std::vector<int> m1(N1 + 1), m2(N2 + 1), m12(N1 + 1);
    int nFound = 0;
    const int rc = ygzf_search_by_sim3(lease.get(), &k1, &k2, &p1.view, &p2.view, skip1.data(), skip2.data(), &T, th, TH_HIGH, m1.data(), m2.data(),
                                       m12.data(), &nFound);
    if (rc != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
        return 0;
    }
    for (int i1 = 0; i1 < N1; i1++)
        if (m12[i1] >= 0) vpMatches12[i1] = vpMapPoints2[m12[i1]];   // :1209
    return nFound;
}

}  // namespace ygz
