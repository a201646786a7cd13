// loop_restate.h -- test support for the loop-closing projection searches over the stand-alone ygz_compat.h classes: C++ restatements of
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:888-1004) with LoopClosing::SearchAndFuse's loop
// (src/LoopClosing.cc:546-569), ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:265-373) and ORBmatcher::SearchBySim3
// (:1006-1216) -- sequential, in the reference's order, with the cv::Mat arithmetic include/ygzf.h fixes (OpenCV 2.4 / 3.2) -- over the seeded
// maps of fuse_restate.h, plus the restated searches in the shape of host/LoopApply.h's queries.  Compiled with -ffp-contract=off.
#ifndef YGZF_TESTS_LOOP_RESTATE_H
#define YGZF_TESTS_LOOP_RESTATE_H

#include <algorithm>
#include <set>
#include <utility>

#include "fuse_restate.h"

namespace loop_test {
using namespace fuse_test;

struct Pose { float R[9], t[3], Ow[3]; };   // a decomposed Scw

inline cv::Mat mat32(int r, int c, const float *v) {
    cv::Mat m(r, c, CV_32F);
    for (int i = 0; i < r; i++)
        for (int j = 0; j < c; j++) m.ptr<float>(i)[j] = v[i * c + j];
    return m;
}

// Scw = [s R | s t] for the keyframe's pose: the corrected Sim3 of LoopClosing::CorrectLoop, scale s
inline cv::Mat make_scw(const KeyFrame &K, float s) {
    float v[16] = {0};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) v[4 * r + c] = s * K.mRcw(r, c);
        v[4 * r + 3] = s * K.mtcw[r];
    }
    v[15] = 1;
    return mat32(4, 4, v);
}

// src/ORBmatcher.cc:274-278 / :897-901 in scalars (this project's stand-alone definition, written out here a second time on purpose):
// scw = (float) sqrt of the double sum of squares of row 0; entries times the double 1 / scw; Ow = -(Rcw' tcw) as float dots left to right
inline Pose decompose(const cv::Mat &Scw) {
    Pose p;
    const float *r0 = Scw.ptr<float>(0);
    double s = (double) r0[0] * (double) r0[0];
    s += (double) r0[1] * (double) r0[1];
    s += (double) r0[2] * (double) r0[2];
    const float scw = (float) std::sqrt(s);
    const double inv = 1.0 / (double) scw;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) p.R[3 * r + c] = (float) ((double) Scw.ptr<float>(r)[c] * inv);
        p.t[r] = (float) ((double) Scw.ptr<float>(r)[3] * inv);
    }
    for (int c = 0; c < 3; c++) p.Ow[c] = -((p.R[c] * p.t[0] + p.R[3 + c] * p.t[1]) + p.R[6 + c] * p.t[2]);
    return p;
}

inline float norm_cv(const float v[3]) {   // cv::norm on three floats
    double s = (double) v[0] * (double) v[0];
    s += (double) v[1] * (double) v[1];
    s += (double) v[2] * (double) v[2];
    return (float) std::sqrt(s);
}
inline void transform(const float R[9], const float t[3], const float p[3], float o[3]) {
    for (int r = 0; r < 3; r++) o[r] = ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + t[r];
}
inline int hamming(const unsigned char *a, const unsigned char *b) {
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned) (a[k] ^ b[k]));
    return d;
}

// the candidate list of one point: (distance, position in GetFeaturesInArea's list, key), ascending.  mode 0: Fuse(.., Scw, ..), 1:
// SearchByProjection(.., Scw, ..) (keys with taken[idx] passed over), 2: one SearchBySim3 direction (R2 / t2 chained; fx .. cy given: the
// reference projects both directions with pKF1's)
struct Cand { int dist, pos, idx; bool operator<(const Cand &o) const { return dist != o.dist ? dist < o.dist : pos < o.pos; } };
inline std::vector<Cand> candidates(KeyFrame *pKF, const Grid &G, MapPoint *pMP, float th, int mode, const Pose &pose, const float *R2 = nullptr,
                                    const float *t2 = nullptr, const std::vector<MapPoint *> *taken = nullptr, const KeyFrame *camOf = nullptr) {
    std::vector<Cand> out;
    const KeyFrame *C = camOf ? camOf : pKF;
    const ygz::Vector3f pw = pMP->GetWorldPos();
    const float p[3] = {pw[0], pw[1], pw[2]};
    float pc[3];
    transform(pose.R, pose.t, p, pc);
    if (mode == 2) {
        float q[3];
        transform(R2, t2, pc, q);
        pc[0] = q[0]; pc[1] = q[1]; pc[2] = q[2];
    }
    if (pc[2] < 0.0f) return out;
    const float invz = 1 / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = C->fx * x + C->cx, v = C->fy * y + C->cy;
    if (!pKF->IsInImage(u, v)) return out;
    const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
    const float PO[3] = {p[0] - pose.Ow[0], p[1] - pose.Ow[1], p[2] - pose.Ow[2]};
    const float dist = mode == 2 ? norm_cv(pc) : norm_cv(PO);
    if (dist < minDistance || dist > maxDistance) return out;
    if (mode != 2) {
        const ygz::Vector3f Pn = pMP->GetNormal();
        double dot = (double) PO[0] * (double) Pn[0];
        dot += (double) PO[1] * (double) Pn[1];
        dot += (double) PO[2] * (double) Pn[2];
        if (dot < 0.5 * dist) return out;
    }
    const int nPredictedLevel = pMP->PredictScale(dist, pKF);
    const float radius = th * pKF->mvScaleFactors[nPredictedLevel];
    const std::vector<size_t> vIndices = features_in_area(pKF, G, u, v, radius);
    const cv::Mat dMP = pMP->GetDescriptor();
    for (size_t k = 0; k < vIndices.size(); k++) {
        const size_t idx = vIndices[k];
        if (mode == 1 && taken && (*taken)[idx]) continue;
        const int kpLevel = pKF->mvKeys[idx].octave;
        if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
        const int d = hamming(dMP.data, pKF->mDescriptors.ptr((int) idx));
        if (d < 256) out.push_back({d, (int) k, (int) idx});
    }
    std::sort(out.begin(), out.end());
    return out;
}

// ---- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), :888-1004 ---------------------------------------------------------------------------------
inline int fuse_scw_sequential(KeyFrame *pKF, const cv::Mat &Scw, const std::vector<MapPoint *> &vpPoints, float th,
                               std::vector<MapPoint *> &vpReplacePoint) {
    const Pose pose = decompose(Scw);
    const Grid G(pKF);
    const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();
    int nFused = 0;
    for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
        MapPoint *pMP = vpPoints[iMP];
        if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        const std::vector<Cand> c = candidates(pKF, G, pMP, th, 0, pose);
        if (c.empty() || c[0].dist > 50) continue;
        MapPoint *pMPinKF = pKF->GetMapPoint(c[0].idx);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
        } else {
            pMP->AddObservation(pKF, c[0].idx);
            pKF->AddMapPoint(pMP, c[0].idx);
        }
        nFused++;
    }
    return nFused;
}

// LoopClosing::SearchAndFuse, src/LoopClosing.cc:546-569
struct LoopCount { long fused = 0, replaced = 0, added = 0, sameSlot = 0; };
inline LoopCount search_and_fuse_sequential(const std::vector<KeyFrame *> &kfs, const std::vector<cv::Mat> &scw, const std::vector<MapPoint *> &loopPoints,
                                            float th, std::vector<int> *perKf = nullptr) {
    LoopCount n;
    for (size_t k = 0; k < kfs.size(); k++) {
        std::vector<MapPoint *> vpReplacePoints(loopPoints.size(), nullptr);
        const int f = fuse_scw_sequential(kfs[k], scw[k], loopPoints, th, vpReplacePoints);
        n.fused += f;
        if (perKf) perKf->push_back(f);
        for (size_t i = 0; i < loopPoints.size(); i++)
            if (vpReplacePoints[i]) {
                n.sameSlot += std::count(loopPoints.begin(), loopPoints.end(), vpReplacePoints[i]) > 0;   // a listed point found in the slot
                vpReplacePoints[i]->Replace(loopPoints[i]);
                n.replaced++;
            }
    }
    return n;
}

// ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), :265-373 -------------------------------------------------------------------------
inline int search_by_projection_sequential(KeyFrame *pKF, const cv::Mat &Scw, const std::vector<MapPoint *> &vpPoints,
                                           std::vector<MapPoint *> &vpMatched, int th) {
    const Pose pose = decompose(Scw);
    const Grid G(pKF);
    std::set<MapPoint *> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPoint *>(nullptr));
    int nmatches = 0;
    for (MapPoint *pMP : vpPoints) {
        if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        const std::vector<Cand> c = candidates(pKF, G, pMP, (float) th, 1, pose, nullptr, nullptr, &vpMatched);
        if (c.empty() || c[0].dist > 50) continue;
        vpMatched[c[0].idx] = pMP;
        nmatches++;
    }
    return nmatches;
}

// ---- SearchBySim3, :1006-1216 ----------------------------------------------------------------------------------------------------------------
struct Sim3T { float sR12[9], t12[3], sR21[9], t21[3]; };
// :1022-1024 in scalars: s12 * R12 (the double product of two floats, rounded once), (1.0 / s12) * R12' with the double quotient, t21 = -(sR21 t12)
inline Sim3T sim3_transforms(float s12, const float R12[9], const float t12[3]) {
    Sim3T T;
    const double inv = 1.0 / (double) s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            T.sR12[3 * r + c] = (float) ((double) s12 * (double) R12[3 * r + c]);
            T.sR21[3 * r + c] = (float) (inv * (double) R12[3 * c + r]);
        }
    for (int r = 0; r < 3; r++) {
        T.t12[r] = t12[r];
        T.t21[r] = -((T.sR21[3 * r] * t12[0] + T.sR21[3 * r + 1] * t12[1]) + T.sR21[3 * r + 2] * t12[2]);
    }
    return T;
}
inline Pose pose_of(const KeyFrame *K) {
    Pose p;
    for (int i = 0; i < 9; i++) p.R[i] = K->mRcw.m[i];
    for (int i = 0; i < 3; i++) { p.t[i] = K->mtcw[i]; p.Ow[i] = K->mOw[i]; }
    return p;
}
inline int search_by_sim3_sequential(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, float s12, const float R12[9],
                                     const float t12[3], float th, int *oneSided = nullptr) {
    const Sim3T T = sim3_transforms(s12, R12, t12);
    const Pose P1 = pose_of(pKF1), P2 = pose_of(pKF2);
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int) vpMapPoints1.size(), N2 = (int) vpMapPoints2.size();
    std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);
    for (int i = 0; i < N1; i++) {
        MapPoint *pMP = vpMatches12[i];
        if (pMP) {
            vbAlreadyMatched1[i] = true;
            const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
            if (idx2 >= 0 && idx2 < N2) vbAlreadyMatched2[idx2] = true;
        }
    }
    std::vector<int> vnMatch1(N1, -1), vnMatch2(N2, -1);
    const Grid G1(pKF1), G2(pKF2);
    for (int i1 = 0; i1 < N1; i1++) {
        MapPoint *pMP = vpMapPoints1[i1];
        if (!pMP || vbAlreadyMatched1[i1] || pMP->isBad()) continue;
        const std::vector<Cand> c = candidates(pKF2, G2, pMP, th, 2, P1, T.sR21, T.t21, nullptr, pKF1);
        if (!c.empty() && c[0].dist <= 100) vnMatch1[i1] = c[0].idx;
    }
    for (int i2 = 0; i2 < N2; i2++) {
        MapPoint *pMP = vpMapPoints2[i2];
        if (!pMP || vbAlreadyMatched2[i2] || pMP->isBad()) continue;
        const std::vector<Cand> c = candidates(pKF1, G1, pMP, th, 2, P2, T.sR12, T.t12, nullptr, pKF1);
        if (!c.empty() && c[0].dist <= 100) vnMatch2[i2] = c[0].idx;
    }
    int nFound = 0, one = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0) {
            if (vnMatch2[idx2] == i1) {
                vpMatches12[i1] = vpMapPoints2[idx2];
                nFound++;
            } else {
                one++;
            }
        }
    }
    if (oneSided) *oneSided = one;
    return nFound;
}

// ---- the restated searches as host/LoopApply.h's queries -------------------------------------------------------------------------------------
inline bool cpu_fuse_query(const std::vector<KeyFrame *> &kfs, const std::vector<cv::Mat> &scw, const std::vector<int> &rows,
                           const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi, std::vector<int> &bd, float th) {
    for (size_t r = 0; r < rows.size(); r++) {
        KeyFrame *K = kfs[rows[r]];
        const Grid G(K);
        const Pose pose = decompose(scw[rows[r]]);
        for (size_t i = 0; i < pts.size(); i++) {
            const size_t o = r * pts.size() + i;
            bi[o] = -1;
            bd[o] = 256;
            if (skip[o]) continue;
            const std::vector<Cand> c = candidates(K, G, pts[i], th, 0, pose);
            if (!c.empty()) { bi[o] = c[0].idx; bd[o] = c[0].dist; }
        }
    }
    return true;
}
inline bool cpu_projection_query(KeyFrame *K, const cv::Mat &Scw, const std::vector<MapPoint *> &pts, size_t first, const std::vector<uint8_t> &skip,
                                 const std::vector<uint8_t> &mask, int nBest, std::vector<int> &ci, std::vector<int> &cd, float th) {
    const Grid G(K);
    const Pose pose = decompose(Scw);
    std::vector<MapPoint *> taken(mask.size(), nullptr);
    for (size_t j = 0; j < mask.size(); j++) taken[j] = mask[j] ? pts[0] : nullptr;   // (any non-null value)
    for (size_t i = first; i < pts.size(); i++) {
        int *oi = &ci[(i - first) * (size_t) nBest], *od = &cd[(i - first) * (size_t) nBest];
        for (int k = 0; k < nBest; k++) { oi[k] = -1; od[k] = 256; }
        if (skip[i - first]) continue;
        const std::vector<Cand> c = candidates(K, G, pts[i], th, 1, pose, nullptr, nullptr, &taken);
        int n = 0;
        for (const Cand &x : c)
            if (x.dist <= 50 && n < nBest) { oi[n] = x.idx; od[n] = x.dist; n++; }
    }
    return true;
}

// the loop-point list of a world: LoopClosing's mvpLoopMapPoints holds every good MapPoint of the loop keyframe and its neighbours once; the
// restatement and the resolver must also agree on lists with duplicates and bad points, so those of make_world stay in (its nullptr does not:
// the reference dereferences every entry)
inline std::vector<MapPoint *> loop_points(World &w) {
    std::vector<MapPoint *> v;
    for (int i : w.points)
        if (i >= 0) v.push_back(&w.mps[i]);
    return v;
}
inline std::vector<KeyFrame *> all_kfs(World &w) {
    std::vector<KeyFrame *> v;
    for (KeyFrame &k : w.kfs) v.push_back(&k);
    return v;
}
inline std::vector<cv::Mat> world_scw(World &w) {
    std::vector<cv::Mat> v;
    const float s[4] = {1.07f, 0.93f, 1.21f, 0.88f};
    for (size_t k = 0; k < w.kfs.size(); k++) v.push_back(make_scw(w.kfs[k], s[k % 4]));
    return v;
}
inline int compare_matched(const World &a, const std::vector<MapPoint *> &va, const World &b, const std::vector<MapPoint *> &vb, const char *what) {
    int bad = va.size() != vb.size();
    for (size_t i = 0; i < va.size() && i < vb.size(); i++)
        if (mp_index(a, va[i]) != mp_index(b, vb[i]) && bad++ < 10) std::printf("%s differs at %zu\n", what, i);
    return bad;
}
}  // namespace loop_test
#endif
