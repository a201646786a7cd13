// fuse_restate.h -- test support for ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) over the stand-alone ygz_compat.h classes:
// a seeded synthetic map (keyframes, MapPoints with duplicates, bad points, stereo and mono keys), its deep copy, a C++ restatement of the
// reference's candidate search (src/ORBmatcher.cc:764-868 + KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:774-809), the sequential Fuse loop
// (:748-886), and a comparison of two final graphs.  Compiled with -ffp-contract=off so that the search rounds as the device does.
#ifndef YGZF_TESTS_FUSE_RESTATE_H
#define YGZF_TESTS_FUSE_RESTATE_H

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ygz_compat.h"

namespace fuse_test {
using ygz::KeyFrame;
using ygz::MapPoint;

struct World {
    std::vector<KeyFrame> kfs;   // contiguous: pointer order = index order in every copy (std::map<KeyFrame*, ...> iterates alike)
    std::vector<MapPoint> mps;
    std::vector<int> targets;    // indices into kfs (with duplicates)
    std::vector<int> points;     // indices into mps (with duplicates), -1 = nullptr
    std::vector<KeyFrame *> target_ptrs() { std::vector<KeyFrame *> v; for (int t : targets) v.push_back(&kfs[t]); return v; }
    std::vector<MapPoint *> point_ptrs() { std::vector<MapPoint *> v; for (int i : points) v.push_back(i < 0 ? nullptr : &mps[i]); return v; }
};

inline int kf_index(const World &w, const KeyFrame *p) { return p ? (int) (p - w.kfs.data()) : -1; }
inline int mp_index(const World &w, const MapPoint *p) { return p ? (int) (p - w.mps.data()) : -1; }

inline World deep_copy(const World &a) {
    World b;
    b.kfs = a.kfs;
    b.mps = a.mps;
    b.targets = a.targets;
    b.points = a.points;
    for (KeyFrame &k : b.kfs) {
        k.mDescriptors = k.mDescriptors.clone();
        for (MapPoint *&p : k.mvpMapPoints) p = p ? &b.mps[mp_index(a, p)] : nullptr;
    }
    for (MapPoint &m : b.mps) {
        m.mDescriptor = m.mDescriptor.clone();
        std::map<KeyFrame *, size_t> obs;
        for (auto &o : m.mObservations) obs[&b.kfs[kf_index(a, o.first)]] = o.second;
        m.mObservations = obs;
        m.mpReplaced = m.mpReplaced ? &b.mps[mp_index(a, m.mpReplaced)] : nullptr;
    }
    return b;
}

// ---- the map ------------------------------------------------------------------------------------------------------------------
inline World make_world(unsigned seed, int nKf = 8, int nLand = 500, double pSeen = 0.4) {
    std::mt19937 rng(seed);
    auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto I = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    const float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f;
    World w;
    w.kfs.resize(nKf);
    struct Land { double X[3]; unsigned char d[32]; };
    std::vector<Land> land(nLand);
    for (Land &l : land) {
        l.X[0] = U(-3, 3); l.X[1] = U(-2, 2); l.X[2] = U(3, 9);
        for (int b = 0; b < 32; b++) l.d[b] = (unsigned char) I(0, 255);
    }
    std::vector<std::vector<std::pair<int, int>>> seen(nLand);   // landmark -> (kf, key index)
    for (int k = 0; k < nKf; k++) {
        KeyFrame &K = w.kfs[k];
        K.mnId = (unsigned long) k + 1;
        const bool five = (k % 4 == 3);   // another pyramid: 5 levels of 1.5
        const int L = five ? 5 : 8;
        const float s = five ? 1.5f : 1.2f;
        K.mnScaleLevels = L;
        K.mfLogScaleFactor = std::log(s);
        K.mvScaleFactors.assign(L, 1.f);
        for (int l = 1; l < L; l++) K.mvScaleFactors[l] = K.mvScaleFactors[l - 1] * s;
        K.mvInvLevelSigma2.resize(L);
        K.mvLevelSigma2.resize(L);
        for (int l = 0; l < L; l++) { K.mvLevelSigma2[l] = K.mvScaleFactors[l] * K.mvScaleFactors[l]; K.mvInvLevelSigma2[l] = 1.0f / K.mvLevelSigma2[l]; }
        K.fx = fx; K.fy = fy; K.cx = cx; K.cy = cy;
        K.mbf = (k % 2 == 0) ? 40.f : 0.f;
        K.mnMinX = 0; K.mnMinY = 0; K.mnMaxX = 752; K.mnMaxY = 480;
        const double ay = U(-0.08, 0.08), ax = U(-0.05, 0.05);
        const double R[9] = {std::cos(ay), 0, std::sin(ay), std::sin(ax) * std::sin(ay), std::cos(ax), -std::sin(ax) * std::cos(ay),
                             -std::cos(ax) * std::sin(ay), std::sin(ax), std::cos(ax) * std::cos(ay)};
        const double t[3] = {U(-0.3, 0.3), U(-0.1, 0.1), U(-0.2, 0.2)};
        for (int i = 0; i < 9; i++) K.mRcw.m[i] = (float) R[i];
        for (int i = 0; i < 3; i++) {
            K.mtcw[i] = (float) t[i];
            K.mOw[i] = (float) -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
        }
        std::vector<cv::KeyPoint> keys;
        std::vector<float> ur;
        std::vector<unsigned char> desc;
        for (int l = 0; l < nLand; l++) {
            if (U(0, 1) >= pSeen) continue;
            const double *X = land[l].X;
            double pc[3];
            for (int r = 0; r < 3; r++) pc[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
            const double u = fx * pc[0] / pc[2] + cx + U(-0.6, 0.6), v = fy * pc[1] / pc[2] + cy + U(-0.6, 0.6);
            if (u < 0 || u >= 752 || v < 0 || v >= 480) continue;
            const int reps = U(0, 1) < 0.05 ? 2 : 1;   // a landmark detected twice: equal distances
            for (int rep = 0; rep < reps; rep++) {
                cv::KeyPoint kp{};
                kp.pt.x = (float) u; kp.pt.y = (float) v;
                kp.octave = I(0, std::min(L - 1, 3));
                kp.size = 31;
                keys.push_back(kp);
                ur.push_back(K.mbf > 0 && U(0, 1) < 0.5 ? (float) (u - K.mbf / pc[2]) : -1.f);
                unsigned char d[32];
                std::memcpy(d, land[l].d, 32);
                const int flips = I(4, 34);
                for (int f = 0; f < flips; f++) { const int b = I(0, 255); d[b >> 3] ^= (unsigned char) (1 << (b & 7)); }
                desc.insert(desc.end(), d, d + 32);
                seen[l].push_back({k, (int) keys.size() - 1});
            }
        }
        for (int j = 0; j < 80; j++) {   // clutter
            cv::KeyPoint kp{};
            kp.pt.x = (float) U(0, 752); kp.pt.y = (float) U(0, 480); kp.octave = I(0, L - 1); kp.size = 31;
            keys.push_back(kp);
            ur.push_back(-1.f);
            for (int b = 0; b < 32; b++) desc.push_back((unsigned char) I(0, 255));
        }
        K.N = (int) keys.size();
        K.mvKeys = keys;
        K.mvuRight = ur;
        K.mDescriptors = cv::Mat(K.N, 32, CV_8U);
        std::memcpy(K.mDescriptors.data, desc.data(), desc.size());
        K.mvpMapPoints.assign(K.N, nullptr);
    }
    // MapPoints: every landmark's observations split among up to three MapPoints (the duplicates Fuse merges); some slots stay empty
    w.mps.reserve((size_t) nLand * 3);
    for (int l = 0; l < nLand; l++) {
        if (seen[l].empty()) continue;
        const int parts = I(1, 3);
        std::vector<int> owner(seen[l].size());
        for (size_t o = 0; o < owner.size(); o++) owner[o] = U(0, 1) < 0.15 ? -1 : I(0, parts - 1);
        for (int p = 0; p < parts; p++) {
            std::vector<std::pair<int, int>> mine;
            for (size_t o = 0; o < owner.size(); o++)
                if (owner[o] == p && !w.kfs[seen[l][o].first].mvpMapPoints[seen[l][o].second]) {
                    bool dupKf = false;
                    for (auto &m : mine) dupKf = dupKf || m.first == seen[l][o].first;
                    if (!dupKf) mine.push_back(seen[l][o]);
                }
            if (mine.empty()) continue;
            w.mps.emplace_back();
            MapPoint &M = w.mps.back();
            M.mnId = w.mps.size();
            M.nObs = 0;
            for (int r = 0; r < 3; r++) M.mWorldPos[r] = (float) (land[l].X[r] + U(-0.01, 0.01));
            for (auto &m : mine) {
                M.AddObservation(&w.kfs[m.first], m.second);
                w.kfs[m.first].mvpMapPoints[m.second] = &M;
            }
            // normal: mean viewing direction; distances as MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:291-341) of the first observation
            double n[3] = {0, 0, 0}, d0 = 0;
            for (auto &m : mine) {
                double v[3], nn = 0;
                for (int r = 0; r < 3; r++) { v[r] = M.mWorldPos[r] - w.kfs[m.first].mOw[r]; nn += v[r] * v[r]; }
                nn = std::sqrt(nn);
                if (d0 == 0) d0 = nn;
                for (int r = 0; r < 3; r++) n[r] += v[r] / nn;
            }
            const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int r = 0; r < 3; r++) M.mNormalVector[r] = (float) (n[r] / nl);
            const KeyFrame &K0 = w.kfs[mine[0].first];
            const int oct = K0.mvKeys[mine[0].second].octave;
            M.mfMaxDistance = (float) d0 * K0.mvScaleFactors[oct];
            M.mfMinDistance = M.mfMaxDistance / K0.mvScaleFactors[K0.mnScaleLevels - 1];
            M.ComputeDistinctiveDescriptors();
            if (U(0, 1) < 0.03) M.mbBad = true;   // a bad point still held by its keyframes (pMPinKF->isBad())
        }
    }
    for (int k = 0; k < nKf; k++) w.targets.push_back(k);
    w.targets.push_back(1);
    w.targets.push_back(4);
    for (size_t i = 0; i < w.mps.size(); i++)
        if (U(0, 1) < 0.5) w.points.push_back((int) i);
    for (int j = 0; j < 20; j++) w.points.push_back(w.points[I(0, (int) w.points.size() - 1)]);   // the same point listed twice
    w.points.push_back(-1);
    return w;
}

// the shapes of tools/fuse_rate.py: targets 0 .. nKf-1 plus nDup duplicates and the first nPoints MapPoints (forward pass), or with nDup < 0
// every point into keyframe 0 (reverse pass, sparser keyframes)
inline World timing_world(int nKf, int nLand, int nPoints, int nDup) {
    World base = make_world(7, nKf, nLand, nDup < 0 ? 0.07 : 0.4);
    base.targets.clear();
    for (int k = 0; k < (nDup < 0 ? 1 : nKf); k++) base.targets.push_back(k);
    for (int d = 0; d < nDup; d++) base.targets.push_back(d % nKf);
    base.points.clear();
    for (int i = 0; i < (int) base.mps.size() && (int) base.points.size() < nPoints; i++) base.points.push_back(i);
    return base;
}

// ---- KeyFrame::GetFeaturesInArea over the grid of Frame::AssignFeaturesToGrid (src/Frame.cc:314-330, 483-493) -------------------------------
struct Grid {
    std::vector<std::vector<size_t>> cells;   // 64 x 48, column-major as mGrid[ix][iy]
    explicit Grid(const KeyFrame *K) : cells(64 * 48) {
        const float wInv = (float) 64 / (float) (K->mnMaxX - K->mnMinX), hInv = (float) 48 / (float) (K->mnMaxY - K->mnMinY);
        for (int i = 0; i < K->N; i++) {
            const int px = (int) std::round((K->mvKeys[i].pt.x - K->mnMinX) * wInv), py = (int) std::round((K->mvKeys[i].pt.y - K->mnMinY) * hInv);
            if (px < 0 || px >= 64 || py < 0 || py >= 48) continue;
            cells[px * 48 + py].push_back(i);
        }
    }
};
inline std::vector<size_t> features_in_area(const KeyFrame *K, const Grid &G, float x, float y, float r) {
    const int COLS = 64, ROWS = 48;
    const float wInv = (float) COLS / (float) (K->mnMaxX - K->mnMinX), hInv = (float) ROWS / (float) (K->mnMaxY - K->mnMinY);
    const std::vector<std::vector<size_t>> &grid = G.cells;
    std::vector<size_t> v;
    const int nMinCellX = std::max(0, (int) std::floor((x - K->mnMinX - r) * wInv));
    if (nMinCellX >= COLS) return v;
    const int nMaxCellX = std::min(COLS - 1, (int) std::ceil((x - K->mnMinX + r) * wInv));
    if (nMaxCellX < 0) return v;
    const int nMinCellY = std::max(0, (int) std::floor((y - K->mnMinY - r) * hInv));
    if (nMinCellY >= ROWS) return v;
    const int nMaxCellY = std::min(ROWS - 1, (int) std::ceil((y - K->mnMinY + r) * hInv));
    if (nMaxCellY < 0) return v;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
            for (size_t j : grid[ix * ROWS + iy]) {
                const float distx = K->mvKeys[j].pt.x - x, disty = K->mvKeys[j].pt.y - y;
                if (std::fabs(distx) < r && std::fabs(disty) < r) v.push_back(j);
            }
    return v;
}

// ---- the candidate search of src/ORBmatcher.cc:764-868 -----------------------------------------------------------------------------------
inline void search(KeyFrame *pKF, const Grid &G, MapPoint *pMP, float th, int &bestIdx, int &bestDist) {
    bestDist = 256;
    bestIdx = -1;
    const ygz::Matrix3f Rcw = pKF->GetRotation();
    const ygz::Vector3f tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter(), p = pMP->GetWorldPos();
    float pc[3];
    for (int r = 0; r < 3; r++) pc[r] = (Rcw(r, 0) * p[0] + Rcw(r, 1) * p[1] + Rcw(r, 2) * p[2]) + tcw[r];
    if (pc[2] < 0.0f) return;
    const float invz = 1 / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = pKF->fx * x + pKF->cx, v = pKF->fy * y + pKF->cy;
    if (!pKF->IsInImage(u, v)) return;
    const float ur = u - pKF->mbf * invz;
    const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
    const float PO[3] = {p[0] - Ow[0], p[1] - Ow[1], p[2] - Ow[2]};
    const float dist3D = std::sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
    if (dist3D < minDistance || dist3D > maxDistance) return;
    const ygz::Vector3f Pn = pMP->GetNormal();
    if (PO[0] * Pn[0] + PO[1] * Pn[1] + PO[2] * Pn[2] < 0.5 * dist3D) return;
    const int nPredictedLevel = pMP->PredictScale(dist3D, pKF);
    const float radius = th * pKF->mvScaleFactors[nPredictedLevel];
    const std::vector<size_t> vIndices = features_in_area(pKF, G, u, v, radius);
    if (vIndices.empty()) return;
    const cv::Mat dMP = pMP->GetDescriptor();
    for (size_t idx : vIndices) {
        const cv::KeyPoint &kp = pKF->mvKeys[idx];
        const int kpLevel = kp.octave;
        if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
        const float ex = u - kp.pt.x, ey = v - kp.pt.y;
        if (pKF->mvuRight[idx] >= 0) {
            const float er = ur - pKF->mvuRight[idx];
            const float e2 = ex * ex + ey * ey + er * er;
            if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 7.8) continue;
        } else {
            const float e2 = ex * ex + ey * ey;
            if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 5.99) continue;
        }
        int dist = 0;
        for (int b = 0; b < 32; b++) dist += __builtin_popcount((unsigned) (dMP.data[b] ^ pKF->mDescriptors.ptr((int) idx)[b]));
        if (dist < bestDist) {
            bestDist = dist;
            bestIdx = (int) idx;
        }
    }
}

// ---- the sequential reference: ORBmatcher::Fuse, src/ORBmatcher.cc:748-886 -----------------------------------------------------------------
struct BranchCount { int intoKf = 0, intoMp = 0, equalObs = 0, badInKf = 0, added = 0; };   // pMP->Replace(pMPinKF) / pMPinKF->Replace(pMP) / ties / bad pMPinKF / Add
inline BranchCount g_branches;
inline int fuse_sequential(KeyFrame *pKF, const std::vector<MapPoint *> &vpMapPoints, float th) {
    int nFused = 0;
    const Grid G(pKF);
    for (MapPoint *pMP : vpMapPoints) {
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        int bestIdx, bestDist;
        search(pKF, G, pMP, th, bestIdx, bestDist);
        if (bestDist <= 50) {
            MapPoint *pMPinKF = pKF->GetMapPoint(bestIdx);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    g_branches.equalObs += pMPinKF->Observations() == pMP->Observations();
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF), g_branches.intoKf++;
                    else pMPinKF->Replace(pMP), g_branches.intoMp++;
                } else {
                    g_branches.badInKf++;
                }
            } else {
                g_branches.added++;
                pMP->AddObservation(pKF, bestIdx);
                pKF->AddMapPoint(pMP, bestIdx);
            }
            nFused++;
        }
    }
    return nFused;
}

// the restated search as FuseApply's query
inline bool cpu_query(const std::vector<KeyFrame *> &kfs, const std::vector<MapPoint *> &pts, const std::vector<uint8_t> &skip, std::vector<int> &bi,
                      std::vector<int> &bd, float th) {
    for (size_t r = 0; r < kfs.size(); r++) {
        const Grid G(kfs[r]);
        for (size_t i = 0; i < pts.size(); i++) {
            const size_t o = r * pts.size() + i;
            bi[o] = -1;
            bd[o] = 256;
            if (!skip[o]) search(kfs[r], G, pts[i], th, bi[o], bd[o]);
        }
    }
    return true;
}

// ---- whole-graph comparison --------------------------------------------------------------------------------------------------------------
inline int compare(const World &a, const World &b, const char *what) {
    int bad = 0;
    auto err = [&](const char *m, int i) { if (bad++ < 10) std::printf("%s: %s differs at %d\n", what, m, i); };
    for (size_t k = 0; k < a.kfs.size(); k++)
        for (size_t j = 0; j < a.kfs[k].mvpMapPoints.size(); j++)
            if (mp_index(a, a.kfs[k].mvpMapPoints[j]) != mp_index(b, b.kfs[k].mvpMapPoints[j])) err("mvpMapPoints", (int) k);
    for (size_t i = 0; i < a.mps.size(); i++) {
        const MapPoint &p = a.mps[i], &q = b.mps[i];
        if (p.mbBad != q.mbBad) err("bad flag", (int) i);
        if (mp_index(a, p.mpReplaced) != mp_index(b, q.mpReplaced)) err("replacement", (int) i);
        if (p.nObs != q.nObs) err("nObs", (int) i);
        if (p.mnVisible != q.mnVisible || p.mnFound != q.mnFound) err("visible/found", (int) i);
        if (p.mObservations.size() != q.mObservations.size()) err("observations", (int) i);
        else
            for (auto ia = p.mObservations.begin(), ib = q.mObservations.begin(); ia != p.mObservations.end(); ++ia, ++ib)
                if (kf_index(a, ia->first) != kf_index(b, ib->first) || ia->second != ib->second) { err("observations", (int) i); break; }
        if (p.mDescriptor.empty() != q.mDescriptor.empty() || (!p.mDescriptor.empty() && std::memcmp(p.mDescriptor.data, q.mDescriptor.data, 32)))
            err("descriptor", (int) i);
    }
    return bad;
}
}  // namespace fuse_test
#endif
