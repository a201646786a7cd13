// bow_kf_shell.cc -- GPU test of the SearchByBoW(KeyFrame, KeyFrame) shells (tests/test_gpu_bow_kf.py).
// `bow_kf_shell <scene file>`: builds the KeyFrames of a scene the Python test wrote (keys, descriptors, mFeatVec maps, MapPoints -- some bad,
// some slots NULL), runs ORBmatcher(0.75, true).SearchByBoW(kf1, kf2, v) per candidate and then ygz::SearchByBoWBatch, and prints for both
// forms, per candidate, the return value and per KF1 slot the KF2 slot of the MapPoint returned (-1: NULL).  Python compares with its restatement.
// `bow_kf_shell time <candidates> <features> <min repeats> <min seconds>` (tools/bow_kf_rate.py): the batch call, one call per candidate, and
// the sequential search of src/ORBmatcher.cc:480-595 restated on the host, each as the median of its timed repeats with their range, on one
// generated scene of 100 vocabulary nodes.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>

#include "ORBmatcher.h"
#include "ORBmatcherLoop.h"
#include "ygzf_pool.h"

using namespace ygz;

namespace ygz {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;   // (ORBmatcher.cc reads them)
}

struct Kf {
    KeyFrame kf;
    std::vector<MapPoint> mps;    // slot i's MapPoint when it has one (sized once: the KeyFrame holds pointers into it)
};

static bool read_kf(FILE *f, Kf &K) {
    int n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
    K.kf.N = n;
    K.kf.mvKeys.resize(n);
    K.kf.mDescriptors.create(std::max(n, 1), 32, CV_8U);
    std::vector<uint8_t> state(n);
    if (n && (fread(K.kf.mvKeys.data(), sizeof(cv::KeyPoint), n, f) != (size_t) n || fread(K.kf.mDescriptors.ptr(0), 32, n, f) != (size_t) n ||
              fread(state.data(), 1, n, f) != (size_t) n))
        return false;
    K.mps.resize(n);
    K.kf.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) {      // 0: no MapPoint in the slot; 1: a good one; 2: a bad one
        if (!state[i]) continue;
        K.mps[i].mbBad = state[i] == 2;
        K.kf.mvpMapPoints[i] = &K.mps[i];
    }
    int nodes = 0;
    if (fread(&nodes, 4, 1, f) != 1) return false;
    for (int k = 0; k < nodes; k++) {
        int id = 0, cnt = 0;
        if (fread(&id, 4, 1, f) != 1 || fread(&cnt, 4, 1, f) != 1 || cnt < 0) return false;
        std::vector<unsigned int> idx(cnt);
        if (cnt && fread(idx.data(), 4, cnt, f) != (size_t) cnt) return false;
        K.kf.mFeatVec[(unsigned) id] = idx;
    }
    return true;
}

static void print_row(const char *form, size_t k, int ret, const Kf &K2, const std::vector<MapPoint *> &v) {
    std::printf("%s %zu %d", form, k, ret);
    for (MapPoint *p : v) {
        const bool own = p && !K2.mps.empty() && p >= &K2.mps.front() && p <= &K2.mps.back();
        std::printf(" %d", p ? (own ? (int) (p - &K2.mps.front()) : -3) : -1);
    }
    std::printf("\n");
}

// src/ORBmatcher.cc:480-595 restated on the host (the timing's third form): match12 per KF1 slot (-1 none), returns nmatches
static int search_by_bow_host(KeyFrame *pKF1, KeyFrame *pKF2, float nnratio, bool checkOri, std::vector<int> &match12) {
    const std::vector<MapPoint *> mp1 = pKF1->GetMapPointMatches(), mp2 = pKF2->GetMapPointMatches();
    match12.assign(mp1.size(), -1);
    std::vector<char> matched2(mp2.size(), 0);
    std::vector<int> rotHist[30];
    int nmatches = 0;
    auto it1 = pKF1->mFeatVec.begin(), it2 = pKF2->mFeatVec.begin();
    while (it1 != pKF1->mFeatVec.end() && it2 != pKF2->mFeatVec.end()) {
        if (it1->first == it2->first) {
            for (unsigned idx1 : it1->second) {
                if (!mp1[idx1] || mp1[idx1]->isBad()) continue;
                int best1 = 256, best2 = 256, bestIdx = -1;
                for (unsigned idx2 : it2->second) {
                    if (matched2[idx2] || !mp2[idx2] || mp2[idx2]->isBad()) continue;
                    const int d = ORBmatcher::DescriptorDistance(pKF1->mDescriptors.row(idx1), pKF2->mDescriptors.row(idx2));
                    if (d < best1) { best2 = best1; best1 = d; bestIdx = (int) idx2; }
                    else if (d < best2) best2 = d;
                }
                if (best1 < ORBmatcher::TH_LOW && (float) best1 < nnratio * (float) best2) {
                    match12[idx1] = bestIdx;
                    matched2[bestIdx] = 1;
                    if (checkOri) {
                        float rot = pKF1->mvKeys[idx1].angle - pKF2->mvKeys[bestIdx].angle;
                        if (rot < 0.0) rot += 360.0f;
                        int bin = (int) roundf(rot * (1.0f / 30));
                        if (bin == 30) bin = 0;
                        rotHist[bin].push_back((int) idx1);
                    }
                    nmatches++;
                }
            }
            it1++;
            it2++;
        } else if (it1->first < it2->first) {
            it1 = pKF1->mFeatVec.lower_bound(it2->first);
        } else {
            it2 = pKF2->mFeatVec.lower_bound(it1->first);
        }
    }
    if (checkOri) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < 30; i++) {
            const int s = (int) rotHist[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float) max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float) max1) { ind3 = -1; }
        for (int i = 0; i < 30; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int idx1 : rotHist[i]) { match12[idx1] = -1; nmatches--; }
        }
    }
    return nmatches;
}

template <class F>
static void timed(F &&f, int minReps, double minSeconds, double out[3]) {
    std::vector<double> ms;
    double total = 0;
    while ((int) ms.size() < minReps || total < minSeconds * 1000.0) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        total += ms.back();
    }
    std::sort(ms.begin(), ms.end());
    out[0] = ms[ms.size() / 2]; out[1] = ms.front(); out[2] = ms.back();
}

static unsigned g_rng = 12345u;
static unsigned rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// n features in 100 nodes; src: copy two thirds of the features from it with 3..40 bits flipped (same node), the rest unrelated
static void timing_kf(Kf &K, int n, const Kf *src) {
    K.kf.N = n;
    K.kf.mvKeys.resize(n);
    K.kf.mDescriptors.create(n, 32, CV_8U);
    K.mps.resize(n);
    K.kf.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
        uint8_t *d = K.kf.mDescriptors.ptr(i);
        unsigned node = rnd() % 100;
        float angle = (float) (rnd() % 360);
        if (src && rnd() % 3 != 0) {
            const int s = (int) (rnd() % (unsigned) src->kf.N);
            std::memcpy(d, src->kf.mDescriptors.ptr(s), 32);
            for (int k = 3 + (int) (rnd() % 38); k > 0; k--) { const unsigned b = rnd() % 256; d[b >> 3] ^= (uint8_t) (1u << (b & 7)); }
            for (const auto &kv : src->kf.mFeatVec)
                if (std::find(kv.second.begin(), kv.second.end(), (unsigned) s) != kv.second.end()) node = kv.first;
            angle = src->kf.mvKeys[s].angle - (rnd() % 8 ? 30.0f : (float) (rnd() % 360));
            if (angle < 0) angle += 360.0f;
        } else {
            for (int b = 0; b < 32; b++) d[b] = (uint8_t) rnd();
        }
        K.kf.mvKeys[i] = cv::KeyPoint{{(float) (i % 700), (float) (i / 700)}, 31.0f, angle, 1.0f, 0, -1};
        K.kf.mFeatVec[node].push_back((unsigned) i);
        if (rnd() % 100 < 85) K.kf.mvpMapPoints[i] = &K.mps[i];
    }
}

static int time_mode(int nCand, int nFeat, int minReps, double minSeconds) {
    Kf k1;
    std::deque<Kf> k2((size_t) nCand);
    timing_kf(k1, nFeat, nullptr);
    std::vector<KeyFrame *> cands;
    for (Kf &k : k2) { timing_kf(k, nFeat, &k1); cands.push_back(&k.kf); }
    const size_t K = cands.size();
    std::vector<std::vector<MapPoint *>> vb, vs(K);
    std::vector<int> nb, ns(K), nh(K);
    ygz::SearchByBoWBatch(&k1.kf, cands, 0.75f, true, vb, nb);   // (first lease: context creation outside the timed region)
    const unsigned long failures0 = ygzf_host::failure_count();
    double tb[3], ts[3], th[3];
    timed([&] { ygz::SearchByBoWBatch(&k1.kf, cands, 0.75f, true, vb, nb); }, minReps, minSeconds, tb);
    timed([&] {
        ygz::ORBmatcher matcher(0.75f, true);
        for (size_t k = 0; k < K; k++) ns[k] = matcher.SearchByBoW(&k1.kf, cands[k], vs[k]);
    }, minReps, minSeconds, ts);
    std::vector<std::vector<int>> mh(K);
    timed([&] { for (size_t k = 0; k < K; k++) nh[k] = search_by_bow_host(&k1.kf, cands[k], 0.75f, true, mh[k]); }, minReps, minSeconds, th);
    bool same = ygzf_host::failure_count() == failures0 && nb == ns && nb == nh && vb == vs;
    long matches = 0;
    for (size_t k = 0; k < K && same; k++) {
        matches += nb[k];
        for (size_t i = 0; i < mh[k].size(); i++)
            same = same && vb[k][i] == (mh[k][i] >= 0 ? cands[k]->mvpMapPoints[mh[k][i]] : nullptr);
    }
    std::printf("{\"candidates\": %zu, \"features\": %d, \"nodes\": 100, \"matches\": %ld, \"batch_ms\": [%.3f, %.3f, %.3f], "
                "\"singles_ms\": [%.3f, %.3f, %.3f], \"host_restatement_ms\": [%.3f, %.3f, %.3f], \"same_result\": %s}\n",
                K, nFeat, matches, tb[0], tb[1], tb[2], ts[0], ts[1], ts[2], th[0], th[1], th[2], same ? "true" : "false");
    return same ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 6 && std::string(argv[1]) == "time") return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atof(argv[5]));
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int nCand = 0;
    Kf k1;
    if (fread(&nCand, 4, 1, f) != 1 || nCand < 0 || !read_kf(f, k1)) return 2;
    std::deque<Kf> k2((size_t) nCand);
    std::vector<KeyFrame *> cands;
    for (Kf &k : k2) {
        if (!read_kf(f, k)) return 2;
        cands.push_back(&k.kf);
    }
    std::fclose(f);
    const unsigned long failures0 = ygzf_host::failure_count();
    ygz::ORBmatcher matcher(0.75f, true);
    for (size_t k = 0; k < cands.size(); k++) {
        std::vector<MapPoint *> v(3, nullptr);     // (the member resizes it)
        const int n = matcher.SearchByBoW(&k1.kf, cands[k], v);
        print_row("single", k, n, k2[k], v);
    }
    std::vector<std::vector<MapPoint *>> vv;
    std::vector<int> nm;
    const int enough = ygz::SearchByBoWBatch(&k1.kf, cands, 0.75f, true, vv, nm);
    for (size_t k = 0; k < cands.size(); k++) print_row("batch", k, nm[k], k2[k], vv[k]);
    std::printf("enough %d\n", enough);
    if (ygzf_host::failure_count() != failures0) {
        std::printf("device failure: %s\n", ygzf_host::last_failure().c_str());
        return 1;
    }
    std::printf("bow kf shell ok\n");
    return 0;
}
