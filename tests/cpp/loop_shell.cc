// loop_shell.cc -- GPU test of the loop-closing shells (tests/test_gpu_loop_search.py): on deep copies of one seeded synthetic map,
// ygz::SearchAndFuseBatch, a loop of ORBmatcher::Fuse(pKF, Scw, ..) + Replace, ORBmatcher::SearchByProjection(pKF, Scw, ..) and
// ORBmatcher::SearchBySim3, all over the device, must give the graph, vpMatched / vpMatches12 and return values of the sequential restatement
// (tests/cpp/loop_restate.h).
// `loop_shell time <kfs> <landmarks> <points> <min repeats> <min seconds>` (tools/loop_rate.py): SearchAndFuseBatch's device query as one call
// and as one call per keyframe, and the restated search on the host, each as the median of its timed repeats with their range.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ORBmatcher.h"
#include "ORBmatcherLoop.h"
#include "loop_restate.h"
#include "ygzf_pool.h"

using namespace loop_test;

namespace ygz {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;   // (ORBmatcher.cc reads them)
}

static std::vector<std::pair<KeyFrame *, cv::Mat>> pose_list(World &w) {
    std::vector<std::pair<KeyFrame *, cv::Mat>> v;
    const std::vector<cv::Mat> scw = world_scw(w);
    for (size_t k = 0; k < w.kfs.size(); k++) v.push_back({&w.kfs[k], scw[k]});
    return v;
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

static int time_mode(int nKf, int nLand, int nPoints, int minReps, double minSeconds) {
    World w = timing_world(nKf, nLand, nPoints, 0);
    const std::vector<std::pair<KeyFrame *, cv::Mat>> poses = pose_list(w);
    const std::vector<MapPoint *> pts = loop_points(w);
    const size_t K = poses.size(), P = pts.size();
    std::vector<uint8_t> skip(K * P);
    for (size_t k = 0; k < K; k++) {
        const std::set<MapPoint *> in = poses[k].first->GetMapPoints();
        for (size_t i = 0; i < P; i++) skip[k * P + i] = (pts[i]->isBad() || in.count(pts[i])) ? 1 : 0;
    }
    std::vector<int> bi, bd, si, sd, ci(K * P), cd(K * P);
    if (!ygz::SearchAndFuseCandidates(poses, pts, skip, 4.0f, bi, bd)) return 1;   // (first lease: context creation outside the timed region)
    double tb[3], ts[3], tc[3];
    bool ok = true;
    timed([&] { ok = ok && ygz::SearchAndFuseCandidates(poses, pts, skip, 4.0f, bi, bd); }, minReps, minSeconds, tb);
    std::vector<int> one_i(K * P), one_d(K * P);
    timed([&] {
        for (size_t k = 0; k < K; k++) {
            const std::vector<uint8_t> sk(skip.begin() + k * P, skip.begin() + (k + 1) * P);
            ok = ok && ygz::SearchAndFuseCandidates({poses[k]}, pts, sk, 4.0f, si, sd);
            std::copy(si.begin(), si.end(), one_i.begin() + k * P);
            std::copy(sd.begin(), sd.end(), one_d.begin() + k * P);
        }
    }, minReps, minSeconds, ts);
    std::vector<KeyFrame *> kfs;
    std::vector<cv::Mat> scw;
    std::vector<int> rows;
    for (size_t k = 0; k < K; k++) { kfs.push_back(poses[k].first); scw.push_back(poses[k].second); rows.push_back((int) k); }
    timed([&] { cpu_fuse_query(kfs, scw, rows, pts, skip, ci, cd, 4.0f); }, minReps, minSeconds, tc);
    const bool same = ok && bi == one_i && bd == one_d && bi == ci && bd == cd;
    long found = 0, keys = 0;
    for (int d : bd) found += d <= 50;
    for (size_t k = 0; k < K; k++) keys += poses[k].first->N;
    std::printf("{\"keyframes\": %zu, \"points\": %zu, \"keys_per_kf\": %ld, \"within_th_low\": %ld, \"batch_ms\": [%.3f, %.3f, %.3f], "
                "\"singles_ms\": [%.3f, %.3f, %.3f], \"host_restatement_ms\": [%.3f, %.3f, %.3f], \"same_result\": %s}\n",
                K, P, keys / (long) K, found, tb[0], tb[1], tb[2], ts[0], ts[1], ts[2], tc[0], tc[1], tc[2], same ? "true" : "false");
    return same ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 7 && std::string(argv[1]) == "time")
        return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atof(argv[6]));
    const unsigned seed = argc > 1 ? (unsigned) std::atoi(argv[1]) : 1u;
    const float th = 4.0f;
    World base = make_world(seed);
    const unsigned long failures0 = ygzf_host::failure_count();
    int bad = 0;
    // ---- SearchAndFuse: sequential restatement / one batch / the member per keyframe with the caller's Replace pass ----
    World a = deep_copy(base), b = deep_copy(base), c = deep_copy(base);
    const LoopCount cnt = search_and_fuse_sequential(all_kfs(a), world_scw(a), loop_points(a), th);
    const long nB = ygz::SearchAndFuseBatch(pose_list(b), loop_points(b), th);
    long nC = 0;
    {
        ygz::ORBmatcher matcher(0.8f);
        const std::vector<MapPoint *> lp = loop_points(c);
        for (auto &kp : pose_list(c)) {
            std::vector<MapPoint *> vpReplacePoints(lp.size(), nullptr);
            nC += matcher.Fuse(kp.first, kp.second, lp, th, vpReplacePoints);
            for (size_t i = 0; i < lp.size(); i++)
                if (vpReplacePoints[i]) vpReplacePoints[i]->Replace(lp[i]);
        }
    }
    bad += compare(a, b, "SearchAndFuseBatch") + compare(a, c, "ORBmatcher::Fuse(Scw)");
    if (cnt.fused != nB || cnt.fused != nC || cnt.fused == 0 || cnt.replaced == 0) { std::printf("fused %ld %ld %ld\n", cnt.fused, nB, nC); bad++; }
    // ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, 10) ----
    long matched = 0;
    for (int kf = 0; kf < 3; kf++) {
        World d = deep_copy(base), e = deep_copy(base);
        auto setup = [kf](World &w, std::vector<MapPoint *> &pts, std::vector<MapPoint *> &vm) {
            const size_t n = w.mps.size();
            for (size_t j = 0; j < n; j++) pts.push_back(&w.mps[(j * 7) % n]);
            vm.assign(w.kfs[kf].N, nullptr);
            for (int j = 0; j < w.kfs[kf].N; j += 2) vm[j] = w.kfs[kf].mvpMapPoints[j];
        };
        std::vector<MapPoint *> pd, pe, vd, ve;
        setup(d, pd, vd); setup(e, pe, ve);
        const cv::Mat scw = make_scw(base.kfs[kf], 1.13f);
        const int nD = search_by_projection_sequential(&d.kfs[kf], scw, pd, vd, 10);
        ygz::ORBmatcher matcher(0.75f);
        const int nE = matcher.SearchByProjection(&e.kfs[kf], scw, pe, ve, 10);
        bad += compare_matched(d, vd, e, ve, "vpMatched") + compare(d, e, "SearchByProjection(KF, Scw) writes no map");
        if (nD != nE || nD == 0) { std::printf("SearchByProjection(KF, Scw): %d %d\n", nD, nE); bad++; }
        matched += nD;
    }
    // ---- SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5): pairs of keyframes of the map; S12 = T1w T2w^-1 with the scale off by 2 % ----
    long found = 0, oneSided = 0;
    for (int pair = 0; pair < 3; pair++) {
        World d = deep_copy(base), e = deep_copy(base);
        const int i1 = pair, i2 = pair + 4;
        const KeyFrame &K1 = base.kfs[i1], &K2 = base.kfs[i2];
        const float s12 = 1.02f;
        float R12[9], t12[3];
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) {
                double v = 0;
                for (int m = 0; m < 3; m++) v += (double) K1.mRcw(r, m) * (double) K2.mRcw(k, m);   // R1w R2w'
                R12[3 * r + k] = (float) v;
            }
        for (int r = 0; r < 3; r++) {
            double v = K1.mtcw[r];
            for (int m = 0; m < 3; m++) v -= (double) s12 * (double) R12[3 * r + m] * (double) K2.mtcw[m];      // t1w - s12 R12 t2w
            t12[r] = (float) v;
        }
        auto setup = [&](World &w, std::vector<MapPoint *> &vm) {
            vm.assign(w.kfs[i1].N, nullptr);
            int n = 0;
            for (int j = 0; j < w.kfs[i2].N && n < 12; j++)      // a few entries already matched (SearchByBoW's, in LoopClosing), some of them points of KF2
                if (w.kfs[i2].mvpMapPoints[j] && j % 5 == 0) vm[(size_t) (3 * n++) % vm.size()] = w.kfs[i2].mvpMapPoints[j];
        };
        std::vector<MapPoint *> vd, ve;
        setup(d, vd); setup(e, ve);
        int one = 0;
        const int nD = search_by_sim3_sequential(&d.kfs[i1], &d.kfs[i2], vd, s12, R12, t12, 7.5f, &one);
        ygz::ORBmatcher matcher(0.75f);
        const int nE = matcher.SearchBySim3(&e.kfs[i1], &e.kfs[i2], ve, s12, mat32(3, 3, R12), mat32(3, 1, t12), 7.5f);
        bad += compare_matched(d, vd, e, ve, "vpMatches12") + compare(d, e, "SearchBySim3 writes no map");
        if (nD != nE || nD == 0) { std::printf("SearchBySim3: %d %d\n", nD, nE); bad++; }
        found += nD; oneSided += one;
    }
    if (oneSided == 0) { std::printf("no one-sided Sim3 match in this map\n"); bad++; }
    if (ygzf_host::failure_count() != failures0) { std::printf("device failure: %s\n", ygzf_host::last_failure().c_str()); bad++; }
    std::printf("seed %u fused %ld replaced %ld matched %ld sim3 %ld one_sided %ld\n", seed, cnt.fused, cnt.replaced, matched, found, oneSided);
    if (bad) return 1;
    std::printf("loop shell ok\n");
    return 0;
}
