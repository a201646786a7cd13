// loop_apply_cpu.cc -- CPU test of host/LoopApply.h (tests/test_loop_apply.py): on deep copies of one seeded synthetic map,
// (a) LoopClosing::SearchAndFuse restated sequentially and search_and_fuse_apply with the restated candidate search as its query must leave the
//     same final graph and per-keyframe nFused; (b) the same without the survivor re-query, reported as diverged or not;
// (c) SearchByProjection(pKF, Scw, ..) restated sequentially and search_by_projection_apply with n_best = 4 and with n_best = 1 (which forces
//     the exhaustion path) must give the same vpMatched and return value.
#include <cstdio>
#include <cstdlib>

#include "LoopApply.h"
#include "loop_restate.h"

using namespace loop_test;

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned) std::atoi(argv[1]) : 1u;
    const float th = 4.0f;
    World base = make_world(seed);
    World a = deep_copy(base), b = deep_copy(base), c = deep_copy(base);
    int bad0 = 0, inKf0 = 0, dups = 0;
    {
        const std::vector<MapPoint *> lp = loop_points(base);
        for (MapPoint *p : lp) bad0 += p->isBad();
        for (MapPoint *p : lp) inKf0 += p->IsInKeyFrame(&base.kfs[0]);
        dups = (int) lp.size() - (int) std::set<MapPoint *>(lp.begin(), lp.end()).size();
    }
    std::vector<int> nA;
    const LoopCount cnt = search_and_fuse_sequential(all_kfs(a), world_scw(a), loop_points(a), th, &nA);
    auto run = [th](World &w, bool requery) {
        const std::vector<KeyFrame *> kfs = all_kfs(w);
        const std::vector<cv::Mat> scw = world_scw(w);
        auto query = [&](const std::vector<int> &rows, const std::vector<MapPoint *> &p, const std::vector<uint8_t> &s, std::vector<int> &bi,
                         std::vector<int> &bd) { return cpu_fuse_query(kfs, scw, rows, p, s, bi, bd, th); };
        return ygzf_host::search_and_fuse_apply(kfs, loop_points(w), 50, query, requery);
    };
    const ygzf_host::SearchAndFuseResult rb = run(b, true), rc = run(c, false);
    int bad = compare(a, b, "search_and_fuse_apply");
    if (nA != rb.nFused) { std::printf("nFused differs\n"); bad++; }
    if (cnt.replaced != rb.replaced) { std::printf("Replace count differs\n"); bad++; }
    const int diverged = compare(a, c, "no-requery") + (nA != rc.nFused ? 1 : 0);

    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th = 10): every MapPoint of the map (the loop keyframe's neighbourhood), list order =
    // creation order with a stride so that the parts of one landmark are apart; vpMatched starts with every other MapPoint of the keyframe
    long matched = 0, conflicts = 0, requeries4 = 0, requeries1 = 0, preset = 0;
    for (int kf = 0; kf < 3; kf++) {
        World d = deep_copy(base), e = deep_copy(base), f = deep_copy(base);
        auto setup = [kf](World &w, std::vector<MapPoint *> &pts, std::vector<MapPoint *> &vm) {
            const size_t n = w.mps.size();
            for (size_t j = 0; j < n; j++) pts.push_back(&w.mps[(j * 7) % n]);
            vm.assign(w.kfs[kf].N, nullptr);
            for (int j = 0; j < w.kfs[kf].N; j += 2) vm[j] = w.kfs[kf].mvpMapPoints[j];
        };
        std::vector<MapPoint *> pd, pe, pf, vd, ve, vf;
        setup(d, pd, vd); setup(e, pe, ve); setup(f, pf, vf);
        for (MapPoint *p : vd) preset += p != nullptr;
        const cv::Mat scw = make_scw(base.kfs[kf], 1.13f);
        const int nD = search_by_projection_sequential(&d.kfs[kf], scw, pd, vd, 10);
        auto resolve = [&](World &w, std::vector<MapPoint *> &pts, std::vector<MapPoint *> &vm, int nBest) {
            KeyFrame *K = &w.kfs[kf];
            auto query = [&](size_t first, const std::vector<uint8_t> &skip, const std::vector<uint8_t> &mask, int nb, std::vector<int> &ci,
                             std::vector<int> &cd) { return cpu_projection_query(K, scw, pts, first, skip, mask, nb, ci, cd, 10.0f); };
            return ygzf_host::search_by_projection_apply(pts, vm, nBest, query);
        };
        const ygzf_host::ProjectionApplyResult r4 = resolve(e, pe, ve, 4), r1 = resolve(f, pf, vf, 1);
        bad += compare_matched(d, vd, e, ve, "vpMatched (n_best 4)") + compare_matched(d, vd, f, vf, "vpMatched (n_best 1)");
        if (!r4.ok || !r1.ok || r4.nmatches != nD || r1.nmatches != nD) { std::printf("nmatches differs: %d %d %d\n", nD, r4.nmatches, r1.nmatches); bad++; }
        bad += compare(d, e, "SearchByProjection writes no map");
        matched += nD; conflicts += r4.conflicts; requeries4 += r4.requeries; requeries1 += r1.requeries;
    }
    std::printf("seed %u fused %ld replaced %ld added %ld listed_in_slot %ld bad0 %d in_kf0 %d dups %d requeried %lld diverged %d matched %ld preset %ld "
                "conflicts %ld requeries4 %ld requeries1 %ld\n", seed, cnt.fused, cnt.replaced, (long) (cnt.fused - cnt.replaced), cnt.sameSlot, bad0, inKf0,
                dups, rb.requeried, diverged, matched, preset, conflicts, requeries4, requeries1);
    if (!rb.ok || bad) return 1;
    std::printf("loop apply ok\n");
    return 0;
}
