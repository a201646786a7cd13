// kf_store_shell.cc -- GPU test of ygz::KeyFrameDeviceStore behind the Fuse shells (tests/test_gpu_kf_store_shell.py): on deep copies of one
// seeded synthetic map, ygz::FuseBatch and ygz::SearchAndFuseBatch with the store switched on must leave the final graph of the sequential
// restatements (tests/cpp/fuse_restate.h, loop_restate.h) and of the store-off runs, and the store must put each distinct keyframe once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

#include "KeyFrameStore.h"
#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "ORBmatcherFuse.h"
#include "ORBmatcherLoop.h"
#include "loop_restate.h"
#include "ygzf_pool.h"

using namespace loop_test;
typedef ygz::KeyFrameDeviceStore Store;

namespace ygz {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;   // (ORBmatcher.cc reads them)
}

static int bad = 0;
#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); bad++; } \
    } while (0)

static std::vector<std::pair<KeyFrame *, cv::Mat>> pose_list(World &w) {
    std::vector<std::pair<KeyFrame *, cv::Mat>> v;
    const std::vector<cv::Mat> scw = world_scw(w);
    for (size_t k = 0; k < w.kfs.size(); k++) v.push_back({&w.kfs[k], scw[k]});
    return v;
}

// `kf_store_shell time fuse|loop <kfs> <landmarks> <points> <duplicate targets> <min repeats> <min seconds>` (tools/kf_store_rate.py): ygz::FuseBatch /
// ygz::SearchAndFuseBatch end to end with the store off and on, on ONE world whose mutable state is restored before every repeat -- the
// keyframes keep their addresses, as a running system's do, so the store-on repeats after the first find every keyframe resident.
static void restore(World &w, const World &base) {
    for (size_t i = 0; i < w.kfs.size(); i++) {
        w.kfs[i] = base.kfs[i];
        for (MapPoint *&p : w.kfs[i].mvpMapPoints) p = p ? &w.mps[mp_index(base, p)] : nullptr;
    }
    for (size_t i = 0; i < w.mps.size(); i++) {
        MapPoint &m = w.mps[i];
        m = base.mps[i];
        m.mDescriptor = m.mDescriptor.clone();
        std::map<KeyFrame *, size_t> obs;
        for (auto &o : m.mObservations) obs[&w.kfs[kf_index(base, o.first)]] = o.second;
        m.mObservations = obs;
        m.mpReplaced = m.mpReplaced ? &w.mps[mp_index(base, m.mpReplaced)] : nullptr;
    }
}

static int time_mode(bool loop, int nKf, int nLand, int nPoints, int nDup, int minReps, double minSeconds) {
    const World base = timing_world(nKf, nLand, nPoints, loop ? 0 : nDup);
    World w = deep_copy(base), ref = deep_copy(base);
    Store &S = Store::instance(ygz::ORBextractor::sDevice);
    const float th = loop ? 4.0f : 3.0f;
    auto run = [&](World &x) { return loop ? (long) ygz::SearchAndFuseBatch(pose_list(x), loop_points(x), th) : (long) ygz::FuseBatch(x.target_ptrs(), x.point_ptrs(), th); };
    double t[2][3];
    long fused[2] = {0, 0};
    int differ = 0;
    Store::Statistics per[2];
    Store::sResident = false;
    const long nRef = run(ref);
    for (int on = 0; on < 2; on++) {
        Store::sResident = on != 0;
        restore(w, base);
        fused[on] = run(w);                          // the untimed repeat (store on: the puts)
        differ += compare(ref, w, on ? "store on" : "store off") + (fused[on] != nRef);
        std::vector<double> ms;
        double total = 0;
        Store::Statistics s0 = S.Stats();
        while ((int) ms.size() < minReps || total < minSeconds * 1000.0) {
            restore(w, base);
            const auto t0 = std::chrono::steady_clock::now();
            run(w);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            total += ms.back();
        }
        differ += compare(ref, w, on ? "store on, last repeat" : "store off, last repeat");
        Store::Statistics s1 = S.Stats();
        per[on].queries = (s1.queries - s0.queries) / ms.size();
        per[on].puts = s1.puts - s0.puts;
        per[on].hits = (s1.hits - s0.hits) / ms.size();
        std::sort(ms.begin(), ms.end());
        t[on][0] = ms[ms.size() / 2]; t[on][1] = ms.front(); t[on][2] = ms.back();
    }
    Store::sResident = false;
    const Store::Statistics all = S.Stats();
    std::printf("{\"what\": \"%s\", \"keyframes\": %d, \"points\": %zu, \"fused\": %ld, \"off_ms\": [%.3f, %.3f, %.3f], \"on_ms\": [%.3f, %.3f, %.3f], "
                "\"queries_per_call\": %lu, \"hits_per_call\": %lu, \"puts_in_timed_repeats\": %lu, \"puts_first_call\": %lu, \"bytes_first_call\": %llu, "
                "\"same\": %s}\n", loop ? "SearchAndFuseBatch" : "FuseBatch", nKf, loop ? loop_points(w).size() : w.points.size(), nRef, t[0][0], t[0][1], t[0][2],
                t[1][0], t[1][1], t[1][2], per[1].queries, per[1].hits, per[1].puts, all.puts, all.bytesUploaded, differ ? "false" : "true");
    S.Release();
    return differ ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 9 && std::string(argv[1]) == "time")
        return time_mode(std::string(argv[2]) == "loop", std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]),
                         std::atof(argv[8]));
    const unsigned seed = argc > 1 ? (unsigned) std::atoi(argv[1]) : 1u;
    const float th = 3.0f;
    World base = make_world(seed);
    Store &S = Store::instance(ygz::ORBextractor::sDevice);
    const unsigned long failures0 = ygzf_host::failure_count();
    const size_t distinct = std::set<int>(base.targets.begin(), base.targets.end()).size();

    // ---- FuseBatch: sequential restatement / store off / store on ----
    World a = deep_copy(base), b = deep_copy(base), c = deep_copy(base);
    long nA = 0;
    {
        const std::vector<MapPoint *> pts = a.point_ptrs();
        for (KeyFrame *k : a.target_ptrs()) nA += fuse_sequential(k, pts, th);
    }
    Store::sResident = false;
    const long nB = ygz::FuseBatch(b.target_ptrs(), b.point_ptrs(), th);
    CHECK(S.Stats().puts == 0 && S.Stats().queries == 0, "the store is untouched while it is off");
    Store::sResident = true;
    const long nC = ygz::FuseBatch(c.target_ptrs(), c.point_ptrs(), th);
    bad += compare(a, b, "FuseBatch, store off") + compare(a, c, "FuseBatch, store on") + compare(b, c, "store on against store off");
    CHECK(nA == nB && nA == nC && nA > 0, "fused %ld %ld %ld", nA, nB, nC);
    Store::Statistics st = S.Stats();
    CHECK(st.puts == distinct, "puts %lu, distinct targets %zu", st.puts, distinct);
    CHECK(st.queries >= 1 && st.bytesUploaded > 0, "queries %lu bytes %llu", st.queries, st.bytesUploaded);

    // ---- two successive calls over overlapping targets: each distinct keyframe is put once, the overlap hits ----
    S.Clear();
    World d = deep_copy(base), e = deep_copy(base);
    std::vector<int> first(base.targets.begin(), base.targets.begin() + (base.targets.size() * 2) / 3), second(base.targets.begin() + base.targets.size() / 3, base.targets.end());
    auto ptrs = [](World &w, const std::vector<int> &idx) { std::vector<KeyFrame *> v; for (int t : idx) v.push_back(&w.kfs[t]); return v; };
    long nD = 0;
    {
        const std::vector<MapPoint *> pts = d.point_ptrs();
        for (KeyFrame *k : ptrs(d, first)) nD += fuse_sequential(k, pts, th);
        for (KeyFrame *k : ptrs(d, second)) nD += fuse_sequential(k, pts, th);
    }
    const Store::Statistics s0 = S.Stats();
    long nE = ygz::FuseBatch(ptrs(e, first), e.point_ptrs(), th);
    const Store::Statistics s1 = S.Stats();
    nE += ygz::FuseBatch(ptrs(e, second), e.point_ptrs(), th);
    const Store::Statistics s2 = S.Stats();
    bad += compare(d, e, "two FuseBatch calls, store on");
    CHECK(nD == nE, "fused %ld %ld", nD, nE);
    const std::set<int> f1(first.begin(), first.end()), f2(second.begin(), second.end());
    std::set<int> both(f1), overlap;
    both.insert(f2.begin(), f2.end());
    for (int t : f2) if (f1.count(t)) overlap.insert(t);
    CHECK(s1.puts - s0.puts == f1.size(), "first call put %lu of %zu", s1.puts - s0.puts, f1.size());
    CHECK(s2.puts - s0.puts == both.size(), "both calls put %lu, distinct %zu", s2.puts - s0.puts, both.size());
    CHECK(!overlap.empty() && s2.hits - s1.hits >= overlap.size(), "second call: %lu hits, overlap %zu", s2.hits - s1.hits, overlap.size());

    // ---- another keyframe at the same address (another mnId) is put again; Erase, then Fuse, puts again ----
    {
        ygz::ORBmatcher matcher;
        KeyFrame *k = &e.kfs[first[0]];
        const std::vector<MapPoint *> pts = e.point_ptrs();
        Store::Statistics p0 = S.Stats();
        matcher.Fuse(k, pts, th);
        Store::Statistics p1 = S.Stats();
        CHECK(p1.puts == p0.puts && p1.hits > p0.hits, "a resident keyframe is a hit");
        k->mnId += 1000;
        matcher.Fuse(k, pts, th);
        Store::Statistics p2 = S.Stats();
        CHECK(p2.puts == p1.puts + 1, "a new mnId at the address: puts %lu -> %lu", p1.puts, p2.puts);
        S.Erase(k);
        matcher.Fuse(k, pts, th);
        Store::Statistics p3 = S.Stats();
        CHECK(p3.puts == p2.puts + 1, "after Erase: puts %lu -> %lu", p2.puts, p3.puts);
        CHECK(S.Put(k) && S.Stats().puts == p3.puts && S.Stats().hits == p3.hits + 1, "Put of a resident keyframe is a hit");
    }

    // ---- SearchAndFuseBatch against loop_restate.h: sequential / store off / store on ----
    S.Clear();
    const float thL = 4.0f;
    World f = deep_copy(base), g = deep_copy(base), h = deep_copy(base);
    const LoopCount cnt = search_and_fuse_sequential(all_kfs(f), world_scw(f), loop_points(f), thL);
    Store::sResident = false;
    const Store::Statistics l0 = S.Stats();
    const long nG = ygz::SearchAndFuseBatch(pose_list(g), loop_points(g), thL);
    CHECK(S.Stats().puts == l0.puts && S.Stats().queries == l0.queries, "the store is untouched while it is off");
    Store::sResident = true;
    const long nH = ygz::SearchAndFuseBatch(pose_list(h), loop_points(h), thL);
    const Store::Statistics l1 = S.Stats();
    bad += compare(f, g, "SearchAndFuseBatch, store off") + compare(f, h, "SearchAndFuseBatch, store on");
    CHECK(cnt.fused == nG && cnt.fused == nH && cnt.fused > 0 && cnt.replaced > 0, "fused %ld %ld %ld replaced %ld", cnt.fused, nG, nH, cnt.replaced);
    CHECK(l1.puts - l0.puts == h.kfs.size(), "SearchAndFuseBatch put %lu of %zu keyframes", l1.puts - l0.puts, h.kfs.size());
    Store::sResident = false;
    S.Release();
    if (ygzf_host::failure_count() != failures0) { std::printf("device failure: %s\n", ygzf_host::last_failure().c_str()); bad++; }
    std::printf("seed %u fused %ld loop fused %ld puts %lu hits %lu queries %lu\n", seed, nA, cnt.fused, l1.puts, l1.hits, l1.queries);
    if (bad) return 1;
    std::printf("kf store shell ok\n");
    return 0;
}
