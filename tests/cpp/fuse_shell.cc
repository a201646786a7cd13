// fuse_shell.cc -- GPU test of the Fuse shell (tests/test_gpu_fuse.py): on deep copies of one seeded synthetic map, ygz::FuseBatch and a loop of
// ORBmatcher::Fuse, both over the device, must leave the final graph of the sequential restatement (tests/cpp/fuse_restate.h).
// `fuse_shell time <kfs> <landmarks> <points> <duplicate targets> <reps>` (tools/fuse_rate.py): medians of the sequential CPU loop and of
// ygz::FuseBatch end to end (packing, every device call including the re-search of Replace survivors, the host application), each on a fresh copy.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ORBmatcher.h"
#include "ORBmatcherFuse.h"
#include "fuse_restate.h"
#include "ygzf_pool.h"

using namespace fuse_test;

namespace ygz {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;   // (ORBmatcher.cc reads them)
}

static int time_mode(int nKf, int nLand, int nPoints, int nDup, int reps) {
    const World base = timing_world(nKf, nLand, nPoints, nDup);
    std::vector<double> cpu, dev;
    long nCpu = 0, nDev = 0;
    int differ = 0;
    (void) ygz::FuseBatch({}, {}, 3.0f);   // (first lease: context creation outside the timed region)
    {
        World w = deep_copy(base);
        nDev = ygz::FuseBatch(w.target_ptrs(), w.point_ptrs(), 3.0f);
    }
    for (int r = 0; r < reps; r++) {
        World a = deep_copy(base), b = deep_copy(base);
        const std::vector<MapPoint *> pa = a.point_ptrs(), pb = b.point_ptrs();
        const std::vector<KeyFrame *> ta = a.target_ptrs(), tb = b.target_ptrs();
        auto t0 = std::chrono::steady_clock::now();
        nCpu = 0;
        for (KeyFrame *k : ta) nCpu += fuse_sequential(k, pa, 3.0f);
        cpu.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        t0 = std::chrono::steady_clock::now();
        nDev = ygz::FuseBatch(tb, pb, 3.0f);
        dev.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        differ += compare(a, b, "FuseBatch") + (nCpu != nDev);
    }
    std::sort(cpu.begin(), cpu.end());
    std::sort(dev.begin(), dev.end());
    long keys = 0;
    for (int k : base.targets) keys += base.kfs[k].N;
    std::printf("{\"targets\": %zu, \"points\": %zu, \"keys_per_kf\": %ld, \"fused\": %ld, \"cpu_ms\": %.3f, \"fusebatch_ms\": %.3f, "
                "\"same_graph\": %s}\n", base.targets.size(), base.points.size(), keys / (long) base.targets.size(), nCpu, cpu[cpu.size() / 2],
                dev[dev.size() / 2], differ ? "false" : "true");
    return differ ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "time" && argc == 7)
        return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
    const unsigned seed = argc > 1 ? (unsigned) std::atoi(argv[1]) : 1u;
    const float th = 3.0f;
    World base = make_world(seed);
    World a = deep_copy(base), b = deep_copy(base), c = deep_copy(base);
    long nA = 0, nC = 0;
    {
        const std::vector<MapPoint *> pts = a.point_ptrs();
        for (KeyFrame *k : a.target_ptrs()) nA += fuse_sequential(k, pts, th);
    }
    const unsigned long failures0 = ygzf_host::failure_count();
    const long nB = ygz::FuseBatch(b.target_ptrs(), b.point_ptrs(), th);
    {
        ygz::ORBmatcher matcher;
        const std::vector<MapPoint *> pts = c.point_ptrs();
        for (KeyFrame *k : c.target_ptrs()) nC += matcher.Fuse(k, pts, th);
    }
    int bad = compare(a, b, "FuseBatch") + compare(a, c, "ORBmatcher::Fuse");
    if (ygzf_host::failure_count() != failures0) { std::printf("device failure: %s\n", ygzf_host::last_failure().c_str()); bad++; }
    std::printf("seed %u fused %ld %ld %ld\n", seed, nA, nB, nC);
    if (nA != nB || nA != nC || nA == 0) bad++;
    if (bad) return 1;
    std::printf("fuse shell ok\n");
    return 0;
}
