// fuse_apply_cpu.cc -- CPU test of host/FuseApply.h (tests/test_fuse_apply.py): on deep copies of one seeded synthetic map, (a) the sequential
// Fuse loop of the reference and (b) fuse_apply with the restated candidate search as its query must leave the same final graph and the same
// per-target nFused.  Also runs (c) fuse_apply without the survivor re-query and reports whether it diverged.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "FuseApply.h"
#include "fuse_restate.h"

using namespace fuse_test;

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned) std::atoi(argv[1]) : 1u;
    const float th = 3.0f;
    World base = make_world(seed);
    World a = deep_copy(base), b = deep_copy(base), c = deep_copy(base);
    std::vector<int> nA;
    {
        const std::vector<MapPoint *> pts = a.point_ptrs();
        for (KeyFrame *k : a.target_ptrs()) nA.push_back(fuse_sequential(k, pts, th));
    }
    auto query = [th](const std::vector<KeyFrame *> &k, const std::vector<MapPoint *> &p, const std::vector<uint8_t> &s, std::vector<int> &bi,
                      std::vector<int> &bd) { return cpu_query(k, p, s, bi, bd, th); };
    const ygzf_host::FuseApplyResult rb = ygzf_host::fuse_apply(b.target_ptrs(), b.point_ptrs(), 50, query);
    const ygzf_host::FuseApplyResult rc = ygzf_host::fuse_apply(c.target_ptrs(), c.point_ptrs(), 50, query, false);
    // what the map exercised
    int bad0 = 0, stereo = 0, mono = 0;
    for (const MapPoint &m : base.mps) bad0 += m.mbBad;
    for (const KeyFrame &k : base.kfs) for (float u : k.mvuRight) (u >= 0 ? stereo : mono)++;
    long fusedA = 0;
    for (int n : nA) fusedA += n;
    int bad = compare(a, b, "fuse_apply");
    if (nA != rb.nFused) { std::printf("nFused differs\n"); bad++; }
    const int diverged = compare(a, c, "no-requery") + (nA != rc.nFused ? 1 : 0);
    const BranchCount &B = g_branches;
    std::printf("seed %u fused %ld into_kf %d into_mp %d equal_obs %d bad_in_kf %d added %d bad0 %d stereo %d mono %d requeried %lld diverged %d\n",
                seed, fusedA, B.intoKf, B.intoMp, B.equalObs, B.badInKf, B.added, bad0, stereo, mono, rb.requeried, diverged);
    if (!rb.ok || bad) return 1;
    std::printf("fuse apply ok\n");
    return 0;
}
