// extract_sweep.h -- the geometries and pin sets that the stand-alone host programs of the extractor's plans walk (extract_plan_cpu.hip: the plans
// themselves; lds_layout_cpu.hip: the LDS layouts of the launches those plans hold).
#ifndef YGZF_TESTS_EXTRACT_SWEEP_H
#define YGZF_TESTS_EXTRACT_SWEEP_H
#include <cmath>
#include <vector>

#include "ygzf_plan.h"

struct Geo { int w, h, nl, nf; float sf; };
struct Pin { const char *name; ygzf::PlanPins p; };

static std::vector<Pin> pin_sets() {
    using ygzf::PlanPins;
    std::vector<Pin> v;
    auto add = [&](const char *name, auto f) { Pin q{name, PlanPins()};   /* (a default PlanPins is the library's own choice: no environment is read) */ f(q.p); v.push_back(q); };
    add("default", [](PlanPins &) {});
    // tests/test_gpu_octree_groups.py (every context there pins the sort plan)
    add("sort", [](PlanPins &p) { p.octPlan = PlanPins::Sort; });
    add("sort,groups=1", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octOneGroup = true; });
    add("sort,block=256", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 256; });
    add("sort,block=512", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 512; });
    add("sort,block=1024", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 1024; });
    add("sort,block=256,lds=8", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 256; p.octLdsBytes = 8 * 1024; });
    add("sort,block=512,lds=24", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 512; p.octLdsBytes = 24 * 1024; });
    add("sort,block=1024,lds=20", [](PlanPins &p) { p.octPlan = PlanPins::Sort; p.octBlock = 1024; p.octLdsBytes = 20 * 1024; });
    // tests/test_gpu_octree_plans.py
    add("hist", [](PlanPins &p) { p.octPlan = PlanPins::Hist; });
    add("hist,bins=8192", [](PlanPins &p) { p.octPlan = PlanPins::Hist; p.octHistBins = 8192; });
    add("hist,bins=512", [](PlanPins &p) { p.octPlan = PlanPins::Hist; p.octHistBins = 512; });
    add("hist,bins=16", [](PlanPins &p) { p.octPlan = PlanPins::Hist; p.octHistBins = 16; });
    add("hist,helpers=8,spin=0", [](PlanPins &p) { p.octPlan = PlanPins::Hist; p.octHelpers = 8; p.octHelperSpin = 0; });
    // the pins alone (no plan pinned with them)
    add("groups=1", [](PlanPins &p) { p.octOneGroup = true; });
    add("block=256", [](PlanPins &p) { p.octBlock = 256; });
    add("lds=8", [](PlanPins &p) { p.octLdsBytes = 8 * 1024; });
    add("bins=16", [](PlanPins &p) { p.octHistBins = 16; });
    add("bins=512", [](PlanPins &p) { p.octHistBins = 512; });
    // tests/test_gpu_extract.py: the pyramid's pins
    add("strip_frames=0", [](PlanPins &p) { p.pyrStripFrames = 0; });
    add("strips=32", [](PlanPins &p) { p.pyrStrips = 32; });
    add("strips=64", [](PlanPins &p) { p.pyrStrips = 64; });
    add("strip_base=1", [](PlanPins &p) { p.pyrStripBase = 1; });
    add("strip_base=2,strips=48", [](PlanPins &p) { p.pyrStripBase = 2; p.pyrStrips = 48; });
    return v;
}

static std::vector<Geo> geo_sweep() {
    std::vector<Geo> sweep = {{752, 480, 8, 1000, 1.2f}, {640, 480, 8, 1000, 1.2f}, {333, 517, 8, 1500, 1.2f}, {1280, 360, 6, 1200, 1.2f}, {1241, 376, 8, 500, 1.2f},
                              {320, 240, 4, 3000, 1.2f}, {320, 240, 2, 5000, 1.2f}, {200, 150, 3, 150, 1.2f}, {130, 110, 8, 200, 1.2f}, {1920, 1080, 8, 4000, 1.2f},
                              {3840, 2160, 12, 8000, 1.2f}, {752, 480, 12, 1000, 1.1f}, {640, 480, 4, 500, 2.0f}};
    // the level-1 widths of test_pyramid_tiles_of_every_fold (tests/test_gpu_extract.py), as that test turns them into images
    const int level1[] = {31, 32, 33, 64, 95, 128, 129, 160, 223, 224, 225, 255, 256, 257, 266, 288, 320, 383, 448, 479, 512, 522, 544, 767, 1000};
    for (float sf : {1.1f, 1.2f, 1.27f}) {
        int i = 0;
        for (int w1 : level1) {
            const int hs[4] = {64, 97, 130, 301};
            sweep.push_back({(int) std::nearbyint((double) w1 * (double) sf) + 1, hs[i++ % 4], 3, 200, sf});
        }
    }
    return sweep;
}

#endif
