// extract_plan_cpu.hip -- the extractor's planning unit (csrc/ygzf_plan.hip) walked over a sweep of geometries and pins as a stand-alone
// host program: tests/test_extract_plan_cpu.py builds it with AddressSanitizer and UBSan, so every table build_geometry fills and every
// index it computes on the way is checked by the sanitizers, and the facts below by the program itself.  Prints "extract plan ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "extract_sweep.h"

using namespace ygzf;

static int g_failed = 0;
static std::string g_where;
#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            if (g_failed++ < 40) fprintf(stderr, "FAILED %s: %s (line %d)\n", g_where.c_str(), #cond, __LINE__); \
        }                                                                                              \
    } while (0)

// every index build_geometry stored lies inside the table it points into
static void check_geometry(const Geometry &G, int L) {
    CHECK((int) G.lv.size() == L);
    CHECK(G.xalpha.size() == 2 * G.xofs.size() && G.ybeta.size() == 2 * G.yofs.size());
    long long cells = 0, slots = 0, cands = 0, kps = 0, groups = 0;
    for (int l = 0; l < L; l++) {
        const LevelGeom &g = G.lv[l];
        CHECK(g.w >= 1 && g.h >= 1 && g.pitch >= g.w && g.pitch % 64 == 0);
        const int nc = g.nCols * g.nRows;
        CHECK(g.cellBase == cells && g.slotBase == slots && g.candBase == cands && g.kpBase == kps && g.groupBase == groups);
        cells += nc; slots += (long long) nc * g.slotCap; cands += g.candCap; kps += g.kpCap;
        groups += ((g.nCols + 1) / 2) * ((g.nRows + 1) / 2);
        CHECK(g.candCap == nc * g.slotCap);
        CHECK(((g.kpCap + 3) & ~3) <= G.kpCapMax && nc <= G.maxCellsPerLevel);
        if (nc) {
            CHECK(g.wCell <= G.fastWCellMax && g.wCell + 6 < G.fastWinPitch && g.hCell + 6 <= G.fastWinRows && g.hCell + 2 <= G.fastSmapRows);
            CHECK(g.keyBits <= 32 && g.kpCap <= 65535 && g.nIni >= 1);
        }
        if (l == 0) continue;
        const LevelGeom &s = G.lv[l - 1];
        CHECK(g.off >= 0 && g.off + (long long) g.pitch * g.h <= G.pyrBytes);
        CHECK(g.xtab >= 0 && (size_t) g.xtab + g.w <= G.xofs.size() && g.ytab >= 0 && (size_t) g.ytab + g.h <= G.yofs.size());
        for (int x = 0; x < g.w; x++) CHECK(G.xofs[g.xtab + x] >= 0 && G.xofs[g.xtab + x] < s.w);
        for (int y = 0; y < g.h; y++) CHECK(G.yofs[g.ytab + y] >= -1 && G.yofs[g.ytab + y] < s.h);
        CHECK(g.pyrCol >= 0 && (size_t) g.pyrCol + (g.w + 3) / 4 <= G.pyrCols.size());
        CHECK(g.pyrRow >= 0 && (size_t) g.pyrRow + g.h + 7 <= G.pyrRows.size());   // (a wave reads the records of its 8 rows in one go)
        CHECK(g.pyrTile >= 0 && g.nPyrTiles >= 0 && (size_t) g.pyrTile + g.nPyrTiles <= G.pyrTiles.size());
        for (int q = 0; q < (g.w + 3) / 4; q++) CHECK(G.pyrCols[g.pyrCol + q].sx0 >= 0 && G.pyrCols[g.pyrCol + q].sx0 < s.w);
        for (int y = 0; y < g.h + 7; y++) {
            const PyrRowRec &r = G.pyrRows[g.pyrRow + y];
            CHECK((int) (r.r01 & 0xffffu) < s.h || !g.tiledOk);
            CHECK((int) (r.r01 >> 16) < s.h || !g.tiledOk);
        }
        if (g.tiledOk) {
            long long covered = 0;
            for (int t = 0; t < g.nPyrTiles; t++) {
                const PyrTileRec &r = G.pyrTiles[g.pyrTile + t];
                CHECK(r.foldLog2 <= 3 && r.x0 < g.w && r.y0 < g.h && r.sxa < s.w && r.sxa % 4 == 0 && r.nc >= 1 && r.nc <= pyr_fold_chunks(r.foldLog2));
                const int tw = 256 >> r.foldLog2, th = kPyrTileRows << r.foldLog2;
                covered += (long long) (std::min(r.x0 + tw, g.w) - r.x0) * (std::min(r.y0 + th, g.h) - r.y0);
            }
            CHECK(covered == (long long) g.w * g.h);   // the tiles cut the level, no pixel twice
        }
    }
    CHECK(G.totalCells == cells && G.totalSlots == slots && G.candStride == cands && G.kpStride == kps && G.totalGroups == groups);
    // k_fast_tab's records
    CHECK(G.fastCells.size() == (size_t) G.totalGroups * 4);
    long long existing = 0;
    for (const FastCellRec &r : G.fastCells) {
        const unsigned fl = (r.flags >> 8) & 0xffu;
        if (!(fl & kFastCellExists)) continue;
        existing++;
        const int l = (int) (r.flags >> 16);
        CHECK(l < L);
        if (l >= L) continue;
        const LevelGeom &g = G.lv[l];
        CHECK((long long) r.cell >= g.cellBase && (long long) r.cell < g.cellBase + g.nCols * g.nRows);
        CHECK((long long) r.slot >= g.slotBase && (long long) r.slot + g.slotCap <= g.slotBase + (long long) g.nCols * g.nRows * g.slotCap);
        CHECK(r.off == (unsigned) g.off && (r.geo & 0xffffu) == (unsigned) (l ? g.pitch : 0));
        if (fl & kFastCellRun) {
            const int x0 = (int) (r.xy & 0xffffu), y0 = (int) (r.xy >> 16), dw = (int) ((r.geo >> 16) & 0xffu), dh = (int) (r.geo >> 24), wh = (int) (r.flags & 0xffu);
            CHECK(dw >= 1 && dh >= 1 && wh == dh + 6 && dw <= g.wCell && dh <= g.hCell);
            CHECK(x0 >= 0 && x0 + 1 + dw + 6 <= g.w && y0 >= 0 && y0 + wh <= g.h);   // the window lies inside the level image
        }
    }
    CHECK(existing == G.totalCells);
    // k_pyr_strips' plan
    if (!G.pyrPlan.empty()) {
        const int S = (int) G.pyrPlan.size(), base = G.pyrBase;
        CHECK(base >= 0 && L - base >= 3 && G.pyrStripLds <= 160 * 1024 && G.pyrStripOffA <= G.pyrStripOffB && (size_t) G.pyrStripOffB <= G.pyrStripLds);
        for (int l = base; l < L; l++) {
            int next = 0;
            for (int s = 0; s < S; s++) {
                const uint2 v = G.pyrPlan[s].lv[l];
                const int ca = (int) (v.x & 0xffffu), cb = (int) (v.x >> 16), wa = (int) (v.y & 0xffffu), wb = (int) (v.y >> 16);
                CHECK(ca >= 0 && ca <= cb && cb <= G.lv[l].h);
                if (l == base) { CHECK(wa == 0 && wb == 0); }
                else { CHECK(wa == next && wa <= wb && ca <= wa && wb <= cb); next = wb; }
                if (l < L - 1 && G.pyrPlan[s].lv[l + 1].x >> 16 > (G.pyrPlan[s].lv[l + 1].x & 0xffffu)) {   // the rows this strip produces of level l + 1 read rows it holds of level l
                    const LevelGeom &n = G.lv[l + 1];
                    const int pa = (int) (G.pyrPlan[s].lv[l + 1].x & 0xffffu), pb = (int) (G.pyrPlan[s].lv[l + 1].x >> 16);
                    const int hl = G.lv[l].h;
                    const int first = std::min(std::max(G.yofs[n.ytab + pa], 0), hl - 1), last = std::min(std::max(G.yofs[n.ytab + pb - 1] + 1, 0), hl - 1);
                    CHECK(ca <= first && last < cb);
                }
            }
            if (l > base) CHECK(next == G.lv[l].h);
        }
    }
}

static void check_oct_plan(const Geometry &G, int L, const PlanPins &pins, const OctPlan &plan) {
    int next = 0;
    CHECK(!plan.launches.empty());
    for (const OctLaunch &g : plan.launches) {
        CHECK(g.l0 == next && g.n >= 1);
        next += g.n;
        CHECK(g.lds <= 150 * 1024);
        CHECK(g.block == 256 || g.block == 512 || g.block == 1024);
        CHECK(g.cap >= 4 && g.cap % 4 == 0);
        for (int l = g.l0; l < g.l0 + g.n && l < L; l++) CHECK(g.cap >= G.lv[l].kpCap);
        CHECK(!g.arena || (plan.kind == OctPlan::SortOne && plan.launches.size() == 1));
        if (plan.kind == OctPlan::Hist) CHECK(g.histBins >= 4 && g.ldsCand == 0 && g.block == kOctBlock && g.regionInts >= kOctNodeArrays * g.cap && g.lds == oct_lds_bytes(kOctLdsHist, 0, g.cap, 0, g.regionInts, g.histBins));
        else CHECK(g.histBins == 0 && g.regionInts == 0 && (g.ldsCand % 4 == 0 || g.arena));   // (the overlay of the LDS node arrays wants multiples of 4)
        if (plan.kind == OctPlan::SortGroups) CHECK(g.lds >= oct_lds_bytes(kOctLdsSort, 0, g.cap, g.ldsCand, 0, 0));   // (the layout of a launch whose levels have no cells: the least)
    }
    CHECK(next == L);
    if (plan.kind == OctPlan::SortOne) CHECK(plan.launches.size() == 1 && plan.launches[0].block == kOctBlock && plan.launches[0].cap == G.kpCapMax);
    // The small plan: oct_plan=sort alone suppresses it.  Under every other pin it exists wherever ONE histogram-plan launch of all levels can
    // exist at all: not where the node arrays alone (19 ints per list position of the largest level) exceed the 150 KB a launch may take --
    // 320x240 / 2 levels / 5000 features (19 x 2732 x 4 = 207 KB), whose one launch left is the arena's.  The parent commit has no small plan there
    // either: tests/test_gpu_octree_plans.py's arena test sees no small-plan line, and profiles/r13_extract_plan_ab.txt's sweep has the parent's
    // and this library's plan lines equal for that geometry under every pin.
    const bool cannotFit = sizeof(int) * 19 * (size_t) std::max(G.kpCapMax, 4) > 150 * 1024;
    if (pins.octPlan == PlanPins::Sort || cannotFit) CHECK(!plan.haveSmall);
    else CHECK(plan.haveSmall);
    if (plan.haveSmall) {
        const OctLaunch &g = plan.small;
        CHECK(g.l0 == 0 && g.n == L && g.histBins >= 4 && g.lds <= 150 * 1024 && g.cap == std::max(G.kpCapMax, 4) && g.block == kOctBlock && !g.arena && g.ldsCand == 0);
        CHECK(g.lds == oct_lds_bytes(kOctLdsHist, 0, g.cap, 0, g.regionInts, g.histBins) && g.regionInts >= kOctNodeArrays * g.cap);
    }
}

static void check_fast(const Geometry &G0, const PlanPins &base) {
    for (int variant = 0; variant < 4; variant++) {
        Geometry G = G0;
        bool overflow = false;
        if (variant == 1) { G.pyrBytes = 1ll << 32; overflow = true; }
        if (variant == 2) { G.w = 65536; overflow = true; }
        if (variant == 3) { G.totalSlots = 1ll << 32; overflow = true; }
        const bool wide = G.fastWCellMax > kFastTabMaxCell;
        for (int setting : {YGZF_FAST_KERNEL_AUTO, YGZF_FAST_KERNEL_REGISTER_STAGING, YGZF_FAST_KERNEL_CELL_TABLE})
            for (int persist : {-1, 0, 1})
                for (int nFrames : {1, 2, 3, 16, 17, 64, 256, 1024})
                    for (size_t tabLds : {(size_t) 9 * 1024, (size_t) 24 * 1024, (size_t) 100 * 1024, (size_t) 200 * 1024}) {
                        PlanPins p = base;
                        p.fastPersist = persist;
                        const FastChoice c = choose_fast(G, setting, p, 256, nFrames, tabLds);
                        const long long launchGroups = (long long) nFrames * G.totalGroups;
                        if (c.kind == FastChoice::Persist) CHECK(launchGroups >= 64 && c.resident > 0 && persist != 0);
                        if (setting != YGZF_FAST_KERNEL_REGISTER_STAGING) CHECK((c.kind == FastChoice::Quads) == (wide || overflow));
                        else CHECK(c.kind == FastChoice::Quads);
                        if (persist == 1 && launchGroups >= 64 && !wide && !overflow && setting != YGZF_FAST_KERNEL_REGISTER_STAGING && tabLds <= 160 * 1024)
                            CHECK(c.kind == FastChoice::Persist);
                        if (persist == -1 && c.kind == FastChoice::Persist) CHECK(G.totalGroups >= 1000 && launchGroups >= 4ll * c.resident);
                    }
    }
}

int main() {
    const std::vector<Geo> sweep = geo_sweep();
    const std::vector<Pin> pins = pin_sets();
    int walked = 0, wideCells = 0;
    for (const Geo &q : sweep) {
        ygzf_extractor_cfg cfg{};
        cfg.nfeatures = q.nf; cfg.scale_factor = q.sf; cfg.nlevels = q.nl; cfg.ini_th_fast = 20; cfg.min_th_fast = 7;
        Tables T;
        T.init(cfg);
        for (const Pin &pin : pins) {
            char name[160];
            snprintf(name, sizeof name, "%dx%d/%d/%d sf %.2f pins %s", q.w, q.h, q.nl, q.nf, q.sf, pin.name);
            g_where = name;
            Geometry G;
            OctPlan plan;
            std::string err;
            int rc = build_geometry(T, pin.p, q.w, q.h, G, &err);
            CHECK(rc == YGZF_OK);
            if (rc) { fprintf(stderr, "%s: %s\n", name, err.c_str()); continue; }
            check_geometry(G, q.nl);
            rc = plan_octree(G, q.nl, pin.p, plan, &err);
            CHECK(rc == YGZF_OK);
            if (rc) { fprintf(stderr, "%s: %s\n", name, err.c_str()); continue; }
            check_oct_plan(G, q.nl, pin.p, plan);
            check_fast(G, pin.p);
            wideCells += G.fastWCellMax > kFastTabMaxCell;
            walked++;
            const bool dflt = std::string(pin.name) == "default";
            // facts pinned elsewhere (tests/test_octree_sort_plan.py, tests/test_gpu_octree_plans.py)
            if (q.w == 752 && q.h == 480 && q.nl == 8 && (dflt || std::string(pin.name) == "sort")) {
                CHECK(plan.kind == OctPlan::SortGroups && plan.launches.size() == 2);
                if (plan.launches.size() == 2) {
                    const OctLaunch &a = plan.launches[0], &b = plan.launches[1];
                    CHECK(a.l0 == 0 && a.n == 4 && a.block == 512 && a.lds == 44 * 1024 && a.ldsCand == 2816);
                    CHECK(b.l0 == 4 && b.n == 4 && b.block == 256 && b.lds == 36 * 1024 && b.ldsCand == 2304);
                }
            }
            if (q.w == 320 && q.nl == 2 && q.nf == 5000 && dflt) {
                CHECK(plan.kind == OctPlan::SortOne && plan.launches.size() == 1 && plan.launches[0].arena && plan.launches[0].cap == 2732 && !plan.haveSmall);
            }
            // oct_plan=hist: a histogram plan that fits is taken (the bench geometry, which would sort by itself), one that does not fit 150 KB
            // falls back to the sort plan (level 0's node arrays of 320x240 / 2 / 5000 alone are 207 KB: the arena's single launch, as unpinned)
            if (pin.p.octPlan == PlanPins::Hist && q.w == 752 && q.nl == 8) CHECK(plan.kind == OctPlan::Hist && plan.launches[0].histBins > 0);
            if (pin.p.octPlan == PlanPins::Hist && q.w == 320 && q.nl == 2)
                CHECK(plan.kind == OctPlan::SortOne && plan.launches.size() == 1 && plan.launches[0].arena && plan.launches[0].histBins == 0 && !plan.haveSmall);
            if ((q.w == 1920 || q.w == 3840) && dflt) CHECK(plan.kind == OctPlan::Hist && plan.launches.size() >= 2);
            if (std::string(pin.name) == "strip_base=1" && !G.pyrPlan.empty()) CHECK(G.pyrBase >= 1);
            if (std::string(pin.name) == "strips=64" && !G.pyrPlan.empty()) CHECK(G.pyrPlan.size() >= 64);
        }
    }
    g_where = "sweep";
    CHECK(walked == (int) (sweep.size() * pins.size()));
    CHECK(wideCells > 0);   // choose_fast's Quads rule was exercised by real geometries, not only by the overflow variants
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("extract plan ok: %d geometries x %d pin sets\n", (int) sweep.size(), (int) pins.size());
    return 0;
}
