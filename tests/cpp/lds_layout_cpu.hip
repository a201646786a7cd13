// lds_layout_cpu.hip -- walks every dynamic-LDS layout of csrc/lds_layout.h over a sweep as a stand-alone host program.  For every point: each
// array starts at a multiple of min(16, its element's alignment), arrays that are live together do not overlap, every declared overlay lies
// over arrays that are idle in its phase, and every array ends inside the byte count the host launches with.  Prints the byte counts as one
// JSON object; tests/test_lds_layout.py compares them with tests/golden/lds_layout_parent.json (recorded from the functions this header
// replaced).  Arguments: the static LDS of the compiled k_sia_run (the aligner's ceiling follows from it).
//   lds_layout_cpu oct_sort <nCells> <cap> <ldsCand>   prints the sort plan's bytes for one launch instead (tests/test_octree_sort_plan.py)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <tuple>
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

// one array of a layout: bytes [off, off + bytes) of `space` (0: LDS; 1: the matcher's global spill arena)
struct Arr {
    std::string name;
    long long off, bytes;
    int align, space;
    long long end() const { return off + bytes; }
};
static const Arr *find(const std::vector<Arr> &v, const char *name) {
    for (const Arr &a : v) if (a.name == name) return &a;
    return nullptr;
}
static bool overlap(const Arr &a, const Arr &b) { return a.space == b.space && a.bytes > 0 && b.bytes > 0 && a.off < b.end() && b.off < a.end(); }
// `exempt`: the one array that may miss its alignment (nullptr: none)
static void check_aligned_inside(const std::vector<Arr> &v, long long total0, long long total1, const char *exempt) {
    for (const Arr &a : v) {
        if (!(exempt && a.name == exempt)) CHECK(a.off % std::min(16, a.align) == 0);
        CHECK(a.off >= 0 && a.end() <= (a.space ? total1 : total0));
    }
}
static void check_disjoint(const std::vector<Arr> &v, std::initializer_list<const char *> live) {   // a phase: these are live together
    std::vector<const Arr *> s;
    for (const char *n : live) if (const Arr *a = find(v, n)) s.push_back(a);
    for (size_t i = 0; i < s.size(); i++)
        for (size_t j = i + 1; j < s.size(); j++) CHECK(!overlap(*s[i], *s[j]));
}
static void check_all_disjoint(const std::vector<Arr> &v) {
    for (size_t i = 0; i < v.size(); i++)
        for (size_t j = i + 1; j < v.size(); j++) CHECK(!overlap(v[i], v[j]));
}
static bool within(const Arr &in, const Arr &out) { return in.space == out.space && in.off >= out.off && in.end() <= out.end(); }

// ---- matcher: the list as the kernel's carve-up walks it ----
static std::vector<Arr> match_arrays(int capCur, int capLast, bool descInLds, int spill, bool specDeep, size_t *ldsEnd, size_t *spillEnd) {
    std::vector<Arr> v;
    size_t p = 0, gp = 0;
#define REC(member, type, count, bit)                                                                            \
    {                                                                                                            \
        size_t &cur = (spill & (bit)) ? gp : p;                                                                  \
        v.push_back(Arr{#member, (long long) cur, (long long) ((size_t) sizeof(type) * (count)), (int) alignof(type), (spill & (bit)) ? 1 : 0}); \
        cur += al16((size_t) sizeof(type) * (count));                                                            \
    }
#define REC_IF(cond) if (cond) {
#define REC_END }
    YGZF_MATCH_LDS_ARRAYS(REC, REC_IF, REC_END, capCur, capLast)
#undef REC_END
#undef REC_IF
#undef REC
    *ldsEnd = p;
    *spillEnd = gp;
    return v;
}

static void walk_matcher() {
    printf("\"matcher\": [");
    const int caps[] = {0, 1, 15, 16, 17, 1000, 1008, 2000, 4000, 8000, 65535};
    std::vector<std::pair<int, int>> pairs;
    for (int c : caps) pairs.push_back({c, c});
    pairs.push_back({1000, 8000});
    pairs.push_back({8000, 1000});
    bool first = true;
    for (auto pr : pairs)
        for (int deep = 0; deep < 2; deep++)
            for (const MatchLdsPlan &pl : kMatchLdsPlans) {
                char name[96];
                snprintf(name, sizeof name, "matcher %d/%d deep %d desc %d spill %d", pr.first, pr.second, deep, pl.desc, pl.spill);
                g_where = name;
                const MatchLdsBytes m = match_lds_bytes(pr.first, pr.second, pl.desc != 0, pl.spill, deep != 0);
                size_t ldsEnd = 0, spillEnd = 0;
                const std::vector<Arr> v = match_arrays(pr.first, pr.second, pl.desc != 0, pl.spill, deep != 0, &ldsEnd, &spillEnd);
                CHECK(v.size() == (size_t) (19 + (deep ? 2 : 0) + (pl.desc ? 1 : 0)));
                CHECK(ldsEnd + 64 == m.lds && spillEnd == m.spill);
                check_aligned_inside(v, (long long) m.lds, (long long) m.spill, nullptr);
                check_all_disjoint(v);   // no overlays: every array is live for the whole kernel
                for (const Arr &a : v) {   // which arrays a spill bit moves out of LDS
                    static const std::set<std::string> misc = {"events", "qang", "cang", "match", "claim", "extOf", "extKey", "extI2", "extWork"};
                    const int bit = a.name.rfind("spec", 0) == 0 ? kSpillSpec : misc.count(a.name) ? kSpillMisc : 0;
                    CHECK(a.space == ((pl.spill & bit) ? 1 : 0));
                }
                printf("%s[%d, %d, %d, %d, %d, %zu, %zu]", first ? "" : ", ", pr.first, pr.second, deep, pl.desc, pl.spill, m.lds, m.spill);
                first = false;
            }
    // where plan_match_lds changes plans at capCur == capLast: the last count plan k admits (the GPU test runs it and the next one)
    printf("],\n\"matcher_switch\": [");
    first = true;
    for (int deep = 0; deep < 2; deep++)
        for (int k = 0; k < 3; k++) {
            int c = 0;
            while (c < 65535 && match_lds_bytes(c + 1, c + 1, kMatchLdsPlans[k].desc != 0, kMatchLdsPlans[k].spill, deep != 0).lds <= kMatchLdsBudget) c++;
            printf("%s[%d, %d, %d]", first ? "" : ", ", deep, k, c);
            first = false;
        }
    printf("],\n");
}

// ---- octree and FAST: the launches of every geometry x pin set ----
static void check_oct_level(const OctLaunch &g, OctLdsPlan plan, const LevelGeom &lg) {
    const int nCells = lg.nCols * lg.nRows, cap = g.cap;
    const OctLds Y = oct_lds(plan, nCells, cap, g.ldsCand, g.regionInts, g.histBins);
    const OctLds F = oct_lds_front(plan, nCells, cap, g.regionInts, g.histBins);   // what the kernel's carve-up reads
    CHECK(F.cellPref == Y.cellPref && F.nodes == Y.nodes && F.PS == Y.PS && F.xTab == Y.xTab && F.xTabRoom == Y.xTabRoom);
    std::vector<Arr> v;
    auto add = [&](const char *name, int off, long long ints) { if (off >= 0) v.push_back(Arr{name, 4ll * off, 4 * ints, 4, 0}); };
    add("cellPref", Y.cellPref, nCells + 1);
    add("nodes", Y.nodes, (long long) kOctNodeArrays * cap);
    add("cand", Y.cand, Y.candInts);
    add("candB", Y.candB, 2ll * g.ldsCand);
    add("PS", Y.PS, g.histBins + 1);
    // the key tables, where the kernel uses them (k_octree: lenX + lenY + nCells ints, if they fit their room)
    const int lenX = std::max(lg.regW, lg.nCols * lg.wCell) + 9, lenY = std::max(lg.regH, lg.nRows * lg.hCell) + 9;
    const bool useTab = Y.xTab >= 0 && lenX + lenY + nCells <= Y.xTabRoom && lg.depth <= 15;
    if (useTab) add("xTab", Y.xTab, lenX + lenY + nCells);
    check_aligned_inside(v, (long long) g.lds, 0, nullptr);
    CHECK(sizeof(int) * (size_t) Y.ints <= g.lds);
    // the node arrays and the candidate buffers are read in 16-byte pieces where their counts allow it
    if (Y.nodes >= 0) CHECK(Y.nodes % 4 == 0 && cap % 4 == 0);
    if (Y.cand >= 0 && g.ldsCand % 4 == 0) CHECK(Y.cand % 4 == 0);
    const Arr *nodes = find(v, "nodes"), *xTab = find(v, "xTab"), *candB = find(v, "candB"), *cellPref = find(v, "cellPref");
    if (plan == kOctLdsSort) {
        check_disjoint(v, {"cellPref", "nodes", "cand"});   // outside the sort
        check_disjoint(v, {"candB", "cand"});               // the sort: both pairs of buffers live
        check_disjoint(v, {"cellPref", "xTab", "cand"});    // the path keys
        // overlays: candB over the cell table and the node arrays (both idle while the candidates are sorted), the key tables in the node arrays (idle until the tree passes)
        CHECK(candB && candB->off == 0 && candB->end() <= find(v, "cand")->off);
        if (xTab) CHECK(within(*xTab, *nodes));
    } else if (plan == kOctLdsArena) {
        check_disjoint(v, {"cellPref", "cand"});
        CHECK(!nodes && !xTab && !candB);
    } else {
        check_disjoint(v, {"cellPref", "xTab", "PS"});      // the path keys and the histogram
        check_disjoint(v, {"nodes", "PS"});                 // the tree passes
        // overlays: the node arrays over the cell table and the key tables (dead once the keys exist); all three inside the region, PS behind it
        const Arr region{"region", 0, 4ll * g.regionInts, 4, 0};
        CHECK(within(*nodes, region) && within(*cellPref, region) && (!xTab || within(*xTab, region)) && find(v, "PS")->off == region.end());
        CHECK(!candB && Y.cand < 0);
    }
}

static void walk_extractor() {
    const std::vector<Geo> sweep = geo_sweep();
    const std::vector<Pin> pins = pin_sets();
    std::set<std::tuple<int, int, long long, int>> candSet;
    std::string fastJson;
    printf("\"octree\": {");
    bool firstGeo = true;
    for (const Geo &q : sweep) {
        ygzf_extractor_cfg cfg{};
        cfg.nfeatures = q.nf; cfg.scale_factor = q.sf; cfg.nlevels = q.nl; cfg.ini_th_fast = 20; cfg.min_th_fast = 7;
        Tables T;
        T.init(cfg);
        char geoName[64];
        snprintf(geoName, sizeof geoName, "%dx%d/%d/%d/%.2f", q.w, q.h, q.nl, q.nf, q.sf);
        std::set<std::vector<long long>> rows;   // [0 sort / 1 arena / 2 hist, l0, n, largest cell count, cap, ldsCand, regionInts, histBins, bytes], each once
        Geometry G0;
        for (const Pin &pin : pins) {
            g_where = std::string(geoName) + " pins " + pin.name;
            Geometry G;
            OctPlan plan;
            std::string err;
            int rc = build_geometry(T, pin.p, q.w, q.h, G, &err);
            if (!rc) rc = plan_octree(G, q.nl, pin.p, plan, &err);
            CHECK(rc == YGZF_OK);
            if (rc) continue;
            G0 = G;
            std::vector<OctLaunch> all = plan.launches;
            if (plan.haveSmall) all.push_back(plan.small);
            for (const OctLaunch &g : all) {
                const OctLdsPlan kind = g.histBins > 0 ? kOctLdsHist : g.arena ? kOctLdsArena : kOctLdsSort;
                int cells = 0;
                for (int l = g.l0; l < g.l0 + g.n; l++) {
                    cells = std::max(cells, G.lv[l].nCols * G.lv[l].nRows);
                    check_oct_level(g, kind, G.lv[l]);   // carved with the level's own cell count, against the launch's bytes
                }
                const size_t b = oct_lds_bytes(kind, cells, g.cap, g.ldsCand, g.regionInts, g.histBins);
                CHECK(b == g.lds);
                rows.insert({kind == kOctLdsHist ? 2 : kind == kOctLdsArena ? 1 : 0, g.l0, g.n, cells, g.cap, g.ldsCand, g.regionInts, g.histBins, (long long) b});
                if (kind == kOctLdsSort)
                    for (long long budget : {36 * 1024ll, 44 * 1024ll, 71 * 1024ll, 8 * 1024ll, 20 * 1024ll, 24 * 1024ll}) {
                        const int c = octree_lds_cand(cells, g.cap, (size_t) budget);
                        // the inverse of the layout: what it returns fits the budget, unless not even the floor of 256 candidates does
                        if (c > 0) CHECK(oct_lds_bytes(kOctLdsSort, cells, g.cap, c, 0, 0) <= (size_t) budget);
                        candSet.insert({cells, g.cap, budget, c});
                    }
            }
        }
        printf("%s\n \"%s\": [", firstGeo ? "" : ",", geoName);
        bool first = true;
        for (const auto &r : rows) {
            printf("%s[", first ? "" : ", ");
            for (size_t i = 0; i < r.size(); i++) printf("%s%lld", i ? ", " : "", r[i]);
            printf("]");
            first = false;
        }
        printf("]");
        // FAST: k_fast_quads at the geometry's pitch, the table forms at kTabPitch with 1, 2 and 4 waves
        g_where = std::string(geoName) + " fast";
        long long bytes[4];
        int k = 0;
        for (const auto &form : {std::make_pair(G0.fastWinPitch, kFastBlock / 64), std::make_pair(kTabPitch, 1), std::make_pair(kTabPitch, 2), std::make_pair(kTabPitch, 4)}) {
            const FastWaveLds W = fast_wave_lds(form.first, G0.fastWinRows, G0.fastSmapRows, G0.fastQuadCap);
            const size_t total = fast_lds_bytes(W, form.second);
            std::vector<Arr> v;
            for (int wv = 0; wv < form.second; wv++) {
                const long long base = (long long) wv * W.perWave;
                const std::string w = std::to_string(wv);
                v.push_back(Arr{"win" + w, base, (long long) G0.fastWinRows * form.first + 16, 16, 0});   // (16: LDS-DMA pieces and 32-bit quad reads)
                v.push_back(Arr{"smap" + w, base + W.winBytes, (long long) G0.fastSmapRows * form.first, 16, 0});
                v.push_back(Arr{"clist" + w, base + W.winBytes + W.smapBytes, kCornerCap * 2, 2, 0});
                // overlay: the quad list lies over the score map (the list lives between pass 1 and the expansion, the map only after it)
                const Arr quads{"quads" + w, base + W.winBytes, 4ll * G0.fastQuadCap, 4, 0};
                CHECK(quads.off == v[v.size() - 2].off && quads.end() <= v.back().off && !overlap(quads, v[v.size() - 3]));
                CHECK(quads.end() <= (long long) total);
            }
            check_aligned_inside(v, (long long) total, 0, nullptr);
            check_all_disjoint(v);
            CHECK(W.perWave % 16 == 0);
            bytes[k++] = (long long) total;
        }
        char buf[256];
        snprintf(buf, sizeof buf, "%s\n \"%s\": [%d, %d, %d, %d, %lld, %lld, %lld, %lld]", firstGeo ? "" : ",", geoName, G0.fastWinPitch, G0.fastWinRows, G0.fastSmapRows,
                 G0.fastQuadCap, bytes[0], bytes[1], bytes[2], bytes[3]);
        fastJson += buf;
        firstGeo = false;
    }
    printf("},\n\"octree_cand\": [");
    bool first = true;
    for (const auto &t : candSet) {
        printf("%s[%d, %d, %lld, %d]", first ? "" : ", ", std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t));
        first = false;
    }
    printf("],\n\"fast\": {%s},\n", fastJson.c_str());
}

alignas(16) static unsigned char g_lds[160 * 1024 + 64];   // the carve functions that return pointers are walked over this

static void walk_grid() {
    printf("\"grid\": [");
    const int ns[] = {0, 1, 1000, 30000, kGridMaxKeys, kGridMaxKeys + 1};
    for (int i = 0; i < 6; i++) {
        const int n = ns[i];
        g_where = "grid " + std::to_string(n);
        const size_t total = grid_lds_bytes(n);
        CHECK((total <= (size_t) kMaxDynLds) == (n <= kGridMaxKeys));
        const GridPtrs P = grid_carve(g_lds);
        std::vector<Arr> v = {Arr{"cellStart", (unsigned char *) P.cellStart - g_lds, 4ll * (GRID_CELLS + 1), 4, 0},
                              Arr{"cellFill", (unsigned char *) P.cellFill - g_lds, 4ll * GRID_CELLS, 4, 0}, Arr{"list", (unsigned char *) P.list - g_lds, 4ll * n, 4, 0}};
        check_aligned_inside(v, (long long) total, 0, nullptr);
        check_all_disjoint(v);
        printf("%s[%d, %zu]", i ? ", " : "", n, total);
    }
    printf("],\n\"grid_max_n\": %d,\n", kGridMaxKeys);
}

static void walk_aligner(int staticLds) {
    const int ceiling = sia_ceiling((size_t) staticLds);
    printf("\"aligner\": {\"static_lds\": %d, \"ceiling\": %d, \"rows\": [", staticLds, ceiling);
    const int feats[] = {0, 1, 2, 3, 999, 1000, 1755, 1756, 4000, 6400};
    const size_t largest[] = {(size_t) 384 * 240, (size_t) 128 * 60};   // 376x240 and 94x60 at the pyramid's 64-byte pitch
    bool first = true;
    for (size_t lg : largest)
        for (int n : feats) {
            g_where = "aligner " + std::to_string(n) + " features, level of " + std::to_string(lg) + " bytes";
            const SiaLds L = sia_lds(n, lg, (size_t) ceiling, 0);
            const SiaPtrs P = sia_carve((float4 *) g_lds, L);
            const long long total = (long long) sia_lds_bytes(L);
            std::vector<Arr> v = {Arr{"s_feat", 0, 16ll * n, (int) alignof(float4), 0}, Arr{"s_uv", (unsigned char *) P.uv - g_lds, 8ll * n, (int) alignof(float2), 0},
                                  Arr{"s_img", (unsigned char *) P.img - g_lds, L.stageBytes, 16, 0}};
            if (L.jac) v.push_back(Arr{"s_jac", (unsigned char *) P.jac - g_lds, 32ll * n, (int) alignof(float4), 0});
            // The one exception to the alignment rule: s_jac lies at byte 24 * feat, 8 mod 16 for an odd feature count (the one-pair entry passes the
            // pair's own count).  gfx950 serves its 128-bit LDS accesses correctly there, only slower; moving it is a change of the layout and not
            // part of stating it (lds_layout.h).
            check_aligned_inside(v, total, 0, n % 2 ? "s_jac" : nullptr);
            if (L.jac) CHECK(find(v, "s_jac")->off % 8 == 0 && (find(v, "s_jac")->off % 16 == 0) == (n % 2 == 0));
            check_all_disjoint(v);
            CHECK(sia_fits(L) == (n <= kSiaMaxFeatures));
            if (sia_fits(L)) CHECK(total <= ceiling);
            CHECK(L.stageBytes == 0 || L.stageBytes >= 4096);
            // a capped launch (many pairs in flight) stages less or nothing, and never moves the feature table
            const SiaLds Lc = sia_lds(n, lg, (size_t) ceiling, (size_t) 74 * 1024);
            CHECK(Lc.feat == L.feat && Lc.jac == L.jac && Lc.stageOff == L.stageOff && Lc.stageBytes <= L.stageBytes);
            CHECK(Lc.stageBytes == 0 || ((long long) sia_lds_bytes(Lc) <= 74 * 1024 && Lc.stageBytes >= 4096));
            printf("%s[%d, %zu, %zu, %d, %d, %d, %lld]", first ? "" : ", ", n, lg, sia_feat_bytes(n, L.jac != 0), L.jac, L.stageOff, L.stageBytes, total);
            first = false;
        }
    printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc == 5 && std::string(argv[1]) == "oct_sort") {
        printf("%zu\n", oct_lds_bytes(kOctLdsSort, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0, 0));
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: lds_layout_cpu <static LDS bytes of k_sia_run> | oct_sort <nCells> <cap> <ldsCand>\n");
        return 2;
    }
    printf("{\n");
    walk_matcher();
    walk_extractor();
    walk_grid();
    walk_aligner(atoi(argv[1]));
    printf("}\n");
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    return 0;
}
