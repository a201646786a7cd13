// ygzf_plan.h -- what the extractor's kernels are launched with, decided on the host once per geometry (product code, internal).  Everything
// declared here is defined in ygzf_plan.hip: pure arithmetic on the configuration, the image size and the pins -- no device, no runtime call, and
// no environment: the pins arrive as a PlanPins record, and only PlanPins::from_env() reads YGZF_FORCE (a context's member initialiser and the
// *_plan_host entry points call it) -- so that it can be run (and sanitized) without the device library.
#ifndef YGZF_PLAN_H
#define YGZF_PLAN_H
#include "kernels.h"

#define YGZF_HIDDEN __attribute__((visibility("hidden")))

namespace ygzf {
YGZF_HIDDEN int cv_round_host(double v);
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

struct Geometry {
    int w = 0, h = 0;
    std::vector<LevelGeom> lv;
    std::vector<int> xofs, yofs;
    std::vector<short> xalpha, ybeta;
    std::vector<PyrColRec> pyrCols;      // k_pyr_resize_tiled's tables (levels >= 1, LevelGeom::pyrCol / pyrRow / pyrTile index them)
    std::vector<PyrRowRec> pyrRows;
    std::vector<PyrTileRec> pyrTiles;
    long long pyrBytes = 0;   // per frame, levels >= 1
    std::vector<PyrStripPlan> pyrPlan;   // k_pyr_strips: one entry per strip (empty: this geometry takes one launch per level)
    int pyrStripOffA = 0, pyrStripOffB = 0;
    int pyrBase = 0;                     // the strips start from this level (0: the image; > 0: levels 1 .. pyrBase come from k_pyr_resize_tiled first)
    PyrStripLevel pyrLevels[kMaxLevels];
    size_t pyrStripLds = 0;
    int totalCells = 0, maxCellsPerLevel = 0;
    int totalGroups = 0, fastSmapRows = 3, fastWinPitch = 16, fastWinRows = 7, fastQuadCap = 4;   // 2x2 cell groups of k_fast_quads
    int fastWCellMax = 1;
    std::vector<FastCellRec> fastCells;   // [group * 4 + position]: k_fast_tab's per-cell records
    long long totalSlots = 0;
    long long candStride = 0;
    int kpStride = 0, kpCapMax = 0;
};

// Every YGZF_FORCE key that pins one of the extractor's plans (ygzf_internal.h).  The defaults are the library's own choice;
// from_env() is the one place that reads the keys: a context holds the record from its creation on, so a pinned context stays pinned whatever
// image size it meets later.
struct PlanPins {
    int pyrStrips = 0;               // at least this many strips (tests: the strip plans of large images on small ones)
    int pyrStripBase = 0;            // the strips start not below this level
    int pyrStripFrames = 16;         // k_pyr_strips up to this many frames per launch (0: never)
    bool octOneGroup = false;        // oct_groups=1: the sort plan as one launch of all levels
    int octBlock = 0;                // ... the workgroup size of every launch (256 / 512 / 1024)
    size_t octLdsBytes = 0;          // oct_lds_kb: ... the LDS of every launch
    enum OctPlanPin { Auto, Hist, Sort } octPlan = Auto;
    bool octSortPrefix = true;       // oct_sort=prefix|full: the sort plan orders path keys longer than two radix digits on their top two digits first (full: on every bit, always)
    int octHistBins = 0;             // bounds the histogram
    int octHelpers = -1, octHelperSpin = 1 << 16;
    int fastPersist = -1, fastPersistWgs = 8;   // fastPersist: 1 always, 0 never (tests)
    static PlanPins from_env() {
        PlanPins p;
        p.pyrStrips = (int) forced("pyr_strips", p.pyrStrips);
        p.pyrStripBase = (int) forced("pyr_strip_base", p.pyrStripBase);
        p.pyrStripFrames = (int) forced("pyr_strip_frames", p.pyrStripFrames);
        p.octOneGroup = forced("oct_groups", 0) == 1;
        p.octBlock = (int) forced("oct_block", p.octBlock);
        p.octLdsBytes = (size_t) forced("oct_lds_kb", 0) * 1024;
        p.octPlan = forced_is("oct_plan", "hist") ? Hist : forced_is("oct_plan", "sort") ? Sort : Auto;
        p.octSortPrefix = forced_is("oct_sort", "full") ? false : forced_is("oct_sort", "prefix") ? true : p.octSortPrefix;
        p.octHistBins = (int) forced("oct_hist_bins", p.octHistBins);
        p.octHelpers = (int) forced("oct_helpers", p.octHelpers);
        p.octHelperSpin = (int) forced("oct_helper_spin", p.octHelperSpin);
        p.fastPersist = (int) forced("fast_persist", p.fastPersist);
        p.fastPersistWgs = (int) forced("fast_persist_wgs", p.fastPersistWgs);
        return p;
    }
};

// Functions that can fail return the YGZF_ERR_* code and leave the message in *err.
YGZF_HIDDEN int build_geometry(const Tables &T, const PlanPins &pins, int w, int h, Geometry &G, std::string *err);

// One launch of k_octree: levels [l0, l0 + n), `block` threads per workgroup, list capacity `cap`, `lds` bytes of dynamic LDS.  Sort plan: candidate
// budget `ldsCand` (more candidates sort through global memory), arena: the node arrays in global memory.  Histogram plan: histBins > 0, regionInts.
struct OctLaunch {
    int l0 = 0, n = 0, block = kOctBlock, cap = 0, ldsCand = 0, regionInts = 0, histBins = 0;
    size_t lds = 0;
    bool arena = false;
};
// What one geometry's octree runs.  SortGroups: level groups of their own workgroup size and LDS; SortOne: all levels in one launch sized by the
// plan choice's yardstick (oct_sort_budget), node arrays in LDS or in the arena; Hist: level groups of the histogram plan.  small: all levels in
// ONE histogram-plan launch, taken instead of `launches` by launches of a few frames (run_extract).
struct OctPlan {
    enum Kind { SortGroups, SortOne, Hist } kind = SortOne;
    std::vector<OctLaunch> launches;
    bool haveSmall = false;
    OctLaunch small;
    // the key tables of the geometry (kernels.h: oct_tab_words per level, every level's first word a multiple of four, behind a header of
    // kMaxLevels words that repeats the offsets for the kernel): written once when the geometry is planned, read by every launch of every plan
    int keyTabOff[kMaxLevels] = {0};
    int keyTabWords = 0;
};
// oneGroup: all levels in one launch of kOctBlock threads (YGZF_FORCE=oct_groups=1); block > 0 / ldsBytes > 0 pin every launch's workgroup / LDS
YGZF_HIDDEN std::vector<OctLaunch> plan_oct_sort(const Geometry &G, int L, bool oneGroup, int block, size_t ldsBytes);
YGZF_HIDDEN int plan_octree(const Geometry &G, int L, const PlanPins &pins, OctPlan &plan, std::string *err);

// Which form of the FAST cell loop a launch of nFrames frames takes and, for Persist, how many workgroups the device holds at once.
// fastKernelSetting: ygzf_set_fast_kernel's; tabLds: the persistent form's LDS for the geometry (fast_lds_bytes, kFastPersistWaves).
struct FastChoice {
    enum Kind { Quads, Tab, Persist } kind;
    int resident;
};
YGZF_HIDDEN FastChoice choose_fast(const Geometry &G, int fastKernelSetting, const PlanPins &pins, int cuCount, int nFrames, size_t tabLds);

}  // namespace ygzf
#endif
