// lds_layout.h -- the dynamic LDS of every kernel that takes some (k_describe's per-wave region: describe_lds.h), stated once: the kernel takes its
// pointers from the description here and the host its byte count.  constexpr arithmetic and a few small host / device functions, so that a host
// program can walk all of it: tests/cpp/lds_layout_cpu.hip walks each layout over a sweep for tests/test_lds_layout.py (alignment, overlap, extent; the byte counts
// against tests/golden/lds_layout_parent.json).
#ifndef YGZF_LDS_LAYOUT_H
#define YGZF_LDS_LAYOUT_H
#include "ygzf_internal.h"

namespace ygzf {

constexpr size_t al16(size_t b) { return (b + 15) & ~(size_t) 15; }
constexpr int lds_max(int a, int b) { return a > b ? a : b; }

// ---- the frame grid (grid_lds.h: build_grid_lds; k_features_in_area, k_proj_search, k_kf_grid_build) -------------------------------------------
constexpr int GRID_COLS = 64, GRID_ROWS = 48, GRID_CELLS = GRID_COLS * GRID_ROWS;
// cellStart[GRID_CELLS + 1] (+ 3 pad) | cellFill[GRID_CELLS] | list[n] | 16 bytes
constexpr int kGridCellStartInts = GRID_CELLS + 4, kGridCellFillInts = GRID_CELLS;
struct GridPtrs {
    int *cellStart, *cellFill, *list;
};
__host__ __device__ inline GridPtrs grid_carve(unsigned char *dyn) {
    int *const cellStart = (int *) dyn, *const cellFill = cellStart + kGridCellStartInts;
    return GridPtrs{cellStart, cellFill, cellFill + kGridCellFillInts};
}
constexpr size_t grid_lds_bytes(int n) { return sizeof(int) * ((size_t) kGridCellStartInts + kGridCellFillInts + (size_t) n) + 16; }
constexpr int kGridMaxKeys = (int) ((kMaxDynLds - 16) / sizeof(int)) - kGridCellStartInts - kGridCellFillInts;   // the most keypoints one grid holds
static_assert(grid_lds_bytes(kGridMaxKeys) <= (size_t) kMaxDynLds && grid_lds_bytes(kGridMaxKeys + 1) > (size_t) kMaxDynLds, "kGridMaxKeys");

// ---- k_match_last -----------------------------------------------------------------------------------------------------------------------------
// Every array of MatchLds in carve order: X(member, element type, count, spill bit); the two optional groups stand between IF(condition) and
// END, and an array that is not carved stays null.  An array starts at the next multiple of 16 bytes of the space it lives in: LDS, or
// the pair's global spill arena when the plan (MatchArgs::spill) has the array's bit.  The kernel expands the list into its carve-up,
// match_lds_bytes below into the two sums.
constexpr int kExtSlots = 64;
constexpr int kSpillSpec = 1, kSpillMisc = 2;
#define YGZF_MATCH_LDS_ARRAYS(X, IF, END, capCur, capLast)                      \
    X(cellStart, int, GRID_CELLS + 1, 0)                                       \
    X(cellFill, int, GRID_CELLS, 0)                                            \
    X(list, int, capCur, 0)                                                    \
    X(cx, float, capCur, 0)                                                    \
    X(cy, float, capCur, 0)                                                    \
    X(owner, unsigned char, capCur, 0)                                         \
    X(octave, unsigned char, capCur, 0)                                        \
    X(qobs, unsigned char, capLast, 0)                                         \
    X(specKey, uint4, capLast, kSpillSpec)                                     \
    X(specI2, ushort4, capLast, kSpillSpec)                                    \
    IF(specDeep)                                                               \
    X(specKeyB, uint4, capLast, kSpillSpec)                                    \
    X(specI2B, ushort4, capLast, kSpillSpec)                                   \
    END                                                                        \
    X(events, int, capLast, kSpillMisc)                                        \
    X(qang, float, capLast, kSpillMisc)                                        \
    X(cang, float, capCur, kSpillMisc)                                         \
    X(match, int, capCur, kSpillMisc)                                          \
    X(claim, int, capCur, kSpillMisc)                                          \
    X(extOf, unsigned char, 2 * (size_t) (capLast), kSpillMisc)                \
    X(extKey, unsigned, 8 * kExtSlots, kSpillMisc)                             \
    X(extI2, unsigned short, 8 * kExtSlots, kSpillMisc)                        \
    X(extWork, int, kExtSlots, kSpillMisc)                                     \
    IF(descInLds)                                                              \
    X(desc, unsigned long long, 4 * (size_t) (capCur), 0)                      \
    END

struct MatchLdsBytes {
    size_t lds, spill;   // dynamic LDS of the launch (64 bytes of slack behind the last array); global spill bytes per pair
};
constexpr MatchLdsBytes match_lds_bytes(int capCur, int capLast, bool descInLds, int spill, bool specDeep) {
    size_t lds = 0, gl = 0;
#define YGZF_SUM(member, type, count, bit) ((spill & (bit)) ? gl : lds) += al16((size_t) sizeof(type) * (count));
#define YGZF_IF(cond) if (cond) {
#define YGZF_END }
    YGZF_MATCH_LDS_ARRAYS(YGZF_SUM, YGZF_IF, YGZF_END, capCur, capLast)
#undef YGZF_END
#undef YGZF_IF
#undef YGZF_SUM
    return MatchLdsBytes{lds + 64, gl};
}
// The plans a launch tries, in order of preference: everything in LDS; descriptors in global memory; + the speculative lists; + the misc
// arrays.  The first whose LDS stays within the budget is taken (plan_match_lds, ygzf_api_match.hip).
struct MatchLdsPlan {
    int desc, spill;
};
constexpr MatchLdsPlan kMatchLdsPlans[] = {{1, 0}, {0, 0}, {0, kSpillSpec}, {0, kSpillSpec | kSpillMisc}};
constexpr size_t kMatchLdsBudget = 156 * 1024;

// ---- the FAST cell loop (k_fast_quads, k_fast_tab, k_fast_tab_persist): one region per wave ----------------------------------------------------
// window (winRows rows of `pitch` bytes and 16 bytes of slack: the last quad of the last row reads past its row) | score map, which shares
// its bytes with the quad list (the list lives only between pass 1 and the expansion, the map only after it) | corner list (kCornerCap
// u16).  All three multiples of 16.
constexpr int kCornerCap = 512;   // corners listed per cell before the dense fallback takes over
constexpr int kTabPitch = 48;     // window pitch of the table-driven forms
constexpr int kFastPersistWaves = 4;
struct FastWaveLds {
    int winBytes, smapBytes, perWave;   // the score map at winBytes, the corner list at winBytes + smapBytes
};
constexpr FastWaveLds fast_wave_lds(int pitch, int winRows, int smapRows, int quadCap) {
    const int winBytes = (winRows * pitch + 16 + 15) & ~15;
    const int smapBytes = (lds_max(smapRows * pitch, quadCap * 4) + 15) & ~15;
    return FastWaveLds{winBytes, smapBytes, winBytes + smapBytes + kCornerCap * 2};
}
// `waves`: of the kernel that is launched (kFastBlock / 64, kFastTabWaves, kFastPersistWaves)
constexpr size_t fast_lds_bytes(const FastWaveLds &w, int waves) { return (size_t) waves * (size_t) w.perWave + 64; }

// ---- k_octree ---------------------------------------------------------------------------------------------------------------------------------
// Three plans share one description, in ints from the start of dynamic LDS (-1: the plan has no such array in LDS):
//   Sort   cell prefix table | node arrays | candidates' first sort buffer; the SECOND buffer (candB) lies over the cell table and the node
//          arrays, both idle while the candidates are sorted, so the first one starts behind whichever is longer.  The key tables lie in the
//          node arrays (idle until the tree passes).
//   Arena  cell prefix table | both candidate buffers; the node arrays (and the key tables in them) live in global memory.
//   Hist   one region of regionInts ints shared by the cell prefix table, the key tables behind it and -- once the keys exist -- the node
//          arrays from its start; behind the region PS, histBins + 1 ints.
// The node arrays are kOctNodeArrays arrays of `cap` ints each (cap: a multiple of 4, so they and what follows stay 16-byte aligned).
// nCells: the level's own for the kernel, the launch's largest for the host's byte count (every offset grows with nCells).
constexpr int kOctNodeArrays = 19;
enum OctLdsPlan { kOctLdsSort, kOctLdsArena, kOctLdsHist };
struct OctLds {
    int cellPref;          // nCells + 1 ints
    int nodes;             // kOctNodeArrays * cap ints
    int PS;                // histBins + 1 ints (Hist)
    int xTab, xTabRoom;    // the key tables and the ints they may take
    int cand, candInts;    // S.cand: the candidates' sort buffers (Sort: the first pair of them)
    int candB;             // Sort: the second pair, 2 * ldsCand ints, over the cell table and the node arrays
    int ints;              // where it all ends
};
constexpr int oct_lds_region(int nCells, int cap) { return ((nCells + 1 + 3) & ~3) + kOctNodeArrays * cap; }   // Sort: cell table and node arrays
// Sort: where the candidates' first buffer starts -- behind the region (regionEnd) and behind candB, which lies over it
constexpr int oct_lds_sort_cand(int regionEnd, int ldsCand) { return lds_max(regionEnd, 2 * ldsCand); }
// the ints the key tables (a level's lenX + lenY + nCells) may take: k_octree builds them only if they fit
constexpr int oct_lds_tab_room(bool hist, int nCells, int cap, int regionInts) { return hist ? regionInts - (nCells + 1) : kOctNodeArrays * cap; }
// What lies in front of the candidate buffers, which is all the kernel's carve-up takes from here before it has walked its node arrays (a
// term in ldsCand up there moves the kernel's scalar code); `ints`: where the front ends -- Arena: where the candidate buffers start.
constexpr OctLds oct_lds_front(OctLdsPlan plan, int nCells, int cap, int regionInts, int histBins) {
    if (plan == kOctLdsHist) return OctLds{0, 0, regionInts, nCells + 1, oct_lds_tab_room(true, nCells, cap, regionInts), -1, 0, -1, regionInts + histBins + 1};
    const int behindCells = (nCells + 1 + 3) & ~3;
    if (plan == kOctLdsArena) return OctLds{0, -1, -1, -1, 0, -1, 0, -1, behindCells};
    return OctLds{0, behindCells, -1, behindCells, oct_lds_tab_room(false, nCells, cap, regionInts), -1, 0, -1, oct_lds_region(nCells, cap)};
}
constexpr OctLds oct_lds(OctLdsPlan plan, int nCells, int cap, int ldsCand, int regionInts, int histBins) {
    OctLds y = oct_lds_front(plan, nCells, cap, regionInts, histBins);
    if (plan == kOctLdsArena) {
        y.cand = y.ints;
        y.candInts = 4 * ldsCand;
        // (the launch is sized without rounding the cell table up: the buffers may start up to 3 ints lower than the count assumes)
        y.ints = nCells + 1 + 3 + 4 * ldsCand;
    } else if (plan == kOctLdsSort) {
        y.candB = 0;
        y.cand = oct_lds_sort_cand(y.ints, ldsCand);
        y.candInts = 2 * ldsCand;
        y.ints = y.cand + y.candInts;
    }
    return y;
}
constexpr size_t oct_lds_bytes(OctLdsPlan plan, int maxCells, int cap, int ldsCand, int regionInts, int histBins) {
    return sizeof(int) * (size_t) oct_lds(plan, maxCells, cap, ldsCand, regionInts, histBins).ints;
}

// ---- k_sia_run --------------------------------------------------------------------------------------------------------------------------------
// float4 s_feat[feat] | float2 s_uv[feat] | float4 s_jac[2 * feat] (when jac) | 16 bytes | up to the next multiple of 16: the staged current
// image, stageBytes.  s_jac starts at byte 24 * feat: a multiple of 16 for an even feat only.  The batched entry passes the keypoint stride (a
// multiple of 4); the one-pair entry passes the pair's own feature count, and for an odd one s_jac is 8 mod 16.  Its 128-bit LDS accesses are
// then off their natural alignment: gfx950 still serves them correctly but replays each (some 60 cycles), so an odd count costs time, not
// results.  The placement is kept as it is here; every other array of every layout in this file starts at a multiple of min(16, its element's alignment).
struct SiaLds {
    int feat;                  // feature slots
    int stageOff, stageBytes;  // the staged image's byte offset and size
    int jac;                   // 1: the point-only Jacobian terms are staged
};
struct SiaPtrs {
    float2 *uv;
    float4 *jac;
    uint8_t *img;
};
__host__ __device__ inline SiaPtrs sia_carve(float4 *feat, const SiaLds &l) {   // feat: the start of dynamic LDS
    float2 *const uv = (float2 *) (feat + l.feat);
    return SiaPtrs{uv, (float4 *) (uv + l.feat), (uint8_t *) feat + l.stageOff};
}
constexpr size_t sia_lds_bytes(const SiaLds &l) { return (size_t) l.stageOff + (size_t) l.stageBytes; }
constexpr size_t kSiaMaxFeatBytes = 150 * 1024;   // a feature table beyond this is refused
constexpr int kSiaMaxFeatures = (int) ((kSiaMaxFeatBytes - 16) / (sizeof(float4) + sizeof(float2)));   // (no Jacobian terms in LDS at that size)
// features: slots; largestLevelBytes: of the levels the run visits; ceiling: the dynamic LDS the kernel may take (160 KB minus its static part);
// cap: 0, or the most the workgroup should take (the staged image gives way).  The Jacobian terms are staged while the table stays under 96 KB;
// the image only if 4 KB or more are left for it.
constexpr size_t sia_feat_bytes(int features, bool jac) { return (size_t) features * (sizeof(float4) + sizeof(float2) + (jac ? 2 * sizeof(float4) : 0)) + 16; }
constexpr SiaLds sia_lds(int features, size_t largestLevelBytes, size_t ceiling, size_t cap) {
    const bool jac = sia_feat_bytes(features, true) <= 96 * 1024;
    const size_t off = al16(sia_feat_bytes(features, jac));
    size_t stage = 0;
    if (ceiling >= off + 4096) {
        const size_t avail = (ceiling - off) & ~(size_t) 15, want = al16(largestLevelBytes + 8);
        stage = avail < want ? avail : want;
    }
    if (cap) {
        const long room = (long) cap - (long) off;
        stage = room > 4096 ? (stage < (size_t) (room & ~15L) ? stage : (size_t) (room & ~15L)) : 0;
    }
    return SiaLds{features, (int) off, (int) stage, jac ? 1 : 0};
}
constexpr bool sia_fits(const SiaLds &l) { return sia_feat_bytes(l.feat, l.jac != 0) <= kSiaMaxFeatBytes; }
// the dynamic LDS k_sia_run may take: the CU's 160 KB minus the kernel's static part (in allocation units of 256 bytes)
constexpr int sia_ceiling(size_t staticLdsBytes) {
    const size_t c = 160 * 1024 - ((staticLdsBytes + 255) & ~(size_t) 255);
    return (int) (c < (size_t) kMaxDynLds ? c : (size_t) kMaxDynLds);
}

}  // namespace ygzf
#endif
