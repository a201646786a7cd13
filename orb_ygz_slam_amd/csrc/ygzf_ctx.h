// ygzf_ctx.h -- the context of libygzf and the small helpers every translation unit of the C ABI shares (product code, internal: nothing here
// is part of include/ygzf.h).  The entry points live in
//   ygzf_plan.hip        the extractor's launch plans per geometry: host arithmetic only, no kernel and no runtime call (ygzf_plan.h)
//   ygzf_api.hip         context, device tables, buffers, the extractor's launch sequence, batch fetches, timers / profile
//   ygzf_api_match.hip   ORBmatcher: SearchByProjection / SearchByBoW / SearchForInitialization / SearchForTriangulation, the Frame grid, isInFrustum,
//                        distinctive descriptors, the vocabulary
//   ygzf_api_align.hip   SparseImgAlign (one pair, cached, resident batch), the image cache, FindDirectProjection
//   ygzf_api_detect.hip  Thirdparty/fast replacement, DSO / FAST_KEYPOINT detectors, descriptors of existing keys
//   ygzf_api_stereo.hip  Frame::ComputeStereoMatches
//   ygzf_api_kfdb.hip    KeyFrameDatabase: the BowVector store and its query
//   ygzf_api_kfstore.hip the resident keyframes: put / erase / clear / grid (their searches are in ygzf_api_match.hip beside the non-resident ones)
//   ygzf_api_remap.hip   Frame::ComputeImagePyramid's undistortion (cv::remap): maps, device / host / pyramid forms (the plan: ygzf_remap_plan.hip)
#ifndef YGZF_CTX_H
#define YGZF_CTX_H
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <set>
#include <type_traits>
#include <unordered_map>

#include "ygzf_plan.h"

namespace ygzf {
enum KernelKind { KK_PYR = 0, KK_FAST, KK_OCTREE, KK_DESCRIBE, KK_HAMMING, KK_BACKPROJ, KK_MATCH, KK_SIA, KK_FAST10, KK_DSO, KK_STEREO, KK_DIRECT, KK_BOW, KK_FRUSTUM, KK_DISTINCTIVE, KK_BOWNODES, KK_GRID, KK_FASTQ, KK_TRI, KK_FASTP, KK_FUSE, KK_PROJ, KK_BOWKF, KK_KFDB, KK_KFGRID, KK_COUNT };
// (the KK_FUSE slot keeps the name ygzf_profile_read has always reported for it; it times k_proj_search<PM_FUSE>)
static const char *kKernelNames[KK_COUNT] = {"k_pyr_resize", "k_fast_tab", "k_octree", "k_describe", "k_hamming_pairs",
                                             "k_backproject_unit", "k_match_last", "k_sia_run", "k_f10_*", "k_dso_cells", "k_stereo_*", "k_direct_projection", "k_bow_descend", "k_frustum", "k_distinctive", "k_bow_nodes", "k_features_in_area", "k_fast_quads", "k_tri_nodes", "k_fast_tab_persist", "k_fuse", "k_proj_search", "k_bow_kf_nodes", "k_kfdb_query", "k_kf_grid_build"};

}  // namespace ygzf

using namespace ygzf;

// What a context's device buffers hold from one call to the next (include/ygzf.h states the rules; ygzf_set_carry_previous / _extract_ahead
// and the pyramid carry's switch stay settings of ygzf_ctx).  Invariants:
//   - frames > 0: output slots 1 .. frames hold the extracted batch `fs` and its levels; 0 after any call that takes the output buffers
//     for its own inputs, a geometry change or output growth.
//   - carry: the slot the next extraction copies into slot 0 (0: none, an empty slot), the last batch's last frame: carry == frames while
//     frames > 0, and it stays when a plain ygzf_compute_pyramid ends the batch (the Frame path's ygzf_extract_resident carries it).
//   - slot0Stale: the last extraction ran with the carry off, slot 0 does not hold its predecessor (the batch matchers refuse).
//   - carryQueued: k_carry_slot is already queued for the extraction being set up (ahead of its upload); false between calls.
//   - carryPyr: dCarryPyr holds the pyramid of the frame in slot 0 (pair 0's reference in ygzf_align_batch_prev).
//   - matchPairs / alignPairs / stereoPairs: results of the last ygzf_match_batch_prev / _align_batch_prev / _stereo_batch still valid.
//   - image: dImg0 / dPyr frame 0 hold one w x h image with its complete pyramid (Extracted and up); Pyramid: ygzf_compute_pyramid was the
//     previous image operation (ygzf_extract_resident's input); PyramidAhead: and it already queued the extraction (ygzf_set_extract_ahead).
struct Held {
    int frames = 0;
    FrameSet fs{};
    int carry = 0;
    bool slot0Stale = false, carryQueued = false, carryPyr = false;
    int matchPairs = 0, alignPairs = 0, stereoPairs = 0;
    enum Image { None, Extracted, Pyramid, PyramidAhead } image = None;
    int w = 0, h = 0;
};

struct ygzf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Tables tab;
    int maxW = 0, maxH = 0, maxBatch = 0;
    Geometry geo;
    std::string err;
    // A device buffer (grow-only through ensure()).  It owns its allocation: the destructor frees it, so a buffer declared anywhere in the
    // context -- or as a local, while an arena is rebuilt -- needs no line elsewhere to be given back.  ygzf_destroy selects the device and
    // drains the stream before the context, and with it every Buf, is deleted.
    struct Buf {
        void *p = nullptr;
        size_t bytes = 0;
        Buf() = default;
        Buf(const Buf &) = delete;
        Buf &operator=(const Buf &) = delete;
        Buf(Buf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
        Buf &operator=(Buf &&o) noexcept {
            if (this != &o) {
                (void) release();
                p = o.p; bytes = o.bytes;
                o.p = nullptr; o.bytes = 0;
            }
            return *this;
        }
        ~Buf() { (void) release(); }
        hipError_t release() {
            const hipError_t e = p ? hipFree(p) : hipSuccess;
            p = nullptr;
            bytes = 0;
            return e;
        }
    };
    static_assert(!std::is_copy_constructible<Buf>::value, "a Buf owns its allocation: a copy would free it twice");
    static_assert(std::is_nothrow_move_constructible<Buf>::value, "a Buf moves (the arenas are rebuilt in locals and moved into the context)");
    Buf dGeom, dXofs, dXalpha, dYofs, dYbeta, dImg0, dPyr, dCellCnt, dSlots, dK0, dV0, dK1, dV1, dXY, dLvlXY, dLvlScore,
        dLvlCnt, dLvlBase, dLvlCand, dOutKp, dOutDesc, dOutCnt, dWorld, dOwner, dMatch, dNMatch, dPoses, dQp,
        dProcOrder, dSpill, dCarryPyr, dCacheImg, dCachePyr, dSplitCnt, dSplitX, dPyrPlan, dPyrCols, dPyrRows, dPyrTiles, dOctHist;
    // Scratch shared by the entry points that need a few arrays for the length of one call (the matcher's fallback uploads of ygzf_features_in_area,
    // _distinctive_descriptors_batch and _descriptor_distance, level packing and re-pitching, the describe-list descriptors, the octree's and the
    // aligner's YGZF_DEBUG clocks).  The rule: contents are valid only inside the entry point that wrote them, every such entry point synchronises
    // before it returns, and no two uses of one buffer overlap inside one call.
    struct Scratch { Buf a, b, c; } tmp;
    Buf dMatchClk;                         // YGZF_DEBUG=match: k_match_last's phase stamps (not in tmp: ygzf_match_batch_prev returns without synchronising)
    // One record per stage: the buffers of its entry points, named as the *Args records they feed name them.
    struct Stereo { Buf rec, uRight, depth, sad, keys, desc, bins; } st;   // ComputeStereoMatches; keys / desc: the one-pair entry's uploads; results stay in uRight / depth for the fetches
    struct Direct { Buf refSlot, refTcw7, refKp, mpWorld, pxCurr, searchLevel, success, patches; } dir;   // FindDirectProjection
    struct Fast10 { Buf img, scores, rowCnt, xy, scoreList, nonmax; } f10;   // Thirdparty/fast (FAST_KEYPOINT keeps every level's lists in the last three)
    struct Align { Buf levels, poses, patchCache, out; } al;   // ygzf_align_batch_prev: SiaLevel tables, poses, reference patches, results (ygzf_align_fetch)
    struct Sia { Buf images, patchCache; } sia;                // ygzf_sia_run: both frames' levels from host memory, reference patches
    struct Voc { Buf childOff, childIdx, nodeDesc; } voc;      // the vocabulary tree as CSR children lists + node descriptors
    struct Bow { Buf desc, leaf, levelNode; } bow;             // ygzf_bow_transform
    // The DSO / FAST_KEYPOINT grid detectors and ygzf_describe_keys (which uses list and angles only).  Three allocations serve one role in the
    // two DSO detectors and another in FAST_KEYPOINT -- never both in one call -- and carry both names:
    //   occXY_voteKey      the existing keys' packed level-0 positions | the vote key of every 5-px cell
    //   cellCnt_lvlTotals  corners per grid cell                       | every level's corner totals
    //   total_lvlOff       the pass's corner count                     | every level's offset into the corner lists
    struct Grid {
        Buf occ, cellXY, list, newXY, angles;   // occupancy (a bitmap / a byte per cell), winners per cell, describe-list entries, new keys' positions, angles
        Buf occXY_voteKey, cellCnt_lvlTotals, total_lvlOff;
    } grid;
    Buf dTriBinOf;                         // SearchForTriangulation: the bin of every keypoint of the first keyframe
    int vocNodes = 0, vocLevels = 0;
    int cacheSlots = 0, cacheW = 0, cacheH = 0, cachePitch = 0;
    long long cachePyrBytes = 0;
    std::vector<unsigned char> cacheFilled;
    bool alignCarry = false;      // keep the last frame's pyramid across batches (enabled by the first ygzf_align_batch_prev)
    std::vector<unsigned char> alKey;   // cache key of the uploaded SiaLevel tables
    int identityPoses = 0;
    void *identityPosesPtr = nullptr;
    PlanPins pins = PlanPins::from_env();   // the YGZF_FORCE plan pins as they stood when this context was constructed (ygzf_plan.h)
    OctPlan oct;               // what the geometry's octree launches with (plan_octree)
    bool carryOff = false;     // ygzf_set_carry_previous(0): extractions do not carry the previous batch's last frame into slot 0
    struct OctHistLayout {     // what dOctHist's hand-over counters were last cleared for (k_octree's helper workgroups)
        int frames = 0, helpers = 0, histBins = 0;
        size_t bytes = 0;      // the allocation: ensure() reallocates only to a larger size
        bool operator==(const OctHistLayout &o) const { return frames == o.frames && helpers == o.helpers && histBins == o.histBins && bytes == o.bytes; }
    } octHistLayout;
    int octDoneTarget = 0;     // what the launches since that clear have brought every (level, frame) counter of the layout to
    static constexpr int octSmallWgs = 128;   // launches of up to this many workgroups take oct.small (752x480: 16 frames 0.211 against 0.221 ms, 64 frames 0.439 against 0.430)
    Buf dOctNodes;
    Buf dOctKeyTabs;           // k_octree's key tables of the current geometry (OctPlan::keyTabOff; written by apply_geometry with the geometry's other tables)
    // FAST threshold plan (extract_kernels.hip, fast_cell): 0 = chosen per batch from the statistics the kernel leaves behind, 1 = one pass at
    // minTh, 2 = iniTh first.  Identical results either way.
    int fastPlan = 0;
    bool fastIniFirst = false;
    unsigned fastLaunches = 0;             // statistics are collected on the first launches and on every 8th one after that
    double fastExtraRounds = 0.0;          // score rounds beyond the first per cell, last measured by the one-pass plan
    double fastCornerQuadsPerRun = 0.0, fastRunsPerCell = 0.0;   // last sampled: corner-bearing quads per pass-1 run, pass-1 runs per cell (ygzf_get_fast_stats)
    Buf dFastStats;
    Buf dFastCells;                        // FastCellRec table of the current geometry (k_fast_tab)
    Buf dMatchStat;                        // the matcher's counters (kernels.h: kMatchStat*; ygzf_match_fallbacks, ygzf_match_path_stats)
    Buf dPack;                             // inputs + outputs of a one-frame entry point, one copy each way (PackedTransfer)
    int fastKernel = 0;                    // ygzf_fast_kernel: 0 chosen per geometry, 1 k_fast_quads (register staging), 2 k_fast_tab (cell table + LDS-DMA)
    unsigned *hFastStats = nullptr;        // page-locked mirror, refreshed by an asynchronous copy after every FAST launch
    Buf dFastCtr;                          // eight draw counters of k_fast_tab_persist (one per XCD), zeroed before every launch
    int cuCount = 256;
    Buf dResPack;                          // [counts | keypoint rows | descriptor rows] of a small launch, contiguous (ygzf_batch_fetch_packed)
    Buf dUpStage;                          // linear landing area of uploads that are re-pitched on the device (upload_rows)
    hipEvent_t evShare = nullptr;
    hipEvent_t evPyrDone = nullptr;        // recorded by mark_pyramid_done, which creates it (null: no pyramid computed yet)
    // one-frame uploads from pageable caller memory (a cv::Mat): the rows are copied into this page-locked, device-visible buffer by the host and
    // read from there by a kernel that writes them at the context's pitch -- the runtime's own pageable path (pin / stage / blit) cost ~50 us for a
    // 752x480 frame, this ~25.  evIn marks the moment the kernel has read the buffer (the next upload waits for it before overwriting).
    uint8_t *hIn = nullptr;                // (one tight frame: at most maxW x maxH bytes, apply_geometry refuses anything larger)
    void *hInDev = nullptr;
    size_t hInBytes = 0;
    hipEvent_t evIn = nullptr;
    bool evInPending = false;
    uint8_t *hStage = nullptr;             // page-locked staging for results that go back to pageable caller memory in many small pieces
    size_t hStageBytes = 0;
    void *hStageDev = nullptr;             // the same memory as the device addresses it (kernels write small results straight into it)
    // The keyframe database (ygzf_api_kfdb.hip).  Buffers of its own: no other entry point reads or writes them, and it touches nothing of `held`.
    //   arena: dIds / dVals hold `cap` entries, rows are appended at `top`; an erased row leaves a hole until the arena grows (then the live rows
    //   are repacked).  slots: the host's copy of the slot table is the authority, dTable follows it -- records [dirtyLo, dirtyHi) have not been
    //   sent yet (the next query sends them with its own upload).
    struct Kfdb {
        Buf dIds, dVals, dTable;
        size_t cap = 0, top = 0, liveEntries = 0;
        std::vector<KfdbSlot> slots;
        std::vector<uint64_t> keys;                 // per slot (valid while live)
        std::unordered_map<uint64_t, int> slotOf;   // live keys
        std::set<int> freeSlots;                    // reused lowest first
        int dirtyLo = 0, dirtyHi = 0;
    } kfdb;
    // The resident keyframes (ygzf_api_kfstore.hip).  Buffers of its own, as the database above: no other entry point reads or writes them and
    // it touches nothing of `held`.  One arena of bytes; a row holds what never changes after a keyframe's construction, in sections aligned
    // as PackedTransfer aligns them: [keys | descriptors | mvuRight (stereo) | cellStart | list].  Rows are appended at `top`, an erased row
    // leaves a hole until the arena grows (then the live rows are repacked).  The slot table lives on the host only: a search copies the
    // slot's FuseKf -- camera, bounds, tables, section offsets relative to the row -- into its row table and adds `off` and the call's pose.
    struct KfStore {
        struct Slot {
            long long off = 0;                      // the row's first byte in the arena
            size_t bytes = 0;
            bool live = false, hasSigma = false;    // hasSigma: put with mvInvLevelSigma2 (the first Fuse reads it)
            FuseKf kf;                              // keys / desc / uRight relative to `off`; Rcw / tcw / Ow unset
            long long cellStart = 0, list = 0;      // relative to `off`
        };
        Buf dArena;
        size_t cap = 0, top = 0, liveBytes = 0;
        std::vector<Slot> slots;
        std::vector<uint64_t> keys;                 // per slot (valid while live)
        std::unordered_map<uint64_t, int> slotOf;   // live keys
        std::set<int> freeSlots;                    // reused lowest first
    } kfs;
    // The undistortion maps (ygzf_api_remap.hip; src/Frame.cc:775-805).  Buffers of its own, as the database above: no other entry point reads or
    // writes them.  Per map id (one per eye) the plan's device tables; `in` / `out`: the raw image of ygzf_remap_host and
    // ygzf_compute_pyramid_remapped, and the former's result, tight.  stats: what the last launch ran (ygzf_remap_stats).
    struct Remap {
        struct Map {
            Buf rec, xy, tiles, listStaged, listGather;   // the lists: tile indices in launch order, per kernel
            bool set = false;
            int srcW = 0, srcH = 0, w = 0, h = 0, recPitch = 0, tilesX = 0, tilesY = 0, nStaged = 0, nGather = 0;
            int count[4] = {0, 0, 0, 0};   // tiles per RemapClass
        } map[kRemapMaps];
        Buf in, out;
        int path = 0;                      // ygzf_remap_path
        int framesPerRun = (int) forced("remap_frames_per_run", kRemapFramesPerRun);
        bool xcdOrder = forced("remap_xcd_order", 1) != 0;   // staged tiles listed so that neighbours share an XCD (ygzf_remap_set)
        int stats[4] = {0, 0, 0, 0};
    } remap;
    Held held;                             // what the buffers hold between calls (the transitions below ygzf_ctx are its only writers)
    int img0Pitch = 0;
    // timing
    hipEvent_t tStart = nullptr, tStop = nullptr;
    // ygzf_set_extract_ahead: ygzf_compute_pyramid queues the extraction behind the pyramid and reads the levels back on a second stream
    // one-frame pyramid chain as a captured graph: seven dependent launches cost the host more than the kernels take (pyramid_chain)
    bool useGraphs = !debug_flag("nograph");
    PyrChainGraph pyrGraph = {};
    const void *pyrGraphKey[6] = {nullptr};   // geometry tables + size the graph was built for
    bool extractAhead = false;
    hipStream_t streamCopy = nullptr;
    hipEvent_t evPyramid = nullptr;
    bool profile = false;
    // debugging aids, read once per context (never on the launch path): synchronise after every kernel and name it on stderr /
    // phase clocks of the octree, matcher and aligner kernels printed to stderr
    bool debugSync = debug_flag("sync");
    // fill: ensure() fills what it allocates, ensure_scratch() and PackedTransfer::upload() fill the per-call scratch again (ygzf_internal.h);
    // what they did, for ygzf_destroy's line on stderr
    bool fill = debug_flag("fill");
    struct FillStats { unsigned long long allocs = 0, refills = 0, bytes = 0; } fillStats;
    // the plans below are the library's own choice unless YGZF_FORCE pins them (tests: every plan against the oracle; ygzf_internal.h)
    // (per-call switches, read once when the context is created like the ones below)
    bool linkKernels = forced("fetch_kernel", 1) != 0, pyrLink = forced("pyr_link", 1) != 0;
    int uploadKernelFrames = (int) forced("upload_kernel_frames", 2);
    size_t uploadKernelBytes = (size_t) forced("upload_kernel_bytes", 16l << 20);
    int matchSplit = (int) forced("match_split", 0);   // 0 automatic, 1 off, n workgroups per pair
    int matchFixedLanes = forced_is("match_lanes", "fixed");   // eight lanes per query whatever the launch
    // form of the speculative scan in launches with one workgroup per pair: descriptors read for the keypoints that passed the window filters
    // only (filtered), or for every keypoint of the cell window (predicated: what several workgroups per pair always run)
    int matchScanFiltered = forced_is("match_scan", "predicated") ? 0 : forced_is("match_scan", "filtered") ? 1 : kMatchScanFilteredDefault;
    int matchFence = (int) forced("match_fence", 0);   // 1: full fences around the matcher's hand-over
    int matchSerial = (int) forced("match_serial", 0);   // 1: the one-wave in-order pass instead of the fixpoint; 2: fixpoint that hands over at the first exhausted list (tests)
    bool siaPerLevel = forced("sia_precompute", 1) != 0;   // reference patches of all levels in a kernel of their own (0: inside k_sia_run, as until round 4)
    bool octDebug = debug_flag("oct"), matchDebug = debug_flag("match"), siaDebug = debug_flag("sia");
    struct Rec { int kind; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    float profMs[KK_COUNT] = {0};
    int profN[KK_COUNT] = {0};
};

// last failed ygzf_create of THIS thread (the reference constructs its left / right extractors from different threads)
extern YGZF_HIDDEN thread_local std::string g_create_err;

// Every error return goes through here.  Entry points queue asynchronous uploads from caller-owned or local host arrays and synchronise
// at their end: an early error return must not leave such a copy in flight behind a source that is about to disappear, so the stream is
// drained first (errors are not a fast path).
static int fail(ygzf_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) {
        if (c->stream) (void) hipStreamSynchronize(c->stream);
        c->err = buf;
    } else {
        g_create_err = buf;
    }
    return code;
}

#define HIPCHECK(c, expr)                                                                                         \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) return fail(c, YGZF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                                    \
    } while (0)

// a buffer that grows loses its contents (the caller forgets what it held: apply_geometry, upload_frames)
static int ensure(ygzf_ctx *c, ygzf_ctx::Buf &b, size_t bytes) {
    if (bytes <= b.bytes) return YGZF_OK;
    HIPCHECK(c, b.release());
    HIPCHECK(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    if (c->fill) {   // (blocking, on the null stream: no ensure() runs inside a stream capture, hipMalloc could not either)
        HIPCHECK(c, hipMemset(b.p, kDebugFillByte, bytes));
        HIPCHECK(c, hipStreamSynchronize(nullptr));
        c->fillStats.allocs++;
        c->fillStats.bytes += bytes;
    }
    return YGZF_OK;
}

// YGZF_DEBUG=fill: a buffer whose contents are dead between calls (dPack, tmp.a/b/c) is filled again over its whole size, on the context's
// stream, where a call begins to use it
static int refill_scratch(ygzf_ctx *c, ygzf_ctx::Buf &b) {
    if (!c->fill || !b.bytes) return YGZF_OK;
    HIPCHECK(c, hipMemsetAsync(b.p, kDebugFillByte, b.bytes, c->stream));
    c->fillStats.refills++;
    c->fillStats.bytes += b.bytes;
    return YGZF_OK;
}
// ensure() for tmp.a/b/c: the call that sizes one of them is about to write it, and nothing it held is valid any more (ygzf_ctx::Scratch)
static int ensure_scratch(ygzf_ctx *c, ygzf_ctx::Buf &b, size_t bytes) {
    const int rc = ensure(c, b, bytes);
    return rc ? rc : refill_scratch(c, b);
}

// ---- the transitions of ygzf_ctx::held (its only writers) ----------------------------------------------------------------------------
static void forget_outputs(ygzf_ctx *c) { c->held.frames = 0; c->held.carry = 0; }
static void forget_image(ygzf_ctx *c) { c->held.image = Held::None; }
// the resident pyramid is taken (an extraction runs on dPyr, or collects what compute_pyramid queued): the image stays, ygzf_extract_resident's input is gone
static void pyramid_taken(ygzf_ctx *c) { if (c->held.image > Held::Extracted) c->held.image = Held::Extracted; }
// ygzf_set_extract_ahead(0): a queued extraction is not collected -- ygzf_extract_resident extracts the pyramid again, without a carried pyramid
static void ahead_dropped(ygzf_ctx *c) {
    if (c->held.image != Held::PyramidAhead) return;
    c->held.image = Held::Pyramid;
    c->held.carryPyr = false;
}
static void set_match_pairs(ygzf_ctx *c, int n) { c->held.matchPairs = n; }
static void set_align_pairs(ygzf_ctx *c, int n) { c->held.alignPairs = n; }
static void set_stereo_pairs(ygzf_ctx *c, int n) { c->held.stereoPairs = n; }

// Slot 0 of the outputs <- the carried frame (k_carry_slot; an empty slot when there is none), once per extraction.  early: queued ahead of the
// host frames' upload by the entry point (it depends on nothing the upload brings: it runs while they cross the link -- 6 us of a one-frame
// call); run_extract's own call then queues nothing.
static void queue_carry(ygzf_ctx *c, bool early) {
    Held &s = c->held;
    if (!s.carryQueued) {
        s.slot0Stale = c->carryOff;
        const int ks = c->geo.kpStride;
        if (!c->carryOff) launch_carry_slot(c->stream, (ygzf_kp *) c->dOutKp.p, (uint8_t *) c->dOutDesc.p, (int *) c->dOutCnt.p, ks > 0 ? s.carry : 0, ks);
    }
    s.carryQueued = early;
}

// dCarryPyr <- the pyramid of the frame the next extraction carries (pair 0's reference in ygzf_align_batch_prev), before dPyr is overwritten
static int save_carry_pyramid(ygzf_ctx *c) {
    const Geometry &G = c->geo;
    if (!c->alignCarry || c->carryOff || G.pyrBytes <= 0) return YGZF_OK;
    int rc = ensure(c, c->dCarryPyr, (size_t) G.pyrBytes + 256);
    if (rc) return rc;
    Held &s = c->held;
    s.carryPyr = s.carry > 0 && s.frames > 0;
    if (s.carryPyr)
        HIPCHECK(c, hipMemcpyAsync(c->dCarryPyr.p, (uint8_t *) c->dPyr.p + (size_t) (s.carry - 1) * G.pyrBytes, (size_t) G.pyrBytes, hipMemcpyDeviceToDevice, c->stream));
    return YGZF_OK;
}

// the end of run_extract: the outputs hold the batch fs; the image buffers hold its frame 0 when fs lies in them
static void extracted(ygzf_ctx *c, const FrameSet &fs, int nFrames) {
    Held &s = c->held;
    s.frames = s.carry = nFrames;
    s.fs = fs;
    s.matchPairs = s.alignPairs = s.stereoPairs = 0;
    s.image = fs.img0 == (const uint8_t *) c->dImg0.p && fs.pyr == (uint8_t *) c->dPyr.p ? Held::Extracted : Held::None;
    s.w = c->geo.w;
    s.h = c->geo.h;
}

// the end of ygzf_compute_pyramid: a w x h image and its pyramid in the buffers.  Ahead: its extraction is queued (and is the batch);
// plain: the batch ends, and the carried pyramid with it -- the carried frame's keypoints stay
static void pyramid_computed(ygzf_ctx *c, int w, int h, bool ahead) {
    Held &s = c->held;
    if (!ahead) {
        s.frames = 0;
        s.carryPyr = false;
    }
    s.image = ahead ? Held::PyramidAhead : Held::Pyramid;
    s.w = w;
    s.h = h;
}

// ---- readers whose check is a rule ----
static bool holds_image(const ygzf_ctx *c, int w, int h) { return c->held.image != Held::None && c->held.w == w && c->held.h == h; }
static bool pyramid_resident(const ygzf_ctx *c) { return c->held.image >= Held::Pyramid; }
// ygzf_match_batch_prev / ygzf_align_batch_prev: pair 0 is (slot 0, frame 0)
static int need_carried_batch(ygzf_ctx *c) {
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    if (c->held.slot0Stale) return fail(c, YGZF_ERR_STATE, "the previous frame was not carried (ygzf_set_carry_previous is off)");
    return YGZF_OK;
}
// the FrameSet of the context's own buffers (frames of w x h at the context's pitch)
static FrameSet own_frames(const ygzf_ctx *c, int w, int h) {
    FrameSet fs;
    fs.img0_pitch = align_up(w, 64);
    fs.img0 = (const uint8_t *) c->dImg0.p;
    fs.img0_stride = (long long) fs.img0_pitch * h;
    fs.pyr = (uint8_t *) c->dPyr.p;
    fs.pyr_stride = c->geo.pyrBytes;
    return fs;
}

static int ensure_stage(ygzf_ctx *c, size_t bytes) {
    if (bytes <= c->hStageBytes) return YGZF_OK;
    if (c->hStage) HIPCHECK(c, hipHostFree(c->hStage));
    c->hStage = nullptr;
    c->hStageBytes = 0;
    HIPCHECK(c, hipHostMalloc((void **) &c->hStage, bytes, hipHostMallocMapped));
    c->hStageDev = nullptr;
    if (hipHostGetDevicePointer(&c->hStageDev, c->hStage, 0) != hipSuccess) { (void) hipGetLastError(); c->hStageDev = nullptr; }
    c->hStageBytes = bytes;
    return YGZF_OK;
}

// One-frame entry points hand over a dozen small host arrays and take a few back.  From pageable memory every hipMemcpyAsync is a staged copy
// of its own (10-20 us of runtime work apiece; twelve of them cost more than the kernel they feed): the arrays are packed into the context's
// page-locked staging area and cross the link as ONE copy each way.
// callers with more than this in flight keep their own copies (the staging area is page-locked memory); YGZF_FORCE=packed_max=<bytes> lowers it so
// that tests reach the large-transfer paths with ordinary frames
static const size_t kPackedMax = (size_t) forced("packed_max", 4l << 20);
struct PackedTransfer {
    ygzf_ctx *c;
    struct Seg { const void *src; void *dst; size_t bytes, off; };
    std::vector<Seg> in, out;
    size_t inBytes = 0, outBytes = 0;
    size_t deviceOnly = 0;   // bytes behind the outputs that live in dPack alone: never staged, never downloaded
    explicit PackedTransfer(ygzf_ctx *c_) : c(c_) {}
    static size_t al(size_t b) { return (b + 255) & ~(size_t) 255; }
    size_t add_in(const void *src, size_t bytes) { const size_t o = inBytes; in.push_back({src, nullptr, bytes, o}); inBytes += al(bytes); return o; }
    size_t add_out(void *dst, size_t bytes) { const size_t o = outBytes; out.push_back({nullptr, dst, bytes, o}); outBytes += al(bytes); return o; }
    // device layout: [inputs | outputs] in c->dPack; returns the base
    // A transfer beyond kPackedMax (a KeyFrame with tens of thousands of features) does not grow the page-locked staging area: its arrays cross
    // one by one from / to the caller's own memory -- same device layout, so the kernels' pointers do not care which way the bytes came.
    bool direct() const { return inBytes + outBytes > kPackedMax; }
    // the packed blocks cross the link by a kernel (the staging area as the device addresses it) unless YGZF_FORCE=fetch_kernel=0
    bool link_kernel() const { return c->hStageDev != nullptr && c->linkKernels; }
    // what the transfer needs of dPack.  dPack only grows, and upload() asks for exactly this: once dPack holds it, its base is the transfer's
    size_t device_bytes() const { return inBytes + outBytes + deviceOnly + 256; }
    int upload(uint8_t **dBase) {
        int rc;
        if ((rc = ensure(c, c->dPack, device_bytes())) || (rc = refill_scratch(c, c->dPack))) return rc;   // (every caller clears its outputs after upload())
        if (direct()) {
            for (const Seg &s : in)
                if (s.bytes) HIPCHECK(c, hipMemcpyAsync((uint8_t *) c->dPack.p + s.off, s.src, s.bytes, hipMemcpyHostToDevice, c->stream));
        } else {
            if ((rc = ensure_stage(c, inBytes + outBytes + 256))) return rc;
            for (const Seg &s : in)
                if (s.bytes) memcpy(c->hStage + s.off, s.src, s.bytes);
            if (inBytes && link_kernel()) { ygzf::launch_link_copy(c->stream, c->dPack.p, c->hStageDev, inBytes); HIPCHECK(c, hipGetLastError()); }
            else if (inBytes) HIPCHECK(c, hipMemcpyAsync(c->dPack.p, c->hStage, inBytes, hipMemcpyHostToDevice, c->stream));
        }
        *dBase = (uint8_t *) c->dPack.p;
        return YGZF_OK;
    }
    uint8_t *d_out(size_t off) const { return (uint8_t *) c->dPack.p + inBytes + off; }
    int download() {   // one copy back, then scattered to the caller's arrays; synchronises the stream
        if (direct()) {
            for (const Seg &s : out)
                if (s.bytes && s.dst) HIPCHECK(c, hipMemcpyAsync(s.dst, d_out(s.off), s.bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(c, hipStreamSynchronize(c->stream));
            return YGZF_OK;
        }
        if (outBytes && link_kernel()) { ygzf::launch_link_copy(c->stream, (uint8_t *) c->hStageDev + inBytes, (uint8_t *) c->dPack.p + inBytes, outBytes); HIPCHECK(c, hipGetLastError()); }
        else if (outBytes) HIPCHECK(c, hipMemcpyAsync(c->hStage + inBytes, (uint8_t *) c->dPack.p + inBytes, outBytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        for (const Seg &s : out)
            if (s.bytes && s.dst) memcpy(s.dst, c->hStage + inBytes + s.off, s.bytes);
        return YGZF_OK;
    }
};

// The batched solvers (ygzf_api_pose / _sim3 / _sim3_opt / _pnp.hip) lay the problems of one call out in ONE host block each way, so that a call
// crosses the link as one copy up and one down whatever the number of problems (beyond kPackedMax PackedTransfer copies segment by segment: one
// segment each way here, several copies per problem otherwise):
//   up [records | the callers' arrays]     down [result records | result arrays]     behind it, on the device only [arrays nobody downloads]
// Every array starts on a 64-byte boundary of its part.  Use: reserve the slots; commit(), after which dev() is final; fill the records;
// upload(); launch; download(), which scatters every output slot that has a destination.
struct ProblemBlock {
    enum Part { Up, Down, DeviceOnly };
    struct Slot { Part part = Up; size_t off = 0, bytes = 0; };
    ProblemBlock(ygzf_ctx *c, size_t recordBytes, size_t outRecordBytes = 0) : P(c), size{al(recordBytes), al(outRecordBytes), 0} {}
    Slot in(const void *src, size_t bytes) { return reserve(Up, src ? bytes : 0, src, nullptr); }   // a caller's array; null or empty: an empty slot
    Slot in_own(size_t bytes) { return reserve(Up, bytes, nullptr, nullptr); }                      // filled by the caller through host()
    Slot out(void *dst, size_t bytes) { return reserve(Down, bytes, nullptr, dst); }                // dst null: downloaded, read through host()
    Slot device_only(size_t bytes) { return reserve(DeviceOnly, bytes, nullptr, nullptr); }
    int commit() {
        block[Up].assign(size[Up], 0);
        block[Down].assign(size[Down], 0);
        P.add_in(block[Up].data(), size[Up]);   // one segment each way, at offset 0 of its side
        P.add_out(block[Down].data(), size[Down]);
        P.deviceOnly = size[DeviceOnly];
        int rc;
        if ((rc = ensure(P.c, P.c->dPack, P.device_bytes()))) return rc;
        base[Up] = (uint8_t *) P.c->dPack.p;
        base[Down] = P.d_out(0);
        base[DeviceOnly] = base[Down] + size[Down];
        for (const Copy &k : copies)
            if (k.src) memcpy(host(k.at), k.src, k.at.bytes);
        return YGZF_OK;
    }
    template <typename T> T *dev(const Slot &s) const { return (T *) (base[s.part] + s.off); }
    uint8_t *host(const Slot &s) { return block[s.part].data() + s.off; }   // Up: before upload(); Down: after download()
    // the record tables at the start of the two blocks, as the host and as the device address them
    template <typename T> T *records() { return (T *) block[Up].data(); }
    template <typename T> const T *dev_records() const { return (const T *) base[Up]; }
    template <typename T> const T *out_records() const { return (const T *) block[Down].data(); }
    template <typename T> T *dev_out_records() const { return (T *) base[Down]; }
    int upload() { uint8_t *d; return P.upload(&d); }
    int download() {
        int rc;
        if ((rc = P.download())) return rc;
        for (const Copy &k : copies)
            if (k.dst) memcpy(k.dst, host(k.at), k.at.bytes);
        return YGZF_OK;
    }

private:
    static size_t al(size_t b) { return (b + 63) & ~(size_t) 63; }
    struct Copy { const void *src; void *dst; Slot at; };
    Slot reserve(Part part, size_t bytes, const void *src, void *dst) {
        const Slot s = {part, size[part], bytes};
        size[part] += al(bytes);
        if (bytes && (src || dst)) copies.push_back({src, dst, s});
        return s;
    }
    PackedTransfer P;
    size_t size[3];
    std::vector<uint8_t> block[2];
    uint8_t *base[3] = {nullptr, nullptr, nullptr};
    std::vector<Copy> copies;
};

// ---- per-kernel event bracketing ------------------------------------------------------------------------------------
static hipEvent_t take_event(ygzf_ctx *c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void) hipEventCreate(&e);
    return e;
}
struct ProfScope {
    ygzf_ctx *c;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    ProfScope(ygzf_ctx *c_, int k, hipStream_t s_ = nullptr) : c(c_), kind(k), s(s_ ? s_ : c_->stream) {
        if (c->profile) {
            a = take_event(c);
            b = take_event(c);
            (void) hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (c->debugSync) {
            fprintf(stderr, "[ygzf] %s ...", kKernelNames[kind]);
            const hipError_t e = hipStreamSynchronize(s);
            fprintf(stderr, " %s\n", hipGetErrorString(e));
        }
        if (c->profile) {
            (void) hipEventRecord(b, s);
            c->recs.push_back({kind, a, b});
        }
    }
};
static void drain_profile(ygzf_ctx *c) {
    if (c->recs.empty()) return;
    (void) hipStreamSynchronize(c->stream);
    for (auto &r : c->recs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            c->profMs[r.kind] += ms;
            c->profN[r.kind]++;
        }
        c->pool.push_back(r.a);
        c->pool.push_back(r.b);
    }
    c->recs.clear();
}

static inline ygzf::PyrTabs pyr_tabs(const ygzf_ctx *c) {
    return ygzf::PyrTabs{(const int *) c->dXofs.p, (const short *) c->dXalpha.p, (const int *) c->dYofs.p, (const short *) c->dYbeta.p,
                         (const ygzf::PyrColRec *) c->dPyrCols.p, (const ygzf::PyrRowRec *) c->dPyrRows.p, (const ygzf::PyrTileRec *) c->dPyrTiles.p};
}

// ---- defined in ygzf_api.hip, used by the other translation units ---------------------------------------------------------------------
YGZF_HIDDEN int apply_geometry(ygzf_ctx *c, int w, int h, int nFrames);
YGZF_HIDDEN int pyramid_chain(ygzf_ctx *c, const ygzf::FrameSet &fs, int nFrames);
YGZF_HIDDEN int stereo_across(ygzf_ctx *l, ygzf_ctx *r, float mb, float mbf);   // ygzf_api_stereo.hip
YGZF_HIDDEN int mark_pyramid_done(ygzf_ctx *c);
YGZF_HIDDEN int pyramid_readback(ygzf_ctx *c, const ygzf::FrameSet &fs, int w, int h, const uint8_t *hostLevel0, int stride, uint8_t *const *levels_out);
YGZF_HIDDEN int run_extract(ygzf_ctx *c, const ygzf::FrameSet &fs, int nFrames, bool pyramidReady = false);
YGZF_HIDDEN int upload_rows(ygzf_ctx *c, void *dst, size_t dstPitch, const uint8_t *src, size_t srcPitch, int w, size_t rows);
// ygzf_api_match.hip: a keyframe's argument checks (needSigma: mvInvLevelSigma2 is read) and the pose-free part of its device record
YGZF_HIDDEN int kf_args_check(ygzf_ctx *c, const ygzf_frame_view &view, const ygzf_camera &cam, const float *inv_level_sigma2, int k, bool needSigma);
YGZF_HIDDEN void kf_record_static(ygzf_ctx *c, const ygzf_frame_view &view, const ygzf_camera &cam, const float *inv_level_sigma2, float log_scale_factor,
                                  ygzf::FuseKf &F);
YGZF_HIDDEN int upload_frames(ygzf_ctx *c, const uint8_t *imgs, int nFrames, int w, int h, int row_pitch, size_t frame_stride, ygzf::FrameSet *fs);
#endif
