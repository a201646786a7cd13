// kernels.h -- launcher declarations shared by the HIP translation units of libygzf (product code).
#ifndef YGZF_KERNELS_H
#define YGZF_KERNELS_H
#include "ygzf_internal.h"
#include "ygzf_remap_plan.h"
#include "lds_layout.h"

namespace ygzf {

hipError_t upload_constants(const int *umax16);

struct PyrTabs {   // device tables of one geometry's pyramid
    const int *xofs;
    const short *xalpha;
    const int *yofs;
    const short *ybeta;
    const PyrColRec *cols;
    const PyrRowRec *rows;
    const PyrTileRec *tiles;
};
void launch_pyr_resize(hipStream_t st, const FrameSet &fs, const LevelGeom *dGeom, const LevelGeom &g, int level, int nFrames, const PyrTabs &T);
// k_pyr_resize_tiled's staging area per fold (a wave's lanes cover `fold` rows x 256 / fold columns per pass): 16-byte chunks per staged
// source row, staged rows, LDS row pitch
constexpr int kPyrFolds = 4;
__host__ __device__ constexpr int pyr_fold_chunks(int foldLog2) { return foldLog2 == 0 ? 21 : foldLog2 == 1 ? 11 : foldLog2 == 2 ? 6 : 3; }
__host__ __device__ constexpr int pyr_fold_pitch(int foldLog2) { return 16 * pyr_fold_chunks(foldLog2); }
__host__ __device__ constexpr int pyr_fold_rows(int foldLog2) { return foldLog2 == 0 ? 44 : foldLog2 == 1 ? 84 : foldLog2 == 2 ? 166 : 330; }
constexpr int kPyrTileRows = 32;   // output rows of a tile at fold 1 (fold f: 32 f rows x 256 / f columns)
void launch_repitch_rows(hipStream_t st, const uint8_t *src, size_t srcPitch, uint8_t *dst, size_t dstPitch, int w, size_t rows);
constexpr int kHostFrameListMax = 128;
struct HostFrameList { unsigned long long addr[kHostFrameListMax]; };   // device-visible addresses of page-locked host frames (by value: kernel argument)
void launch_gather_host_frames(hipStream_t st, const HostFrameList &L, int nFrames, size_t srcPitch, uint8_t *dst, size_t dstPitch, size_t dstFrameStride, int w, int h);
struct PyrChainGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    hipGraphNode_t nodes[kMaxLevels];
    int nNodes;                  // nodes 1 .. nNodes
    FrameSet fs;                 // argument storage of the nodes
    const LevelGeom *geom;
    PyrTabs tabs;
    int level[kMaxLevels];
    LevelGeom lv[kMaxLevels];
};
hipError_t pyr_chain_graph_build(PyrChainGraph *pg, const FrameSet &fs, const LevelGeom *dGeom, const LevelGeom *lv, int nlevels, const PyrTabs &T);
hipError_t pyr_chain_graph_retarget(PyrChainGraph *pg, const FrameSet &fs);
void pyr_chain_graph_destroy(PyrChainGraph *pg);
// one frame's whole pyramid chain in one launch (k_pyr_strips): per strip and level, the rows [ca, cb) the strip produces in LDS (level 0:
// stages) and the rows [wa, wb) of them it owns, i.e. writes to the pyramid slab
struct PyrStripPlan {
    uint2 lv[kMaxLevels];   // x = ca | cb << 16, y = wa | wb << 16 (32-bit words: the kernel reads them with scalar loads)
};
struct PyrStripLevel {   // what the kernel needs of a level, 32 bytes
    int w, h, pitch, xtab, ytab, pad;
    long long off;
};
constexpr int kPyrStripMaxThreads = 1024;
__host__ __device__ inline int pyr_strip_lds_pitch(int w) { return ((w + 3) & ~3) + 12; }
// LDS: row table (8 bytes per produced row of the levels >= 1), region A from
// offA (even levels), region B from offB (odd levels)
hipError_t pyr_strips_prepare(size_t ldsBytes);
void launch_pyr_strips(hipStream_t st, const FrameSet &fs, int nlevels, const PyrStripPlan *plans, const PyrStripLevel *levels, int nStrips,
                       int offA, int offB, size_t ldsBytes, int nFrames, const int *xofs, const short *xalpha, const int *yofs, const short *ybeta);
// dst[0 .. bytes) = src[0 .. bytes), bytes a multiple of 16, both 16-byte aligned: small blocks between the page-locked staging area (as the device addresses it) and
// device memory -- a launch where the copy engine would start ~10 us after the copy is queued and hand over ~8 us after it ends
void launch_link_copy(hipStream_t st, void *dst, const void *src, size_t bytes);
void launch_carry_slot(hipStream_t st, ygzf_kp *outKp, uint8_t *outDesc, int *outCnt, long long srcSlot, int kpStride);
void launch_pack_results(hipStream_t st, const int *cnt, const ygzf_kp *kp, const uint8_t *desc, int nFrames, int kpStride, void *dst, size_t offKp, size_t offDesc);
void launch_pack_levels(hipStream_t st, const FrameSet &fs, const LevelGeom *dGeom, int firstLevel, int nlevels, const unsigned *offsets, uint8_t *dst);
void launch_fast_cells(hipStream_t st, const FrameSet &fs, const LevelGeom *dGeom, int nlevels, int iniTh, int minTh,
                       unsigned short *cellCnt, unsigned *slots, int totalCells, long long totalSlots, int totalGroups, int smapRows,
                       int nFrames, int winPitch, int winRows, int quadCap, const int *groupBaseHost, bool iniFirst, unsigned *stats);
// table-driven form of the same cell loop (k_fast_tab): per-cell records built on the host, window staged by LDS-DMA; cells up to 41 px wide
constexpr int kFastTabMaxCell = 41;
void launch_fast_tab(hipStream_t st, const FrameSet &fs, const FastCellRec *dCells, int iniTh, int minTh, unsigned short *cellCnt, unsigned *slots,
                     int totalCells, long long totalSlots, int totalGroups, int smapRows, int nFrames, int winRows, int quadCap, bool iniFirst,
                     unsigned *stats);
hipError_t phase_clocks_read(int kernel, unsigned long long *out16, bool reset);   // -DYGZF_PHASE_CLOCK builds only (hipErrorNotSupported otherwise)
constexpr size_t kFastPersistCounterBytes = 64 * 256;
void launch_fast_tab_persist(hipStream_t st, const FrameSet &fs, const FastCellRec *dCells, int iniTh, int minTh, unsigned short *cellCnt, unsigned *slots,
                             int totalCells, long long totalSlots, int totalGroups, int smapRows, int nFrames, int winRows, int quadCap, bool iniFirst,
                             unsigned *stats, unsigned *counters, int nWorkgroups);
constexpr int kFastStatWords = 8 * 64;   // `stats`: 64 x {cells sampled, cells whose keypoints are FAST(minTh)'s, score rounds beyond the first, plan: 1 one pass / 2 iniTh first, corner-bearing quads, quads, -, pass-1 runs}
// k_octree's key tables of a level: a key word per column (lenX) and per row (lenY) of the level's candidate region, the origin of every cell.  They
// depend on the geometry alone: k_oct_key_tables writes them once per geometry and k_octree copies them into LDS where they fit (oct_lds_tab_room).
__host__ __device__ inline int oct_tab_len_x(const LevelGeom &g) { return (g.regW > g.nCols * g.wCell ? g.regW : g.nCols * g.wCell) + 9; }
__host__ __device__ inline int oct_tab_len_y(const LevelGeom &g) { return (g.regH > g.nRows * g.hCell ? g.regH : g.nRows * g.hCell) + 9; }
__host__ __device__ inline int oct_tab_words(const LevelGeom &g) { return g.nCols <= 0 || g.nRows <= 0 ? 0 : oct_tab_len_x(g) + oct_tab_len_y(g) + g.nCols * g.nRows; }
void launch_oct_key_tables(hipStream_t st, const LevelGeom *dGeom, int nlevels, const int *offHost, unsigned *tabs);   // offHost: nlevels word offsets into tabs, behind its kMaxLevels-word header
int octree_lds_cand(int maxCellsPerLevel, int cap, size_t budget);   // the sort plan's candidate budget within `budget` bytes of LDS node arrays + buffers (0: < 256)
hipError_t octree_prepare(size_t ldsBytes, bool globalNodes, bool hist);
// One launch of k_octree: levels [levelBase, levelBase + gridDim.x) of gridDim.y frames, one workgroup per (level, frame) -- the histogram plan
// with gridDim.z - 1 helper workgroups beside it.  histBins > 0 selects the histogram plan, nodeArena the sort plan with node arrays in global memory.
struct OctArgs {
    // inputs from FAST (frame f at f * totalCells / f * totalSlots)
    const LevelGeom *geom;
    int nlevels, levelBase;
    const unsigned short *cellCnt;   // candidates per cell
    const unsigned *slots;           // x | y << 8 | score << 16 within the cell
    int totalCells;
    long long totalSlots;
    // candidate scratch, frame f at f * candStride: key / value double buffers of the sort (levels whose candidates exceed ldsCand), positions
    unsigned *candKey0, *candVal0, *candKey1, *candVal1, *candXY;
    long long candStride;
    // outputs, frame f at f * kpStride (the counts: f * nlevels + level); procRec is k_describe's work list
    unsigned *lvlKpXY;
    unsigned char *lvlKpScore;
    int *lvlKpCnt, *lvlCandCnt;
    uint2 *procRec;
    int kpStride;
    // list and LDS sizes: list capacity of the launch's levels (a multiple of 4); sort plan: candidates of a level that are sorted in LDS (0 in the
    // histogram plan); nullable: 19 * cap ints per (frame, level) for the node arrays instead of LDS
    int cap, ldsCand;
    int *nodeArena;
    // sort plan with LDS node arrays: 1 = a level whose key is longer than two radix digits is sorted on its top two digits only and starts over
    // with the full sort if its tree reads a digit below them (YGZF_FORCE=oct_sort=prefix|full; the other two plans sort on every bit)
    int sortPrefix;
    // the geometry's key tables (launch_oct_key_tables): level l's xTab | yTab | orgTab from word keyTabs[l] on (the first kMaxLevels words are the offsets)
    const unsigned *keyTabs;
    // histogram plan (histBins > 0): regionInts ints shared by the cell table, the key tables and the node arrays, then histBins + 1 ints of prefix table
    int regionInts, histBins;
    // helper hand-over (gHist non-null: gridDim.z workgroups per (level, frame)): one slice of histBins counts per helper; per (frame, level) the helpers
    // that have left, only ever growing, and the value this launch brings it to; sleeps after which workgroup 0 stops waiting
    int *gHist, *gDone;
    int doneTarget, spinBudget;
    long long *dbg;                  // nullable: kOctDbgWords phase stamps and counters (YGZF_DEBUG=oct)
};
// block: threads per workgroup of the sort plan with LDS node arrays (1024, 512 or 256); the other two plans run kOctBlock.  helpers: gridDim.z
void launch_octree(hipStream_t st, const OctArgs &a, int nLaunchLevels, int nFrames, size_t ldsBytes, int block, int helpers);
constexpr int kOctDbgAlone = 16 * 8 + 16 + 16 * 16;  // per level: six phase stamps, M, n; then per level the workgroups that left the histogram plan; then per level up to 8 (list size, time) pairs of the tree passes;
constexpr int kOctDbgAloneFrames = kOctDbgAlone + 16; // then per level the workgroups 0 that gave up waiting for their helpers (computed the level alone); then a mask of the frames (< 64) where that happened
constexpr int kOctDbgWords = kOctDbgAloneFrames + 1;
void launch_describe(hipStream_t st, const FrameSet &fs, const LevelGeom *dGeom, int nlevels, const int *lvlKpCnt, int *lvlBase,
                     const uint2 *procRec, int kpStride, ygzf_kp *outKp, uint8_t *outDesc, int *outCnt, int outStride, int nFrames, int cvMode);
void launch_hamming_pairs(hipStream_t st, const void *a, const void *b, int n, int *out);

// ---- matcher (match_kernels.hip) -----------------------------------------------------------------------------------
struct MatchQueryScratch;  // opaque: per-query parameters when they do not fit in LDS
struct MatchArgs {
    // Cur side, pair p uses base + p*kpStrideCur
    const ygzf_kp *curKeys;
    const uint8_t *curDesc;
    const float *curURight;        // nullable (mono): all "-1"
    const int *curCnt;             // count of pair p at curCnt[p*cntStrideCur + cntOffCur]
    long long kpStrideCur;
    int cntStrideCur, cntOffCur;
    const uint8_t *ownerIn;        // nullable: initial Cur.mvpMapPoints state (0 free / 1 owned, 0 obs / 2 owned, obs > 0)
    // Last side
    const ygzf_kp *lastKeys;
    const uint8_t *mpDesc;
    const float *world;
    const uint8_t *mpValid, *outlier, *hasObs;  // nullable: all valid / none outlier / all observed
    const int *lastCnt;
    long long kpStrideLast;
    int cntStrideLast, cntOffLast;
    const float *poses;            // per pair: Rcw[9] tcw[3] Rlw[9] tlw[3]
    // mode 1 = SearchByProjection(F, MapPoints): queries come projected (Frame::isInFrustum); mpValid = mbTrackInView, outlier = isBad()
    // mode 2 = SearchByProjection(Cur, KeyFrame, found, th, ORBdist): queries come projected with their predicted level (the host keeps
    //          the scalar prologue incl. MapPoint::PredictScale's logf); window th*scale[lvl], levels lvl-1..lvl+1, accept <= maxDist
    // mode 3 = SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize): Last = F1 (keys, descriptors in mpDesc),
    //          Cur = F2, mpProjX/Y = vbPrevMatched, th = windowSize; TH_LOW + ratio accept, take-over bookkeeping, result in match12
    int mode;
    const float *mpProjX, *mpProjY, *mpProjXR, *mpViewCos, *mpAngle;
    const int *mpLevel;
    float nnratio;
    int maxDist;                   // accept threshold of the in-order pass (TH_HIGH, or ORBdist in mode 2)
    // camera / frame statics
    float fx, fy, cx, cy, mb, mbf, minX, minY, maxX, maxY, gridInvW, gridInvH;
    float scaleFactors[kMaxLevels];
    float th;
    int bMono, checkLevel, checkOri;
    // outputs
    uint8_t *owner;                // per pair kpStrideCur
    int *match;                    // per pair kpStrideCur
    int *nmatches;                 // per pair
    int *match12;                  // mode 3 (SearchForInitialization): vnMatches12, per pair kpStrideLast
    // LDS plan
    int capCur, capLast, descInLds, qpInLds;
    int spill;                     // kSpill* bits: array groups that live in spillScratch instead of LDS
    int specDeep;                  // speculative lists of eight entries instead of four (mode 1)
    void *spillScratch;
    long long spillStride;         // bytes per pair
    void *qpScratch;               // capLast * 32 bytes per pair when !qpInLds
    long long *dbg;                // nullable: 8 wall_clock64 stamps per pair (phase timing, debug)
    // A pair spread over `split` workgroups (few pairs per launch: one Tracking frame): every workgroup builds the grid, takes the queries
    // i % split == its part through projection + speculative lists and leaves them in splitX; the workgroup that arrives last at
    // splitCnt[pair] gathers all lists and runs the in-order pass.  split <= 1: one workgroup per pair, nothing crosses global memory.
    int handoverFence;             // 1: __threadfence() on both sides of the hand-over as well (A/B runs: YGZF_MATCH_FENCE)
    int fixedLanes;                // 1: eight lanes per query in the multi-workgroup scan whatever its level (A/B runs: YGZF_MATCH_LANES=fixed)
    int scanFiltered;              // 1: with one workgroup per pair the speculative scan reads a descriptor only after the window filters have passed
                                   // (k_match_last; YGZF_FORCE=match_scan=filtered|predicated).  Several workgroups per pair always scan predicated.
    int unitWorld;                 // mode 0: the world point of Last keypoint i is ((x - cx) / fx, (y - cy) / fy, 1), not world[3 i ..]
    int serialOrder;               // 1: the one-wave in-order pass instead of the block-wide fixpoint; 2: fixpoint without list extensions, i.e. the
                                   // hand-over to the one-wave pass at the first exhausted list (tests, A/B runs: YGZF_MATCH_SERIAL)
    int split;
    int *splitCnt;                 // one counter per pair, zero between launches (the last workgroup resets it)
    unsigned char *splitX;         // kMatchSplitRec * capLast bytes per pair
    unsigned *matchStat;     // nullable: the context's matcher counters (kMatchStat*); [0] counts the pairs whose in-order resolution fell back
                                   // from the block-wide fixpoint to the one-wave pass
};
// The words of MatchArgs::matchStat (ygzf_match_fallbacks reads the first, ygzf_match_path_stats the five): pairs handed to the one-wave
// pass, of which: out of rounds / out of extension room (a third block for one query, or the 65th slot); extension blocks handed out by the
// fixpoint; full rescans of the one-wave pass (all modes, SearchForInitialization included).  Each is written by one thread per pair and only
// when non-zero.
constexpr int kMatchStatFallbacks = 0, kMatchStatRoundCap = 1, kMatchStatExtRoom = 2, kMatchStatExtended = 3, kMatchStatRescans = 4, kMatchStatWords = 5;
constexpr int kMatchCauseRounds = 1, kMatchCauseExtRoom = 2;   // why a pair left the fixpoint (k_match_last: s_tmp[15])
constexpr int kMatchScanFilteredDefault = 1;   // MatchArgs::scanFiltered unless YGZF_FORCE=match_scan pins it (profiles/r18_match_scan_ab.txt)
constexpr int kMatchScanQueue = 8;             // keypoints a lane of the filtered scan holds back before the wave scores them (a register each)
constexpr int kMatchSplitRec = 56;   // uint4 + uint4 (lists of eight) + ushort4 + ushort4 + float angle + hasObs word
hipError_t match_prepare(size_t ldsBytes);
void launch_backproject_unit(hipStream_t st, const ygzf_kp *keys, const int *cnt, long long kpStride, int maxKp, int nFrames, float fx,
                             float fy, float cx, float cy, float *world);
void launch_match_last(hipStream_t st, const MatchArgs &A, int nPairs, size_t ldsBytes);


// SearchByBoW per-node brute force (match_kernels.hip); match (nF ints) must be pre-set to -1, hist (30 ints) and nmatches to 0
void launch_bow(hipStream_t st, int nNodes, const int *kfOff, const int *kfIdx, const int *fOff, const int *fIdx, const uint8_t *kfValid,
                const ygzf_kp *kfKeys, const uint8_t *kfDesc, int nF, const ygzf_kp *fKeys, const uint8_t *fDesc, float nnratio, int checkOri, int *match,
                unsigned char *binOf, int *hist, int *nmatches);

// SearchByBoW(KeyFrame, KeyFrame) for one KF1 against nCand candidates (match_kernels.hip: k_bow_kf_nodes, k_bow_kf_finish).  Every array lives
// in one device block; a candidate's arrays are byte offsets from `base`.  match12 (nCand x n1 ints) pre-set to -1; tail (kBowKfTail ints per
// candidate: [0] nmatches, [4 .. 34) the rotation histogram) to 0; binOf (nCand x n1 bytes) is scratch.
constexpr int kBowKfTail = 64;
struct BowKfCand {
    long long keys2, desc2, valid2, off1, idx1, off2, idx2;
};
struct BowKfArgs {
    int nCand, nItems, n1;          // nItems = itemBase[nCand]: one wave per (candidate, joined node)
    const uint8_t *base;
    const BowKfCand *cands;
    const int *itemBase;            // nCand + 1 entries: prefix of the candidates' node counts
    const ygzf_kp *keys1;
    const uint8_t *desc1, *valid1;
    float nnratio;
    int checkOri;
    int *match12;
    unsigned char *binOf;
    int *tail;
};
void launch_bow_kf(hipStream_t st, const BowKfArgs &A);

// The keyframe database (kfdb_kernels.hip).  Every stored BowVector is a row of (word id, value) pairs ascending by id in one arena (ids and
// values in parallel arrays); KfdbSlot locates a row, in entries.  k_kfdb_query writes every (query, slot) cell of common / first / score
// (nQueries x nSlots, free slots 0 / -1 / 0.0): nothing to pre-set.  A query's ids are qIds[qOff[q] .. qOff[q + 1]), ascending, at most
// kKfdbMaxQueryWords of them (they are held in LDS).
constexpr int kKfdbMaxQueryWords = 8192;
constexpr unsigned kKfdbMaxWordId = 0x7fffffffu;   // `first` is an int with -1 for "none": the entry points refuse larger ids
struct KfdbSlot {
    long long off;
    int len, live;
};
struct KfdbQueryArgs {
    int nSlots;
    const KfdbSlot *slots;
    const unsigned *ids;
    const double *vals;
    const int *qOff;
    const unsigned *qIds;
    const double *qVals;
    int *common, *first;
    double *score;
};
void launch_kfdb_query(hipStream_t st, const KfdbQueryArgs &A, int nQueries, int maxQueryWords, int cuCount);
void launch_kfdb_repack(hipStream_t st, int nSlots, const KfdbSlot *slots, const long long *newOff, const unsigned *ids, const double *vals,
                        unsigned *idsNew, double *valsNew);

// SearchForTriangulation per-node brute force with the epipolar tests (match_kernels.hip); match12 (n1 ints) pre-set to -1, hist (30 ints) and
// nmatches to 0
struct TriArgs {
    int nEntries, nNodes, n1;       // nEntries = off1[nNodes]
    const int *off1, *idx1, *off2, *idx2;
    const ygzf_kp *keys1, *keys2;
    const uint8_t *desc1, *desc2, *hasMp1, *hasMp2;
    const float *uR1, *uR2;         // nullable: monocular
    const float *sf2, *sigma2;      // mvScaleFactors / mvLevelSigma2 of KF2
    float F[9];                     // F12 row-major
    float ex, ey;                   // epipole of KF1's centre in KF2
    int onlyStereo, checkOri;
    int *match12;
    unsigned char *binOf;
    int *hist, *nmatches;
};
void launch_triangulation(hipStream_t st, const TriArgs &A);

// Frame::isInFrustum over a MapPoint batch (match_kernels.hip); outputs are the mode-1 inputs of k_match_last
struct FrustumArgs {
    int n;
    const uint8_t *candidate;      // nullable: evaluate only where nonzero
    const float *world, *normal, *maxDistInv, *minDistInv, *mfMaxDistance;
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, mbf, minX, minY, maxX, maxY;
    float viewingCosLimit;
    float levelStep[kMaxLevels];   // levelStep[k] = smallest ratio with PredictScale >= k (k = 1 .. nLevels-1), tabulated on the host
    int nLevels;
    uint8_t *inView;
    float *projX, *projY, *projXR, *viewCos;
    int *level;
};
void launch_frustum(hipStream_t st, const FrustumArgs &A);
// MapPoint::ComputeDistinctiveDescriptors over a MapPoint batch (<= 256 observations per point)
void launch_distinctive(hipStream_t st, int nPoints, const int *obsOff, const uint8_t *desc, int *best, int nLarge, const int *large);   // large: points with > 256 observations

// Frame::ComputeBoW: descriptor -> vocabulary tree descent (match_kernels.hip)
void launch_bow_descend(hipStream_t st, int n, const uint8_t *desc, const int *childOff, const int *childIdx, const uint8_t *nodeDesc, int nidLevel,
                        int *leafNode, int *levelNode);

// ---- FAST-10 (fast10_kernels.hip): Thirdparty/fast replacement -------------------------------------------------------
void launch_fast10(hipStream_t st, const uint8_t *img, int pitch, int x0, int y0, int w, int h, int dx0, int dx1, int dy0, int dy1, int barrier,
                   short *S, int *rowCnt, int *rowKept, int *totals, short *xy, int *scores, int *nonmax, int cap);

// ---- FAST-10 grid detector of the DSO_KEYPOINT path (dso_kernels.hip) + list describe (extract_kernels.hip) -----------------
constexpr int kDsoMaxGrid = 64;   // largest supported mnGridSize (cell side in px)
void launch_dso_occ(hipStream_t st, const unsigned *xy, int n, int w, int h, unsigned *occ);
void launch_dso_cells(hipStream_t st, const uint8_t *img, int pitch, int w, int h, int grid, int nCols, int nRows, unsigned *occ, int *cellCnt,
                      unsigned *cellXY, int *total, int th0, int th1, int take, int occW, bool mark);
void launch_dso_compact(hipStream_t st, const int *cellCnt, const unsigned *cellXY, int nInner, int nExisting, void *list, unsigned *newXY, int level);
// ComputeKeyPointsFast: per-cell Shi-Tomasi vote over the levels' non-max-suppressed libfast corners, then the winners' coordinates
void launch_fgrid_vote(hipStream_t st, const uint8_t *img, int pitch, int w, int h, int level, float scale, const short *xy, const int *nonmax,
                       const int *totals, int maxNonmax, int gridCols, long long nCells, const uint8_t *occ, unsigned long long *cellKey);
void launch_fgrid_gather(hipStream_t st, const unsigned long long *cellKey, long long nCells, const short *xyAll, const int *nmAll, const long long *lvlOff,
                         unsigned *cellXY);
void launch_describe_list(hipStream_t st, const FrameSet &fs, const LevelGeom *dGeom, const void *list, int n, int frame,
                          float *outAngle, uint8_t *outDesc, int cvMode);

// ---- Frame::ComputeStereoMatches (stereo_kernels.hip) ---------------------------------------------------------------------
struct StereoRec {   // per right keypoint: x, row band (min | max << 16), octave | index << 16 (octave 1000: empty band)
    float x;
    unsigned band;
    int octave;
};
constexpr int kStereoBinInts = 4096 + 1;   // bin table of one pair (k_stereo_prep): first sorted record of every bin of rows, then the count
struct StereoArgs {
    // keys / descriptors of pair p: left at keys[p*keyStride + keyOffL + i], right at keys[p*keyStride + keyOffR + i] (desc alike, x32)
    const ygzf_kp *keys;
    const uint8_t *desc;
    long long keyStride;
    int keyOffL, keyOffR;
    const int *cnt;                // counts of pair p at cnt[p*cntStride + cntOffL / cntOffR]
    int cntStride, cntOffL, cntOffR;
    // The right eye may live in ANOTHER context's arrays (ygzf_stereo_pair_host: the two eyes of one pair extracted on two streams): keysR / descR /
    // cntR non-null = the right keys of pair p at keysR[p*keyStride + keyOffR + i] etc., its pyramid = frame frame0 + p*frameStep + 1 of fsR
    const ygzf_kp *keysR;
    const uint8_t *descR;
    const int *cntR;
    FrameSet fsR;
    // pyramids: left image of pair p = frame frame0 + p*frameStep of fs, right = the next frame
    FrameSet fs;
    const LevelGeom *geom;
    int frame0, frameStep;
    float scale[kMaxLevels], invScale[kMaxLevels];
    float mb, mbf;
    int nRows;                     // rows of level 0
    StereoRec *rec;                // scratch, pair p at rec + p*recStride: the right keypoints' records sorted by the bin of their band's first row
    long long recStride;
    int *binStart;                 // scratch, pair p at binStart + p*kStereoBinInts
    int nBins, binShift;           // bins of 2^binShift rows, nBins = ((nRows - 1) >> binShift) + 1 <= 4096
    int bandMax;                   // >= last row - first row of every band: 2 * (2 * largest scale factor) + 2
    float *uRight, *depth;         // outputs, pair p at + p*outStride, one per left keypoint
    int *sad;                      // accepted SAD per left keypoint (-1: no match), same stride
    long long outStride;
};
void launch_stereo(hipStream_t st, const StereoArgs &A, int nPairs, int maxLeft, int maxRight);

// ---- ORBmatcher::FindDirectProjection + Align2D over a candidate batch (direct_kernels.hip) ---------------------------------
struct DirectArgs {
    FrameSet cache;                // the image cache: slot s = frame s of this FrameSet
    const LevelGeom *geom;
    int nlevels;
    int curSlot;
    float curTcw[7];
    float fx, fy, cx, cy;
    float scale[kMaxLevels], invScale[kMaxLevels];
    float invLevelSigma2_1;        // mvInvLevelSigma2[1]
    int n;
    const int *refSlot;
    const float *refTcw7;          // n x 7 (quaternion x,y,z,w + translation)
    const ygzf_kp *refKp;
    const float *mpWorld;          // n x 3
    float *pxCurr;                 // n x 2, in/out
    int *searchLevel;
    uint8_t *success;
    uint8_t *patches;              // nullable: n x 100 (_patch_with_border, tests)
};
void launch_direct_projection(hipStream_t st, const DirectArgs &A);

// ---- sparse image alignment (align_kernels.hip) ----------------------------------------------------------------------
struct SiaLevel {
    const uint8_t *img;
    int w, h, pitch;
};
struct FiaArgs {                    // Frame::GetFeaturesInArea queries against one frame's keypoints
    const ygzf_kp *keys;
    int n;
    float minX, minY, gridInvW, gridInvH;
    int nq;
    const float *xyr;               // 3 per query
    const int *levels;              // 2 per query (minLevel, maxLevel) or null (-1, -1)
    int cap;
    int *outIdx, *outN;             // nq x cap indices (reference order), nq counts (uncapped)
};
hipError_t launch_features_in_area(hipStream_t st, const FiaArgs &A);

// The projection searches of one snapshot (match_kernels.hip: k_proj_search<mode>): ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th),
// K keyframes x P points, per pair the bestIdx / bestDist of src/ORBmatcher.cc:764-868 before any map update (-1 / 256: none); and
// LoopClosing's Fuse(pKF, Scw, ...), SearchByProjection(pKF, Scw, ...) and the two directions of SearchBySim3.  A row is one target keyframe
// with its own point list.
struct FuseKf {                     // one keyframe; keys / desc / uRight are byte offsets from ProjArgs::base (uRight -1: monocular),
                                    // from ProjArgs::kfBase when the launch is a resident one
    long long keys, desc, uRight;
    int n, nLevels;
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, mbf, minX, minY, maxX, maxY, gridInvW, gridInvH;
    float levelStep[kMaxLevels];    // PredictScale steps of this keyframe's mfLogScaleFactor / mnScaleLevels (as FrustumArgs::levelStep)
    float scale[kMaxLevels];        // mvScaleFactors
    float invSigma2[kMaxLevels];    // mvInvLevelSigma2 (read by PM_FUSE only)
};
enum ProjMode { PM_FUSE = 0, PM_FUSE_SCW = 1, PM_PROJ_SCW = 2, PM_SIM3 = 3 };
struct ProjRow {
    FuseKf kf;                      // the target keyframe; Rcw / tcw = the (first) transform, Ow = its camera centre (unused by PM_SIM3)
    float R2[9], t2[3];             // PM_SIM3: the second transform, Pc = R2 * (Rcw * P + tcw) + t2
    long long world, normal, maxDistInv, minDistInv, mfMaxDistance, mpDesc;   // byte offsets from ProjArgs::base (normal -1 for PM_SIM3 only)
    long long skip, keyMatched;     // byte offsets from ProjArgs::base, -1: none.  skip: nPoints bytes; keyMatched: kf.n bytes (PM_PROJ_SCW)
    int nPoints;
    long long out;                  // first point of this row in bestIdx / bestDist (in points; times nBest entries)
    long long cellStart, list;      // resident launches: the keyframe's stored grid (k_kf_grid_build), byte offsets from ProjArgs::kfBase
};
struct ProjArgs {
    int mode;                       // any ProjMode
    int nRows, maxPoints, slice;    // slice = points per workgroup; grid = (ceil(maxPoints / slice), nRows)
    const uint8_t *base;            // the call's packed staging area: the point arrays, masks and (non-resident) the keyframes' arrays
    const uint8_t *kfBase;          // null, or the keyframe store's arena: every row's keyframe and its grid lie there (PM_FUSE, PM_FUSE_SCW)
    const ProjRow *rows;
    float th;
    int nBest, maxHamming;          // candidates kept per point (1 unless PM_PROJ_SCW) and the largest distance kept (<= 255)
    int *bestIdx, *bestDist;        // nBest entries per point, ascending (dist, list position), padded with -1 / 256
};
hipError_t launch_proj_search(hipStream_t st, const ProjArgs &A, int maxKeys);

// The resident keyframes (kfstore_kernels.hip; entry points in ygzf_api_kfstore.hip): k_kf_grid_build writes the CSR build_grid_lds produces --
// cellStart[GRID_CELLS + 1] (64 x 48 cells, column-major px * 48 + py) and list[n], key indices ascending inside a cell, the entries behind
// cellStart[GRID_CELLS] (keys outside the cells are in no list) set to -1 -- once per keyframe.  n is at most kGridMaxKeys.
constexpr int kKfGridCells = 64 * 48;
struct KfGridArgs {
    const ygzf_kp *keys;
    int n;
    float minX, minY, gridInvW, gridInvH;
    int *cellStart, *list;
};
hipError_t launch_kf_grid_build(hipStream_t st, const KfGridArgs &A);

struct SiaArgs {
    SiaLds lds;                     // the dynamic LDS of the launch (lds_layout.h: sia_lds)
    const ygzf_kp *keys;            // ref keypoints, pair p at keys + p*kpStride
    const float *world;             // MapPoint world positions, 3 per keypoint
    const uint8_t *mpValid, *outlier;  // nullable
    long long kpStride;
    const int *nRef;                // per-pair count, or null -> n
    int n;
    const float *poses;             // per pair 14 floats: ref Tcw (qx qy qz qw tx ty tz), cur Tcw
    const SiaLevel *refLv, *curLv;  // per pair lvStride entries, indexed by pyramid level
    int lvStride;
    float invScale[kMaxLevels];
    float fx, fy, cx, cy;
    int maxLevel, minLevel, nIter;
    float eps;
    float *patchCache;              // kpStride*48 floats per pair (16-byte aligned): 12 planes of kpStride float4, plane 3*row + {patch, dx, dy}
    float *jacCache;                // unused (Jacobians are rebuilt from dx, dy each iteration)
    float *momCache;                // 4 floats per keypoint (16-byte aligned), pair p at + p*kpStride*4: gradient moments of the reference patch
    uint8_t *visible;               // kpStride per pair
    // perLevel: the reference patches of all levels come from k_sia_precompute (launch_sia_precompute) instead of k_sia_run's own per-level
    // phase: patchCache / momCache hold one block per level (level l at + (l - minLevel) * pcLevelStride / momLevelStride floats, pairs inside
    // a block as before), levelFlags one byte per (level, pair, keypoint): visible at this level or a coarser one
    int unitWorld;                  // the world point of keypoint i is ((x - cx) / fx, (y - cy) / fy, 1), not world[3 i ..]
    int perLevel;
    size_t pcLevelStride, momLevelStride, flagLevelStride;
    uint8_t *levelFlags;
    float *out;                     // 48 floats per pair: TCR[7], ret, iters, chi2, pad[2], H[36]
    long long *dbg;                 // nullable: phase clocks of pair 0 (debug)
};
// fills A.lds for pairs of up to `features` feature slots (capBytes: 0, or the LDS a workgroup should keep to); false: the feature table does not fit
bool sia_plan_lds(SiaArgs &A, int features, size_t largestLevelBytes, size_t capBytes);
hipError_t sia_prepare(size_t ldsBytes);
void launch_sia_precompute(hipStream_t st, const SiaArgs &A, int nPairs, int maxN);
void launch_sia(hipStream_t st, const SiaArgs &A, int nPairs, size_t ldsBytes);

// ---- cv::remap, fixed-point bilinear (remap_kernels.hip; the plan: ygzf_remap_plan.h) ----
// One launch of either kernel: tile list[i] (null: tile i) of the map, for the frames [0, nFrames) in runs of framesPerRun.  src / dst: frame 0,
// rows and frames the given bytes apart; srcAligned / dstAligned: base, row pitch and frame stride are all multiples of 4 (32-bit accesses allowed).
struct RemapArgs {
    const uint32_t *rec, *xy;       // [h][recPitch]
    const RemapTileRec *tiles;
    const int *list;
    int w, h, recPitch, tilesX, srcW, srcH;
    const uint8_t *src;
    long long srcPitch, srcStride;
    uint8_t *dst;
    long long dstPitch, dstStride;
    int nFrames, framesPerRun, srcAligned, dstAligned;
};
void launch_remap_tiles(hipStream_t st, const RemapArgs &A, int nTiles);    // Inside / Lds / Empty tiles only (the box is staged in LDS)
void launch_remap_gather(hipStream_t st, const RemapArgs &A, int nTiles);   // any tile (bounds-checked byte loads from global memory)

// ---- Optimizer::PoseOptimization(Frame *) (pose_kernels.hip): one workgroup of 256 threads per problem, all four rounds in one launch ----
struct PoseProblemDev {             // one frame; device pointers
    const ygzf_kp *keys;
    const float *uRight;            // null: all monocular
    const uint8_t *mpValid;
    const float *world;             // n x 3
    uint8_t *outlier;               // n bytes, in / out (mvbOutlier); doubles as the edges' level between the rounds
    double *stored;                 // n doubles of scratch: chi2 of every edge's last computeError
    int n;
    float Tcw[7];
};
struct PoseOut {                    // per problem
    double T[7];                    // the last round's estimate (not written when ret == 0 for want of correspondences)
    double lambda[4], chi2[4];
    int iters[4], trials[4], stop[4];   // stop: the values of lm::Stop (lm_math.h)
    int ret, nInitial;
};
struct PoseArgs {
    const PoseProblemDev *probs;
    PoseOut *out;
    double fx, fy, cx, cy, bf;
    double deltaMono, deltaStereo;  // double(float(sqrt(5.991))), double(float(sqrt(7.815)))
    float invSigma2[kMaxLevels];
};
void launch_pose_opt(hipStream_t st, const PoseArgs &A, int nProblems);

// ---- Sim3Solver's RANSAC hypotheses (sim3_kernels.hip): one wave per hypothesis, four waves per workgroup, all problems in one launch ----
struct Sim3ProblemDev {             // one solver with at least one hypothesis to evaluate; device pointers
    const float *X1, *X2;           // mvX3Dc1 / mvX3Dc2, n x 3
    const float *maxErr1, *maxErr2; // mvnMaxError1 / 2 as floats, n
    const int *samples;             // nHyp x 3 indices into [0, n), distinct within a triple (checked by the host)
    float *hyp;                     // nHyp x 13: R12 row-major, t12, s12
    int *nInliers;                  // nHyp
    uint64_t *bits;                 // nHyp x ceil(n / 64) words, bit i of word j = correspondence 64 j + i; null: not wanted
    int n, nHyp, fixScale;
    int firstHyp;                   // the problem's first wave in the launch (ascending over the table)
    float K1[4], K2[4];             // fx fy cx cy
};
struct Sim3Args {
    const Sim3ProblemDev *probs;
    int nProblems, totalHyp;
};
void launch_sim3_ransac(hipStream_t st, const Sim3Args &A);

// ---- Optimizer::OptimizeSim3 (sim3_opt_kernels.hip): one workgroup of 256 threads per problem, both rounds in one launch ----
struct Sim3OptProblemDev {          // one loop candidate; device pointers
    const float *P1c, *P2c;         // n x 3
    const float *obs1, *obs2;       // n x 2
    const float *invSigma2_1, *invSigma2_2;   // n
    uint8_t *removed;               // n bytes out: 0 kept, 1 removed after round 0, 2 failed the final test; the pairs' state between the rounds
    double *stored;                 // 2 n doubles of scratch: chi2 of e12 / e21's last computeError
    int n, fixScale;
    double K1[4], K2[4];            // fx fy cx cy, widened from float
    double S12[8];                  // r.x r.y r.z r.w, t, s
    double th2, delta;              // double(th2), double(float(sqrt(th2)))
};
struct Sim3OptOut {                 // per problem
    double S[8];                    // the estimate; S12 itself where the function returns before writing g2oS12
    double lambda[2], chi2[2];
    int iters[2], trials[2], stop[2];   // stop: the values of lm::Stop
    int ret, nBad;
};
struct Sim3OptArgs {
    const Sim3OptProblemDev *probs;
    Sim3OptOut *out;
};
void launch_sim3_opt(hipStream_t st, const Sim3OptArgs &A, int nProblems);

// ---- PnPsolver's EPnP RANSAC (pnp_kernels.hip): one wave per hypothesis, four waves per workgroup, all problems in one launch; then one
// wave per hypothesis again, of which only the records run Refine ----
struct PnpProblemDev {              // one solver with at least one hypothesis to evaluate; device pointers
    const float *P3D, *P2D;         // mvP3Dw n x 3, mvP2D n x 2
    const float *maxErr;            // mvMaxError, n
    const int *samples;             // nHyp x minSet indices into [0, n), distinct within a set (checked by the host)
    double *hyp;                    // nHyp x 12: R row-major, t
    int *nInliers;                  // nHyp
    uint64_t *bits;                 // nHyp x ceil(n / 64) words (always there: k_pnp_refine reads the records' rows)
    int *refinedN;                  // nHyp: -1 where the hypothesis is no record
    double *refinedHyp;             // nHyp x 12, written for records
    uint64_t *refinedBits;   // nHyp x ceil(n / 64) words (zero rows where no record); null: not wanted
    int n, nHyp, minSet, minInliers;
    int firstHyp;                   // the problem's first wave in the launch (ascending over the table)
    double K[4];                    // fu fv uc vc
};
struct PnpArgs {
    const PnpProblemDev *probs;
    int nProblems, totalHyp;
};
void launch_pnp(hipStream_t st, const PnpArgs &A);   // k_pnp_hyp, then k_pnp_refine

// ---- LocalMapping::CreateNewMapPoints' per-pair triangulation (tri_kernels.hip): one lane per pair, the pairs of all problems of a call as
// one flat list in one launch ----
struct TriKfPose {                  // the layout of tri::Kf (tri_math.h; tri_kernels.hip asserts it), stated here so that only the two units of
    float fx, fy, cx, cy, invfx, invfy, mbf;   // this row include that header
    float Rcw[9], tcw[3], Ow[3];
    float q[4], t[3];
};
struct TriKfDev {                   // one keyframe: what tri::triangulate_pair reads of it, and its per-feature arrays (device pointers)
    TriKfPose k;
    const ygzf_kp *keys;            // mvKeys (distorted)
    const float *uRight, *depth, *cosStereo;   // null: monocular
    const float *sigma2, *scale;    // mvLevelSigma2 / mvScaleFactors, nlevels each (resolved by the host)
};
struct TriProblemDev {              // one neighbour with at least one pair
    TriKfDev kf2;
    const int *idx1, *idx2;         // nPairs each, checked by the host: inside [0, n) of their keyframes
    float *x3d;                     // nPairs x 3
    uint8_t *status;                // nPairs
    int nPairs;
    int firstHyp;                   // the problem's first pair in the launch (ascending over the table; the name ransac::problem_of reads)
};
struct TriPairArgs {
    TriKfDev kf1;
    const TriProblemDev *probs;
    int nProblems, totalPairs;
    float ratioFactor;
};
void launch_triangulate(hipStream_t st, const TriPairArgs &A);

}  // namespace ygzf
#endif
