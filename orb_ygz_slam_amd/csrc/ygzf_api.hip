// ygzf_api.hip -- the C ABI of libygzf (include/ygzf.h): context, geometry tables, buffer management and the launch
// sequence of the extractor hot path.  Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>

#include "ygzf_ctx.h"

using namespace ygzf;

thread_local std::string g_create_err;   // last failed ygzf_create of THIS thread

int apply_geometry(ygzf_ctx *c, int w, int h, int nFrames) {
    if (w < 1 || h < 1) return fail(c, YGZF_ERR_INVALID, "image size %dx%d", w, h);
    if (w > c->maxW || h > c->maxH) return fail(c, YGZF_ERR_INVALID, "image %dx%d exceeds the context maximum %dx%d", w, h, c->maxW, c->maxH);
    if (nFrames < 1 || nFrames > c->maxBatch) return fail(c, YGZF_ERR_INVALID, "batch of %d frames (context maximum %d)", nFrames, c->maxBatch);
    const int L = c->tab.cfg.nlevels;
    if (c->geo.w != w || c->geo.h != h) {
        Geometry G;
        OctPlan oct;
        std::string msg;
        int rc = build_geometry(c->tab, c->pins, w, h, G, &msg);
        if (!rc) rc = plan_octree(G, L, c->pins, oct, &msg);
        if (rc) return fail(c, rc, "%s", msg.c_str());
        // c->geo is committed only after every fallible step below has succeeded: a failed attempt leaves (w, h) unset, so that a retry
        // runs the whole setup again instead of continuing on partial device tables
        c->geo.w = c->geo.h = 0;
        forget_outputs(c);
        forget_image(c);
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        rc = ensure(c, c->dGeom, sizeof(LevelGeom) * L);
        if (rc) return rc;
        HIPCHECK(c, hipMemcpy(c->dGeom.p, G.lv.data(), sizeof(LevelGeom) * L, hipMemcpyHostToDevice));
        struct { ygzf_ctx::Buf *b; const void *src; size_t bytes; } up[4] = {
            {&c->dXofs, G.xofs.data(), G.xofs.size() * sizeof(int)},
            {&c->dXalpha, G.xalpha.data(), G.xalpha.size() * sizeof(short)},
            {&c->dYofs, G.yofs.data(), G.yofs.size() * sizeof(int)},
            {&c->dYbeta, G.ybeta.data(), G.ybeta.size() * sizeof(short)}};
        for (auto &u : up) {
            rc = ensure(c, *u.b, std::max<size_t>(u.bytes, 16));
            if (rc) return rc;
            if (u.bytes) HIPCHECK(c, hipMemcpy(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice));
        }
        {
            struct { ygzf_ctx::Buf *b; const void *src; size_t bytes; } up2[3] = {
                {&c->dPyrCols, G.pyrCols.data(), G.pyrCols.size() * sizeof(PyrColRec)},
                {&c->dPyrRows, G.pyrRows.data(), G.pyrRows.size() * sizeof(PyrRowRec)},
                {&c->dPyrTiles, G.pyrTiles.data(), G.pyrTiles.size() * sizeof(PyrTileRec)}};
            for (auto &u : up2) {
                rc = ensure(c, *u.b, std::max<size_t>(u.bytes, 64));
                if (rc) return rc;
                if (u.bytes) HIPCHECK(c, hipMemcpy(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice));
            }
        }
        if (!G.pyrPlan.empty()) {
            rc = ensure(c, c->dPyrPlan, sizeof G.pyrLevels + G.pyrPlan.size() * sizeof(PyrStripPlan));   // level table, then one plan per strip
            if (rc) return rc;
            {   // the kernel counts levels from the strips' base level: both tables go up shifted
                PyrStripLevel lv[kMaxLevels];
                std::memset(lv, 0, sizeof lv);
                for (int l = G.pyrBase; l < L; l++) lv[l - G.pyrBase] = G.pyrLevels[l];
                std::vector<PyrStripPlan> rel(G.pyrPlan.size());
                for (size_t q = 0; q < rel.size(); q++) {
                    std::memset(&rel[q], 0, sizeof rel[q]);
                    for (int l = G.pyrBase; l < L; l++) rel[q].lv[l - G.pyrBase] = G.pyrPlan[q].lv[l];
                }
                HIPCHECK(c, hipMemcpy(c->dPyrPlan.p, lv, sizeof lv, hipMemcpyHostToDevice));
                HIPCHECK(c, hipMemcpy((char *) c->dPyrPlan.p + sizeof G.pyrLevels, rel.data(), rel.size() * sizeof(PyrStripPlan), hipMemcpyHostToDevice));
            }
            if (pyr_strips_prepare(G.pyrStripLds) != hipSuccess) {   // no such LDS allotment on this device: one launch per level
                (void) hipGetLastError();
                G.pyrPlan.clear();
            }
        }
        rc = ensure(c, c->dFastCells, std::max<size_t>(G.fastCells.size() * sizeof(FastCellRec), 32));
        if (rc) return rc;
        if (!G.fastCells.empty()) HIPCHECK(c, hipMemcpy(c->dFastCells.p, G.fastCells.data(), G.fastCells.size() * sizeof(FastCellRec), hipMemcpyHostToDevice));
        rc = ensure(c, c->dOctKeyTabs, std::max<size_t>((size_t) oct.keyTabWords * sizeof(unsigned), 16));
        if (rc) return rc;
        launch_oct_key_tables(c->stream, (const LevelGeom *) c->dGeom.p, L, oct.keyTabOff, (unsigned *) c->dOctKeyTabs.p);   // (stream order puts it ahead of every octree launch)
        HIPCHECK(c, hipGetLastError());
        if (oct.haveSmall || oct.kind == OctPlan::Hist) HIPCHECK(c, octree_prepare(0, false, true));
        if (oct.kind != OctPlan::Hist) HIPCHECK(c, octree_prepare(oct.launches[0].lds, oct.launches[0].arena, false));
        c->oct = oct;
        c->geo = G;
    }
    const Geometry &G = c->geo;
    const size_t B = (size_t) nFrames;
    int rc = 0;
    // (a buffer that grows loses its contents -- the image and pyramid, the carried frame with the outputs -- even where the new allocation lands
    // at the old address or fails)
    const size_t oldPyr = c->dPyr.bytes;
    rc = ensure(c, c->dPyr, std::max<size_t>(B * G.pyrBytes, 16) + 256);
    if (oldPyr != c->dPyr.bytes) forget_image(c);
    if (rc) return rc;
    if ((rc = ensure(c, c->dCellCnt, std::max<size_t>(B * G.totalCells * sizeof(unsigned short), 16)))) return rc;
    if ((rc = ensure(c, c->dSlots, std::max<size_t>(B * G.totalSlots * sizeof(unsigned), 16)))) return rc;
    const size_t cb = std::max<size_t>(B * G.candStride * sizeof(unsigned), 16);
    if ((rc = ensure(c, c->dK0, cb)) || (rc = ensure(c, c->dV0, cb)) || (rc = ensure(c, c->dK1, cb)) || (rc = ensure(c, c->dV1, cb)) ||
        (rc = ensure(c, c->dXY, cb)))
        return rc;
    if (c->oct.launches[0].arena && (rc = ensure(c, c->dOctNodes, B * L * 19 * (size_t) G.kpCapMax * sizeof(int) + 64))) return rc;
    const size_t kp = std::max<size_t>(B * G.kpStride, 16);
    const size_t kp1 = std::max<size_t>((B + 1) * G.kpStride, 16);  // + carry slot
    const size_t oldCnt = c->dOutCnt.bytes, oldKp = c->dOutKp.bytes, oldDesc = c->dOutDesc.bytes;
    if ((rc = ensure(c, c->dLvlXY, kp * sizeof(unsigned))) || (rc = ensure(c, c->dLvlScore, kp)) ||
        (rc = ensure(c, c->dLvlCnt, B * L * sizeof(int))) || (rc = ensure(c, c->dLvlBase, B * kMaxLevels * sizeof(int))) || (rc = ensure(c, c->dProcOrder, kp * sizeof(uint2))) || (rc = ensure(c, c->dLvlCand, B * L * sizeof(int))))
        return rc;
    if (!(rc = ensure(c, c->dOutKp, kp1 * sizeof(ygzf_kp))) && !(rc = ensure(c, c->dOutDesc, kp1 * 32))) rc = ensure(c, c->dOutCnt, (B + 1) * sizeof(int));
    if (oldCnt != c->dOutCnt.bytes || oldKp != c->dOutKp.bytes || oldDesc != c->dOutDesc.bytes) forget_outputs(c);
    return rc;
}

// The launch sequence of ORBextractor::operator()(image...) for a batch resident on the device.
// Pyramid levels 1 .. L-1 of the frames in fs.  For ONE frame the chain is seven (nlevels - 1) small dependent kernels whose launches take the
// host longer than the kernels run; it is captured once per (buffers, geometry) into a graph and replayed with one call.
int pyramid_chain(ygzf_ctx *c, const FrameSet &fs, int nFrames) {
    const Geometry &G = c->geo;
    const int L = c->tab.cfg.nlevels;
    const LevelGeom *dGeom = (const LevelGeom *) c->dGeom.p;
    auto launch_all = [&](bool prof) {
        for (int l = 1; l < L; l++) {
            if (prof) {
                ProfScope ps(c, KK_PYR);
                launch_pyr_resize(c->stream, fs, dGeom, G.lv[l], l, nFrames, pyr_tabs(c));
            } else
                launch_pyr_resize(c->stream, fs, dGeom, G.lv[l], l, nFrames, pyr_tabs(c));
        }
    };
    if (!G.pyrPlan.empty() && nFrames <= c->pins.pyrStripFrames) {   // a few frames: the whole chain in one launch (large images: from the plan's base level on)
        FrameSet fb = fs;
        for (int l = 1; l <= G.pyrBase; l++) {
            ProfScope ps(c, KK_PYR);
            launch_pyr_resize(c->stream, fs, dGeom, G.lv[l], l, nFrames, pyr_tabs(c));
        }
        if (G.pyrBase > 0) {
            fb.img0 = fs.pyr + G.lv[G.pyrBase].off;
            fb.img0_stride = fs.pyr_stride;
            fb.img0_pitch = G.lv[G.pyrBase].pitch;
        }
        ProfScope ps(c, KK_PYR);
        launch_pyr_strips(c->stream, fb, L - G.pyrBase, (const PyrStripPlan *) ((const char *) c->dPyrPlan.p + sizeof G.pyrLevels), (const PyrStripLevel *) c->dPyrPlan.p,
                          (int) G.pyrPlan.size(), G.pyrStripOffA, G.pyrStripOffB, G.pyrStripLds, nFrames,
                          (const int *) c->dXofs.p, (const short *) c->dXalpha.p, (const int *) c->dYofs.p, (const short *) c->dYbeta.p);
        return YGZF_OK;
    }
    if (nFrames != 1 || L < 3 || !c->useGraphs || c->profile || c->debugSync) {
        launch_all(true);
        return YGZF_OK;
    }
    const void *key[6] = {c->dGeom.p, c->dXofs.p, c->dPyrCols.p, c->dPyrRows.p, c->dPyrTiles.p,
                          (const void *) (((uintptr_t) G.w << 32) | (uintptr_t) (unsigned) G.h)};
    if (!c->pyrGraph.exec || memcmp(key, c->pyrGraphKey, sizeof key) != 0) {
        pyr_chain_graph_destroy(&c->pyrGraph);
        const hipError_t e = pyr_chain_graph_build(&c->pyrGraph, fs, dGeom, G.lv.data(), L, pyr_tabs(c));
        if (e != hipSuccess) {   // no graphs on this runtime: plain launches from now on
            (void) hipGetLastError();
            c->useGraphs = false;
            launch_all(true);
            return YGZF_OK;
        }
        memcpy(c->pyrGraphKey, key, sizeof key);
    } else if (memcmp(&c->pyrGraph.fs, &fs, sizeof fs) != 0) {
        HIPCHECK(c, pyr_chain_graph_retarget(&c->pyrGraph, fs));
    }
    HIPCHECK(c, hipGraphLaunch(c->pyrGraph.exec, c->stream));
    return YGZF_OK;
}

// marks "the pyramid of frame 0 is complete" on the context's stream: what another context waits for before it copies that pyramid
// (ygzf_image_cache_put_resident) -- not the end of the stream, where an extraction queued ahead may still be running
int mark_pyramid_done(ygzf_ctx *c) {
    if (!c->evPyrDone) HIPCHECK(c, hipEventCreateWithFlags(&c->evPyrDone, hipEventDisableTiming));
    HIPCHECK(c, hipEventRecord(c->evPyrDone, c->stream));
    return YGZF_OK;
}

// ---- the steps of run_extract, in launch order ---------------------------------------------------------------------------------------
// threshold plan of this launch: from the statistics of an earlier launch of this context (whatever the asynchronous copy has
// delivered by now; a stale or half-written snapshot only affects speed -- both plans return the same keypoints)
static void fast_threshold_plan(ygzf_ctx *c, bool *iniFirst, bool *collect) {
    unsigned cells = 0, usedMin = 0, extra = 0, planBits = 0, cornerQuads = 0, runs = 0;
    const volatile unsigned *hs = c->hFastStats;   // written by the copy engine, possibly right now
    for (int k = 0; k < 64; k++) {
        cells += hs[8 * k]; usedMin += hs[8 * k + 1]; extra += hs[8 * k + 2]; planBits |= hs[8 * k + 3];
        cornerQuads += hs[8 * k + 4]; runs += hs[8 * k + 7];
    }
    const unsigned plan = planBits & 3u;
    if (cells >= 32 && (plan == 1 || plan == 2)) {
        if (plan == 1) c->fastExtraRounds = (double) extra / cells;   // only the one-pass plan sees every FAST(minTh) corner
        // a score round costs ~180 vector instructions per wave, a second pass 1 ~700: iniTh first pays when the rounds it saves
        // outweigh the second passes of the cells that are empty at iniTh
        c->fastIniFirst = c->fastExtraRounds * 180.0 > ((double) usedMin / cells) * 700.0;
        if (runs > 0) {
            c->fastCornerQuadsPerRun = (double) cornerQuads / runs;
            c->fastRunsPerCell = (double) runs / cells;
        }
    }
    *iniFirst = c->fastPlan == 2 || (c->fastPlan == 0 && c->fastIniFirst);
    *collect = c->fastPlan == 0 && (c->fastLaunches < 4 || (c->fastLaunches & 7) == 0);   // content drifts slowly: sample it
    c->fastLaunches++;
}

// the cell loop in the form choose_fast (ygzf_plan.hip) picked, with the statistics and draw counters it needs cleared ahead of it
static int launch_fast(ygzf_ctx *c, const FrameSet &fs, int nFrames, const FastChoice &choice, bool iniFirst, bool collect) {
    const Geometry &G = c->geo;
    const ygzf_extractor_cfg &cfg = c->tab.cfg;
    unsigned short *cellCnt = (unsigned short *) c->dCellCnt.p;
    unsigned *slots = (unsigned *) c->dSlots.p;
    if (collect) {
        int rcS = ensure(c, c->dFastStats, kFastStatWords * sizeof(unsigned));
        if (rcS) return rcS;
        HIPCHECK(c, hipMemsetAsync(c->dFastStats.p, 0, kFastStatWords * sizeof(unsigned), c->stream));
    }
    unsigned *stats = collect ? (unsigned *) c->dFastStats.p : nullptr;
    if (choice.kind == FastChoice::Persist) {
        int rcC = ensure(c, c->dFastCtr, kFastPersistCounterBytes);
        if (rcC) return rcC;
        HIPCHECK(c, hipMemsetAsync(c->dFastCtr.p, 0, kFastPersistCounterBytes, c->stream));
    }
    {
        ProfScope ps(c, choice.kind == FastChoice::Persist ? KK_FASTP : choice.kind == FastChoice::Tab ? KK_FAST : KK_FASTQ);
        if (choice.kind == FastChoice::Persist)
            launch_fast_tab_persist(c->stream, fs, (const FastCellRec *) c->dFastCells.p, cfg.ini_th_fast, cfg.min_th_fast, cellCnt, slots, G.totalCells,
                                    G.totalSlots, G.totalGroups, G.fastSmapRows, nFrames, G.fastWinRows, G.fastQuadCap, iniFirst, stats,
                                    (unsigned *) c->dFastCtr.p, (int) std::min<long long>(choice.resident, (long long) nFrames * G.totalGroups));
        else if (choice.kind == FastChoice::Tab)
            launch_fast_tab(c->stream, fs, (const FastCellRec *) c->dFastCells.p, cfg.ini_th_fast, cfg.min_th_fast, cellCnt, slots, G.totalCells,
                            G.totalSlots, G.totalGroups, G.fastSmapRows, nFrames, G.fastWinRows, G.fastQuadCap, iniFirst, stats);
        else {
            const int L = cfg.nlevels;
            int groupBase[kMaxLevels];
            for (int l = 0; l < L; l++) groupBase[l] = G.lv[l].groupBase;
            launch_fast_cells(c->stream, fs, (const LevelGeom *) c->dGeom.p, L, cfg.ini_th_fast, cfg.min_th_fast, cellCnt, slots, G.totalCells,
                              G.totalSlots, G.totalGroups, G.fastSmapRows, nFrames, G.fastWinPitch, G.fastWinRows, G.fastQuadCap, groupBase, iniFirst, stats);
        }
    }
    if (collect) HIPCHECK(c, hipMemcpyAsync(c->hFastStats, c->dFastStats.p, kFastStatWords * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    return YGZF_OK;
}

// k_octree's argument record for one launch of the plan: what every launch shares, then the launch's levels, list and LDS sizes and what is
// its plan's own (the histogram plan sorts nothing in LDS: its ldsCand is 0)
static OctArgs oct_args(const ygzf_ctx *c, const OctLaunch &grp, long long *odbg) {
    const Geometry &G = c->geo;
    OctArgs a{};
    a.geom = (const LevelGeom *) c->dGeom.p; a.nlevels = c->tab.cfg.nlevels; a.levelBase = grp.l0; a.cap = grp.cap; a.dbg = odbg;
    a.cellCnt = (const unsigned short *) c->dCellCnt.p; a.slots = (const unsigned *) c->dSlots.p; a.totalCells = G.totalCells; a.totalSlots = G.totalSlots;
    a.candKey0 = (unsigned *) c->dK0.p; a.candVal0 = (unsigned *) c->dV0.p; a.candKey1 = (unsigned *) c->dK1.p; a.candVal1 = (unsigned *) c->dV1.p;
    a.candXY = (unsigned *) c->dXY.p; a.candStride = G.candStride; a.procRec = (uint2 *) c->dProcOrder.p; a.kpStride = G.kpStride;
    a.lvlKpXY = (unsigned *) c->dLvlXY.p; a.lvlKpScore = (unsigned char *) c->dLvlScore.p; a.lvlKpCnt = (int *) c->dLvlCnt.p; a.lvlCandCnt = (int *) c->dLvlCand.p;
    a.ldsCand = grp.ldsCand; a.regionInts = grp.regionInts; a.histBins = grp.histBins;
    a.nodeArena = grp.arena ? (int *) c->dOctNodes.p : nullptr;
    a.sortPrefix = c->pins.octSortPrefix && !grp.arena && grp.histBins == 0;
    a.keyTabs = (const unsigned *) c->dOctKeyTabs.p;
    return a;
}

// The small plan's helper workgroups: how many this launch takes, and their hand-over counters brought to the state the launch expects.
static int arm_oct_helpers(ygzf_ctx *c, int nFrames, int L, const OctLaunch &small, OctArgs *a, int *helpersOut) {
    const Geometry &G = c->geo;
    // helper workgroups for the keys of a level (k_octree): as many as keep the WHOLE launch resident at one workgroup per compute unit
    // (workgroup 0 of a level waits for its helpers), at most 8, and only where a level is worth the hand-over (a few microseconds)
    int helpers = c->pins.octHelpers;
    if (helpers < 0) helpers = G.totalCells >= 2000 ? std::min(8, std::max(1, c->cuCount) / std::max(1, nFrames * L)) : 1;
    helpers = std::max(1, std::min(helpers, std::min(8, std::max(1, c->cuCount / std::max(1, nFrames * L)))));
    if (helpers > 1) {
        const size_t words = (size_t) nFrames * L * (helpers - 1) * small.histBins, bytes = (words + 64) * sizeof(int) + (size_t) nFrames * L * sizeof(int);
        int rcH = ensure(c, c->dOctHist, bytes);
        if (rcH) return rcH;
        // The counters only grow -- by helpers - 1 per launch, each of the nFrames * L that the launch addresses -- and are zeroed once per
        // layout.  The layout is everything that decides which counters a launch bumps and by how much: frames, helpers, bins and the
        // allocation (ensure() only ever reallocates to a larger size, which may come back at the same address).  words alone is not a
        // key: 6 frames x 5 helpers and 8 x 4 give the same (256 CUs, 8 levels), and after 8, 6, 8 frames counters 48..63 would lag
        // the target for good.  Everything behind the helpers' slices is cleared, not only the launch's counters (the slices are
        // written before they are read).
        const ygzf_ctx::OctHistLayout lay{nFrames, helpers, small.histBins, c->dOctHist.bytes};
        if (!(lay == c->octHistLayout) || c->octDoneTarget > (1 << 30)) {
            HIPCHECK(c, hipMemsetAsync((int *) c->dOctHist.p + words, 0, c->dOctHist.bytes - words * sizeof(int), c->stream));
            c->octHistLayout = lay;
            c->octDoneTarget = 0;
        }
        c->octDoneTarget += helpers - 1;
        a->gHist = (int *) c->dOctHist.p;       // (helpers only with a gHist: without one the launch has one workgroup per level)
        a->gDone = a->gHist + words;
    }
    a->doneTarget = c->octDoneTarget; a->spinBudget = c->pins.octHelperSpin;
    *helpersOut = helpers;
    return YGZF_OK;
}

// YGZF_DEBUG=oct: the phase clocks and counters k_octree left in odbg, and which plan ran.  smallHelpers: workgroups per (level, frame) of the
// small plan's launch (0: the geometry's own launches ran).  tools/oct_phases.py and the tests parse these lines.
static int report_octree(ygzf_ctx *c, int nFrames, int L, const long long *odbg, int smallHelpers) {
    const OctPlan &plan = c->oct;
    long long st[kOctDbgWords];
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, hipMemcpy(st, odbg, sizeof st, hipMemcpyDeviceToHost));
    for (int l = 0; l < L; l++)
        fprintf(stderr, "[ygzf octree lvl %d, 10ns ticks] prefix %lld keys %lld sort %lld bfs %lld final %lld  M=%lld n=%lld\n", l, st[l * 8 + 1] - st[l * 8],
                st[l * 8 + 2] - st[l * 8 + 1], st[l * 8 + 3] - st[l * 8 + 2], st[l * 8 + 4] - st[l * 8 + 3], st[l * 8 + 5] - st[l * 8 + 4], st[l * 8 + 6], st[l * 8 + 7]);
    for (int l = 0; l < L; l++) {   // the tree passes (-DYGZF_PHASE_CLOCK builds only): list size after the one-wave head, after every full pass (+) and every expand round (-), ticks since the passes began
        const long long *ev = st + 16 * 8 + 16 + l * 16;
        if (!ev[1]) continue;
        fprintf(stderr, "[ygzf octree lvl %d passes]", l);
        for (int k = 0; k < 8 && ev[2 * k + 1]; k++) fprintf(stderr, " %+lld@%lld", ev[2 * k], ev[2 * k + 1] - st[l * 8 + 3]);
        fprintf(stderr, "\n");
    }
    if (plan.kind == OctPlan::Hist) {   // (printed for every geometry that has histogram groups, also when the small plan ran the launch)
        fprintf(stderr, "[ygzf octree histogram plan: %zu launches;", plan.launches.size());
        for (const auto &grp : plan.launches) fprintf(stderr, " levels %d-%d cap %d bins %d lds %zu;", grp.l0, grp.l0 + grp.n - 1, grp.cap, grp.histBins, grp.lds);
        fprintf(stderr, " workgroups of %d frames that fell back to the sort, per level:", nFrames);
        for (int l = 0; l < L; l++) fprintf(stderr, " %lld", st[16 * 8 + l]);
        fprintf(stderr, "]\n");
    }
    if (!smallHelpers && plan.kind == OctPlan::SortGroups) {   // (a level of frame 0 whose M above exceeds its launch's candidate budget sorted through global memory)
        fprintf(stderr, "[ygzf octree sort plan: %zu launches;", plan.launches.size());
        for (const auto &grp : plan.launches)
            fprintf(stderr, " levels %d-%d threads %d cap %d candidates %d lds %zu;", grp.l0, grp.l0 + grp.n - 1, grp.block, grp.cap, grp.ldsCand, grp.lds);
        fprintf(stderr, "]\n");
    }
    if (!smallHelpers && plan.kind == OctPlan::SortOne) {
        const OctLaunch &one = plan.launches[0];
        fprintf(stderr, "[ygzf octree single launch: levels 0-%d cap %d candidates %d lds %zu node arrays in %s]\n", L - 1, one.cap, one.ldsCand, one.lds,
                one.arena ? "the arena" : "lds");
    }
    if (!smallHelpers && plan.kind != OctPlan::Hist) {   // (a line of its own: the two above are parsed by their launch lists)
        const bool prefix = c->pins.octSortPrefix && !plan.launches[0].arena;
        fprintf(stderr, "[ygzf octree key order: %s; workgroups of %d frames that started over with the full sort, per level:", prefix ? "prefix" : "full", nFrames);
        for (int l = 0; l < L; l++) fprintf(stderr, " %lld", st[16 * 8 + l]);
        fprintf(stderr, "]\n");
    }
    if (smallHelpers) {
        fprintf(stderr, "[ygzf octree small plan: %d frames, %d workgroups per level; workgroups 0 that gave up waiting for their helpers, per level:", nFrames, smallHelpers);
        for (int l = 0; l < L; l++) fprintf(stderr, " %lld", st[kOctDbgAlone + l]);
        fprintf(stderr, "; frames mask 0x%llx]\n", (unsigned long long) st[kOctDbgAloneFrames]);
    }
    return YGZF_OK;
}

// The launch sequence of one extraction: carry, pyramid, FAST, octree, describe.
// pyramidReady: dPyr already holds the pyramid of the frame to extract (ygzf_compute_pyramid / ygzf_extract_resident) -- the previous
// extraction's pyramid is gone from it: the pyramid carry of ygzf_align_batch_prev is what ygzf_compute_pyramid saved before overwriting dPyr
// (in extract-ahead mode; none otherwise).
int run_extract(ygzf_ctx *c, const FrameSet &fs, int nFrames, bool pyramidReady) {
    const Geometry &G = c->geo;
    pyramid_taken(c);
    const int L = c->tab.cfg.nlevels;
    int rc;
    // slot 0 of the output arrays carries the last frame of the previous batch (Last frame of pair 0 in ygzf_match_batch_prev); frame f goes to slot f + 1
    queue_carry(c, false);
    ygzf_kp *outKp = (ygzf_kp *) c->dOutKp.p + G.kpStride;
    uint8_t *outDesc = (uint8_t *) c->dOutDesc.p + (size_t) G.kpStride * 32;
    int *outCnt = (int *) c->dOutCnt.p + 1;
    if (!pyramidReady && ((rc = save_carry_pyramid(c)) || (rc = pyramid_chain(c, fs, nFrames)) || (rc = mark_pyramid_done(c)))) return rc;
    if (G.totalCells > 0) {
        bool iniFirst = false, collect = false;
        fast_threshold_plan(c, &iniFirst, &collect);
        const FastChoice fast = choose_fast(G, c->fastKernel, c->pins, c->cuCount, nFrames, fast_lds_bytes(fast_wave_lds(kTabPitch, G.fastWinRows, G.fastSmapRows, G.fastQuadCap), kFastPersistWaves));
        if ((rc = launch_fast(c, fs, nFrames, fast, iniFirst, collect))) return rc;
        long long *odbg = nullptr;
        if (c->octDebug) {
            if ((rc = ensure_scratch(c, c->tmp.a, kOctDbgWords * sizeof(long long)))) return rc;
            odbg = (long long *) c->tmp.a.p;
            HIPCHECK(c, hipMemsetAsync(odbg, 0, kOctDbgWords * sizeof(long long), c->stream));
        }
        // launches of a few frames take the small plan (all levels in one histogram-plan launch, with helper workgroups), every other one the geometry's launches
        int smallHelpers = 0;
        {
            ProfScope ps(c, KK_OCTREE);
            if (c->oct.haveSmall && nFrames * L <= c->octSmallWgs) {
                const OctLaunch &grp = c->oct.small;
                OctArgs a = oct_args(c, grp, odbg);
                if ((rc = arm_oct_helpers(c, nFrames, L, grp, &a, &smallHelpers))) return rc;
                launch_octree(c->stream, a, grp.n, nFrames, grp.lds, grp.block, smallHelpers);
            } else
                for (const OctLaunch &grp : c->oct.launches) launch_octree(c->stream, oct_args(c, grp, odbg), grp.n, nFrames, grp.lds, grp.block, 1);
        }
        if (odbg && (rc = report_octree(c, nFrames, L, odbg, smallHelpers))) return rc;
        {
            ProfScope ps(c, KK_DESCRIBE);
            launch_describe(c->stream, fs, (const LevelGeom *) c->dGeom.p, L, (const int *) c->dLvlCnt.p, (int *) c->dLvlBase.p, (const uint2 *) c->dProcOrder.p, G.kpStride,
                            outKp, outDesc, outCnt, G.kpStride, nFrames, c->tab.cfg.cv_mode);
        }
    } else {
        HIPCHECK(c, hipMemsetAsync(outCnt, 0, sizeof(int) * nFrames, c->stream));
        HIPCHECK(c, hipMemsetAsync(c->dLvlCnt.p, 0, sizeof(int) * nFrames * L, c->stream));
        HIPCHECK(c, hipMemsetAsync(c->dLvlCand.p, 0, sizeof(int) * nFrames * L, c->stream));
    }
    HIPCHECK(c, hipGetLastError());
    extracted(c, fs, nFrames);
    return YGZF_OK;
}

// `rows` rows of `w` bytes from host memory (row pitch srcPitch) into a pitched device image.  The copy engine executes a pitched copy whose
// width or pitches are not multiples of 4 row by row (measured: 2.6-3.3 ms for one 1241x376 or 641x479 frame); such images travel as ONE
// linear copy into a landing buffer and are re-pitched by a kernel.
int upload_rows(ygzf_ctx *c, void *dst, size_t dstPitch, const uint8_t *src, size_t srcPitch, int w, size_t rows) {
    if (rows == 0 || w <= 0) return YGZF_OK;
    if ((w & 3) == 0 && (srcPitch & 3) == 0 && (dstPitch & 3) == 0 && ((uintptr_t) src & 3) == 0) {
        HIPCHECK(c, hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, (size_t) w, rows, hipMemcpyHostToDevice, c->stream));
        return YGZF_OK;
    }
    const size_t bytes = (rows - 1) * srcPitch + (size_t) w;
    int rc = ensure(c, c->dUpStage, bytes + 64);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpyAsync(c->dUpStage.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    launch_repitch_rows(c->stream, (const uint8_t *) c->dUpStage.p, srcPitch, (uint8_t *) dst, dstPitch, w, rows);
    HIPCHECK(c, hipGetLastError());
    return YGZF_OK;
}

int upload_frames(ygzf_ctx *c, const uint8_t *imgs, int nFrames, int w, int h, int row_pitch, size_t frame_stride,
                         FrameSet *fs) {
    forget_image(c);
    const int pitch = align_up(w, 64);
    int rc = ensure(c, c->dImg0, (size_t) nFrames * pitch * h);
    if (rc) return rc;
    *fs = own_frames(c, w, h);
    if (nFrames == 1) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        bool pageable = true;
        if (hipPointerGetAttributes(&at, imgs) == hipSuccess) pageable = at.type != hipMemoryTypeHost && at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged;
        else (void) hipGetLastError();
        if (!pageable && at.type == hipMemoryTypeHost && at.devicePointer && (size_t) w * h <= c->uploadKernelBytes) {
            // a page-locked frame of a Tracking-sized call: a kernel reads it over the link where it lies (ygzf_extract_batch_host_frames says why)
            HostFrameList L;
            L.addr[0] = (unsigned long long) (uintptr_t) at.devicePointer;
            launch_gather_host_frames(c->stream, L, 1, (size_t) row_pitch, (uint8_t *) c->dImg0.p, (size_t) pitch, (size_t) pitch * h, w, h);
            HIPCHECK(c, hipGetLastError());
            return YGZF_OK;
        }
        if (pageable) {
            const size_t bytes = (size_t) w * h;
            if (bytes > c->hInBytes) {
                if (c->evInPending) { HIPCHECK(c, hipEventSynchronize(c->evIn)); c->evInPending = false; }
                if (c->hIn) HIPCHECK(c, hipHostFree(c->hIn));
                c->hIn = nullptr;
                c->hInBytes = 0;
                HIPCHECK(c, hipHostMalloc((void **) &c->hIn, bytes + 64, hipHostMallocMapped));
                HIPCHECK(c, hipHostGetDevicePointer(&c->hInDev, c->hIn, 0));
                c->hInBytes = bytes;
            }
            if (!c->evIn) HIPCHECK(c, hipEventCreateWithFlags(&c->evIn, hipEventDisableTiming));
            if (c->evInPending) { HIPCHECK(c, hipEventSynchronize(c->evIn)); c->evInPending = false; }   // the previous upload's kernel has read the buffer
            if (row_pitch == w) memcpy(c->hIn, imgs, bytes);
            else for (int y = 0; y < h; y++) memcpy(c->hIn + (size_t) y * w, imgs + (size_t) y * row_pitch, (size_t) w);
            HostFrameList L;
            L.addr[0] = (unsigned long long) (uintptr_t) c->hInDev;
            launch_gather_host_frames(c->stream, L, 1, (size_t) w, (uint8_t *) c->dImg0.p, (size_t) pitch, (size_t) pitch * h, w, h);
            HIPCHECK(c, hipGetLastError());
            HIPCHECK(c, hipEventRecord(c->evIn, c->stream));
            c->evInPending = true;
            return YGZF_OK;
        }
    }
    // Host frames that already carry the device's row pitch (ygzf_host_row_pitch): the copy engine pays per ROW of a pitched copy whose source rows
    // are not multiples of 64 bytes (752-byte rows: 48 GB/s where 1920-byte rows reach 55), so a whole frame -- (h - 1) x pitch + w bytes, padding
    // included -- is handed to it as ONE row (runs of 8 / 60 image rows measured the same: profiles/r05_a_h2d_shapes.txt)
    if (row_pitch == pitch && (nFrames == 1 || frame_stride >= (size_t) pitch * h) && ((uintptr_t) imgs & 3) == 0 && (w & 3) == 0 &&
        (frame_stride & 3) == 0) {
        const size_t fsd = (size_t) pitch * h, fss = nFrames == 1 ? fsd : frame_stride;
        HIPCHECK(c, hipMemcpy2DAsync(c->dImg0.p, fsd, imgs, fss, (size_t) (h - 1) * pitch + w, (size_t) nFrames, hipMemcpyHostToDevice, c->stream));
    } else if (nFrames == 1 || frame_stride == (size_t) row_pitch * h) {   // frames back to back: one copy of nFrames * h rows
        if ((rc = upload_rows(c, c->dImg0.p, (size_t) pitch, imgs, (size_t) row_pitch, w, (size_t) nFrames * h))) return rc;
    } else {
        for (int f = 0; f < nFrames; f++) {
            // (the landing buffer is reused: stream order keeps frame f's re-pitch ahead of frame f + 1's copy)
            if ((rc = upload_rows(c, (uint8_t *) c->dImg0.p + (size_t) f * pitch * h, (size_t) pitch, imgs + f * frame_stride, (size_t) row_pitch, w, (size_t) h)))
                return rc;
        }
    }
    return YGZF_OK;
}

// The rest of ygzf_compute_pyramid once level 0 of the one frame lies in fs: the pyramid chain, the levels' way back, the queued extraction.
// hostLevel0: the caller's image IS level 0 (rows `stride` apart): it is copied on the host while the other levels are on the link; null: level 0 was
// made on the device (ygzf_compute_pyramid_remapped) and comes back with them.
int pyramid_readback(ygzf_ctx *c, const FrameSet &fs, int w, int h, const uint8_t *hostLevel0, int stride, uint8_t *const *levels_out) {
    int rc;
    const uint8_t *img = hostLevel0;
    const int first = hostLevel0 ? 1 : 0;
    const Geometry &G = c->geo;
    const int L = c->tab.cfg.nlevels;
    if ((rc = pyramid_chain(c, fs, 1)) || (rc = mark_pyramid_done(c))) return rc;
    HIPCHECK(c, hipGetLastError());
    // The levels go back tight (pitch = width) into caller memory that is pageable as a rule (cv::Mat buffers).  Eight pitched device-to-host
    // copies took 10-13 ms for a 752x480 pyramid (the copy engine works an odd-width pitched copy off row by row, into page-locked memory
    // as well): the levels are packed on the device and leave in one linear copy through the context's page-locked staging buffer.
    // Level 0 IS the caller's image: it is copied on the host while the other levels are on the link.
    unsigned offs[kMaxLevels + 1];
    offs[0] = 0;
    offs[1] = first ? 0u : (unsigned) w * (unsigned) h;
    for (int l = 1; l < L; l++) offs[l + 1] = offs[l] + (unsigned) G.lv[l].w * (unsigned) G.lv[l].h;
    const size_t total = offs[L];
    if ((rc = ensure_stage(c, total + 64)) || (rc = ensure_scratch(c, c->tmp.c, total + 64))) return rc;
    // (the page-locked staging area as the device addresses it: the packing kernel -- 16-byte stores -- writes the levels over the link itself, on the
    // stream the copy would have taken; a byte-per-thread packing kernel doing so was slower than the copy engine: ComputePyramid 94 -> 97 us)
    const bool linkPack = c->hStageDev != nullptr && c->linkKernels && c->pyrLink;
    if (!linkPack) {
        launch_pack_levels(c->stream, fs, (const LevelGeom *) c->dGeom.p, first, L, offs, (uint8_t *) c->tmp.c.p);
        HIPCHECK(c, hipGetLastError());
    }
    // extract-ahead: FAST / octree / descriptors of this image are queued behind the pyramid now and run while the levels travel back on
    // the copy stream and the caller works on them (a Frame constructor clones them); ygzf_extract_resident then only collects the results.
    // (Measured alternatives: the copy on the context's own stream with an event behind it and the extraction queued after that event --
    // the event is reported 30 us later than on a stream that ends there; two half copies to overlap the host's copy-out -- slower too.)
    hipStream_t rd = c->stream;
    bool ahead = false;
    if (c->extractAhead && c->streamCopy) {
        HIPCHECK(c, hipEventRecord(c->evPyramid, c->stream));
        HIPCHECK(c, hipStreamWaitEvent(c->streamCopy, c->evPyramid, 0));
        rd = c->streamCopy;
        ahead = true;
    }
    if (total && linkPack) {
        launch_pack_levels(rd, fs, (const LevelGeom *) c->dGeom.p, first, L, offs, (uint8_t *) c->hStageDev);
        HIPCHECK(c, hipGetLastError());
    } else if (total) HIPCHECK(c, hipMemcpyAsync(c->hStage, c->tmp.c.p, total, hipMemcpyDeviceToHost, rd));
    if (ahead && (rc = run_extract(c, fs, 1, true))) return rc;   // (queued after the copy so that the copy starts while these launches are issued)
    if (img && (levels_out[0] != img || stride != w))
        for (int y = 0; y < h; y++) memcpy(levels_out[0] + (size_t) y * w, img + (size_t) y * stride, (size_t) w);
    HIPCHECK(c, hipStreamSynchronize(rd));
    for (int l = first; l < L; l++) memcpy(levels_out[l], c->hStage + offs[l], offs[l + 1] - offs[l]);
    pyramid_computed(c, w, h, ahead);
    return YGZF_OK;
}

extern "C" {

int ygzf_create(int device, const ygzf_extractor_cfg *cfg, int max_width, int max_height, int max_batch, ygzf_ctx **out) {
    if (!cfg || !out) return fail(nullptr, YGZF_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 0 || !(cfg->scale_factor > 1.0f) || cfg->ini_th_fast < 0 ||
        cfg->min_th_fast < 0 || cfg->ini_th_fast > 255 || cfg->min_th_fast > 255 || cfg->min_th_fast > cfg->ini_th_fast)
        return fail(nullptr, YGZF_ERR_INVALID, "bad extractor configuration (nlevels 1..%d, scale_factor > 1, 0 <= minTh <= iniTh <= 255)",
                    kMaxLevels);
    if (cfg->cv_mode < YGZF_CV_LEGACY_SSE2 || cfg->cv_mode > YGZF_CV_4) return fail(nullptr, YGZF_ERR_INVALID, "cv_mode %d (0 legacy SSE2, 1 legacy integer, 2 OpenCV >= 3.4.11 / 4.x)", cfg->cv_mode);
    if (max_width < 1 || max_height < 1 || max_batch < 1) return fail(nullptr, YGZF_ERR_INVALID, "bad maximum sizes");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, YGZF_ERR_NO_DEVICE, "no HIP device available (%s): libygzf has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, YGZF_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
    ygzf_ctx *c = new ygzf_ctx();
    c->device = device;
    c->maxW = max_width;
    c->maxH = max_height;
    c->maxBatch = max_batch;
    c->tab.init(*cfg);
    auto bail = [&](int rc) {
        g_create_err = c->err;   // thread-local
        ygzf_destroy(c);
        return rc;
    };
#define CK(expr)                                                                                                   \
    do {                                                                                                           \
        hipError_t _e = (expr);                                                                                    \
        if (_e != hipSuccess) {                                                                                    \
            fail(c, YGZF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));                                  \
            return bail(YGZF_ERR_HIP);                                                                             \
        }                                                                                                          \
    } while (0)
    CK(hipSetDevice(device));
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {
        int cus = 0;
        CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        c->cuCount = cus > 0 ? cus : 256;
    }
    CK(hipEventCreate(&c->tStart));
    CK(hipEventCreate(&c->tStop));
    CK(upload_constants(c->tab.umax));
    CK(hipHostMalloc((void **) &c->hFastStats, kFastStatWords * sizeof(unsigned)));
    memset(c->hFastStats, 0, kFastStatWords * sizeof(unsigned));
#undef CK
    // validate the largest configuration up front (and size the buffers once)
    int rc = apply_geometry(c, max_width, max_height, max_batch);
    if (rc) return bail(rc);
    *out = c;
    return YGZF_OK;
}

void ygzf_destroy(ygzf_ctx *c) {
    if (!c) return;
    (void) hipSetDevice(c->device);
    if (c->stream) (void) hipStreamSynchronize(c->stream);
    if (c->hFastStats) (void) hipHostFree(c->hFastStats);
    if (c->hStage) (void) hipHostFree(c->hStage);
    if (c->hIn) (void) hipHostFree(c->hIn);
    if (c->evIn) (void) hipEventDestroy(c->evIn);
    for (auto &r : c->recs) { (void) hipEventDestroy(r.a); (void) hipEventDestroy(r.b); }
    for (auto e : c->pool) (void) hipEventDestroy(e);
    pyr_chain_graph_destroy(&c->pyrGraph);
    if (c->evShare) (void) hipEventDestroy(c->evShare);
    if (c->evPyrDone) (void) hipEventDestroy(c->evPyrDone);
    if (c->evPyramid) (void) hipEventDestroy(c->evPyramid);
    if (c->streamCopy) (void) hipStreamDestroy(c->streamCopy);
    if (c->tStart) (void) hipEventDestroy(c->tStart);
    if (c->tStop) (void) hipEventDestroy(c->tStop);
    if (c->stream) (void) hipStreamDestroy(c->stream);
    if (c->fill) fprintf(stderr, "[ygzf] fill: %llu allocations, %llu scratch refills, %llu bytes\n", c->fillStats.allocs, c->fillStats.refills, c->fillStats.bytes);
    delete c;   // every Buf frees itself here: on the device selected above, with the stream drained
}

const char *ygzf_last_error(const ygzf_ctx *c) {
    if (c) return c->err.c_str();
    return g_create_err.c_str();
}

int ygzf_device_mem_info(ygzf_ctx *c, size_t *free_bytes, size_t *total_bytes) {
    if (!c || !free_bytes || !total_bytes) return fail(c, YGZF_ERR_INVALID, "null argument");
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, hipMemGetInfo(free_bytes, total_bytes));
    return YGZF_OK;
}

int ygzf_set_fast_plan(ygzf_ctx *c, int plan) {
    if (!c) return YGZF_ERR_INVALID;
    if (plan < YGZF_FAST_PLAN_AUTO || plan > YGZF_FAST_PLAN_INI_FIRST) return fail(c, YGZF_ERR_INVALID, "FAST plan %d (0 auto, 1 one pass, 2 iniTh first)", plan);
    c->fastPlan = plan;
    return YGZF_OK;
}

int ygzf_get_fast_stats(const ygzf_ctx *c, float *corner_quads_per_pass, float *passes_per_cell) {
    if (!c) return YGZF_ERR_INVALID;
    if (corner_quads_per_pass) *corner_quads_per_pass = (float) c->fastCornerQuadsPerRun;
    if (passes_per_cell) *passes_per_cell = (float) c->fastRunsPerCell;
    return YGZF_OK;
}

int ygzf_phase_clocks(ygzf_ctx *c, int kernel, unsigned long long *out16, int reset) {
    if (!c || !out16 || kernel < 0 || kernel > 1) return YGZF_ERR_INVALID;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    const hipError_t e = phase_clocks_read(kernel, out16, reset != 0);
    if (e == hipErrorNotSupported) return fail(c, YGZF_ERR_INVALID, "this library was built without -DYGZF_PHASE_CLOCK (python -m orb_ygz_slam_amd.build --phase-clock)");
    HIPCHECK(c, e);
    return YGZF_OK;
}

int ygzf_set_fast_kernel(ygzf_ctx *c, int kernel) {
    if (!c) return YGZF_ERR_INVALID;
    if (kernel < YGZF_FAST_KERNEL_AUTO || kernel > YGZF_FAST_KERNEL_CELL_TABLE) return fail(c, YGZF_ERR_INVALID, "FAST kernel %d (0 auto, 1 register staging, 2 cell table + LDS-DMA)", kernel);
    c->fastKernel = kernel;
    return YGZF_OK;
}

int ygzf_set_carry_previous(ygzf_ctx *c, int on) {
    if (!c) return YGZF_ERR_INVALID;
    c->carryOff = !on;
    return YGZF_OK;
}

int ygzf_set_extract_ahead(ygzf_ctx *c, int on) {
    if (!c) return YGZF_ERR_INVALID;
    HIPCHECK(c, hipSetDevice(c->device));
    if (on && !c->streamCopy) {
        HIPCHECK(c, hipStreamCreateWithFlags(&c->streamCopy, hipStreamNonBlocking));
        HIPCHECK(c, hipEventCreateWithFlags(&c->evPyramid, hipEventDisableTiming));
    }
    c->extractAhead = on != 0;
    if (!on) ahead_dropped(c);
    return YGZF_OK;
}

int ygzf_get_fast_plan(const ygzf_ctx *c, int *plan) {
    if (!c || !plan) return YGZF_ERR_INVALID;
    *plan = c->fastPlan == YGZF_FAST_PLAN_AUTO ? (c->fastIniFirst ? YGZF_FAST_PLAN_INI_FIRST : YGZF_FAST_PLAN_ONE_PASS) : c->fastPlan;
    return YGZF_OK;
}

int ygzf_get_levels(const ygzf_ctx *c) { return c ? c->tab.cfg.nlevels : YGZF_ERR_INVALID; }

int ygzf_get_scale_tables(const ygzf_ctx *c, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2) {
    if (!c) return YGZF_ERR_INVALID;
    const size_t n = sizeof(float) * c->tab.cfg.nlevels;
    if (scale) memcpy(scale, c->tab.scale.data(), n);
    if (inv_scale) memcpy(inv_scale, c->tab.invScale.data(), n);
    if (sigma2) memcpy(sigma2, c->tab.sigma2.data(), n);
    if (inv_sigma2) memcpy(inv_sigma2, c->tab.invSigma2.data(), n);
    return YGZF_OK;
}

int ygzf_get_features_per_level(const ygzf_ctx *c, int *nfeat) {
    if (!c || !nfeat) return YGZF_ERR_INVALID;
    memcpy(nfeat, c->tab.nFeat.data(), sizeof(int) * c->tab.cfg.nlevels);
    return YGZF_OK;
}

int ygzf_level_size(const ygzf_ctx *c, int w, int h, int level, int *lw, int *lh) {
    if (!c || !lw || !lh || level < 0 || level >= c->tab.cfg.nlevels) return YGZF_ERR_INVALID;
    c->tab.levelSize(w, h, level, lw, lh);
    return YGZF_OK;
}

int ygzf_host_row_pitch(int w) { return w > 0 ? align_up(w, 64) : YGZF_ERR_INVALID; }

int ygzf_max_keypoints(const ygzf_ctx *c_, int w, int h) {
    ygzf_ctx *c = const_cast<ygzf_ctx *>(c_);
    if (!c) return YGZF_ERR_INVALID;
    if (c->geo.w == w && c->geo.h == h) return c->geo.kpStride;
    Geometry G;
    std::string msg;
    const int rc = build_geometry(c->tab, c->pins, w, h, G, &msg);
    return rc ? fail(c, rc, "%s", msg.c_str()) : G.kpStride;
}

int ygzf_sync(ygzf_ctx *c) {
    if (!c) return YGZF_ERR_INVALID;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_compute_pyramid(ygzf_ctx *c, const uint8_t *img, int w, int h, int stride, uint8_t *const *levels_out) {
    if (!c || !img || !levels_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = apply_geometry(c, w, h, 1);
    if (rc) return rc;
    FrameSet fs;
    // extract-ahead counts as an extraction for ygzf_align_batch_prev: the previous extraction's last pyramid (the reference image of pair 0)
    // leaves dPyr before this frame's pyramid is written over it
    if (c->extractAhead && c->streamCopy && (rc = save_carry_pyramid(c))) return rc;
    if ((rc = upload_frames(c, img, 1, w, h, stride, 0, &fs))) return rc;
    return pyramid_readback(c, fs, w, h, img, stride, levels_out);
}

int ygzf_extract_batch_device(ygzf_ctx *c, const uint8_t *d_imgs, int n_frames, int w, int h, int row_pitch, size_t frame_stride) {
    if (!c || !d_imgs) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (row_pitch < w) return fail(c, YGZF_ERR_INVALID, "row_pitch %d < width %d", row_pitch, w);
    if (((uintptr_t) d_imgs & 3) || (row_pitch & 3) || (frame_stride & 3))
        return fail(c, YGZF_ERR_UNSUPPORTED, "device frames must be 4-byte aligned (base pointer, row_pitch and frame_stride multiples of 4)");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = apply_geometry(c, w, h, n_frames);
    if (rc) return rc;
    FrameSet fs;
    fs.img0 = d_imgs;
    fs.img0_stride = (long long) frame_stride;
    fs.img0_pitch = row_pitch;
    fs.pyr = (uint8_t *) c->dPyr.p;
    fs.pyr_stride = c->geo.pyrBytes;
    return run_extract(c, fs, n_frames);
}

int ygzf_extract_batch_host(ygzf_ctx *c, const uint8_t *imgs, int n_frames, int w, int h, int row_pitch, size_t frame_stride) {
    if (!c || !imgs) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (row_pitch < w) return fail(c, YGZF_ERR_INVALID, "row_pitch %d < width %d", row_pitch, w);
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = apply_geometry(c, w, h, n_frames);
    if (rc) return rc;
    queue_carry(c, true);
    FrameSet fs;
    if ((rc = upload_frames(c, imgs, n_frames, w, h, row_pitch, frame_stride, &fs))) return rc;
    return run_extract(c, fs, n_frames);
}

// The same from a list of frame pointers (frames that do not sit at one stride: the rows of an array of cv::Mat, a round-robin share of a
// larger clip).  Each frame is one (asynchronous, when the memory is page-locked) copy on the context's stream; the call returns once the
// extraction is queued, like ygzf_extract_batch_host.
int ygzf_extract_batch_host_frames(ygzf_ctx *c, const uint8_t *const *frames, int n_frames, int w, int h, int row_pitch) {
    if (!c || !frames) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n_frames < 1) return fail(c, YGZF_ERR_INVALID, "no frames");
    if (row_pitch < w) return fail(c, YGZF_ERR_INVALID, "row_pitch %d < width %d", row_pitch, w);
    for (int f = 0; f < n_frames; f++)
        if (!frames[f]) return fail(c, YGZF_ERR_INVALID, "frame %d is null", f);
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = apply_geometry(c, w, h, n_frames);
    if (rc) return rc;
    queue_carry(c, true);
    forget_image(c);
    const int pitch = align_up(w, 64);
    if ((rc = ensure(c, c->dImg0, (size_t) n_frames * pitch * h))) return rc;
    {
        // Into a tight staging buffer with the copy engine's fast paths, then ONE launch per 128 frames that lays the rows out at the context's
        // pitch.  Frames that come as runs of u back-to-back frames at one distance S (a device slot's round-robin share of a tight clip: units of u
        // frames, S = slots x u frames) go up as ONE two-dimensional copy whose "rows" are the runs; anything else as one linear copy per frame.
        // ONE page-locked frame (a Tracking-sized call): a kernel reads it over the link where it lies.  The copy engine starts ~10 us after the copy
        // is queued and hands over to the first kernel ~8 us after it ends; a kernel's launch and hand-over are a third of that.
        if (n_frames <= c->uploadKernelFrames && (size_t) n_frames * w * h <= c->uploadKernelBytes) {
            HostFrameList L;
            bool mapped = true;
            for (int f = 0; f < n_frames && mapped; f++) {
                hipPointerAttribute_t at;
                memset(&at, 0, sizeof at);
                mapped = hipPointerGetAttributes(&at, frames[f]) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer != nullptr;
                if (!mapped) (void) hipGetLastError();
                L.addr[f] = (unsigned long long) (uintptr_t) at.devicePointer;
            }
            if (mapped) {
                launch_gather_host_frames(c->stream, L, n_frames, (size_t) row_pitch, (uint8_t *) c->dImg0.p, (size_t) pitch, (size_t) pitch * h, w, h);
                HIPCHECK(c, hipGetLastError());
                goto uploaded;
            }
        }
        const size_t frameBytes = (size_t) (h - 1) * row_pitch + w;
        const size_t tight = (size_t) h * row_pitch;
        int u = n_frames;
        for (int f = 1; f < n_frames; f++)
            if (frames[f] != frames[f - 1] + tight) { u = f; break; }
        const int runs = n_frames / u;
        bool regular = n_frames % u == 0;
        ptrdiff_t S = 0;
        if (regular && runs > 1) {
            S = frames[u] - frames[0];
            regular = S > 0 && (size_t) S >= (size_t) u * tight;
            for (int f = 0; f < n_frames && regular; f++) regular = frames[f] == frames[0] + (ptrdiff_t) (f / u) * S + (ptrdiff_t) (f % u) * (ptrdiff_t) tight;
        }
        if (regular && row_pitch == pitch && (w & 3) == 0 && ((uintptr_t) frames[0] & 3) == 0 && (S & 3) == 0) {
            // frames that carry the device's pitch (ygzf_host_row_pitch; tight frames whose width is a multiple of 64 -- 640, 1920, 3840 -- do so by
            // themselves): the runs go straight to their place, no staging and no re-pitch launch
            const size_t width = (size_t) u * tight - (size_t) (pitch - w);
            HIPCHECK(c, hipMemcpy2DAsync(c->dImg0.p, (size_t) u * tight, frames[0], runs > 1 ? (size_t) S : (size_t) u * tight, width, (size_t) runs, hipMemcpyHostToDevice, c->stream));
            goto uploaded;
        }
        regular = regular && row_pitch == w;
        const size_t slot = regular ? tight : ((frameBytes + 255) & ~(size_t) 255);
        if ((rc = ensure(c, c->dUpStage, slot * n_frames + 64))) return rc;
        if (regular) {
            if (runs > 1) HIPCHECK(c, hipMemcpy2DAsync(c->dUpStage.p, (size_t) u * tight, frames[0], (size_t) S, (size_t) u * tight, (size_t) runs, hipMemcpyHostToDevice, c->stream));
            else HIPCHECK(c, hipMemcpyAsync(c->dUpStage.p, frames[0], (size_t) n_frames * tight, hipMemcpyHostToDevice, c->stream));
        }
        for (int f0 = 0; f0 < n_frames; f0 += kHostFrameListMax) {
            HostFrameList L;
            const int nf = std::min(kHostFrameListMax, n_frames - f0);
            for (int f = 0; f < nf; f++) {
                uint8_t *d = (uint8_t *) c->dUpStage.p + slot * (size_t) (f0 + f);
                if (!regular) HIPCHECK(c, hipMemcpyAsync(d, frames[f0 + f], frameBytes, hipMemcpyHostToDevice, c->stream));
                L.addr[f] = (unsigned long long) (uintptr_t) d;
            }
            launch_gather_host_frames(c->stream, L, nf, (size_t) row_pitch, (uint8_t *) c->dImg0.p + (size_t) f0 * pitch * h, (size_t) pitch, (size_t) pitch * h, w, h);
        }
        HIPCHECK(c, hipGetLastError());
    }
uploaded:
    return run_extract(c, own_frames(c, w, h), n_frames);
}

int ygzf_batch_counts(ygzf_ctx *c, int *n_kp) {
    if (!c || !n_kp) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    HIPCHECK(c, hipMemcpyAsync(n_kp, (int *) c->dOutCnt.p + 1, sizeof(int) * c->held.frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_batch_fetch(ygzf_ctx *c, int frame, ygzf_kp *kps, uint8_t *desc, int cap, int *n_out) {
    if (!c || !n_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    if (frame < 0 || frame >= c->held.frames) return fail(c, YGZF_ERR_INVALID, "frame %d out of range", frame);
    int n = 0;
    HIPCHECK(c, hipMemcpyAsync(&n, (int *) c->dOutCnt.p + frame + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    *n_out = n;
    if (n == 0) return YGZF_OK;
    if (n > cap || !kps || !desc) return fail(c, YGZF_ERR_INVALID, "capacity %d < %d keypoints", cap, n);
    const size_t base = (size_t) (frame + 1) * c->geo.kpStride;
    HIPCHECK(c, hipMemcpyAsync(kps, (ygzf_kp *) c->dOutKp.p + base, sizeof(ygzf_kp) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(desc, (uint8_t *) c->dOutDesc.p + base * 32, (size_t) 32 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_batch_fetch_all(ygzf_ctx *c, ygzf_kp *kps, uint8_t *desc, int *n_kp, int stride) {
    if (!c || !kps || !desc || !n_kp) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    if (stride < c->geo.kpStride) return fail(c, YGZF_ERR_INVALID, "stride %d < %d (ygzf_max_keypoints)", stride, c->geo.kpStride);
    const int B = c->held.frames, ks = c->geo.kpStride;
    HIPCHECK(c, hipMemcpyAsync(n_kp, (int *) c->dOutCnt.p + 1, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    // slot f + 1 holds frame f; rows of `stride` keypoints on the host side, kpStride on the device side
    HIPCHECK(c, hipMemcpy2DAsync(kps, sizeof(ygzf_kp) * (size_t) stride, (ygzf_kp *) c->dOutKp.p + ks, sizeof(ygzf_kp) * (size_t) ks,
                                 sizeof(ygzf_kp) * (size_t) ks, B, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpy2DAsync(desc, 32 * (size_t) stride, (uint8_t *) c->dOutDesc.p + 32 * (size_t) ks, 32 * (size_t) ks, 32 * (size_t) ks, B,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

// queues the gather kernel and the ONE copy of ygzf_batch_fetch_packed on the context's stream; the caller synchronises
int queue_packed_fetch(ygzf_ctx *c, void *host, size_t host_bytes, size_t *off_kps, size_t *off_desc, int *row_entries, size_t *bytes_out) {
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    const size_t B = (size_t) c->held.frames, ks = (size_t) c->geo.kpStride;
    const size_t oK = (B * sizeof(int) + 255) & ~(size_t) 255, oD = oK + ((B * ks * sizeof(ygzf_kp) + 255) & ~(size_t) 255), total = oD + B * ks * 32;
    if (total > host_bytes) return fail(c, YGZF_ERR_INVALID, "packed results need %zu bytes, %zu given", total, host_bytes);
    if (total >= (1ull << 32)) return fail(c, YGZF_ERR_UNSUPPORTED, "packed results of %zu bytes: use ygzf_batch_fetch_all", total);
    // page-locked memory the device can address: the gather kernel writes the block over the link itself (no copy-engine start-up / hand-over)
    void *direct = nullptr;
    if (c->linkKernels) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, host) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer && ((uintptr_t) at.devicePointer & 3) == 0) direct = at.devicePointer;
        else (void) hipGetLastError();
    }
    int rc = direct ? YGZF_OK : ensure(c, c->dResPack, total + 256);
    if (rc) return rc;
    launch_pack_results(c->stream, (const int *) c->dOutCnt.p + 1, (const ygzf_kp *) c->dOutKp.p + ks, (const uint8_t *) c->dOutDesc.p + ks * 32, (int) B, (int) ks,
                        direct ? direct : c->dResPack.p, oK, oD);
    HIPCHECK(c, hipGetLastError());
    if (!direct) HIPCHECK(c, hipMemcpyAsync(host, c->dResPack.p, total, hipMemcpyDeviceToHost, c->stream));
    *off_kps = oK;
    *off_desc = oD;
    *row_entries = (int) ks;
    if (bytes_out) *bytes_out = total;
    return YGZF_OK;
}

int ygzf_batch_fetch_packed(ygzf_ctx *c, void *host, size_t host_bytes, size_t *off_kps, size_t *off_desc, int *row_entries, size_t *bytes_out) {
    if (!c || !host || !off_kps || !off_desc || !row_entries) return fail(c, YGZF_ERR_INVALID, "null argument");
    int rc = queue_packed_fetch(c, host, host_bytes, off_kps, off_desc, row_entries, bytes_out);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

// One stereo pair from host memory with its two eyes on TWO contexts / streams of the same device (ygzf_mgpu_extract_stereo for a slot that is handed
// exactly one pair: BASELINE.json's 3840x2160 configuration, a pair per GPU).  In one context the pair is one upload of both frames followed by one
// kernel chain: 16.6 MB on the link (300 us) during which no kernel of the pair can run.  Here the right eye's upload waits for the LEFT eye's upload
// only, so it crosses the link while the left eye's pyramid / FAST / octree / descriptors run; the right eye's chain then overlaps the left one's
// tail; ComputeStereoMatches runs on the left context's stream once both are done, reading the right eye's keypoints, descriptors and pyramid where
// the right context left them.  Same kernels on the same inputs: the bytes of ygzf_extract_batch_host(both frames) + ygzf_stereo_batch.
int ygzf_stereo_pair_host(ygzf_ctx *l, ygzf_ctx *r, const uint8_t *left, const uint8_t *right, int w, int h, int row_pitch, float mb, float mbf,
                          void *host_left, void *host_right, size_t host_bytes, size_t *off_kps, size_t *off_desc, int *row_entries,
                          float *u_right, float *depth) {
    if (!l || !r || l == r || !left || !right || !host_left || !host_right || !off_kps || !off_desc || !row_entries || !u_right || !depth)
        return fail(l, YGZF_ERR_INVALID, "null argument");
    if (l->device != r->device) return fail(l, YGZF_ERR_INVALID, "the two contexts of a pair must be on one device");
    if (row_pitch < w) return fail(l, YGZF_ERR_INVALID, "row_pitch %d < width %d", row_pitch, w);
    HIPCHECK(l, hipSetDevice(l->device));
    int rc;
    if ((rc = apply_geometry(l, w, h, 1))) return rc;
    if ((rc = apply_geometry(r, w, h, 1))) { l->err = r->err; return rc; }
    if (!l->evShare) HIPCHECK(l, hipEventCreateWithFlags(&l->evShare, hipEventDisableTiming));
    if (!r->evShare) HIPCHECK(l, hipEventCreateWithFlags(&r->evShare, hipEventDisableTiming));
    queue_carry(l, true);
    queue_carry(r, true);
    FrameSet fl, fr;
    if ((rc = upload_frames(l, left, 1, w, h, row_pitch, 0, &fl))) return rc;
    HIPCHECK(l, hipEventRecord(l->evShare, l->stream));                 // the left eye is on the device ...
    HIPCHECK(l, hipStreamWaitEvent(r->stream, l->evShare, 0));          // ... and only then does the right eye take the link
    if ((rc = upload_frames(r, right, 1, w, h, row_pitch, 0, &fr))) { l->err = r->err; return rc; }
    if ((rc = run_extract(l, fl, 1))) return rc;
    if ((rc = run_extract(r, fr, 1))) { l->err = r->err; return rc; }
    HIPCHECK(l, hipEventRecord(r->evShare, r->stream));
    size_t ok2 = 0, od2 = 0;
    int re2 = 0;
    if ((rc = queue_packed_fetch(r, host_right, host_bytes, &ok2, &od2, &re2, nullptr))) { l->err = r->err; return rc; }
    if ((rc = queue_packed_fetch(l, host_left, host_bytes, off_kps, off_desc, row_entries, nullptr))) return rc;
    HIPCHECK(l, hipStreamWaitEvent(l->stream, r->evShare, 0));
    if ((rc = stereo_across(l, r, mb, mbf))) return rc;
    const size_t ks = (size_t) l->geo.kpStride;
    HIPCHECK(l, hipMemcpyAsync(u_right, l->st.uRight.p, 4 * ks, hipMemcpyDeviceToHost, l->stream));
    HIPCHECK(l, hipMemcpyAsync(depth, l->st.depth.p, 4 * ks, hipMemcpyDeviceToHost, l->stream));
    HIPCHECK(l, hipStreamSynchronize(r->stream));
    HIPCHECK(l, hipStreamSynchronize(l->stream));
    return YGZF_OK;
}

// Results of frame 0 of a one-frame extraction with ONE synchronisation: the count and the frame's whole keypoint / descriptor rows (kpStride
// entries, ~60 KB: a microsecond on the link) come back together through the page-locked staging area, the first n entries go on to the
// caller.  ygzf_batch_fetch reads the count, waits, then copies exactly n entries and waits again: two host wake-ups of 10-20 us each, which
// is what a Tracking thread's ORBextractor::operator() spent beside 74 us of kernels.
static int fetch_frame0_packed(ygzf_ctx *c, ygzf_kp *kps, uint8_t *desc, int cap, int *n_out) {
    const size_t ks = (size_t) c->geo.kpStride;
    if (ks == 0) { *n_out = 0; return YGZF_OK; }
    const size_t oK = 256, oD = oK + ((ks * sizeof(ygzf_kp) + 255) & ~(size_t) 255), total = oD + ks * 32;
    int rc = ensure_stage(c, total + 256);
    if (rc) return rc;
    if (c->hStageDev && c->linkKernels) {
        // count, keypoint row and descriptor row written into the page-locked staging area by a kernel, over the link: three copies by the copy engine
        // start ~10 us after they are queued and the last one hands back ~8 us after it ends -- a launch does neither
        launch_pack_results(c->stream, (const int *) c->dOutCnt.p + 1, (const ygzf_kp *) c->dOutKp.p + ks, (const uint8_t *) c->dOutDesc.p + ks * 32, 1, (int) ks, c->hStageDev, oK, oD);
        HIPCHECK(c, hipGetLastError());
    } else {
        HIPCHECK(c, hipMemcpyAsync(c->hStage, (int *) c->dOutCnt.p + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipMemcpyAsync(c->hStage + oK, (ygzf_kp *) c->dOutKp.p + ks, ks * sizeof(ygzf_kp), hipMemcpyDeviceToHost, c->stream));   // slot 1 = frame 0
        HIPCHECK(c, hipMemcpyAsync(c->hStage + oD, (uint8_t *) c->dOutDesc.p + ks * 32, ks * 32, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    const int n = *(const int *) c->hStage;
    *n_out = n;
    if (n == 0) return YGZF_OK;
    if (n > cap || !kps || !desc) return fail(c, YGZF_ERR_INVALID, "capacity %d < %d keypoints", cap, n);
    memcpy(kps, c->hStage + oK, sizeof(ygzf_kp) * (size_t) n);
    memcpy(desc, c->hStage + oD, (size_t) 32 * n);
    return YGZF_OK;
}

int ygzf_extract(ygzf_ctx *c, const uint8_t *img, int w, int h, int stride, ygzf_kp *kps, uint8_t *desc, int cap, int *n_out) {
    if (!c || !n_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    *n_out = 0;
    if (!img || w <= 0 || h <= 0) return YGZF_OK;  // reference: `if (_image.empty()) return;`
    int rc = ygzf_extract_batch_host(c, img, 1, w, h, stride, 0);
    if (rc) return rc;
    return fetch_frame0_packed(c, kps, desc, cap, n_out);
}

int ygzf_extract_resident(ygzf_ctx *c, ygzf_kp *kps, uint8_t *desc, int cap, int *n_out) {
    if (!c || !n_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    *n_out = 0;
    if (!pyramid_resident(c)) return fail(c, YGZF_ERR_STATE, "no resident pyramid (ygzf_compute_pyramid must be the context's previous image operation)");
    HIPCHECK(c, hipSetDevice(c->device));
    const int w = c->held.w, h = c->held.h;
    int rc = apply_geometry(c, w, h, 1);   // same geometry as the compute_pyramid call: no reallocation
    if (rc) return rc;
    if (c->held.image == Held::PyramidAhead) pyramid_taken(c);   // queued by ygzf_compute_pyramid (ygzf_set_extract_ahead): nothing to launch
    else if ((rc = run_extract(c, own_frames(c, w, h), 1, true))) return rc;
    return fetch_frame0_packed(c, kps, desc, cap, n_out);
}

int ygzf_batch_fetch_level(ygzf_ctx *c, int frame, int level, uint8_t *out) {
    if (!c || !out) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    if (frame < 0 || frame >= c->held.frames || level < 0 || level >= c->tab.cfg.nlevels) return fail(c, YGZF_ERR_INVALID, "bad frame/level");
    int pitch;
    const LevelGeom &g = c->geo.lv[level];
    const uint8_t *p = level_ptr(c->held.fs, g, level, frame, &pitch);
    // packed on the device, then one linear copy (a pitched copy of an odd-width level is executed row by row)
    const size_t bytes = (size_t) g.w * g.h;
    int rc = ensure_scratch(c, c->tmp.c, bytes + 64);
    if (rc) return rc;
    launch_repitch_rows(c->stream, p, (size_t) pitch, (uint8_t *) c->tmp.c.p, (size_t) g.w, g.w, (size_t) g.h);
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(out, c->tmp.c.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_batch_fetch_candidates(ygzf_ctx *c, int frame, int level, int *xs, int *ys, int *scores, int cap, int *n_out) {
    if (!c || !n_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    if (frame < 0 || frame >= c->held.frames || level < 0 || level >= c->tab.cfg.nlevels) return fail(c, YGZF_ERR_INVALID, "bad frame/level");
    const Geometry &G = c->geo;
    const LevelGeom &g = G.lv[level];
    const int nc = g.nCols * g.nRows;
    *n_out = 0;
    if (nc == 0) return YGZF_OK;
    std::vector<unsigned short> cnt(nc);
    std::vector<unsigned> sl((size_t) nc * g.slotCap);
    HIPCHECK(c, hipMemcpyAsync(cnt.data(), (unsigned short *) c->dCellCnt.p + (size_t) frame * G.totalCells + g.cellBase,
                               sizeof(unsigned short) * nc, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(sl.data(), (unsigned *) c->dSlots.p + (size_t) frame * G.totalSlots + g.slotBase,
                               sizeof(unsigned) * sl.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    int n = 0;
    for (int ci = 0; ci < nc; ci++) {
        const int i = ci / g.nCols, j = ci % g.nCols;
        for (int k = 0; k < cnt[ci]; k++, n++) {
            if (n < cap && xs && ys && scores) {
                const unsigned e = sl[(size_t) ci * g.slotCap + k];
                xs[n] = (int) (e & 255u) + j * g.wCell;
                ys[n] = (int) ((e >> 8) & 255u) + i * g.hCell;
                scores[n] = (int) (e >> 16);
            }
        }
    }
    *n_out = n;
    return n > cap ? fail(c, YGZF_ERR_INVALID, "capacity %d < %d candidates", cap, n) : YGZF_OK;
}

int ygzf_batch_fetch_level_keypoints(ygzf_ctx *c, int frame, int level, int *xs, int *ys, int *scores, int cap, int *n_out) {
    if (!c || !n_out) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (c->held.frames < 1) return fail(c, YGZF_ERR_STATE, "no extracted batch");
    const int L = c->tab.cfg.nlevels;
    if (frame < 0 || frame >= c->held.frames || level < 0 || level >= L) return fail(c, YGZF_ERR_INVALID, "bad frame/level");
    const Geometry &G = c->geo;
    const LevelGeom &g = G.lv[level];
    int n = 0;
    HIPCHECK(c, hipMemcpyAsync(&n, (int *) c->dLvlCnt.p + frame * L + level, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    *n_out = n;
    if (n == 0) return YGZF_OK;
    if (n > cap) return fail(c, YGZF_ERR_INVALID, "capacity %d < %d keypoints", cap, n);
    std::vector<unsigned> xy(n);
    std::vector<unsigned char> sc(n);
    const size_t base = (size_t) frame * G.kpStride + g.kpBase;
    HIPCHECK(c, hipMemcpyAsync(xy.data(), (unsigned *) c->dLvlXY.p + base, sizeof(unsigned) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipMemcpyAsync(sc.data(), (unsigned char *) c->dLvlScore.p + base, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) {
        xs[i] = (int) (xy[i] & 0xFFFFu);
        ys[i] = (int) (xy[i] >> 16);
        scores[i] = sc[i];
    }
    return YGZF_OK;
}

int ygzf_descriptor_distance(ygzf_ctx *c, const uint8_t *a, const uint8_t *b, int n, int *dist) {
    if (!c || !a || !b || !dist || n < 0) return fail(c, YGZF_ERR_INVALID, "null argument");
    if (n == 0) return YGZF_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc;
    if ((size_t) n * 68 <= kPackedMax) {   // a frame's worth of pairs: one packed copy each way
        PackedTransfer P(c);
        const size_t iA = P.add_in(a, (size_t) n * 32), iB = P.add_in(b, (size_t) n * 32), oD = P.add_out(dist, (size_t) n * sizeof(int));
        uint8_t *d;
        if ((rc = P.upload(&d))) return rc;
        {
            ProfScope ps(c, KK_HAMMING);
            launch_hamming_pairs(c->stream, d + iA, d + iB, n, (int *) P.d_out(oD));
        }
        HIPCHECK(c, hipGetLastError());
        return P.download();
    }
    if ((rc = ensure_scratch(c, c->tmp.a, (size_t) n * 32)) || (rc = ensure_scratch(c, c->tmp.b, (size_t) n * 32)) ||
        (rc = ensure_scratch(c, c->tmp.c, (size_t) n * sizeof(int))))
        return rc;
    HIPCHECK(c, hipMemcpyAsync(c->tmp.a.p, a, (size_t) n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(c, hipMemcpyAsync(c->tmp.b.p, b, (size_t) n * 32, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, KK_HAMMING);
        launch_hamming_pairs(c->stream, c->tmp.a.p, c->tmp.b.p, n, (int *) c->tmp.c.p);
    }
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(dist, c->tmp.c.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return YGZF_OK;
}

int ygzf_timer_start(ygzf_ctx *c) {
    if (!c) return YGZF_ERR_INVALID;
    HIPCHECK(c, hipEventRecord(c->tStart, c->stream));
    return YGZF_OK;
}

int ygzf_timer_stop(ygzf_ctx *c, float *elapsed_ms) {
    if (!c || !elapsed_ms) return YGZF_ERR_INVALID;
    HIPCHECK(c, hipEventRecord(c->tStop, c->stream));
    HIPCHECK(c, hipEventSynchronize(c->tStop));
    HIPCHECK(c, hipEventElapsedTime(elapsed_ms, c->tStart, c->tStop));
    return YGZF_OK;
}

int ygzf_profile_enable(ygzf_ctx *c, int on) {
    if (!c) return YGZF_ERR_INVALID;
    drain_profile(c);
    c->profile = on != 0;
    return YGZF_OK;
}

int ygzf_profile_read(ygzf_ctx *c, const char **names, float *total_ms, int *launches, int cap) {
    if (!c) return YGZF_ERR_INVALID;
    drain_profile(c);
    for (int k = 0; k < KK_COUNT && k < cap; k++) {
        if (names) names[k] = kKernelNames[k];
        if (total_ms) total_ms[k] = c->profMs[k];
        if (launches) launches[k] = c->profN[k];
    }
    return KK_COUNT;
}

int ygzf_profile_reset(ygzf_ctx *c) {
    if (!c) return YGZF_ERR_INVALID;
    drain_profile(c);
    for (int k = 0; k < KK_COUNT; k++) { c->profMs[k] = 0; c->profN[k] = 0; }
    return YGZF_OK;
}

void *ygzf_stream(ygzf_ctx *c) { return c ? (void *) c->stream : nullptr; }

}  // extern "C"
