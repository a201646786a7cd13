// ygzf_plan.hip -- the extractor's launch plans as host arithmetic (ygzf_plan.h).  No kernel, no runtime call, no environment of its own (the entry points at the end take the pins from PlanPins::from_env()): this file links into a
// stand-alone program without the device library (tests/cpp/extract_plan_cpu.hip runs it under the host sanitizers).
#include "ygzf_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace ygzf {

int cv_round_host(double v) { return (int) std::nearbyint(v); }  // cvRound: round half to even

// ORBextractor::ORBextractor, reference src/ORBextractor.cc:412-470 (scale tables, per-level quota, umax)
void Tables::init(const ygzf_extractor_cfg &c) {
    cfg = c;
    const int L = c.nlevels;
    scale.assign(L, 1.f);
    sigma2.assign(L, 1.f);
    invScale.assign(L, 1.f);
    invSigma2.assign(L, 1.f);
    for (int i = 1; i < L; i++) {
        scale[i] = scale[i - 1] * c.scale_factor;
        sigma2[i] = scale[i] * scale[i];
    }
    for (int i = 0; i < L; i++) {
        invScale[i] = 1.0f / scale[i];
        invSigma2[i] = 1.0f / sigma2[i];
    }
    nFeat.assign(L, 0);
    const float factor = 1.0f / c.scale_factor;
    float want = c.nfeatures * (1 - factor) / (1 - (float) std::pow((double) factor, (double) L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        nFeat[l] = cv_round_host(want);
        sum += nFeat[l];
        want *= factor;
    }
    nFeat[L - 1] = std::max(c.nfeatures - sum, 0);
    // circular patch row ends (:455-469)
    int v, v0;
    const int vmax = (int) std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int) std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (v = 0; v <= vmax; ++v) umax[v] = cv_round_host(std::sqrt(hp2 - v * v));
    for (v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
}

void Tables::levelSize(int w, int h, int level, int *lw, int *lh) const {  // :1131-1132
    const float s = invScale[level];
    *lw = cv_round_host((float) w * s);
    *lh = cv_round_host((float) h * s);
}

static inline short sat_short(float v) {
    int i = cv_round_host((double) v);
    return (short) (i < -32768 ? -32768 : i > 32767 ? 32767 : i);
}

static int plan_fail(std::string *err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

// Per-(w,h) geometry: level sizes, resize coefficient tables (cv::resize INTER_LINEAR fixed point, restated from the
// OpenCV 2.4/3.2 algorithm: fx = (float)((dx+0.5)*scale - 0.5), 11-bit coefficients), FAST cell grid (:733-745),
// octree root layout (:537-557) and buffer offsets.
// Row ranges of k_pyr_strips (extract_kernels.hip): the last level is cut into S strips; walking up, a strip needs of level l the source
// rows of the rows it produces of level l + 1 (yofs is monotone: first row's sy .. last row's sy + 1, clamped as the kernel clamps) and
// owns the S-th part of every level.  S grows until the two LDS regions (even / odd levels) fit.
static bool plan_pyr_strips_from(Geometry &G, int L, int base, bool only32, int minS) {
    if (L - base < 3) return false;
    if (G.lv[base].h >= 65536) return false;   // the strip plan packs row ranges into 16-bit fields: taller images keep one launch per level
    for (int l = base + 1; l < L; l++)
        if (G.lv[l].area2x || !G.lv[l].tiledOk || (G.lv[l].w + 3) / 4 > kPyrStripMaxThreads) return false;
    // 752x480, one frame: 16 strips 148 us per resident extraction, 24 146, 32 144, 48 143 (the halo rows grow with the strip count: 1.23 x
    // the pixels of the pyramid at 16); eight frames: 16 strips 218 us, 32 215
    // (more strips when the LDS regions do not fit, fewer for images whose last level has fewer than 64 rows).
    const int candidates[] = {32, 48, 64, 16, 8};
    // (minS: at least this many strips -- PlanPins::pyrStrips)
    for (int S : candidates) {
        if (S < minS) continue;
        if (only32 && S != 32) continue;
        if (G.lv[L - 1].h < 2 * S) continue;
        std::vector<PyrStripPlan> plan(S);
        size_t bytes[2] = {0, 0};
        int maxRows = 0;
        for (int s = 0; s < S; s++) {
            int rows = 0, pca = 0, pcb = 0;   // the range produced of the level below the one in hand
            PyrStripPlan &p = plan[s];
            std::memset(&p, 0, sizeof p);
            for (int l = L - 1; l >= base; l--) {
                const int hl = G.lv[l].h;
                int wa = (int) ((long long) hl * s / S), wb = (int) ((long long) hl * (s + 1) / S), ca = wa, cb = wb;
                if (l < L - 1) {
                    const LevelGeom &n = G.lv[l + 1];
                    const int na = std::min(std::max(G.yofs[n.ytab + pca], 0), hl - 1);
                    const int nb = std::min(std::max(G.yofs[n.ytab + pcb - 1] + 1, 0), hl - 1) + 1;
                    if (l == base) { ca = na; cb = nb; wa = wb = 0; }   // the base level is staged, not produced
                    else { ca = std::min(wa, na); cb = std::max(wb, nb); }
                }
                p.lv[l] = make_uint2((unsigned) ca | ((unsigned) cb << 16), (unsigned) wa | ((unsigned) wb << 16));
                pca = ca; pcb = cb;
                bytes[(l - base) & 1] = std::max(bytes[(l - base) & 1], (size_t) (cb - ca) * pyr_strip_lds_pitch(G.lv[l].w));
                if (l > base) rows += cb - ca;
            }
            maxRows = std::max(maxRows, rows);
        }
        if (maxRows > kPyrStripMaxThreads) continue;   // one thread per row fills the row table
        const size_t rowBytes = ((size_t) maxRows * 8 + 15) & ~(size_t) 15, head = rowBytes;   // (the column coefficients stay in global memory: k_pyr_strips)
        const size_t a = (bytes[0] + 16 + 15) & ~(size_t) 15, b = (bytes[1] + 16 + 15) & ~(size_t) 15;   // hrow reads up to 11 bytes past a row's pixels
        if (head + a + b > 160 * 1024) continue;
        G.pyrPlan = plan;
        G.pyrBase = base;
        G.pyrStripOffA = (int) head;
        G.pyrStripOffB = (int) (head + a);
        G.pyrStripLds = head + a + b;
        std::memset(G.pyrLevels, 0, sizeof G.pyrLevels);
        for (int l = 0; l < L; l++) {
            const LevelGeom &g = G.lv[l];
            G.pyrLevels[l] = PyrStripLevel{g.w, g.h, g.pitch, g.xtab, g.ytab, 0, (long long) g.off};
        }
        return true;
    }
    return false;
}

// The whole chain from the image when that fits LDS; otherwise (3840x2160: a strip of the last level would need 270 KB of level 0) the first levels
// come from k_pyr_resize_tiled, one launch each, and the strips start from the first level whose chain fits -- a one-frame call then pays 3-4
// launches instead of 11.  YGZF_FORCE=pyr_strip_base=s: not below level s (tests).
static void plan_pyr_strips(Geometry &G, int L, const PlanPins &pins) {
    G.pyrPlan.clear();
    G.pyrBase = 0;
    // (a 3840x2160 pair, same box: from level 3 with 48 strips 0.774 ms -- and two clusters of calls, 0.72 and 0.78 --, from level 4 with 32 strips 0.710,
    // from level 5 / 6 / 9 0.76 / 0.75 / 0.75: above the image the plan of 32 strips is preferred to an earlier level with more)
    const int first = pins.pyrStripBase;
    if (first == 0 && plan_pyr_strips_from(G, L, 0, false, pins.pyrStrips)) return;
    for (int base = std::max(first, 1); base + 3 <= L; base++)
        if (plan_pyr_strips_from(G, L, base, true, pins.pyrStrips)) return;
    for (int base = std::max(first, 1); base + 3 <= L; base++)
        if (plan_pyr_strips_from(G, L, base, false, pins.pyrStrips)) return;
}

int build_geometry(const Tables &T, const PlanPins &pins, int w, int h, Geometry &G, std::string *err) {
    const int L = T.cfg.nlevels;
    G = Geometry();
    G.w = w;
    G.h = h;
    G.lv.assign(L, LevelGeom());
    long long off = 0, slotBase = 0, candBase = 0;
    int cellBase = 0, kpBase = 0, groupBase = 0;
    for (int l = 0; l < L; l++) {
        LevelGeom &g = G.lv[l];
        memset(&g, 0, sizeof g);
        T.levelSize(w, h, l, &g.w, &g.h);
        if (g.w < 1 || g.h < 1) return plan_fail(err, YGZF_ERR_UNSUPPORTED, "pyramid level %d of a %dx%d image is empty", l, w, h);
        if (g.w > 4096 + 2 * kBorder || g.h > 4096 + 2 * kBorder)
            return plan_fail(err, YGZF_ERR_UNSUPPORTED, "level %d is %dx%d: larger than 4128 px is not supported", l, g.w, g.h);
        g.pitch = align_up(g.w, 64);
        g.scale = T.scale[l];
        g.kpSize = (float) (int) (kPatchSize * T.scale[l]);  // :789 int truncation of a float product
        g.nFeat = T.nFeat[l];
        if (l > 0) {
            g.off = off;
            off += (long long) g.pitch * g.h;
            const LevelGeom &s = G.lv[l - 1];
            g.area2x = (s.w == 2 * g.w && s.h == 2 * g.h);
            g.xtab = (int) G.xofs.size();
            g.ytab = (int) G.yofs.size();
            const double scale_x = 1. / ((double) g.w / s.w), scale_y = 1. / ((double) g.h / s.h);
            for (int dx = 0; dx < g.w; dx++) {
                float fx = (float) ((dx + 0.5) * scale_x - 0.5);
                int sx = (int) std::floor(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                if (sx >= s.w - 1) { fx = 0; sx = s.w - 1; }
                G.xofs.push_back(sx);
                G.xalpha.push_back(sat_short((1.f - fx) * 2048));
                G.xalpha.push_back(sat_short(fx * 2048));
            }
            for (int dy = 0; dy < g.h; dy++) {
                float fy = (float) ((dy + 0.5) * scale_y - 0.5);
                int sy = (int) std::floor(fy);
                fy -= sy;
                G.yofs.push_back(sy);
                G.ybeta.push_back(sat_short((1.f - fy) * 2048));
                G.ybeta.push_back(sat_short(fy * 2048));
            }
            // k_pyr_resize_tiled's tables.  A level is cut into tiles of 8192 output pixels: 256-column tiles of 32 rows while >= 225 columns
            // remain, then the rest in binary pieces of 128 / 64 / 32 columns whose waves fold 2 / 4 / 8 rows into one pass.  True for the
            // usual scale factors (<= ~1.27): steeper pyramids (a tile's source region would not fit the staging area) take the per-pixel kernel.
            g.tiledOk = 1;
            g.pyrCol = (int) G.pyrCols.size();
            g.pyrRow = (int) G.pyrRows.size();
            g.pyrTile = (int) G.pyrTiles.size();
            for (int xb = 0; xb < g.w; xb += 4) {
                PyrColRec r;
                memset(&r, 0, sizeof r);
                r.sx0 = G.xofs[g.xtab + xb];
                for (int k = 0; k < 4; k++) {
                    const int x = std::min(xb + k, g.w - 1);
                    const int sx = G.xofs[g.xtab + x], sx1 = std::min(sx + 1, s.w - 1);
                    if (sx1 - r.sx0 > 7 || sx < r.sx0) g.tiledOk = 0;   // the pair of every column comes out of the eight bytes from sx0 on
                    r.sel[k] = (unsigned) ((sx - r.sx0) & 7) | 0x0C00u | ((unsigned) ((sx1 - r.sx0) & 7) << 16) | 0x0C000000u;
                    r.ap[k] = (unsigned) (unsigned short) G.xalpha[2 * (g.xtab + x)] | ((unsigned) (unsigned short) G.xalpha[2 * (g.xtab + x) + 1] << 16);
                    if (G.xalpha[2 * (g.xtab + x)] < 0 || G.xalpha[2 * (g.xtab + x) + 1] < 0) g.tiledOk = 0;
                }
                G.pyrCols.push_back(r);
            }
            for (int y = 0; y < g.h; y++) {
                const int sy = G.yofs[g.ytab + y];
                const int r0 = std::min(std::max(sy, 0), s.h - 1), r1 = std::min(std::max(sy + 1, 0), s.h - 1);
                const int b0 = G.ybeta[2 * (g.ytab + y)], b1 = G.ybeta[2 * (g.ytab + y) + 1];
                if (b0 < 0 || b1 < 0 || b0 > 2048 || b1 > 2048 || s.h > 65535) g.tiledOk = 0;
                G.pyrRows.push_back(PyrRowRec{(unsigned) r0 | ((unsigned) r1 << 16), (unsigned) b0 << 12, (unsigned) b1 << 12, 0u});
            }
            for (int p = 1; p < 8; p++) G.pyrRows.push_back(G.pyrRows.back());   // a wave reads the records of its 8 rows in one go
            for (int x0 = 0; x0 < g.w && g.tiledOk;) {
                const int rest = g.w - x0;
                int fl = 0;   // fold: the widest piece of the binary decomposition of the rest, in units of 32 columns
                if (rest <= 224) {
                    const int units = (rest + 31) / 32;
                    fl = units >= 4 ? 1 : units >= 2 ? 2 : 3;
                }
                const int tw = 256 >> fl, th = kPyrTileRows << fl;
                const int xl = std::min(x0 + tw, g.w) - 1;
                const int sxa = G.xofs[g.xtab + x0] & ~3, sxb = std::min(G.xofs[g.xtab + xl] + 1, s.w - 1);
                const int nc = (sxb - sxa) / 16 + 1;
                if (nc > pyr_fold_chunks(fl) || sxa > 65535) g.tiledOk = 0;
                for (int y0 = 0; y0 < g.h && g.tiledOk; y0 += th) {
                    const int yl = std::min(y0 + th, g.h) - 1;
                    const int sya = (int) (G.pyrRows[g.pyrRow + y0].r01 & 0xffffu), syb = (int) (G.pyrRows[g.pyrRow + yl].r01 >> 16);
                    if (syb - sya + 1 > pyr_fold_rows(fl) || syb < sya) g.tiledOk = 0;
                    G.pyrTiles.push_back(PyrTileRec{(unsigned short) x0, (unsigned short) y0, (unsigned short) sxa, (unsigned char) nc, (unsigned char) fl});
                }
                x0 += tw;
            }
            g.nPyrTiles = (int) G.pyrTiles.size() - g.pyrTile;
        }
        // FAST cells
        g.maxBorderX = g.w - kEdgeThreshold + 3;
        g.maxBorderY = g.h - kEdgeThreshold + 3;
        const float width = (float) (g.maxBorderX - kBorder), height = (float) (g.maxBorderY - kBorder);
        g.regW = g.maxBorderX - kBorder;
        g.regH = g.maxBorderY - kBorder;
        int nCols = width > 0 ? (int) (width / 30.f) : 0, nRows = height > 0 ? (int) (height / 30.f) : 0;
        if (nCols < 1 || nRows < 1) nCols = nRows = 0;  // reference: division by zero (UB) -> defined as "no keypoints"
        g.nCols = nCols;
        g.nRows = nRows;
        g.cellBase = cellBase;
        g.groupBase = groupBase;
        g.slotBase = slotBase;
        g.candBase = candBase;
        g.kpBase = kpBase;
        if (nCols) {
            g.wCell = (int) std::ceil(width / nCols);
            g.hCell = (int) std::ceil(height / nRows);
            g.slotCap = ((g.wCell + 1) / 2) * ((g.hCell + 1) / 2);
            const int nc = nCols * nRows;
            cellBase += nc;
            groupBase += ((nCols + 1) / 2) * ((nRows + 1) / 2);
            G.fastSmapRows = std::max(G.fastSmapRows, g.hCell + 2);
            G.fastWinPitch = std::max(G.fastWinPitch, (g.wCell + 6 + 1 + 3) / 4 * 4);   // per-wave window of k_fast_quads: column 0 unused
            G.fastWinRows = std::max(G.fastWinRows, g.hCell + 6);
            G.fastQuadCap = std::max(G.fastQuadCap, ((g.wCell + 3) / 4 * g.hCell + 3) / 4 * 4);
            G.fastWCellMax = std::max(G.fastWCellMax, g.wCell);
            slotBase += (long long) nc * g.slotCap;
            g.candCap = nc * g.slotCap;
            candBase += g.candCap;
            G.maxCellsPerLevel = std::max(G.maxCellsPerLevel, nc);
            // octree roots
            int nIni = (int) std::round((float) g.regW / (float) g.regH);
            if (nIni < 1) nIni = 1;  // reference: UB for tall-narrow regions; defined as one root
            g.nIni = nIni;
            g.hX = (float) g.regW / nIni;
            int rootW = 1;
            for (int i = 0; i < nIni; i++)
                rootW = std::max(rootW, (int) (g.hX * (float) (i + 1)) - (int) (g.hX * (float) i));
            int D = 1;
            while ((1 << D) < std::max(std::max(rootW, g.regH), 2)) D++;
            g.depth = D + 1;
            int rootBits = 0;
            while ((1 << rootBits) < nIni) rootBits++;
            g.keyBits = rootBits + 2 * g.depth;
            if (g.keyBits > 32) return plan_fail(err, YGZF_ERR_UNSUPPORTED, "octree path key needs %d bits at level %d", g.keyBits, l);
            g.kpCap = std::max(g.nFeat + 3, 4 * nIni) + 1;
            // k_octree's work records carry the list position in 16 bits (score | position << 8 | level << 24)
            if (g.kpCap > 65535) return plan_fail(err, YGZF_ERR_UNSUPPORTED, "level %d would keep up to %d keypoints (at most 65535 per level)", l, g.kpCap);
        } else {
            g.nIni = 1;
            g.hX = 1.f;
            g.kpCap = 0;
        }
        kpBase += g.kpCap;
        G.kpCapMax = std::max(G.kpCapMax, (g.kpCap + 3) & ~3);   // (a multiple of 4: k_octree's per-node arrays stay 16-byte aligned)
    }
    G.pyrBytes = off;
    plan_pyr_strips(G, L, pins);
    G.totalCells = cellBase;
    G.totalGroups = groupBase;
    // per-cell records of k_fast_tab: the cell loop of ComputeKeyPointsOctTree (src/ORBextractor.cc:747-764) evaluated once per geometry
    G.fastCells.assign((size_t) groupBase * 4, FastCellRec{0, 0, 0, 0, 0, 0, 0, 0});
    for (int l = 0; l < L; l++) {
        const LevelGeom &g = G.lv[l];
        if (!g.nCols) continue;
        const int gCols = (g.nCols + 1) / 2;
        for (int ci = 0; ci < g.nRows; ci++)
            for (int cj = 0; cj < g.nCols; cj++) {
                FastCellRec &r = G.fastCells[(size_t) (g.groupBase + (ci / 2) * gCols + cj / 2) * 4 + (ci & 1) * 2 + (cj & 1)];
                const int cidx = ci * g.nCols + cj;
                const int iniX = kBorder + cj * g.wCell, iniY = kBorder + ci * g.hCell;
                const int maxX = std::min(iniX + g.wCell + 6, g.maxBorderX), maxY = std::min(iniY + g.hCell + 6, g.maxBorderY);
                const bool skip = (iniX >= g.maxBorderX - 6) || (iniY >= g.maxBorderY - 3);   // :751, :759
                const int dw = maxX - iniX - 6, dh = maxY - iniY - 6;
                const bool run = !skip && dw > 0 && dh > 0;
                r.xy = (unsigned) (iniX - 1) | ((unsigned) iniY << 16);
                r.geo = (unsigned) (l ? g.pitch : 0) | ((unsigned) (run ? dw : 0) << 16) | ((unsigned) (run ? dh : 0) << 24);
                r.flags = (unsigned) (run ? maxY - iniY : 0) | ((kFastCellExists | (run ? kFastCellRun : 0u)) << 8) | ((unsigned) l << 16);
                r.cell = (unsigned) (g.cellBase + cidx);
                r.slot = (unsigned) (g.slotBase + (long long) cidx * g.slotCap);
                r.off = (unsigned) g.off;
            }
    }
    G.totalSlots = slotBase;
    G.candStride = candBase;
    G.kpStride = kpBase;
    if (G.totalCells > 0 && (size_t) G.candStride > 0xFFFFFEull)
        return plan_fail(err, YGZF_ERR_UNSUPPORTED, "more than 2^24 candidate slots per frame");
    return YGZF_OK;
}

// ---- k_octree's dynamic LDS is oct_lds (lds_layout.h).  Its inverse for the sort plan: the candidates whose two pairs of sort buffers fit `budget` ----
int octree_lds_cand(int maxCellsPerLevel, int cap, size_t budget) {
    const long long region = oct_lds_region(maxCellsPerLevel, cap), ints = (long long) (budget / sizeof(int));
    long long c = ints / 4;                              // the second buffer wider than the region it lies over
    if (2 * c < region) c = (ints - region) / 2;         // ... or inside it
    c &= ~3ll;
    return c < 256 ? 0 : (int) std::min(c, 8192ll);
}

// Which octree plan a geometry takes -- NOT the budgets of the launches that run.  The per-list-position arrays (19 x cap ints) stay in LDS while one
// workgroup fits the CU; very large per-level feature budgets move them to a global arena.  ldsCand = the candidates one 1024-thread launch of all levels
// keeps in LDS at 16 bytes each ON TOP of the cell table and node arrays (the layout before the overlay, and still the layout of the global-arena
// launch): no such budget (or the global arena) -> the histogram plan.  This formula is kept as the plan choice's yardstick so that which geometries
// take the sort plan (and with it every hist-plan workload) stays where it was; it also sizes the one launch of the global-arena plan
// (OctPlan::SortOne).  The launches of the sort plan with LDS node arrays take plan_oct_sort's budgets (octree_lds_cand: the second sort
// buffer over the node arrays) -- a change to one formula does not move the other.
static void oct_sort_budget(const Geometry &G, bool *globalNodes, int *ldsCand) {
    *globalNodes = oct_lds_bytes(kOctLdsSort, G.maxCellsPerLevel, G.kpCapMax, 0, 0, 0) > 142 * 1024;
    const size_t fixed = oct_lds_bytes(*globalNodes ? kOctLdsArena : kOctLdsSort, G.maxCellsPerLevel, G.kpCapMax, 0, 0, 0);
    const size_t budget = (size_t) 71 * 1024;   // two workgroups per CU beside 9 KB of static LDS each (radix histogram)
    *ldsCand = fixed + 16 * 256 < budget ? (int) ((budget - fixed) / 16) : 0;
    if (*ldsCand > 8192) *ldsCand = 8192;
}

// The sort plan's launches.  Two 1024-thread workgroups of k_octree fill a CU's 32 wave slots whatever their LDS, so a level in such a workgroup
// leaves nothing beside it for the other contexts' FAST and describe waves.  Consecutive levels are launched together while their list caps stay
// within a factor of two of the group's first level; a group whose lists hold more than 256 nodes keeps 1024 threads and 71 KB, one of more than
// 128 nodes takes 512 threads and 44 KB, the rest 256 threads and 36 KB.  The candidates fit those budgets at 16 bytes each because their second sort
// buffer lies over the node arrays (k_octree): 2800 / 2300 of them -- what the levels of a 752x480 frame hold (up to ~2700 per level on the
// synthetic clip); a level that holds more sorts through global memory, same result.
std::vector<OctLaunch> plan_oct_sort(const Geometry &G, int L, bool oneGroup, int block, size_t ldsBytes) {
    std::vector<OctLaunch> out;
    auto finish = [&](OctLaunch grp, int cells) {
        if (grp.cap < 4) grp.cap = 4;
        const int b = block == 256 || block == 512 || block == 1024 ? block : grp.block;
        grp.block = b;
        const size_t budget = ldsBytes ? ldsBytes : (size_t) (b == 1024 ? 71 : b == 512 ? 44 : 36) * 1024;
        grp.ldsCand = octree_lds_cand(cells, grp.cap, budget);
        grp.lds = oct_lds_bytes(kOctLdsSort, cells, grp.cap, grp.ldsCand, 0, 0);
        out.push_back(grp);
    };
    if (oneGroup) {
        OctLaunch grp;
        grp.l0 = 0; grp.n = L; grp.cap = G.kpCapMax; grp.block = kOctBlock;
        finish(grp, G.maxCellsPerLevel);
        return out;
    }
    for (int l = 0; l < L;) {
        OctLaunch grp;
        grp.l0 = l;
        int cells = 0;
        for (; l < L && (grp.n == 0 || 2 * G.lv[l].kpCap > G.lv[grp.l0].kpCap); l++, grp.n++) {
            grp.cap = std::max(grp.cap, (G.lv[l].kpCap + 3) & ~3);
            cells = std::max(cells, G.lv[l].nCols * G.lv[l].nRows);
        }
        grp.block = grp.cap > 256 ? 1024 : grp.cap > 128 ? 512 : 256;
        finish(grp, cells);
    }
    return out;
}

// A histogram-plan launch of levels [l0, l0 + n): list capacity, the region the cell table, the key tables and the node arrays share, and the bins
// within 150 KB of LDS -- first the key tables go, then (unless binsEnv pins them) the bins are halved down to 1024.  The bins wanted: 8192, or with
// perNode sixteen per node the largest level may end with (a tree of N leaves rarely splits below the depth that offers 16 N cells; if it does, the
// level restarts on the sorting path) -- the prefix sum over 8192 bins was 3.3 of a level's 29 us, over 2048 it is 1.  False when the launch does not
// fit even so.
static bool size_oct_hist_group(const Geometry &G, int l0, int n, int binsEnv, bool perNode, OctLaunch *out) {
    OctLaunch grp;
    grp.l0 = l0;
    grp.n = n;
    int cells = 0, tabs = 0;
    for (int l = l0; l < l0 + n; l++) {
        const LevelGeom &g = G.lv[l];
        const int nc = g.nCols * g.nRows;
        grp.cap = std::max(grp.cap, (g.kpCap + 3) & ~3);
        cells = std::max(cells, nc + 1);
        if (nc > 0) tabs = std::max(tabs, nc + 1 + std::max(g.regW, g.nCols * g.wCell) + 9 + std::max(g.regH, g.nRows * g.hCell) + 9 + nc);
    }
    if (grp.cap < 4) grp.cap = 4;
    const size_t budget = 150 * 1024;
    int want = perNode ? 1024 : 8192;
    while (want < 16 * grp.cap && want < 8192) want *= 2;
    grp.histBins = binsEnv >= 4 && binsEnv <= 8192 ? binsEnv : want;
    grp.regionInts = std::max(std::max(kOctNodeArrays * grp.cap, cells), tabs);
    if (oct_lds_bytes(kOctLdsHist, 0, grp.cap, 0, grp.regionInts, grp.histBins) > budget) grp.regionInts = std::max(kOctNodeArrays * grp.cap, cells);   // keys without the tables
    while (grp.histBins > 1024 && !binsEnv && oct_lds_bytes(kOctLdsHist, 0, grp.cap, 0, grp.regionInts, grp.histBins) > budget) grp.histBins /= 2;
    grp.lds = oct_lds_bytes(kOctLdsHist, 0, grp.cap, 0, grp.regionInts, grp.histBins);
    *out = grp;
    return grp.lds <= budget;
}

// Everything one geometry's octree launches with.  (oct_plan=hist / sort pins one plan, oct_hist_bins bounds the histogram: the tests run every
// geometry through both plans and through the fall-back from one to the other.)
int plan_octree(const Geometry &G, int L, const PlanPins &pins, OctPlan &plan, std::string *err) {
    plan = OctPlan();
    bool arena = false;
    int ldsCand = 0;
    oct_sort_budget(G, &arena, &ldsCand);
    // Levels too large for LDS-resident candidate buffers (1920x1080 / 4000 and up) take the histogram plan: no sort, tree passes in LDS
    // (extract_kernels.hip, k_octree<.., kHist>).  Consecutive levels are launched together while their list caps stay within a factor of two of
    // the group's first level, so that the small levels do not reserve the LDS of the large ones.
    const bool wantHist = pins.octPlan == PlanPins::Hist ? true : pins.octPlan == PlanPins::Sort ? false : (arena || ldsCand == 0);
    if (wantHist) {
        bool ok = true;
        for (int l = 0; l < L && ok;) {
            int n = 1;
            while (l + n < L && 2 * G.lv[l + n].kpCap > G.lv[l].kpCap) n++;
            OctLaunch grp;
            ok = size_oct_hist_group(G, l, n, pins.octHistBins, false, &grp);
            plan.launches.push_back(grp);
            l += n;
        }
        if (ok) plan.kind = OctPlan::Hist;
        else plan.launches.clear();   // it does not fit: the sort plan
    }
    if (plan.kind != OctPlan::Hist) {
        const size_t lds = oct_lds_bytes(arena ? kOctLdsArena : kOctLdsSort, G.maxCellsPerLevel, G.kpCapMax, ldsCand, 0, 0);
        if (lds > 150 * 1024)
            return plan_fail(err, YGZF_ERR_UNSUPPORTED, "octree kernel needs %zu bytes of LDS (cells/level %d, list cap %d)", lds, G.maxCellsPerLevel, G.kpCapMax);
        // the sort plan's launches with LDS node arrays: level groups of their own workgroup size and LDS (oct_groups=1: one launch of all
        // levels; oct_block / oct_lds_kb pin the size / the LDS of every launch)
        if (!arena && ldsCand > 0) {
            plan.kind = OctPlan::SortGroups;
            plan.launches = plan_oct_sort(G, L, pins.octOneGroup, pins.octBlock, pins.octLdsBytes);
        } else {   // one launch of all levels, sized by the yardstick itself
            OctLaunch one;
            one.n = L; one.cap = G.kpCapMax; one.ldsCand = ldsCand; one.lds = lds; one.arena = arena;
            plan.kind = OctPlan::SortOne;
            plan.launches.push_back(one);
        }
    }
    // A launch of ONE frame is eight workgroups whose duration is a level's: there the histogram plan (no sort: 11 of the sort plan's 40 us
    // per level; its tree passes 12 us against 20) wins even where the candidates would fit LDS -- if all levels go in ONE launch, sized for
    // the largest (with a handful of workgroups nobody else wants the LDS).  Launches of up to 128 workgroups take it (ygzf_ctx::octSmallWgs; oct_plan=sort: never).
    if (pins.octPlan != PlanPins::Sort) plan.haveSmall = size_oct_hist_group(G, 0, L, pins.octHistBins, true, &plan.small);
    plan.keyTabWords = kMaxLevels;   // (the buffer's header: the offsets themselves)
    for (int l = 0; l < L; l++) {
        plan.keyTabOff[l] = plan.keyTabWords;
        plan.keyTabWords += (oct_tab_words(G.lv[l]) + 3) & ~3;
    }
    return YGZF_OK;
}

// which form of the cell loop: the table-driven one (per-cell records, LDS-DMA staging) wherever its 48-byte window pitch holds the
// widest cell and the pyramid offsets / frame sizes fit its 32-bit / 16-bit record fields
FastChoice choose_fast(const Geometry &G, int fastKernelSetting, const PlanPins &pins, int cuCount, int nFrames, size_t tabLds) {
    const bool tab = fastKernelSetting != YGZF_FAST_KERNEL_REGISTER_STAGING && G.fastWCellMax <= kFastTabMaxCell && G.pyrBytes < (1ll << 32) &&
                     G.w < 65536 && G.h < 65536 && G.totalSlots < (1ll << 32);
    // Large frames in large launches: persistent waves that draw their cells from per-XCD counters (extract_kernels.hip, k_fast_tab_persist) -- as many
    // workgroups as the device holds at once.  Measured on MI355X (profiles/r06_fast_persist_ab.txt), isolated and inside the three-context
    // pipeline: 1920x1080 (1620 cell groups per frame) 1484 -> 1248 us per 128 frames, 48.9 -> 51.3 k frames/s; 3840x2160 stereo 3.5 -> 2.7 ms
    // per 64 frames, 11.6 -> 12.7 k frames/s; 752x480 (259 groups) 473 -> 443 us per 256 frames alone but 237 -> 228 k frames/s in the pipeline:
    // waves that never leave keep the other contexts' octree / matcher workgroups (71 KB of LDS each) waiting for a CU, and at that size
    // the cell loop gains less than they lose.  Hence the rule: frames of >= 1000 cell groups.
    const size_t fastLds = tab ? tabLds : 0;
    const int perCu = tab ? (int) std::min<size_t>((size_t) pins.fastPersistWgs, (size_t) (160 * 1024) / std::max<size_t>(fastLds, 1)) : 0;
    const int resident = perCu * cuCount;
    const int persistMode = pins.fastPersist;   // tests: 1 always, 0 never
    // (pinned or not, never for a launch of fewer than 64 cell groups: the items are dealt to the eight XCDs' workgroups, and a launch of two workgroups has none on six of them)
    const bool persist = tab && resident > 0 && (long long) nFrames * G.totalGroups >= 64 &&
                         (persistMode == 1 || (persistMode != 0 && G.totalGroups >= 1000 && (long long) nFrames * G.totalGroups >= 4LL * resident));
    return FastChoice{persist ? FastChoice::Persist : tab ? FastChoice::Tab : FastChoice::Quads, resident};
}

}  // namespace ygzf

using namespace ygzf;

// ---- the entry points of include/ygzf.h that need no device ----

int ygzf_scale_tables_host(const ygzf_extractor_cfg *cfg, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2, int *nfeat) {
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 0 || !(cfg->scale_factor > 1.0f)) return YGZF_ERR_INVALID;
    Tables T;
    T.init(*cfg);
    const size_t n = sizeof(float) * cfg->nlevels;
    if (scale) memcpy(scale, T.scale.data(), n);
    if (inv_scale) memcpy(inv_scale, T.invScale.data(), n);
    if (sigma2) memcpy(sigma2, T.sigma2.data(), n);
    if (inv_sigma2) memcpy(inv_sigma2, T.invSigma2.data(), n);
    if (nfeat) memcpy(nfeat, T.nFeat.data(), sizeof(int) * cfg->nlevels);
    return YGZF_OK;
}

int ygzf_pyramid_plan_host(const ygzf_extractor_cfg *cfg, int w, int h, int *n_strips, int *lds_bytes, int *level_wh, unsigned short *rows, int rows_cap) {
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 0 || !(cfg->scale_factor > 1.0f) || w < 1 || h < 1 || !n_strips)
        return YGZF_ERR_INVALID;
    Tables T;
    T.init(*cfg);
    Geometry G;
    const int rc = build_geometry(T, PlanPins::from_env(), w, h, G, nullptr);
    if (rc) return rc;
    const int L = cfg->nlevels, S = (int) G.pyrPlan.size();
    *n_strips = S;
    if (lds_bytes) *lds_bytes = (int) G.pyrStripLds;
    if (level_wh)
        for (int l = 0; l < L; l++) { level_wh[2 * l] = G.lv[l].w; level_wh[2 * l + 1] = G.lv[l].h; }
    if (rows) {
        if (rows_cap < S * L * 4) return YGZF_ERR_INVALID;
        for (int s = 0; s < S; s++)
            for (int l = 0; l < L; l++) {
                const uint2 v = G.pyrPlan[s].lv[l];
                unsigned short *o = rows + ((size_t) s * L + l) * 4;
                o[0] = (unsigned short) (v.x & 0xFFFFu); o[1] = (unsigned short) (v.x >> 16);
                o[2] = (unsigned short) (v.y & 0xFFFFu); o[3] = (unsigned short) (v.y >> 16);
            }
    }
    return YGZF_OK;
}

int ygzf_octree_sort_plan_host(const ygzf_extractor_cfg *cfg, int w, int h, int *groups, int groups_cap) {
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 0 || !(cfg->scale_factor > 1.0f) || w < 1 || h < 1) return YGZF_ERR_INVALID;
    Tables T;
    T.init(*cfg);
    Geometry G;
    const int rc = build_geometry(T, PlanPins::from_env(), w, h, G, nullptr);
    if (rc) return rc;
    bool globalNodes = false;
    int ldsCand = 0;
    oct_sort_budget(G, &globalNodes, &ldsCand);
    if (globalNodes || ldsCand == 0) return 0;
    const std::vector<OctLaunch> grp = plan_oct_sort(G, cfg->nlevels, false, 0, 0);   // (the library's own plan: the octree pins are not read)
    if (groups) {
        if (groups_cap < (int) grp.size() * 6) return YGZF_ERR_INVALID;
        for (size_t i = 0; i < grp.size(); i++) {
            int *o = groups + 6 * i;
            o[0] = grp[i].l0; o[1] = grp[i].n; o[2] = grp[i].block; o[3] = grp[i].cap; o[4] = grp[i].ldsCand; o[5] = (int) grp[i].lds;
        }
    }
    return (int) grp.size();
}

int ygzf_pyramid_plan_base_host(const ygzf_extractor_cfg *cfg, int w, int h) {
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 0 || !(cfg->scale_factor > 1.0f) || w < 1 || h < 1) return YGZF_ERR_INVALID;
    Tables T;
    T.init(*cfg);
    Geometry G;
    const int rc = build_geometry(T, PlanPins::from_env(), w, h, G, nullptr);
    return rc ? rc : G.pyrBase;
}
