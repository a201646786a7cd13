// ygzf_remap_plan.hip -- the host plan of one undistortion map (ygzf_remap_plan.h): tiles, their source boxes and classes, the packed per-pixel
// records.  Host arithmetic only: no kernel, no runtime call (product code).
#include "ygzf_remap_plan.h"

#include <algorithm>
#include <cstring>

#include "../../include/ygzf.h"

namespace ygzf {

static inline int floor4(int v) { return v & ~3; }   // (two's complement: rounds towards minus infinity for negative v as well)

int build_remap_plan(int srcW, int srcH, int w, int h, const int16_t *mapXY, const uint16_t *mapTab, RemapPlan &P, std::string *err) {
    auto bad = [&](const char *m) {
        if (err) *err = m;
        return (int) YGZF_ERR_INVALID;
    };
    if (!mapXY || !mapTab) return bad("null map");
    if (srcW < 1 || srcH < 1 || w < 1 || h < 1 || srcW > 32768 || srcH > 32768 || w > 32768 || h > 32768) return bad("map or source size out of range");
    const size_t n = (size_t) w * h;
    for (size_t i = 0; i < n; i++)
        if (mapTab[i] > 1023) return bad("map2 entry above 1023 (INTER_BITS = 5: fy * 32 + fx with fx, fy in 0..31)");
    P = RemapPlan();
    P.srcW = srcW; P.srcH = srcH; P.w = w; P.h = h;
    P.tilesX = (w + kRemapTileW - 1) / kRemapTileW;
    P.tilesY = (h + kRemapTileH - 1) / kRemapTileH;
    P.recPitch = (w + 3) & ~3;
    const int nt = P.tilesX * P.tilesY;
    P.tiles.resize(nt);
    P.boxes.resize((size_t) nt * 4);
    P.rec.assign((size_t) P.recPitch * h, 0u);
    P.xy.assign((size_t) P.recPitch * h, 0u);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t) y * w + x;
            P.xy[(size_t) y * P.recPitch + x] = (uint32_t) (uint16_t) mapXY[2 * i] | (uint32_t) (uint16_t) mapXY[2 * i + 1] << 16;
        }
    for (int t = 0; t < nt; t++) {
        const int tx0 = (t % P.tilesX) * kRemapTileW, ty0 = (t / P.tilesX) * kRemapTileH;
        const int tx1 = std::min(tx0 + kRemapTileW, w), ty1 = std::min(ty0 + kRemapTileH, h);
        int bx0 = INT32_MAX, by0 = INT32_MAX, bx1 = INT32_MIN, by1 = INT32_MIN;
        bool allIn = true, anyIn = false;
        for (int y = ty0; y < ty1; y++)
            for (int x = tx0; x < tx1; x++) {
                const size_t i = (size_t) y * w + x;
                const int sx = mapXY[2 * i], sy = mapXY[2 * i + 1];   // (int: sx + 1 at 32767 does not wrap)
                bx0 = std::min(bx0, sx); bx1 = std::max(bx1, sx + 1);
                by0 = std::min(by0, sy); by1 = std::max(by1, sy + 1);
                const bool xin0 = sx >= 0 && sx < srcW, xin1 = sx + 1 >= 0 && sx + 1 < srcW;
                const bool yin0 = sy >= 0 && sy < srcH, yin1 = sy + 1 >= 0 && sy + 1 < srcH;
                allIn = allIn && xin0 && xin1 && yin0 && yin1;
                anyIn = anyIn || ((xin0 || xin1) && (yin0 || yin1));
            }
        int *B = &P.boxes[(size_t) t * 4];
        B[0] = bx0; B[1] = by0; B[2] = bx1; B[3] = by1;
        const int x0 = floor4(bx0);
        const long long pitch = ((long long) bx1 - x0 + 1 + 3) & ~3LL, rows = (long long) by1 - by0 + 1;
        RemapTileRec &T = P.tiles[t];
        T = RemapTileRec{x0, by0, 0u, 0u};
        int cls;
        if (!anyIn) cls = kRemapEmpty;
        else if (pitch * rows > kRemapLdsBytes) cls = kRemapGather;
        else cls = allIn ? kRemapInside : kRemapLds;
        T.cls = (unsigned) cls;
        P.count[cls]++;
        if (cls == kRemapInside || cls == kRemapLds) T.geom = (unsigned) pitch | (unsigned) rows << 16;
        for (int y = ty0; y < ty1; y++)
            for (int x = tx0; x < tx1; x++) {
                const size_t i = (size_t) y * w + x;
                const int fx = mapTab[i] & 31, fy = mapTab[i] >> 5;
                unsigned off = 0;
                if (cls == kRemapInside || cls == kRemapLds) off = (unsigned) ((mapXY[2 * i + 1] - by0) * (int) pitch + (mapXY[2 * i] - x0));
                P.rec[(size_t) y * P.recPitch + x] = remap_record(fx, fy, off);
            }
        (cls == kRemapGather ? P.listGather : P.listStaged).push_back(t);
    }
    return YGZF_OK;
}

}  // namespace ygzf

using namespace ygzf;

int ygzf_remap_plan_host(int src_w, int src_h, int w, int h, const int16_t *map_xy, const uint16_t *map_tab, int *geom, int *boxes, int *staged,
                         uint8_t *classes, uint32_t *records) {
    RemapPlan P;
    const int rc = build_remap_plan(src_w, src_h, w, h, map_xy, map_tab, P, nullptr);
    if (rc) return rc;
    if (geom) {
        const int g[10] = {kRemapTileW, kRemapTileH, P.tilesX, P.tilesY, kRemapLdsBytes, kRemapFramesPerRun, P.count[0], P.count[1], P.count[2], P.count[3]};
        memcpy(geom, g, sizeof g);
    }
    const int nt = P.tilesX * P.tilesY;
    if (boxes) memcpy(boxes, P.boxes.data(), sizeof(int) * 4 * (size_t) nt);
    for (int t = 0; t < nt; t++) {
        if (staged) {
            staged[3 * t] = P.tiles[t].x0;
            staged[3 * t + 1] = (int) (P.tiles[t].geom & 0xFFFFu);
            staged[3 * t + 2] = (int) (P.tiles[t].geom >> 16);
        }
        if (classes) classes[t] = (uint8_t) (P.tiles[t].cls & 0xFFu);
    }
    if (records)
        for (int y = 0; y < h; y++) memcpy(records + (size_t) y * w, &P.rec[(size_t) y * P.recPitch], sizeof(uint32_t) * (size_t) w);
    return YGZF_OK;
}
