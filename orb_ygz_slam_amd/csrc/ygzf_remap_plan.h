// ygzf_remap_plan.h -- how one undistortion map (cv::remap's fixed-point bilinear path: src/Frame.cc:775-805) is cut into output tiles and what
// the remap kernels are launched with, decided on the host once per map (product code, internal).  Defined in ygzf_remap_plan.hip: pure arithmetic on
// the map -- no device, no runtime call, no environment -- so that it can be run (and sanitized) without the device library.
#ifndef YGZF_REMAP_PLAN_H
#define YGZF_REMAP_PLAN_H
#include <stdint.h>

#include <string>
#include <vector>

namespace ygzf {

// An output tile is 64 x 16 pixels: one workgroup of 256 threads, four adjacent pixels of a row per thread (one 32-bit store).  A tile's source box
// is staged in kRemapLdsBytes of LDS; a run of kRemapFramesPerRun consecutive frames shares one read of the map.
constexpr int kRemapTileW = 64, kRemapTileH = 16, kRemapThreads = 256;
constexpr int kRemapLdsBytes = 4096;
constexpr int kRemapFramesPerRun = 8;
constexpr int kRemapMaps = 2;   // one per eye

// What the taps of a tile say (a tap: one of the four source pixels (sx + k, sy + j) of a destination pixel):
//   Inside  every tap lies inside the source                    Lds     some taps lie outside, the box fits kRemapLdsBytes
//   Gather  the box does not fit (whatever the taps say)        Empty   no tap lies inside: the tile is zeros
enum RemapClass { kRemapInside = 0, kRemapLds = 1, kRemapGather = 2, kRemapEmpty = 3 };

// One record per tile, as the kernels read it (16 bytes).  The box is the bounding box of all the tile's taps, unclipped: columns
// [bx0, bx1] x rows [by0, by1].  Staged, it starts at column x0 = bx0 rounded DOWN to a multiple of 4 (aligned 32-bit loads) and its rows are
// `pitch` bytes apart (bx1 - x0 + 1 rounded up to 4); bytes outside the source are zeros.
struct RemapTileRec {
    int x0, y0;          // first staged column / row (= by0)
    unsigned geom;       // pitch | rows << 16 (0 for Gather and Empty tiles)
    unsigned cls;        // RemapClass
};

// One packed record per destination pixel: fx | fy << 5 | offset << 10, offset = (sy - y0) * pitch + (sx - x0), the first tap's byte inside the
// staged box (Inside and Lds tiles; 0 in Gather and Empty tiles, whose pixels are computed from `xy`).
inline uint32_t remap_record(int fx, int fy, unsigned offset) { return (uint32_t) fx | (uint32_t) fy << 5 | offset << 10; }

struct RemapPlan {
    int srcW = 0, srcH = 0, w = 0, h = 0;
    int tilesX = 0, tilesY = 0;
    int recPitch = 0;                      // entries per row of rec / xy: w rounded up to 4 (a thread's four records are one aligned 16-byte load)
    std::vector<RemapTileRec> tiles;
    std::vector<int> boxes;                // per tile bx0, by0, bx1, by1
    std::vector<uint32_t> rec, xy;         // [h][recPitch]; xy = (uint16) sx | (uint16) sy << 16, padding zero
    std::vector<int> listStaged, listGather;   // tile indices by kernel under the library's own path choice (Empty tiles ride with the staged ones)
    int count[4] = {0, 0, 0, 0};           // tiles per RemapClass
};

// YGZF_ERR_INVALID (message in *err) for null pointers, sizes below 1 or beyond 32768, or a map_tab entry above 1023.
__attribute__((visibility("hidden"))) int build_remap_plan(int srcW, int srcH, int w, int h, const int16_t *mapXY, const uint16_t *mapTab, RemapPlan &P, std::string *err);

}  // namespace ygzf
#endif
