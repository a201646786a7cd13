// remap_kernels.hip -- cv::remap(8-bit, one channel, INTER_LINEAR, BORDER_CONSTANT 0) with the CV_16SC2 / CV_16UC1 maps of
// cv::initUndistortRectifyMap: what Frame::ComputeImagePyramid runs on every camera image in front of ORBextractor::ComputePyramid
// (src/Frame.cc:775-805).  Product code; the plan the kernels run is ygzf_remap_plan.h.
//
// Per destination pixel: (sx, sy) from map1, tab = fy * 32 + fx from map2, the four taps p_jk = src(sy + j, sx + k) (0 outside the source),
//     dst = ((32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11) + 512) >> 10
// which is OpenCV's (sum of 15-bit weights * taps + 2^14) >> 15: every weight is the exact integer 32 * b * a (include/ygzf.h says why tab = 0,
// whose weight saturates, gives the same byte).  The largest sum is 32 * 32 * 255 + 512: 32-bit arithmetic throughout.
#include "kernels.h"

namespace ygzf {

__device__ __forceinline__ unsigned remap_px(unsigned r, unsigned p00, unsigned p01, unsigned p10, unsigned p11) {
    const unsigned fx = r & 31u, fy = (r >> 5) & 31u;
    const unsigned top = (32u - fx) * p00 + fx * p01, bot = (32u - fx) * p10 + fx * p11;
    return ((32u - fy) * top + fy * bot + 512u) >> 10;
}

// the four pixels of a thread leave as one 32-bit store where the destination allows it; only the w pixels of a row are ever written
__device__ __forceinline__ void remap_store4(const RemapArgs &a, int f, int x, int y, unsigned out) {
    uint8_t *d = a.dst + (long long) f * a.dstStride + (long long) y * a.dstPitch + x;
    if (a.dstAligned && x + 4 <= a.w) *(uint32_t *) d = out;
    else
        for (int k = 0; k < 4; k++)
            if (x + k < a.w) d[k] = (uint8_t) (out >> (8 * k));
}

// One workgroup per (tile, run of framesPerRun frames).  A thread owns four adjacent pixels of a tile row and keeps their records in registers
// across the run: the map is read once per run.  Per frame the tile's source box is staged into LDS -- aligned 32-bit words, zeros where the box
// leaves the source, single bytes where a word straddles the source's right edge (the bytes beyond it belong to the row's padding or to the next
// row) or where the source is not word-aligned -- and the taps are read from there with no bounds work.  Which words a thread stages (at most
// kRemapStageWords: the budget over the workgroup) and where they lie in a frame is the same for every frame and worked out once; the words of
// kRemapChunk frames are requested together, so that a workgroup waits for memory once per chunk and not once per frame.
constexpr int kRemapStageWords = kRemapLdsBytes / 4 / kRemapThreads;
constexpr int kRemapChunk = 4;
constexpr long long kRemapWordZero = -1, kRemapWordBytes = -2;   // (in the place of a word's byte offset inside a frame)

// a staged word that is not one aligned load: byte by byte, zeros outside the source
__device__ __forceinline__ unsigned remap_word_bytes(const RemapArgs &a, const uint8_t *src, int sx, int sy) {
    unsigned v = 0u;
    if (sy >= 0 && sy < a.srcH)
        for (int k = 0; k < 4; k++)
            if (sx + k >= 0 && sx + k < a.srcW) v |= (unsigned) src[(long long) sy * a.srcPitch + sx + k] << (8 * k);
    return v;
}

// bytes o and o + 1 of the staged box in bits 0 .. 15: the two aligned words around them (one ds_read2_b32) shifted into place.  With sixteen
// byte reads of LDS per thread and frame in their place the kernel took 321 us per 256 frames at 752 x 480 -- whatever the pitches, the run
// length or the number of frames requested together -- and 100 with these eight (profiles/remap_rate.txt).
__device__ __forceinline__ unsigned remap_pair(const uint32_t *box, unsigned o) {
    return __builtin_amdgcn_alignbyte(box[(o >> 2) + 1], box[o >> 2], o & 3u);
}

__global__ __launch_bounds__(kRemapThreads) void k_remap_tiles(const RemapArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t box[kRemapLdsBytes / 4 + 4];   // (+ the word behind the last pair: read, never used)
    const int tile = a.list ? a.list[blockIdx.x] : (int) blockIdx.x;
    const RemapTileRec T = a.tiles[tile];
    const int x = (tile % a.tilesX) * kRemapTileW + (int) (threadIdx.x & 15u) * 4, y = (tile / a.tilesX) * kRemapTileH + (int) (threadIdx.x >> 4);
    const bool live = y < a.h && x < a.w;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (live) r = *(const uint4 *) (a.rec + (size_t) y * a.recPitch + x);
    const unsigned rr[4] = {r.x, r.y, r.z, r.w};
    const unsigned cls = T.cls & 0xFFu;
    const int pitch = (int) (T.geom & 0xFFFFu), rows = (int) (T.geom >> 16), pd = pitch >> 2, nd = pd * rows;
    if (cls == kRemapGather || nd * 4 > kRemapLdsBytes) return;   // (never launched: such a tile belongs to k_remap_gather)
    const uint8_t *__restrict__ src0 = a.src;
    long long wordOff[kRemapStageWords];
    int wordX[kRemapStageWords], wordY[kRemapStageWords];
#pragma unroll
    for (int k = 0; k < kRemapStageWords; k++) {
        const int i = (int) threadIdx.x + k * kRemapThreads;
        wordOff[k] = kRemapWordZero;
        wordX[k] = wordY[k] = 0;
        if (cls != kRemapEmpty && i < nd) {
            const int row = i / pd, sy = T.y0 + row, sx = T.x0 + (i - row * pd) * 4;
            wordX[k] = sx;
            wordY[k] = sy;
            if (sy >= 0 && sy < a.srcH && sx + 4 > 0 && sx < a.srcW)
                wordOff[k] = a.srcAligned && sx >= 0 && sx + 4 <= a.srcW ? (long long) sy * a.srcPitch + sx : kRemapWordBytes;
        }
    }
    const int f0 = (int) blockIdx.y * a.framesPerRun, f1 = min(a.nFrames, f0 + a.framesPerRun);
    for (int fc = f0; fc < f1; fc += kRemapChunk) {
        unsigned v[kRemapChunk][kRemapStageWords];
#pragma unroll
        for (int j = 0; j < kRemapChunk; j++) {
            const uint8_t *src = src0 + (long long) min(fc + j, f1 - 1) * a.srcStride;   // (past the run's end: its last frame once more, never used)
#pragma unroll
            for (int k = 0; k < kRemapStageWords; k++) {
                v[j][k] = 0u;
                if (wordOff[k] >= 0) v[j][k] = *(const uint32_t *) (src + wordOff[k]);
                else if (wordOff[k] == kRemapWordBytes) v[j][k] = remap_word_bytes(a, src, wordX[k], wordY[k]);
            }
        }
#pragma unroll
        for (int j = 0; j < kRemapChunk; j++) {
            const int f = fc + j;
            if (f >= f1) break;
            unsigned out = 0u;
            if (cls != kRemapEmpty) {
                if (f > f0) __syncthreads();   // every thread has read the previous frame's taps
#pragma unroll
                for (int k = 0; k < kRemapStageWords; k++) {
                    const int i = (int) threadIdx.x + k * kRemapThreads;
                    if (i < nd) box[i] = v[j][k];
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned o = rr[k] >> 10, top = remap_pair(box, o), bot = remap_pair(box, o + (unsigned) pitch);
                    out |= remap_px(rr[k], top & 255u, (top >> 8) & 255u, bot & 255u, (bot >> 8) & 255u) << (8 * k);
                }
            }
            if (live) remap_store4(a, f, x, y, out);
        }
    }
}

// The same arithmetic with every tap fetched from global memory behind a bounds check: tiles whose box does not fit the staging budget
// (adversarial maps) and, under YGZF_REMAP_PATH_GATHER, every tile.  Coordinates are widened to int before sx + 1 is formed.  Where a pixel's
// taps lie in a frame and which of them are inside the source is the same for every frame and worked out once; two frames' taps are requested
// together.
__global__ __launch_bounds__(kRemapThreads) void k_remap_gather(const RemapArgs a) {
    const int tile = a.list ? a.list[blockIdx.x] : (int) blockIdx.x;
    const int x = (tile % a.tilesX) * kRemapTileW + (int) (threadIdx.x & 15u) * 4, y = (tile / a.tilesX) * kRemapTileH + (int) (threadIdx.x >> 4);
    if (!(y < a.h && x < a.w)) return;
    const uint4 r4 = *(const uint4 *) (a.rec + (size_t) y * a.recPitch + x), c4 = *(const uint4 *) (a.xy + (size_t) y * a.recPitch + x);
    const unsigned rr[4] = {r4.x, r4.y, r4.z, r4.w}, cc[4] = {c4.x, c4.y, c4.z, c4.w};
    const uint8_t *__restrict__ src0 = a.src;
    long long tapOff[4];          // of p00 inside a frame
    unsigned in = 0u;             // bit 4 k + 2 j + i: tap (j, i) of pixel k lies inside the source
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sx = (int) (short) (cc[k] & 0xFFFFu), sy = (int) (short) (cc[k] >> 16);
        const bool x0in = sx >= 0 && sx < a.srcW, x1in = sx + 1 >= 0 && sx + 1 < a.srcW;
        const bool y0in = sy >= 0 && sy < a.srcH, y1in = sy + 1 >= 0 && sy + 1 < a.srcH;
        tapOff[k] = (long long) sy * a.srcPitch + sx;
        if (x + k < a.w) in |= (unsigned) ((y0in && x0in) | (y0in && x1in) << 1 | (y1in && x0in) << 2 | (y1in && x1in) << 3) << (4 * k);
    }
    constexpr int kFrames = 2;
    const int f0 = (int) blockIdx.y * a.framesPerRun, f1 = min(a.nFrames, f0 + a.framesPerRun);
    for (int fc = f0; fc < f1; fc += kFrames) {
        unsigned p[kFrames][16];
#pragma unroll
        for (int j = 0; j < kFrames; j++) {
            const uint8_t *src = src0 + (long long) min(fc + j, f1 - 1) * a.srcStride;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint8_t *p0 = src + tapOff[k], *p1 = p0 + a.srcPitch;
                p[j][4 * k] = in >> (4 * k) & 1u ? p0[0] : 0u;
                p[j][4 * k + 1] = in >> (4 * k + 1) & 1u ? p0[1] : 0u;
                p[j][4 * k + 2] = in >> (4 * k + 2) & 1u ? p1[0] : 0u;
                p[j][4 * k + 3] = in >> (4 * k + 3) & 1u ? p1[1] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < kFrames; j++) {
            if (fc + j >= f1) break;
            unsigned out = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) out |= remap_px(rr[k], p[j][4 * k], p[j][4 * k + 1], p[j][4 * k + 2], p[j][4 * k + 3]) << (8 * k);
            remap_store4(a, fc + j, x, y, out);
        }
    }
}

static dim3 remap_grid(const RemapArgs &A, int nTiles) { return dim3((unsigned) nTiles, (unsigned) ((A.nFrames + A.framesPerRun - 1) / A.framesPerRun)); }

void launch_remap_tiles(hipStream_t st, const RemapArgs &A, int nTiles) {
    if (nTiles < 1 || A.nFrames < 1) return;
    hipLaunchKernelGGL(k_remap_tiles, remap_grid(A, nTiles), dim3(kRemapThreads), 0, st, A);
}

void launch_remap_gather(hipStream_t st, const RemapArgs &A, int nTiles) {
    if (nTiles < 1 || A.nFrames < 1) return;
    hipLaunchKernelGGL(k_remap_gather, remap_grid(A, nTiles), dim3(kRemapThreads), 0, st, A);
}

}  // namespace ygzf
