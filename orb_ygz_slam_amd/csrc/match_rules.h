// match_rules.h -- the reference's small matching rules, each stated once (product code, device only).  Every kernel of match_kernels.hip and
// stereo_kernels.hip that needs one of them calls it here; a site that keeps an expression of its own says which reference line makes it differ.
// Float expressions are evaluated in source order (library built with -ffp-contract=off).
#ifndef YGZF_MATCH_RULES_H
#define YGZF_MATCH_RULES_H
#include "grid_lds.h"   // GRID_COLS / GRID_ROWS

namespace ygzf {

constexpr int TH_HIGH = 100;
constexpr int HISTO_LENGTH = 30;

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1507-1523): Hamming distance of two 256-bit descriptors held as 4 x u64.
__device__ __forceinline__ unsigned hamming256(unsigned long long q0, unsigned long long q1, unsigned long long q2, unsigned long long q3,
                                               unsigned long long d0, unsigned long long d1, unsigned long long d2, unsigned long long d3) {
    return __popcll(q0 ^ d0) + __popcll(q1 ^ d1) + __popcll(q2 ^ d2) + __popcll(q3 ^ d3);
}
__device__ __forceinline__ unsigned hamming256(unsigned long long q0, unsigned long long q1, unsigned long long q2, unsigned long long q3,
                                               const unsigned long long *d) {
    return hamming256(q0, q1, q2, q3, d[0], d[1], d[2], d[3]);
}

// Rotation-histogram bin of a match (src/ORBmatcher.cc:1318-1324; the same lines at :221-227, :437-443, :554-560, :697-703, :1436-1442 of
// the other searches).  The reference's quirk is kept: factor = 1.0f / HISTO_LENGTH = 1/30, not HISTO_LENGTH / 360, so a rotation of
// [0, 360) degrees lands in bins 0..12 of the 30 and the wrap of bin HISTO_LENGTH to 0 never fires.
__device__ __forceinline__ int rot_bin(float angleQuery, float angleCandidate) {
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = angleQuery - angleCandidate;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int) roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1471-1502) over hist[HISTO_LENGTH]: the bins of the three largest counts, first of equals
// first; -1 for the second / third when its count is below a tenth of the largest.  Returned by value: through reference parameters the same
// body compiled 14 % longer into k_match_last and twice as long into k_bow_finish.
struct ThreeMaxima {
    int ind1, ind2, ind3;
};
__device__ __forceinline__ ThreeMaxima three_maxima(const int *hist) {
    ThreeMaxima m = {-1, -1, -1};
    int max1 = 0, max2 = 0, max3 = 0;
    for (int b = 0; b < HISTO_LENGTH; b++) {
        const int s = hist[b];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; m.ind3 = m.ind2; m.ind2 = m.ind1; m.ind1 = b; }
        else if (s > max2) { max3 = max2; max2 = s; m.ind3 = m.ind2; m.ind2 = b; }
        else if (s > max3) { max3 = s; m.ind3 = b; }
    }
    if (max2 < 0.1f * (float) max1) { m.ind2 = -1; m.ind3 = -1; }
    else if (max3 < 0.1f * (float) max1) { m.ind3 = -1; }
    return m;
}

// Frame::GetFeaturesInArea's cell window (src/Frame.cc:429-447) of the square of half-side r around (u, v): the clamped cell bounds, and
// `empty` when the reference returns at one of its four range tests or its two loops have nothing to visit.
struct CellWindow {
    int minCx, maxCx, minCy, maxCy;
    bool empty;
};
__device__ __forceinline__ CellWindow cell_window(float u, float v, float r, float minX, float minY, float gridInvW, float gridInvH) {
    CellWindow w;
    w.minCx = max(0, (int) floorf((u - minX - r) * gridInvW));
    w.maxCx = min(GRID_COLS - 1, (int) ceilf((u - minX + r) * gridInvW));
    w.minCy = max(0, (int) floorf((v - minY - r) * gridInvH));
    w.maxCy = min(GRID_ROWS - 1, (int) ceilf((v - minY + r) * gridInvH));
    w.empty = !(!(w.minCx >= GRID_COLS || w.maxCx < 0 || w.minCy >= GRID_ROWS || w.maxCy < 0) && w.maxCx >= w.minCx && w.maxCy >= w.minCy);
    return w;
}

// The accept rule of SearchByProjection(Frame &F, const vector<MapPoint*> &) (src/ORBmatcher.cc:112-121) for the best and second-best
// candidates of a MapPoint: secondLevel = -1, secondDist = 256 when there is no runner-up.
__device__ __forceinline__ bool accepts_best_of_two(int bestDist, int bestLevel, int secondDist, int secondLevel, float nnratio) {
    return bestDist <= TH_HIGH && !(bestLevel == secondLevel && (float) bestDist > nnratio * (float) secondDist);
}

}  // namespace ygzf
#endif
