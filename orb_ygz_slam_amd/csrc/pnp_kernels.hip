// pnp_kernels.hip -- PnPsolver's RANSAC (src/PnPsolver.cc:155-308, :341-894): every hypothesis of every problem of a call in one launch
// (k_pnp_hyp: EPnP on the sample set, then CheckInliers), and in a second launch on the same stream Refine for the hypotheses that are records
// (k_pnp_refine: EPnP over the record's own inlier mask, then CheckInliers).  Hypotheses are independent of each other; Refine depends on the
// order only through which inlier set is the best so far, and that set changes exactly at a record.  What iterate does with the results is
// replayed on the host (host/PnPReplay.h).
//
// One wave per hypothesis, four waves per workgroup; wave g of a launch takes hypothesis g of the call's concatenated list, so the waves of
// one workgroup may belong to different problems.  The solve is csrc/pnp_math.h, written for a team of lanes that own elements: each of the 78
// distinct entries of MtM, each centroid coordinate and each entry of ABt is one chain summed in row order by one lane; a Jacobi rotation
// updates the elements of its two rows (and of the two rows of Vt) one per lane, and every lane sums the three dot products itself in index
// order from LDS; the 6 x k and 3 x 3 problems run on lane 0.  So every sum has the source's order and the result equals the host's bit for
// bit.  The work area (pnp::Work, 3 KB) is each wave's own slice of static LDS: waves share nothing, so there is no workgroup barrier, only
// the wave-level ordering of YGZF_PNP_SYNC, and no atomics.  Then the wave counts the inliers (ransac_device.h).  Every loop is bounded by
// an argument (n, the counts) or a constant of pnp_math.h.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pnp_math.h"
#include "ransac_device.h"

namespace ygzf {

namespace {

constexpr int kPnpWaves = 4, kPnpThreads = 64 * kPnpWaves;

// CheckInliers under the pose in w, and the pose itself: -> the count; row = the mask's words or null
__device__ inline int check_inliers(const PnpProblemDev &P, const pnp::Points &Pt, const pnp::Work &w, int lane, uint64_t *row, double *out) {
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = w.R[i];
    for (int i = 0; i < 3; i++) t[i] = w.t[i];
    const int count = ransac::count_inliers(P.n, lane, row, [&](int i) { return pnp::inlier(R, t, Pt, i, P.maxErr[i]); });
    if (lane < 9) out[lane] = w.R[lane];
    else if (lane < 12) out[lane] = w.t[lane - 9];
    return count;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_hyp(PnpArgs A) {
    __shared__ pnp::Work work[kPnpWaves];
    const int lane = threadIdx.x & 63, wv = (int) threadIdx.x >> 6;
    const int g = (int) blockIdx.x * kPnpWaves + wv;   // wave-uniform
    if (g >= A.totalHyp) return;
    const PnpProblemDev &P = ransac::problem_of(A.probs, A.nProblems, g);
    const int h = g - P.firstHyp;
    if (h < 0 || h >= P.nHyp) return;   // (cannot happen with the host's table; a wrong table must not turn into a stray write)
    const pnp::Points Pt = {P.P3D, P.P2D, P.K[0], P.K[1], P.K[2], P.K[3]};
    const pnp::Subset S = {P.samples + (size_t) h * P.minSet, nullptr, P.minSet, P.n};   // checked by the host: inside [0, n)
    pnp::Work &w = work[wv];
    pnp::epnp(Pt, S, w, pnp::Lanes{lane, 64});
    const int words = (P.n + 63) >> 6;
    const int count = check_inliers(P, Pt, w, lane, P.bits + (size_t) h * words, P.hyp + (size_t) pnp::kHypDoubles * h);
    if (lane == 0) P.nInliers[h] = count;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_refine(PnpArgs A) {
    __shared__ pnp::Work work[kPnpWaves];
    const int lane = threadIdx.x & 63, wv = (int) threadIdx.x >> 6;
    const int g = (int) blockIdx.x * kPnpWaves + wv;
    if (g >= A.totalHyp) return;
    const PnpProblemDev &P = ransac::problem_of(A.probs, A.nProblems, g);
    const int h = g - P.firstHyp;
    if (h < 0 || h >= P.nHyp) return;   // (cannot happen with the host's table; a wrong table must not turn into a stray write)
    const int words = (P.n + 63) >> 6;
    // a record: the count reaches min_inliers and beats every earlier count of the problem
    const int mine = P.nInliers[h];
    bool record = mine >= P.minInliers;
    for (int j = 0; j < h && record; j++)
        if (P.nInliers[j] >= mine) record = false;
    double *out = P.refinedHyp + (size_t) pnp::kHypDoubles * h;
    uint64_t *row = P.refinedBits ? P.refinedBits + (size_t) h * words : nullptr;
    if (!record) {   // the outputs are defined everywhere: -1, zeros
        if (lane == 0) P.refinedN[h] = -1;
        if (lane < pnp::kHypDoubles) out[lane] = 0.0;
        if (row)
            for (int j = lane; j < words; j += 64) row[j] = 0;
        return;
    }
    const pnp::Points Pt = {P.P3D, P.P2D, P.K[0], P.K[1], P.K[2], P.K[3]};
    const pnp::Subset S = {nullptr, P.bits + (size_t) h * words, mine, P.n};   // Refine's vIndices: the set bits in ascending order
    pnp::Work &w = work[wv];
    pnp::epnp(Pt, S, w, pnp::Lanes{lane, 64});
    const int count = check_inliers(P, Pt, w, lane, row, out);
    if (lane == 0) P.refinedN[h] = count;
}

}  // namespace

void launch_pnp(hipStream_t st, const PnpArgs &A) {
    if (A.totalHyp <= 0) return;
    const dim3 grid((A.totalHyp + kPnpWaves - 1) / kPnpWaves), block(kPnpThreads);
    hipLaunchKernelGGL(k_pnp_hyp, grid, block, 0, st, A);
    hipLaunchKernelGGL(k_pnp_refine, grid, block, 0, st, A);
}

}  // namespace ygzf
