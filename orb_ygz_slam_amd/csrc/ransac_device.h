// ransac_device.h -- the device side of a RANSAC launch, shared by k_sim3_ransac (sim3_kernels.hip) and k_pnp_hyp / k_pnp_refine
// (pnp_kernels.hip): one wave per hypothesis, wave g of the launch takes hypothesis g of the call's concatenated list; problem_of also serves
// k_triangulate (tri_kernels.hip), one lane per pair.  Device only.
#ifndef YGZF_RANSAC_DEVICE_H
#define YGZF_RANSAC_DEVICE_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ygzf {
namespace ransac {

// The problem whose items [firstHyp, firstHyp + its count) hold g: the last one with firstHyp <= g (problems without items are not in the
// table).  An item is a hypothesis for the RANSAC kernels, where g is wave-uniform and so is everything here, and a matched pair for
// k_triangulate (tri_kernels.hip), where g is the lane's own and the search diverges within a wave (at most 32 steps either way); the field
// keeps the name firstHyp for both.  The caller returns where g - firstHyp is outside the problem's count: the test stays at the call, since
// folded in here (a null result) it cost k_sim3_ransac two VGPRs.
template <typename Problem> __device__ __forceinline__ const Problem &problem_of(const Problem *probs, int nProblems, int g) {
    int lo = 0, hi = nProblems - 1;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const int mid = (lo + hi + 1) >> 1;
        if (probs[mid].firstHyp <= g) lo = mid; else hi = mid - 1;
    }
    return probs[lo];
}

// CheckInliers of one hypothesis by its wave: lane l tests correspondences l, l + 64, ..; a ballot makes each step's 64 decisions one word,
// written by lane 0 where a row is given, and the count is the sum of the words' popcounts.  -> the count, in every lane.  The loop is
// wave-uniform (n is the problem's); inlier(i) is asked for i < n only.  The predicate is taken by value: through a reference the
// compiler no longer proves the loads inside it global and emits flat ones.
template <typename Inlier> __device__ __forceinline__ int count_inliers(int n, int lane, uint64_t *row, Inlier inlier) {
    const int words = (n + 63) >> 6;
    int count = 0;
    for (int j = 0; j < words; j++) {
        const int i = 64 * j + lane;
        const bool ok = i < n && inlier(i);
        const unsigned long long word = __ballot(ok);   // lanes beyond n vote 0: the tail bits of the last word are zero
        count += __popcll(word);
        if (lane == 0 && row) row[j] = (uint64_t) word;
    }
    return count;
}

}  // namespace ransac
}  // namespace ygzf
#endif
