// RansacReplay.h -- what Sim3Solver's and PnPsolver's replays (host/Sim3Replay.h, host/PnPReplay.h) and shells share: the iteration count of
// SetRansacParameters, the draws of the sample sets with the shells' DUtils::Random, and the inlier masks' bits.  What differs between the two
// solvers is the reference's own and stays in their headers: how epsilon and minInliers are derived, `&&` against `||` in the loop, `>=` against
// `>` in the best-so-far gate, Refine.  Nothing of HIP or OpenCV is included, so the stand-alone host programs test it (tests/cpp/sim3_host.cc,
// tests/cpp/pnp_host.cc).
#ifndef YGZF_RANSAC_REPLAY_H
#define YGZF_RANSAC_REPLAY_H
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#ifdef YGZF_WITH_REFERENCE_HEADERS
#include "Thirdparty/DBoW2/DUtils/Random.h"
#else
namespace DUtils {
struct Random {   // Thirdparty/DBoW2/DUtils/Random.cpp:47-50
    static int RandomInt(int min, int max) {
        int d = max - min + 1;
        return int(((double) rand() / ((double) RAND_MAX + 1.0)) * d) + min;
    }
};
}  // namespace DUtils
#endif

namespace ygz {
namespace ransac {

// mRansacMaxIts from the float epsilon a solver derived: nIterations = ceil(log(1 - p) / log(1 - pow(epsilon, 3))) in double, 1 when
// minInliers == N, then max(1, min(nIterations, maxIterations)).  The reference converts the quotient to int, which is undefined beyond
// INT_MAX and for a NaN (N < minInliers: the logarithm of a negative number): the comparison is made in double here, and a NaN takes
// maxIterations -- iterate runs no iteration when N < minInliers, and a count beyond INT_MAX is beyond maxIterations.
inline int max_iterations(float epsilon, bool minInliersIsN, double probability, int maxIterations) {
    double nIterations = minInliersIsN ? 1 : std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double) epsilon, 3)));
    if (std::isnan(nIterations) || nIterations > (double) maxIterations) nIterations = (double) maxIterations;
    if (nIterations < 1) nIterations = 1;   // (max(1, ..), before the conversion: minInliers == 0 gives -infinity)
    return (int) nIterations;
}

// The sample sets of `count` iterations in the reference's draw order (src/Sim3Solver.cc:152-165, src/PnPsolver.cc:175-187), appended to
// `samples`: per iteration a fresh copy of mvAllIndices, setSize draws by randomInt(0, size - 1), each swapped with the back and popped.
// randomInt: DUtils::Random::RandomInt in the shells, a scripted generator in tests.
template <typename RandomInt> void draw_sets(int N, int setSize, int count, RandomInt &&randomInt, std::vector<int> &samples) {
    if (N < setSize) return;
    samples.reserve(samples.size() + (size_t) setSize * count);
    std::vector<int> all(N), avail;
    for (int i = 0; i < N; i++) all[i] = i;
    for (int h = 0; h < count; h++) {
        avail = all;
        for (int i = 0; i < setSize; i++) {
            const int randi = randomInt(0, (int) avail.size() - 1);
            samples.push_back(avail[randi]);
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
}
inline int random_int(int lo, int hi) { return DUtils::Random::RandomInt(lo, hi); }   // the shells' randomInt

inline bool bit(const uint64_t *row, int i) { return (row[i >> 6] >> (i & 63)) & 1; }

// the set bits of a mask over the solver's N correspondences, marked in vbInliers through the solver's index table
inline void mark(const uint64_t *row, int N, const std::vector<size_t> &indices, std::vector<bool> &vbInliers) {
    for (int i = 0; i < N; i++)
        if (bit(row, i)) vbInliers[indices[i]] = true;
}

}  // namespace ransac
}  // namespace ygz
#endif
