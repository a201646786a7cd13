// Sim3Replay.h -- the order-dependent part of Sim3Solver (src/Sim3Solver.cc:107-198), replayed on the host from what the device left behind:
// SetRansacParameters' arithmetic, the draws of a solver's triples, and iterate / find over stored inlier counts and bit masks.  Nothing of
// HIP or OpenCV is included, so a stand-alone host program tests it (tests/cpp/sim3_host.cc against tests/sim3_cases.py: sim3_iterate).
#ifndef YGZF_SIM3_REPLAY_H
#define YGZF_SIM3_REPLAY_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ygz {
namespace sim3 {

// mRansacMaxIts (:107-130): epsilon a float quotient, nIterations = ceil(log(1 - p) / log(1 - pow(epsilon, 3))) in double, 1 when
// minInliers == N, then max(1, min(nIterations, maxIterations)).  The reference converts the quotient to int, which is undefined beyond
// INT_MAX and for a NaN (N < minInliers: the logarithm of a negative number): the comparison is made in double here, and a NaN takes
// maxIterations -- iterate runs no iteration when N < minInliers, and a count beyond INT_MAX is beyond maxIterations.
inline int ransac_max_its(int N, double probability, int minInliers, int maxIterations) {
    double nIterations;
    if (minInliers == N)
        nIterations = 1;
    else {
        const float epsilon = (float) minInliers / N;
        nIterations = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double) epsilon, 3)));
    }
    if (std::isnan(nIterations) || nIterations > (double) maxIterations) nIterations = (double) maxIterations;
    if (nIterations < 1) nIterations = 1;   // (max(1, ..), before the conversion: minInliers == 0 gives -infinity)
    return (int) nIterations;
}

// The triples of `count` iterations in the reference's draw order (:152-165): per iteration a fresh copy of mvAllIndices, three draws by
// randomInt(0, size - 1), each swapped with the back and popped.  randomInt: DUtils::Random::RandomInt in the shell, a scripted generator in tests.
template <typename RandomInt> void draw_triples(int N, int count, RandomInt &&randomInt, std::vector<int> &samples) {
    samples.clear();
    if (N < 3) return;
    samples.reserve(3 * (size_t) count);
    std::vector<int> all(N), avail;
    for (int i = 0; i < N; i++) all[i] = i;
    for (int h = 0; h < count; h++) {
        avail = all;
        for (int i = 0; i < 3; i++) {
            const int randi = randomInt(0, (int) avail.size() - 1);
            samples.push_back(avail[randi]);
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
}

inline bool bit(const uint64_t *row, int i) { return (row[i >> 6] >> (i & 63)) & 1; }

// The solver's RANSAC state and iterate (:132-193) over stored results: hypothesis h of counts / bits is the solver's iteration h + 1.
struct Replay {
    int N = 0, mN1 = 0;
    std::vector<size_t> indices1;          // mvnIndices1
    int minInliers = 6, maxIts = 300;      // mRansacMinInliers, mRansacMaxIts
    int iterations = 0, bestInliers = 0;   // mnIterations, mnBestInliers
    int bestIndex = -1;                    // the hypothesis mBestT12 / mBestRotation / mBestTranslation / mBestScale were taken from

    void set_parameters(double probability, int minInliers_, int maxIterations) {
        minInliers = minInliers_;
        maxIts = ransac_max_its(N, probability, minInliers_, maxIterations);
        iterations = 0;   // (mnBestInliers is not reset: :129 resets mnIterations only)
    }
    // -> the hypothesis iterate returns, or -1 for the empty matrix.  counts: at least maxIts entries; bits: `words` words per hypothesis.
    int iterate(int nIterations, const int *counts, const uint64_t *bits, int words, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < minInliers) {
            bNoMore = true;
            return -1;
        }
        int nCurrentIterations = 0;
        while (iterations < maxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            iterations++;
            const int h = iterations - 1;
            if (counts[h] >= bestInliers) {
                bestInliers = counts[h];
                bestIndex = h;
                if (counts[h] > minInliers) {
                    nInliers = counts[h];
                    const uint64_t *row = bits + (size_t) h * words;
                    for (int i = 0; i < N; i++)
                        if (bit(row, i)) vbInliers[indices1[i]] = true;
                    return h;
                }
            }
        }
        if (iterations >= maxIts) bNoMore = true;
        return -1;
    }
};

}  // namespace sim3
}  // namespace ygz
#endif
