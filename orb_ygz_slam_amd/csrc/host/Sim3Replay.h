// Sim3Replay.h -- the order-dependent part of Sim3Solver (src/Sim3Solver.cc:107-198), replayed on the host from what the device left behind:
// how SetRansacParameters derives epsilon, and iterate / find over stored inlier counts and bit masks; what it shares with PnPsolver's replay
// (the iteration count, the draws, the masks' bits) is host/RansacReplay.h.  Nothing of HIP or OpenCV is included, so a stand-alone host
// program tests it (tests/cpp/sim3_host.cc against tests/sim3_cases.py: sim3_iterate).
#ifndef YGZF_SIM3_REPLAY_H
#define YGZF_SIM3_REPLAY_H
#include <algorithm>

#include "RansacReplay.h"

namespace ygz {
namespace sim3 {

// mRansacMaxIts (:107-130): epsilon is the float quotient minInliers / N
inline int ransac_max_its(int N, double probability, int minInliers, int maxIterations) {
    return ransac::max_iterations((float) minInliers / N, minInliers == N, probability, maxIterations);
}

// The triples of `count` iterations in the reference's draw order (:152-165): ransac::draw_sets with three draws, into a cleared vector
template <typename RandomInt> void draw_triples(int N, int count, RandomInt &&randomInt, std::vector<int> &samples) {
    samples.clear();
    ransac::draw_sets(N, 3, count, randomInt, samples);
}

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
                    ransac::mark(bits + (size_t) h * words, N, indices1, vbInliers);
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
