// PnPReplay.h -- the order-dependent part of PnPsolver (src/PnPsolver.cc:111-237), replayed on the host from what the device left behind:
// how SetRansacParameters derives epsilon and minInliers, and iterate / find over stored inlier counts, masks, poses and the Refine results
// of the records; what it shares with Sim3Solver's replay (the iteration count, the draws, the masks' bits) is host/RansacReplay.h.  Nothing
// of HIP or OpenCV is included, so a stand-alone host program tests it (tests/cpp/pnp_host.cc against tests/pnp_cases.py: pnp_iterate).
//
// Refine (:239-279) always runs on mvbBestInliers, and that set changes only where a hypothesis becomes the best so far: a record.  Its
// result is therefore a function of the record alone; every later qualifying iteration that is no record repeats the same Refine with the
// same result, which the replay reuses.
#ifndef YGZF_PNP_REPLAY_H
#define YGZF_PNP_REPLAY_H
#include <algorithm>

#include "RansacReplay.h"

namespace ygz {
namespace pnp {

// What is known of a solver's hypotheses: entry h is the solver's iteration h + 1.  ygzf_pnp_ransac fills the pre-drawn budget; iterations
// beyond it (the `||` overrun) are appended one by one from the calling thread (host/PnPHost.h).
struct Results {
    int n = 0, words = 0;
    std::vector<double> hyp, refinedHyp;       // 12 per hypothesis: R row-major, t
    std::vector<int> count, refinedN;          // refinedN -1: Refine has not run on this hypothesis' mask
    std::vector<uint64_t> bits, refinedBits;   // words per hypothesis
    int size() const { return (int) count.size(); }
    void resize(int n_, int nHyp) {
        n = n_;
        words = (n + 63) / 64;
        hyp.assign((size_t) 12 * nHyp, 0.0);
        refinedHyp.assign((size_t) 12 * nHyp, 0.0);
        count.assign(nHyp, 0);
        refinedN.assign(nHyp, -1);
        bits.assign((size_t) words * nHyp, 0);
        refinedBits.assign((size_t) words * nHyp, 0);
    }
    void append() {
        hyp.resize(hyp.size() + 12, 0.0);
        refinedHyp.resize(refinedHyp.size() + 12, 0.0);
        count.push_back(0);
        refinedN.push_back(-1);
        bits.resize(bits.size() + words, 0);
        refinedBits.resize(refinedBits.size() + words, 0);
    }
};

// SetRansacParameters (:111-143): -> mRansacMinInliers, mRansacMaxIts.  nMinInliers = int(N * epsilon) is a float product, raised to minInliers
// and minSet; epsilon is raised to the float quotient nMinInliers / N.
inline void ransac_parameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon, int &outMinInliers, int &outMaxIts) {
    int nMinInliers = (int) ((float) N * epsilon);
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    outMinInliers = nMinInliers;
    if (epsilon < (float) nMinInliers / N) epsilon = (float) nMinInliers / N;
    outMaxIts = ransac::max_iterations(epsilon, nMinInliers == N, probability, maxIterations);
}

// The sample sets of `count` iterations in the reference's draw order (:175-187), appended: ransac::draw_sets with minSet draws
template <typename RandomInt> void draw_quads(int N, int minSet, int count, RandomInt &&randomInt, std::vector<int> &samples) {
    ransac::draw_sets(N, minSet, count, randomInt, samples);
}

enum Returned { EMPTY = 0, REFINED = 1, BEST = 2 };   // what iterate hands back: cv::Mat(), mRefinedTcw, mBestTcw

// The solver's RANSAC state and iterate (:155-237) over stored results.
struct Replay {
    int N = 0;
    size_t nMatches = 0;                   // mvpMapPointMatches.size(): the size of vbInliers
    std::vector<size_t> keyIndices;        // mvKeyPointIndices
    int minInliers = 10, maxIts = 300;     // mRansacMinInliers, mRansacMaxIts
    int iterations = 0, bestInliers = 0;   // mnIterations, mnBestInliers
    int bestIndex = -1;                    // the record mBestTcw and mvbBestInliers were taken from

    void set_parameters(double probability, int minInliers_, int maxIterations, int minSet, float epsilon) {
        ransac_parameters(N, probability, minInliers_, maxIterations, minSet, epsilon, minInliers, maxIts);
    }
    void mark(const uint64_t *row, std::vector<bool> &vbInliers) const {
        vbInliers = std::vector<bool>(nMatches, false);
        ransac::mark(row, N, keyIndices, vbInliers);
    }
    // -> what is returned and, in `index`, the record whose pose it is (R.refinedHyp for REFINED, R.hyp for BEST).  evaluate(h) must make
    // hypothesis h exist in R when the loop reaches it (h == R.size(): an iteration beyond what was pre-evaluated); refine(h) must fill the
    // Refine of record h where R.refinedN[h] < 0.
    template <typename Evaluate, typename Refine>
    Returned iterate(int nIterations, Results &R, Evaluate &&evaluate, Refine &&refine, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, int &index) {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        index = -1;
        if (N < minInliers) {
            bNoMore = true;
            return EMPTY;
        }
        int nCurrentIterations = 0;
        while (iterations < maxIts || nCurrentIterations < nIterations) {
            nCurrentIterations++;
            iterations++;
            const int h = iterations - 1;
            if (h >= R.size()) evaluate(h);
            if (R.count[h] >= minInliers) {
                if (R.count[h] > bestInliers) {
                    bestInliers = R.count[h];
                    bestIndex = h;
                }
                if (bestIndex < 0) continue;   // (minInliers >= minSet > 0 = the first bestInliers: a qualifying count always found a record)
                if (R.refinedN[bestIndex] < 0) refine(bestIndex);
                if (R.refinedN[bestIndex] > minInliers) {
                    nInliers = R.refinedN[bestIndex];
                    mark(&R.refinedBits[(size_t) bestIndex * R.words], vbInliers);
                    index = bestIndex;
                    return REFINED;
                }
            }
        }
        if (iterations >= maxIts) {
            bNoMore = true;
            if (bestInliers >= minInliers) {
                nInliers = bestInliers;
                mark(&R.bits[(size_t) bestIndex * R.words], vbInliers);
                index = bestIndex;
                return BEST;
            }
        }
        return EMPTY;
    }
};

}  // namespace pnp
}  // namespace ygz
#endif
