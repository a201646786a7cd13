// PnPHost.h -- csrc/pnp_math.h on the calling thread: what k_pnp_hyp / k_pnp_refine compute for one hypothesis, as a team of one lane.  The
// same text, the same order of every sum, so the same bits.  Used for the iterations beyond a solver's pre-evaluated budget
// (host/PnPsolver.cc), as the one-thread yardstick of tools/pnp_rate.py and by tests/cpp/pnp_host.cc.  Nothing of HIP or OpenCV is included.
#ifndef YGZF_PNP_HOST_H
#define YGZF_PNP_HOST_H
#include <cstring>
#include <memory>

#include "PnPReplay.h"
#include "../pnp_math.h"

namespace ygz {
namespace pnp {

struct HostProblem {
    int n = 0;
    const float *P3D = nullptr, *P2D = nullptr, *maxErr = nullptr;
    double K[4] = {0, 0, 0, 0};   // fu fv uc vc
    int minSet = 4, minInliers = 0;
};

namespace detail {
inline int check(const HostProblem &P, const ygzf::pnp::Points &Pt, const ygzf::pnp::Work &w, uint64_t *row, double *hyp12) {
    const int words = (P.n + 63) / 64;
    for (int j = 0; j < words; j++) row[j] = 0;
    int count = 0;
    for (int i = 0; i < P.n; i++)
        if (ygzf::pnp::inlier(w.R, w.t, Pt, i, P.maxErr[i])) {
            row[i >> 6] |= 1ull << (i & 63);
            count++;
        }
    std::memcpy(hyp12, w.R, 9 * sizeof(double));
    std::memcpy(hyp12 + 9, w.t, 3 * sizeof(double));
    return count;
}
}  // namespace detail

// compute_pose on the minSet correspondences `sample`, then CheckInliers: -> mnInliersi
inline int hypothesis(const HostProblem &P, const int *sample, double *hyp12, uint64_t *row) {
    const ygzf::pnp::Points Pt = {P.P3D, P.P2D, P.K[0], P.K[1], P.K[2], P.K[3]};
    const ygzf::pnp::Subset S = {sample, nullptr, P.minSet, P.n};
    auto w = std::make_unique<ygzf::pnp::Work>();
    ygzf::pnp::epnp(Pt, S, *w, ygzf::pnp::Lanes{0, 1});
    return detail::check(P, Pt, *w, row, hyp12);
}

// Refine's compute_pose over the `count` set bits of `mask`, then CheckInliers: -> mnRefinedInliers
inline int refine(const HostProblem &P, const uint64_t *mask, int count, double *hyp12, uint64_t *row) {
    const ygzf::pnp::Points Pt = {P.P3D, P.P2D, P.K[0], P.K[1], P.K[2], P.K[3]};
    const ygzf::pnp::Subset S = {nullptr, mask, count, P.n};
    auto w = std::make_unique<ygzf::pnp::Work>();
    ygzf::pnp::epnp(Pt, S, *w, ygzf::pnp::Lanes{0, 1});
    return detail::check(P, Pt, *w, row, hyp12);
}

// hypothesis h of R from its sample set (R must hold h entries: it is appended)
inline void append_hypothesis(const HostProblem &P, const int *sample, Results &R) {
    const int h = R.size();
    R.append();
    R.count[h] = hypothesis(P, sample, &R.hyp[(size_t) 12 * h], &R.bits[(size_t) R.words * h]);
}
inline void refine_record(const HostProblem &P, Results &R, int h) {
    R.refinedN[h] = refine(P, &R.bits[(size_t) R.words * h], R.count[h], &R.refinedHyp[(size_t) 12 * h], &R.refinedBits[(size_t) R.words * h]);
}

// what one ygzf_pnp_ransac call leaves for this problem: every hypothesis, and Refine for the records
inline void evaluate_all(const HostProblem &P, const int *samples, int nHyp, Results &R) {
    R.resize(P.n, 0);
    int best = -1;   // the largest count so far
    for (int h = 0; h < nHyp; h++) {
        append_hypothesis(P, samples + (size_t) P.minSet * h, R);
        if (R.count[h] >= P.minInliers && R.count[h] > best) refine_record(P, R, h);
        best = std::max(best, R.count[h]);
    }
}

}  // namespace pnp
}  // namespace ygz
#endif
