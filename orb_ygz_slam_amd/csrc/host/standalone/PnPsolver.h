// PnPsolver.h -- ygz::PnPsolver with the reference's public interface (include/PnPsolver.h:61-73) over the device (host/PnPsolver.cc).  As
// standalone/Sim3Solver.h this header is used in BOTH builds: the class keeps other members than the reference's (the stored results of its
// hypotheses instead of EPnP's work arrays), so inside the reference tree it takes the place of include/PnPsolver.h (same include guard;
// INTEGRATION.md).  Tracking.cc compiles against it unchanged.
//
// What differs from the reference, and nothing else: the RANSAC hypotheses and the Refine of every hypothesis that becomes the best so far are
// evaluated on the device, all of a solver's at once and, through ygz::PnPsolverBatch, all of every relocalisation candidate's in one call
// (ygzf_pnp_ransac).  A hypothesis depends on nothing but its sample set, so SetRansacParameters draws the solver's whole budget of
// mRansacMaxIts sets at once, with DUtils::Random::RandomInt in the reference's per-iteration draw order, and iterate / find replay the
// reference's rules over the stored results (host/PnPReplay.h).  The iterations the reference runs beyond mRansacMaxIts (its loop condition
// is `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`) are drawn when they are reached and evaluated on the calling thread
// with the same arithmetic (host/PnPHost.h).
//
// THIS CONSUMES rand() DIFFERENTLY FROM THE REFERENCE.  The reference draws mRansacMinSet numbers per executed iteration, interleaved between
// the candidates Tracking::Relocalization iterates round-robin and with every other thread that calls rand(); its sequence is therefore not
// reproducible either.  Here a solver draws all its sets in SetRansacParameters, including those of iterations that a return makes
// unnecessary.  The results are equal in distribution, not per seed.
#ifndef YGZ_PNPSOLVER_H_
#define YGZ_PNPSOLVER_H_
#include <cstdint>
#include <vector>

#include "PnPReplay.h"
#include "ygz_compat.h"

extern int ygzf_host_pnp_device_min;   // host/PnPsolver.cc: the solvers of a PnPsolverBatch call from which it goes to the device

namespace ygz {

class PnPsolver {
public:
    PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches);

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991);

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    // Tests: the sample sets of the iterations to come, mRansacMinSet indices into the kept correspondences each, in place of the drawn ones.
    // The first mRansacMaxIts of them are the budget the device evaluates; the rest serve the iterations beyond it, in order, before any is
    // drawn.  Stored results are dropped, and with them the best so far (SetRansacParameters does the same: the reference keeps
    // mnBestInliers across a second SetRansacParameters, which its only caller issues before the first iteration, where there is none).
    void SetSamples(const std::vector<int> &sets);
    int Correspondences() const { return mReplay.N; }        // N: what the constructor kept
    int MinInliers() const { return mReplay.minInliers; }    // mRansacMinInliers as SetRansacParameters adjusted it
    int MaxIterations() const { return mReplay.maxIts; }     // mRansacMaxIts

protected:
    friend void PnPsolverBatch(std::vector<PnPsolver *> &vpSolvers);
    bool Evaluated() const { return mbEvaluated; }
    void Evaluate();            // this solver alone (a batch of one)
    int Budget() const;         // the sets the device evaluates
    cv::Mat Tcw(const double *hyp12) const;

    // what the constructor kept (:61-99), flat
    std::vector<float> mvP3Dw, mvP2D, mvSigma2, mvMaxError;   // N x 3, N x 2, N, N
    double mK[4];                                // fu fv uc vc, widened from the frame's floats
    int mRansacMinSet = 4;

    pnp::Replay mReplay;                         // N, mvKeyPointIndices, mRansacMinInliers, mRansacMaxIts, mnIterations, mnBestInliers
    std::vector<int> mvSamples;                  // mRansacMinSet per iteration
    bool mbEvaluated = false, mbFailed = false;
    pnp::Results mResults;
};

// Every not-yet-evaluated hypothesis of every solver of the vector in one device call (NULL entries are passed over): the solvers of
// Tracking::Relocalization's candidates (vpPnPsolvers after the set-up loop of src/Tracking.cc:1777-1793), before its iterate(5) rounds.  A
// solver that was never batched evaluates itself on its first iterate / find.  A device failure goes through ygzf_host::report_failure; the
// solvers concerned then report bNoMore with an empty matrix.
// A call with fewer than ygzf_host_pnp_device_min solvers to evaluate (default 6, YGZF_PNP_DEVICE_MIN; host/PnPsolver.cc says where the
// number comes from) pre-evaluates nothing: those solvers evaluate every iteration when iterate reaches it, on the calling thread, with
// the same arithmetic and therefore the same returns.
void PnPsolverBatch(std::vector<PnPsolver *> &vpSolvers);

}  // namespace ygz
#endif
