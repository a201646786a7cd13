// Sim3Solver.h -- ygz::Sim3Solver with the reference's public interface (include/Sim3Solver.h:33-48) over the device (host/Sim3Solver.cc).
// Unlike standalone/ORBmatcher.h this header is used in BOTH builds: the class keeps other members than the reference's (the stored results
// of its hypotheses instead of cv::Mat work arrays), so inside the reference tree it takes the place of include/Sim3Solver.h (same include
// guard).  LoopClosing.cc compiles against it unchanged.
//
// What differs from the reference, and nothing else: the RANSAC hypotheses are evaluated on the device, all of a solver's at once and, through
// ygz::Sim3SolverBatch, all of every loop candidate's in one call (ygzf_sim3_ransac).  A hypothesis depends on nothing but its triple, so
// SetRansacParameters draws the solver's whole budget of mRansacMaxIts triples at once, with DUtils::Random::RandomInt in the reference's
// per-iteration draw order, and iterate / find replay the reference's rules over the stored counts (host/Sim3Replay.h).
//
// THIS CONSUMES rand() DIFFERENTLY FROM THE REFERENCE.  The reference draws three numbers per executed iteration, interleaved between the
// candidates LoopClosing::ComputeSim3 iterates round-robin and with every other thread that calls rand(); its sequence is therefore not
// reproducible either.  Here a solver draws all its triples in SetRansacParameters, including those of iterations that a return makes
// unnecessary.  The results are equal in distribution, not per seed.
#ifndef YGZ_SIM3SOLVER_H_
#define YGZ_SIM3SOLVER_H_
#include <cstdint>
#include <vector>

#include "Sim3Replay.h"
#include "ygz_compat.h"

namespace ygz {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    // Tests: the triples of the iterations to come, 3 indices into the kept correspondences each, in place of the drawn ones.  They must cover
    // the iterations the caller will run (at most mRansacMaxIts); stored results are dropped.
    void SetSamples(const std::vector<int> &triples);
    int Correspondences() const { return mReplay.N; }        // N: what the constructor kept

protected:
    friend void Sim3SolverBatch(std::vector<Sim3Solver *> &vpSolvers);
    bool Evaluated() const { return mbEvaluated; }
    void Evaluate();            // this solver alone (a batch of one)
    cv::Mat T12(int h) const;   // mT12i of hypothesis h

    // what the constructor kept (:56-96), flat
    std::vector<float> mvX3Dc1, mvX3Dc2;         // N x 3
    std::vector<float> mvnMaxError1, mvnMaxError2;   // (float) (size_t) (9.210 * sigma2)
    float mK1[4], mK2[4];                        // fx fy cx cy
    bool mbFixScale;

    sim3::Replay mReplay;                        // N, mN1, mvnIndices1, mRansacMinInliers, mRansacMaxIts, mnIterations, mnBestInliers
    std::vector<int> mvSamples;                  // 3 per iteration
    bool mbEvaluated = false, mbFailed = false;
    std::vector<float> mvHyp;                    // 13 per hypothesis: R12, t12, s12
    std::vector<int> mvnInliers;
    std::vector<uint64_t> mvInlierBits;
    float mBestHyp[13] = {0};                    // mBestRotation, mBestTranslation, mBestScale: they outlive a new SetRansacParameters
    bool mbHaveBest = false;
};

// Every not-yet-evaluated hypothesis of every solver of the vector in one device call (NULL entries are passed over): the solvers of
// LoopClosing::ComputeSim3's candidates, before its iterate(5) rounds.  A solver that was never batched evaluates itself on its first iterate /
// find.  A device failure goes through ygzf_host::report_failure; the solvers concerned then report bNoMore with an empty matrix.
void Sim3SolverBatch(std::vector<Sim3Solver *> &vpSolvers);

}  // namespace ygz
#endif
