// PnPsolver.cc -- see standalone/PnPsolver.h (product code, host side).  The constructor keeps what src/PnPsolver.cc:61-101 keeps; the
// hypotheses and the Refine of their records go to the device (ygzf_pnp_ransac); iterate / find replay :155-237 over the stored results
// (PnPReplay.h), and the iterations beyond the budget run on the calling thread (PnPHost.h).
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "PnPsolver.h"
#include "ygz_compat.h"

#include <cstdio>
#include <cstdlib>

#include "../../../include/ygzf.h"
#include "PnPHost.h"
#include "ygzf_pool.h"

static_assert(YGZF_PNP_MAX_MIN_SET == 8, "include/ygzf.h and csrc/pnp_math.h name the same limit");

// The candidates of a PnPsolverBatch call from which it goes to the device.  A device call is bound by latency -- one wave runs one EPnP, and
// most of an EPnP is a chain of dependent fp64 operations -- and costs 1.1 - 2.6 ms for one candidate as for ten (50 - 500 correspondences,
// 35 sample sets each), while the reference's own schedule on this host thread, iterate(5) until the first successful Refine, costs
// 0.1 - 0.55 ms per candidate: the device loses up to five candidates and wins 1.7 - 2.1 x at ten (profiles/pnp_rate.txt).  Below the
// threshold nothing is pre-evaluated: iterate evaluates each iteration when it reaches it, on the calling thread (host/PnPHost.h: the same
// text, so the same results bit for bit), which IS the reference's schedule.
// YGZF_PNP_DEVICE_MIN overrides the default (a non-negative integer; anything else is ignored with a warning).  0 = always the device.
static int pnp_min_from_env() {
    const int dflt = 6;
    const char *e = getenv("YGZF_PNP_DEVICE_MIN");
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (*end != '\0' || v < 0 || v > 100000000) {
        fprintf(stderr, "[ygzf] YGZF_PNP_DEVICE_MIN=%s ignored (want a non-negative integer); using %d\n", e, dflt);
        return dflt;
    }
    return (int) v;
}
int ygzf_host_pnp_device_min = pnp_min_from_env();

namespace ygz {

PnPsolver::PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches) {
    mReplay.nMatches = vpMapPointMatches.size();
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeys[i];
        mvP2D.push_back(kp.pt.x);
        mvP2D.push_back(kp.pt.y);
        mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
        float w[3];
        ygz_compat::world_pos(pMP, w);
        mvP3Dw.insert(mvP3Dw.end(), w, w + 3);
        mReplay.keyIndices.push_back(i);
    }
    mReplay.N = (int) mReplay.keyIndices.size();
    mK[0] = F.fx; mK[1] = F.fy; mK[2] = F.cx; mK[3] = F.cy;
    SetRansacParameters();
}

int PnPsolver::Budget() const {
    // iterate runs no iteration at all when N < mRansacMinInliers (and mRansacMinInliers >= mRansacMinSet)
    if (mReplay.N < mReplay.minInliers || mReplay.N < mRansacMinSet) return 0;
    return std::min(mReplay.maxIts, (int) (mvSamples.size() / (size_t) mRansacMinSet));
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
    mRansacMinSet = minSet;
    mReplay.set_parameters(probability, minInliers, maxIterations, minSet, epsilon);
    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
    // the whole budget at once.  A minSet the device does not take (the reference's callers use 4) leaves the solver without hypotheses:
    // it reports bNoMore with an empty matrix.
    mvSamples.clear();
    const bool usable = minSet >= 4 && minSet <= YGZF_PNP_MAX_MIN_SET && mReplay.N >= mReplay.minInliers;
    if (usable) pnp::draw_quads(mReplay.N, minSet, mReplay.maxIts, ransac::random_int, mvSamples);
    mbEvaluated = false;
    mbFailed = !(minSet >= 4 && minSet <= YGZF_PNP_MAX_MIN_SET);
    mResults.resize(mReplay.N, 0);
    // the stored results are dropped, and with them the state that indexes them.  (The reference resets neither mnIterations nor
    // mnBestInliers here; its only caller sets the parameters before the first iteration, where both are still zero.)
    mReplay.iterations = 0;
    mReplay.bestInliers = 0;
    mReplay.bestIndex = -1;
}

void PnPsolver::SetSamples(const std::vector<int> &sets) {
    mvSamples = sets;
    mbEvaluated = false;
    mResults.resize(mReplay.N, 0);
    mReplay.iterations = 0;
    mReplay.bestInliers = 0;
    mReplay.bestIndex = -1;
}

void PnPsolverBatch(std::vector<PnPsolver *> &vpSolvers) {
    static const char *who = "ygz::PnPsolverBatch";
    std::vector<PnPsolver *> todo;
    for (PnPsolver *s : vpSolvers)
        if (s && !s->Evaluated() && !s->mbFailed) todo.push_back(s);
    if (todo.empty()) return;
    const size_t B = todo.size();
    if ((long) B < (long) ygzf_host_pnp_device_min) {   // too few for the device to win: each solver evaluates its iterations as it reaches them
        for (PnPsolver *s : todo) {
            s->mResults.resize(s->mReplay.N, 0);
            s->mbEvaluated = true;
        }
        return;
    }
    std::vector<ygzf_pnp_problem> prob(B);
    std::vector<double *> hyp(B), rhyp(B);
    std::vector<int *> cnt(B), rcnt(B);
    std::vector<uint64_t *> bits(B), rbits(B);
    bool any = false;
    for (size_t k = 0; k < B; k++) {
        PnPsolver &s = *todo[k];
        const int nHyp = s.Budget();
        s.mResults.resize(s.mReplay.N, nHyp);
        ygzf_pnp_problem &p = prob[k];
        p.n = s.mReplay.N;
        p.P3Dw = s.mvP3Dw.data(); p.P2D = s.mvP2D.data(); p.max_err = s.mvMaxError.data();
        for (int j = 0; j < 4; j++) p.K[j] = s.mK[j];
        p.min_set = s.mRansacMinSet;
        p.min_inliers = s.mReplay.minInliers;
        p.n_hyp = nHyp;
        p.samples = s.mvSamples.data();
        hyp[k] = s.mResults.hyp.data(); cnt[k] = s.mResults.count.data(); bits[k] = s.mResults.bits.data();
        rhyp[k] = s.mResults.refinedHyp.data(); rcnt[k] = s.mResults.refinedN.data(); rbits[k] = s.mResults.refinedBits.data();
        any = any || nHyp > 0;
    }
    bool ok = true;
    if (any) {
        ygzf_host::Lease lease(ORBextractor::sDevice);
        if (!lease)
            ok = false;
        else if (ygzf_pnp_ransac(lease.get(), (int) B, prob.data(), hyp.data(), cnt.data(), bits.data(), rcnt.data(), rhyp.data(), rbits.data()) != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
            ok = false;
        }
    }
    for (PnPsolver *s : todo) {
        s->mbEvaluated = true;
        s->mbFailed = !ok;
    }
}

void PnPsolver::Evaluate() {
    std::vector<PnPsolver *> one(1, this);
    PnPsolverBatch(one);
}

cv::Mat PnPsolver::Tcw(const double *hyp12) const {
    float T16[16];
    ygzf::pnp::pose_to_float(hyp12, T16);
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T.ptr<float>(r)[c] = T16[4 * r + c];
    return T;
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    if (!mbEvaluated && !mbFailed) Evaluate();
    if (mbFailed) {   // a device failure (reported), or a minSet the device does not take: nothing more comes from this solver
        bNoMore = true;
        vbInliers.clear();
        nInliers = 0;
        return cv::Mat();
    }
    pnp::HostProblem P;
    P.n = mReplay.N; P.P3D = mvP3Dw.data(); P.P2D = mvP2D.data(); P.maxErr = mvMaxError.data();
    for (int j = 0; j < 4; j++) P.K[j] = mK[j];
    P.minSet = mRansacMinSet; P.minInliers = mReplay.minInliers;
    int index = -1;
    const pnp::Returned kind = mReplay.iterate(nIterations, mResults,
        [&](int h) {   // an iteration beyond the pre-evaluated budget: its set is drawn now, unless SetSamples provided it
            if ((size_t) (h + 1) * (size_t) mRansacMinSet > mvSamples.size())
                pnp::draw_quads(mReplay.N, mRansacMinSet, 1, ransac::random_int, mvSamples);
            pnp::append_hypothesis(P, &mvSamples[(size_t) h * mRansacMinSet], mResults);
        },
        [&](int h) { pnp::refine_record(P, mResults, h); }, bNoMore, vbInliers, nInliers, index);
    if (kind == pnp::REFINED) return Tcw(&mResults.refinedHyp[(size_t) 12 * index]);
    if (kind == pnp::BEST) return Tcw(&mResults.hyp[(size_t) 12 * index]);
    return cv::Mat();
}

cv::Mat PnPsolver::find(std::vector<bool> &vbInliers, int &nInliers) {
    bool bFlag;
    return iterate(mReplay.maxIts, bFlag, vbInliers, nInliers);
}

}  // namespace ygz
