// Sim3Solver.cc -- see standalone/Sim3Solver.h (product code, host side).  The constructor keeps what src/Sim3Solver.cc:32-105 keeps; the
// hypotheses go to the device (ygzf_sim3_ransac); iterate / find replay :132-198 over the stored results (Sim3Replay.h).
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "Sim3Solver.h"
#include "ygz_compat.h"

#include "../../../include/ygzf.h"
#include "ygzf_pool.h"

namespace ygz {

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale) : mbFixScale(bFixScale) {
    std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    const int mN1 = (int) vpMatched12.size();
    mReplay.mN1 = mN1;
    mvX3Dc1.reserve(3 * (size_t) mN1);
    mvX3Dc2.reserve(3 * (size_t) mN1);
    // Rcw X + tcw as the small gemm evaluates it: a float dot left to right, then the translation (ORBmatcherLoop.h states the choice)
    const auto Rcw1 = pKF1->GetRotation(), Rcw2 = pKF2->GetRotation();
    const auto tcw1 = pKF1->GetTranslation(), tcw2 = pKF2->GetTranslation();
    for (int i1 = 0; i1 < mN1; i1++) {
        if (!vpMatched12[i1]) continue;
        MapPoint *pMP1 = vpKeyFrameMP1[i1];
        MapPoint *pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const cv::KeyPoint &kp1 = pKF1->mvKeys[indexKF1];
        const cv::KeyPoint &kp2 = pKF2->mvKeys[indexKF2];
        const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
        const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
        mvnMaxError1.push_back((float) (size_t) (9.210 * sigmaSquare1));   // std::vector<size_t>::push_back truncates
        mvnMaxError2.push_back((float) (size_t) (9.210 * sigmaSquare2));
        mReplay.indices1.push_back((size_t) i1);
        float w1[3], w2[3];
        ygz_compat::world_pos(pMP1, w1);
        ygz_compat::world_pos(pMP2, w2);
        for (int r = 0; r < 3; r++) {
            mvX3Dc1.push_back(((Rcw1(r, 0) * w1[0] + Rcw1(r, 1) * w1[1]) + Rcw1(r, 2) * w1[2]) + tcw1[r]);
            mvX3Dc2.push_back(((Rcw2(r, 0) * w2[0] + Rcw2(r, 1) * w2[1]) + Rcw2(r, 2) * w2[2]) + tcw2[r]);
        }
    }
    mReplay.N = (int) mReplay.indices1.size();
    mK1[0] = pKF1->fx; mK1[1] = pKF1->fy; mK1[2] = pKF1->cx; mK1[3] = pKF1->cy;   // mK's entries
    mK2[0] = pKF2->fx; mK2[1] = pKF2->fy; mK2[2] = pKF2->cx; mK2[3] = pKF2->cy;
    // (FromCameraToImage of both point sets is part of the device's per-correspondence test)
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mReplay.set_parameters(probability, minInliers, maxIterations);
    // the whole budget at once: iterate runs no iteration at all when N < minInliers
    const int budget = mReplay.N >= mReplay.minInliers ? mReplay.maxIts : 0;
    sim3::draw_triples(mReplay.N, budget, ransac::random_int, mvSamples);
    mbEvaluated = mbFailed = false;
    mReplay.bestIndex = -1;   // (an index into the results that are dropped here; mnBestInliers and mBestHyp stay, as the reference's members do)
}

void Sim3Solver::SetSamples(const std::vector<int> &triples) {
    mvSamples = triples;
    mbEvaluated = mbFailed = false;
    mReplay.bestIndex = -1;
}

void Sim3SolverBatch(std::vector<Sim3Solver *> &vpSolvers) {
    static const char *who = "ygz::Sim3SolverBatch";
    std::vector<Sim3Solver *> todo;
    for (Sim3Solver *s : vpSolvers)
        if (s && !s->Evaluated()) todo.push_back(s);
    if (todo.empty()) return;
    const size_t B = todo.size();
    std::vector<ygzf_sim3_problem> prob(B);
    std::vector<float *> hyp(B);
    std::vector<int *> cnt(B);
    std::vector<uint64_t *> bits(B);
    bool any = false;
    for (size_t k = 0; k < B; k++) {
        Sim3Solver &s = *todo[k];
        const int n = s.mReplay.N, nHyp = n >= 3 ? (int) (s.mvSamples.size() / 3) : 0;
        s.mvHyp.assign((size_t) 13 * nHyp, 0.f);
        s.mvnInliers.assign(nHyp, 0);
        s.mvInlierBits.assign((size_t) nHyp * ((n + 63) / 64), 0);
        ygzf_sim3_problem &p = prob[k];
        p.n = n;
        p.X3Dc1 = s.mvX3Dc1.data(); p.X3Dc2 = s.mvX3Dc2.data();
        p.max_err1 = s.mvnMaxError1.data(); p.max_err2 = s.mvnMaxError2.data();
        for (int j = 0; j < 4; j++) { p.K1[j] = s.mK1[j]; p.K2[j] = s.mK2[j]; }
        p.fix_scale = s.mbFixScale ? 1 : 0;
        p.n_hyp = nHyp;
        p.samples = s.mvSamples.data();
        hyp[k] = s.mvHyp.data(); cnt[k] = s.mvnInliers.data(); bits[k] = s.mvInlierBits.data();
        any = any || nHyp > 0;
    }
    bool ok = true;
    if (any) {
        ygzf_host::Lease lease(ORBextractor::sDevice);
        if (!lease)
            ok = false;
        else if (ygzf_sim3_ransac(lease.get(), (int) B, prob.data(), hyp.data(), cnt.data(), bits.data()) != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
            ok = false;
        }
    }
    for (Sim3Solver *s : todo) {
        s->mbEvaluated = true;
        s->mbFailed = !ok;
    }
}

void Sim3Solver::Evaluate() {
    std::vector<Sim3Solver *> one(1, this);
    Sim3SolverBatch(one);
}

cv::Mat Sim3Solver::T12(int h) const {
    const float *o = &mvHyp[(size_t) 13 * h];
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
        float *row = T.ptr<float>(r);
        for (int c = 0; c < 3; c++) row[c] = (float) ((double) o[12] * (double) o[3 * r + c]);   // ms12i * mR12i: a double factor
        row[3] = o[9 + r];
    }
    float *last = T.ptr<float>(3);
    last[0] = last[1] = last[2] = 0.f;
    last[3] = 1.f;
    return T;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    if (!mbEvaluated) Evaluate();
    const int have = (int) mvnInliers.size();
    if (mbFailed || (mReplay.N >= mReplay.minInliers && have < std::min(mReplay.maxIts, mReplay.iterations + std::max(nIterations, 0)))) {
        // a device failure (reported), or fewer triples than iterations asked for (SetSamples): nothing more comes from this solver
        bNoMore = true;
        vbInliers = std::vector<bool>(mReplay.mN1, false);
        nInliers = 0;
        return cv::Mat();
    }
    const int words = (mReplay.N + 63) / 64;
    const int h = mReplay.iterate(nIterations, mvnInliers.data(), mvInlierBits.data(), words, bNoMore, vbInliers, nInliers);
    if (mReplay.bestIndex >= 0) {
        std::copy(&mvHyp[(size_t) 13 * mReplay.bestIndex], &mvHyp[(size_t) 13 * mReplay.bestIndex] + 13, mBestHyp);
        mbHaveBest = true;
    }
    return h < 0 ? cv::Mat() : T12(h);
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers) {
    bool bFlag;
    return iterate(mReplay.maxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
    if (!mbHaveBest) return cv::Mat();
    cv::Mat R(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R.ptr<float>(r)[c] = mBestHyp[3 * r + c];
    return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation() {
    if (!mbHaveBest) return cv::Mat();
    cv::Mat t(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) t.ptr<float>(r)[0] = mBestHyp[9 + r];
    return t;
}

float Sim3Solver::GetEstimatedScale() { return mbHaveBest ? mBestHyp[12] : 0.f; }

}  // namespace ygz
