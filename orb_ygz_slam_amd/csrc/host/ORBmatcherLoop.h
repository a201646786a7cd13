// ORBmatcherLoop.h -- the loop-closing side of ygz::ORBmatcher over the device (host/ORBmatcherLoop.cc):
//   ygz::SearchByBoWBatch: the SearchByBoW(mpCurrentKF, pKF, ..) loop of LoopClosing::ComputeSim3 as one device batch (declared below).
//   ygz::SearchAndFuseBatch: the loop of LoopClosing::SearchAndFuse (src/LoopClosing.cc:549-568) -- per corrected keyframe
//   Fuse(pKF, Scw, loopPoints, th, vpReplace), then vpReplace[i]->Replace(loopPoints[i]) -- as one device batch with the same final graph
//   (host/LoopApply.h says why).  `poses` in the order the reference iterates CorrectedPosesMap (std::map order).  Returns the summed nFused of
//   the keyframes it applied.  A device failure goes through ygzf_host::report_failure and stops the batch: keyframes before the failing step
//   stay fused and replaced exactly as the sequential loop would have left them.
//   ygz::loop::decompose_scw / sim3_transforms: the pose algebra of src/ORBmatcher.cc:274-278, :897-901 and :1022-1024.  It stays on the
//   host (the device contract takes decomposed poses).  Built with the reference's headers (-DYGZF_WITH_REFERENCE_HEADERS) these evaluate
//   the reference's own cv::Mat expressions, so the user's OpenCV decides the last bits; stand-alone they use the scalar definition written
//   out below, which is THIS PROJECT'S CHOICE of what OpenCV 2.4 / 3.2 computes there.
#ifndef YGZF_ORBMATCHER_LOOP_H
#define YGZF_ORBMATCHER_LOOP_H
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "ygz_compat.h"

namespace ygz {
int SearchAndFuseBatch(const std::vector<std::pair<KeyFrame *, cv::Mat>> &poses, const std::vector<MapPoint *> &loopPoints, float th = 4.0f);
// The device query SearchAndFuseBatch is built on, by itself (tools/loop_rate.py times it): bestIdx / bestDist (poses.size() x points.size(),
// row = keyframe) of every pair with skip[k * P + i] == 0, before any map update.  false: device failure (reported).
bool SearchAndFuseCandidates(const std::vector<std::pair<KeyFrame *, cv::Mat>> &poses, const std::vector<MapPoint *> &points,
                             const std::vector<uint8_t> &skip, float th, std::vector<int> &bestIdx, std::vector<int> &bestDist);

// The loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:238-261) -- per consistent candidate ORBmatcher(nnratio, checkOrientation)
// .SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) -- as one device call.  Callers pass live candidates only (the reference discards
// pKF->isBad() before the search, :244-247).  pKF1's GetMapPointMatches() snapshot is taken ONCE for the batch (the sequential loop takes it
// again per candidate); every candidate's own snapshot is taken once, as in the member.  vvpMatches12[k] / nmatches[k]: vpMatches12 and the
// return value of the k-th call.  Returns the number of candidates with nmatches >= 20 (:251).  A device failure goes through
// ygzf_host::report_failure: every vvpMatches12[k] is all NULL, every nmatches[k] is 0.
int SearchByBoWBatch(KeyFrame *pKF1, const std::vector<KeyFrame *> &candidates, float nnratio, bool checkOrientation,
                     std::vector<std::vector<MapPoint *>> &vvpMatches12, std::vector<int> &nmatches);

namespace loop {
// Scw (4 x 4, CV_32F) -> Rcw (row-major), tcw, Ow
inline void decompose_scw(const cv::Mat &Scw, float Rcw[9], float tcw[3], float Ow[3]) {
#ifdef YGZF_WITH_REFERENCE_HEADERS
    cv::Mat sRcw = Scw.rowRange(0, 3).colRange(0, 3);
    const float scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));
    cv::Mat R = sRcw / scw;
    cv::Mat t = Scw.rowRange(0, 3).col(3) / scw;
    cv::Mat O = -R.t() * t;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[3 * r + c] = R.at<float>(r, c);
        tcw[r] = t.at<float>(r);
        Ow[r] = O.at<float>(r);
    }
#else
    // Mat::dot accumulates in double; sqrt of it, cast to float.  Mat / float scales by the double 1 / scw, each entry rounded to float once.
    // -R' t is the small-matrix gemm: a float dot left to right, negated.
    const float *r0 = Scw.ptr<float>(0);
    double s = (double) r0[0] * (double) r0[0];
    s += (double) r0[1] * (double) r0[1];
    s += (double) r0[2] * (double) r0[2];
    const float scw = (float) std::sqrt(s);
    const double inv = 1.0 / (double) scw;
    for (int r = 0; r < 3; r++) {
        const float *row = Scw.ptr<float>(r);
        for (int c = 0; c < 3; c++) Rcw[3 * r + c] = (float) ((double) row[c] * inv);
        tcw[r] = (float) ((double) row[3] * inv);
    }
    for (int c = 0; c < 3; c++) Ow[c] = -((Rcw[c] * tcw[0] + Rcw[3 + c] * tcw[1]) + Rcw[6 + c] * tcw[2]);
#endif
}

// s12, R12 (3 x 3), t12 (3 x 1) -> sR12 = s12 R12, sR21 = (1 / s12) R12', t21 = -sR21 t12, and t12 itself
inline void sim3_transforms(float s12, const cv::Mat &R12, const cv::Mat &t12, float sR12[9], float t12o[3], float sR21[9], float t21[3]) {
#ifdef YGZF_WITH_REFERENCE_HEADERS
    cv::Mat a = s12 * R12;
    cv::Mat b = (1.0 / s12) * R12.t();
    cv::Mat c = -b * t12;
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) { sR12[3 * r + k] = a.at<float>(r, k); sR21[3 * r + k] = b.at<float>(r, k); }
        t12o[r] = t12.at<float>(r);
        t21[r] = c.at<float>(r);
    }
#else
    // scalar * Mat converts with a double factor: one rounding of the exact product; (1.0 / s12) is a double quotient
    const double inv = 1.0 / (double) s12;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) {
            sR12[3 * r + k] = (float) ((double) s12 * (double) R12.ptr<float>(r)[k]);
            sR21[3 * r + k] = (float) (inv * (double) R12.ptr<float>(k)[r]);
        }
    for (int r = 0; r < 3; r++) t12o[r] = t12.ptr<float>(r)[0];
    for (int r = 0; r < 3; r++) t21[r] = -((sR21[3 * r] * t12o[0] + sR21[3 * r + 1] * t12o[1]) + sR21[3 * r + 2] * t12o[2]);
#endif
}
}  // namespace loop
}  // namespace ygz
#endif
