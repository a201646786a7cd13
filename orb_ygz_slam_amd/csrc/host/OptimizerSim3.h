// OptimizerSim3.h -- Optimizer::OptimizeSim3 (src/Optimizer.cc:2409-2594) on the device, for one loop candidate or all candidates of a current
// keyframe in one call (product code, host side).  Optimizer.cc itself stays the reference's; a user forwards the one function
// (INTEGRATION.md):
//     int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
//                                 const bool bFixScale) { return OptimizeSim3Device(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale); }
// No Eigen is needed to build this library, so the Sim3 type is a template parameter, read and written through rotation().coeffs() (x y z w),
// translation() and scale() -- g2o::Sim3 has all three, const and mutable --, over a core that takes double[8].
#ifndef YGZF_OPTIMIZER_SIM3_H
#define YGZF_OPTIMIZER_SIM3_H

#include <cstddef>
#include <vector>

// The correspondences of a call (summed over its candidates) from which OptimizeSim3Core goes to the device; below it the same arithmetic
// runs on the calling thread (host/Sim3OptHost.h).  Initialised from YGZF_SIM3_OPT_DEVICE_MIN, default 400; 0 = always the device.
extern int ygzf_host_sim3_opt_device_min;

namespace ygz {
class KeyFrame;
class MapPoint;

struct OptimizeSim3Candidate {
    KeyFrame *pKF2;
    std::vector<MapPoint *> *vpMatches1;   // in / out: entries of removed pairs become NULL
    double S12[8];                         // in / out: r.x r.y r.z r.w, t, s
    int nIn;                               // out: the return value
};
// The host part of :2421-2536 for every candidate (the filter -- both points present and not bad, GetIndexInKeyFrame(pKF2) >= 0 --, the float
// R * P + t, the observations and their levels' mvInvLevelSigma2), one device call, and the reference's effects: vpMatches1[idx] = NULL for
// every removed pair, S12 = the estimate (left as it was where the reference returns before writing it), nIn.  A device failure is reported
// through ygzf_host::report_failure; every nIn is 0 then and the arguments are untouched.
void OptimizeSim3Core(KeyFrame *pKF1, std::vector<OptimizeSim3Candidate> &candidates, float th2, bool bFixScale);

template <typename Sim3T> void OptimizeSim3Read(const Sim3T &S, double o[8]) {
    for (int k = 0; k < 4; k++) o[k] = S.rotation().coeffs()[k];
    for (int k = 0; k < 3; k++) o[4 + k] = S.translation()[k];
    o[7] = S.scale();
}
template <typename Sim3T> void OptimizeSim3Write(const double i[8], Sim3T &S) {
    for (int k = 0; k < 4; k++) S.rotation().coeffs()[k] = i[k];
    for (int k = 0; k < 3; k++) S.translation()[k] = i[4 + k];
    S.scale() = i[7];
}

// All candidates of one current keyframe in one device call: vvpMatches1[k] and vS12[k] belong to vpKF2[k].  nIn[k] = what
// OptimizeSim3Device(pKF1, vpKF2[k], vvpMatches1[k], vS12[k], th2, bFixScale) returns.
template <typename Sim3T>
void OptimizeSim3Batch(KeyFrame *pKF1, const std::vector<KeyFrame *> &vpKF2, std::vector<std::vector<MapPoint *>> &vvpMatches1, std::vector<Sim3T> &vS12,
                       const float th2, const bool bFixScale, std::vector<int> &nIn) {
    std::vector<OptimizeSim3Candidate> c(vpKF2.size());
    for (size_t k = 0; k < c.size(); k++) {
        c[k].pKF2 = vpKF2[k];
        c[k].vpMatches1 = &vvpMatches1[k];
        OptimizeSim3Read(vS12[k], c[k].S12);
        c[k].nIn = 0;
    }
    OptimizeSim3Core(pKF1, c, th2, bFixScale);
    nIn.assign(c.size(), 0);
    for (size_t k = 0; k < c.size(); k++) {
        OptimizeSim3Write(c[k].S12, vS12[k]);
        nIn[k] = c[k].nIn;
    }
}

// What the reference's function does to vpMatches1 and g2oS12, and its return value.
template <typename Sim3T>
int OptimizeSim3Device(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale) {
    std::vector<OptimizeSim3Candidate> c(1);
    c[0].pKF2 = pKF2;
    c[0].vpMatches1 = &vpMatches1;
    OptimizeSim3Read(g2oS12, c[0].S12);
    c[0].nIn = 0;
    OptimizeSim3Core(pKF1, c, th2, bFixScale);
    OptimizeSim3Write(c[0].S12, g2oS12);
    return c[0].nIn;
}
}  // namespace ygz
#endif
