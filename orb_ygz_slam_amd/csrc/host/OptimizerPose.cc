// OptimizerPose.cc -- see OptimizerPose.h (product code, host side).  Packs from Frame exactly what src/Optimizer.cc:1696-1763 reads -- per
// correspondence the keypoint, mvuRight, the octave's mvInvLevelSigma2 and the MapPoint's world position, under MapPoint::mGlobalMutex -- and
// writes what :1702 / :1730 / :1796-1825 / :1839 write: mvbOutlier and SetPose.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "OptimizerPose.h"
#include "ygz_compat.h"

#include <cstdio>
#include <mutex>

#include "../../../include/ygzf.h"
#include "ygzf_pool.h"

namespace ygz {

void PoseOptimizationBatch(const std::vector<Frame *> &vpFrames, std::vector<int> &nGood) {
    static const char *who = "ygz::PoseOptimizationBatch";
    const size_t B = vpFrames.size();
    nGood.assign(B, 0);
    if (B == 0) return;
    std::vector<ygzf_pose_problem> prob(B);
    std::vector<std::vector<uint8_t>> valid(B), flags(B);
    std::vector<std::vector<float>> world(B);
    std::vector<uint8_t *> flagPtr(B);
    const std::vector<float> &invSigma2 = vpFrames[0]->mvInvLevelSigma2;   // one extractor configuration serves all frames of a system
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);
        for (size_t k = 0; k < B; k++) {
            Frame *F = vpFrames[k];
            const int N = F->N;
            valid[k].assign((size_t) N + 1, 0);
            flags[k].assign((size_t) N + 1, 0);
            world[k].assign(3 * (size_t) N + 3, 0.f);
            for (int i = 0; i < N; i++) {
                MapPoint *pMP = F->mvpMapPoints[i];
                flags[k][i] = F->mvbOutlier[i];
                if (!pMP) continue;
                if (F->mvKeys[i].octave < 0 || (size_t) F->mvKeys[i].octave >= invSigma2.size() || F->mvInvLevelSigma2.size() != invSigma2.size()) {
                    ygzf_host::report_failure(who, "a keypoint's octave has no entry in mvInvLevelSigma2");
                    return;
                }
                valid[k][i] = 1;
                ygz_compat::world_pos(pMP, &world[k][3 * (size_t) i]);
            }
            ygzf_pose_problem &p = prob[k];
            p.n = N;
            p.keys = (const ygzf_kp *) F->mvKeys.data();
            p.u_right = F->mvuRight.data();
            p.mp_valid = valid[k].data();
            p.mp_world = world[k].data();
            ygz_compat::se3_to7(F->mTcw, p.Tcw);
            flagPtr[k] = flags[k].data();
        }
    }
    ygzf_camera cam = {Frame::fx, Frame::fy, Frame::cx, Frame::cy, 0, vpFrames[0]->mbf, Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY};
    std::vector<float> T((size_t) 7 * B);
    std::vector<int> ret(B, 0);
    ygzf_host::Lease lease(ORBextractor::sDevice);
    if (!lease) return;
    if (ygzf_pose_optimization(lease.get(), &cam, invSigma2.data(), (int) B, prob.data(), T.data(), nullptr, flagPtr.data(), ret.data(), nullptr) != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
        return;
    }
    for (size_t k = 0; k < B; k++) {
        Frame *F = vpFrames[k];
        int nInitial = 0;
        for (int i = 0; i < F->N; i++)
            if (valid[k][i]) { F->mvbOutlier[i] = flags[k][i] != 0; nInitial++; }
        if (nInitial >= 3) F->SetPose(ygz_compat::se3_from7(&T[7 * k]));   // :1767 returns before :1839
        nGood[k] = ret[k];
    }
}

int PoseOptimizationDevice(Frame *pFrame) {
    std::vector<int> nGood;
    PoseOptimizationBatch(std::vector<Frame *>(1, pFrame), nGood);
    return nGood.empty() ? 0 : nGood[0];
}

}  // namespace ygz
