// OptimizerSim3.cc -- see OptimizerSim3.h (product code, host side).  Packs from the keyframes exactly what src/Optimizer.cc:2421-2536 reads
// and writes what :2552 / :2584 / :2591 write: vpMatches1 and g2oS12.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "OptimizerSim3.h"
#include "ygz_compat.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../../include/ygzf.h"
#include "Sim3OptHost.h"
#include "ygzf_pool.h"

// The correspondences of a call (summed over its candidates) from which it goes to the device.  A device call is bound by latency -- one lane
// factorises and updates between the passes of every trial -- and costs 0.65 - 1.0 ms whatever its size up to ten candidates of 300, while
// the same arithmetic on this host thread costs ~2.3 us per correspondence: the device loses below ~350 and wins 6.6 x at 10 x 300
// (profiles/sim3_opt_rate.txt).  Below the threshold the shell runs host/Sim3OptHost.h: the same text, the sums in the reference's order.
// YGZF_SIM3_OPT_DEVICE_MIN overrides the default (a non-negative integer; anything else is ignored with a warning).  0 = always the device.
static int sim3_opt_min_from_env() {
    const int dflt = 400;
    const char *e = getenv("YGZF_SIM3_OPT_DEVICE_MIN");
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (*end != '\0' || v < 0 || v > 100000000) {
        fprintf(stderr, "[ygzf] YGZF_SIM3_OPT_DEVICE_MIN=%s ignored (want a non-negative integer); using %d\n", e, dflt);
        return dflt;
    }
    return (int) v;
}
int ygzf_host_sim3_opt_device_min = sim3_opt_min_from_env();

namespace ygz {

void OptimizeSim3Core(KeyFrame *pKF1, std::vector<OptimizeSim3Candidate> &cands, const float th2, const bool bFixScale) {
    static const char *who = "ygz::OptimizeSim3";
    const size_t B = cands.size();
    for (size_t k = 0; k < B; k++) cands[k].nIn = 0;
    if (B == 0) return;
    struct Packed {
        std::vector<float> P1c, P2c, obs1, obs2, is1, is2;
        std::vector<size_t> index;         // vnIndexEdge
        std::vector<uint8_t> removed;
    };
    std::vector<Packed> pk(B);
    std::vector<ygzf_sim3_opt_problem> prob(B);
    std::vector<uint8_t *> removedPtr(B);
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    // R * P + t as the small gemm evaluates it: a float dot left to right, then the translation (ORBmatcherLoop.h states the choice)
    const auto R1w = pKF1->GetRotation();
    const auto t1w = pKF1->GetTranslation();
    for (size_t k = 0; k < B; k++) {
        KeyFrame *pKF2 = cands[k].pKF2;
        const std::vector<MapPoint *> &vpMatches1 = *cands[k].vpMatches1;
        const auto R2w = pKF2->GetRotation();
        const auto t2w = pKF2->GetTranslation();
        Packed &q = pk[k];
        const int N = (int) vpMatches1.size();
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[i]) continue;
            MapPoint *pMP1 = vpMapPoints1[i];
            MapPoint *pMP2 = vpMatches1[i];
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (!pMP1 || !pMP2) continue;
            if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
            const cv::KeyPoint &kpUn1 = pKF1->mvKeys[i];
            const cv::KeyPoint &kpUn2 = pKF2->mvKeys[i2];
            if (kpUn1.octave < 0 || (size_t) kpUn1.octave >= pKF1->mvInvLevelSigma2.size() || kpUn2.octave < 0 || (size_t) kpUn2.octave >= pKF2->mvInvLevelSigma2.size()) {
                ygzf_host::report_failure(who, "a keypoint's octave has no entry in mvInvLevelSigma2");
                return;
            }
            float w1[3], w2[3];
            ygz_compat::world_pos(pMP1, w1);
            ygz_compat::world_pos(pMP2, w2);
            for (int r = 0; r < 3; r++) {
                q.P1c.push_back(((R1w(r, 0) * w1[0] + R1w(r, 1) * w1[1]) + R1w(r, 2) * w1[2]) + t1w[r]);
                q.P2c.push_back(((R2w(r, 0) * w2[0] + R2w(r, 1) * w2[1]) + R2w(r, 2) * w2[2]) + t2w[r]);
            }
            q.obs1.push_back(kpUn1.pt.x); q.obs1.push_back(kpUn1.pt.y);
            q.obs2.push_back(kpUn2.pt.x); q.obs2.push_back(kpUn2.pt.y);
            q.is1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
            q.is2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
            q.index.push_back((size_t) i);
        }
        q.removed.assign(q.index.size() + 1, 0);
        removedPtr[k] = q.removed.data();
        ygzf_sim3_opt_problem &p = prob[k];
        std::memset(&p, 0, sizeof p);
        p.n = (int) q.index.size();
        p.P1c = q.P1c.data(); p.P2c = q.P2c.data();
        p.obs1 = q.obs1.data(); p.obs2 = q.obs2.data();
        p.inv_sigma2_1 = q.is1.data(); p.inv_sigma2_2 = q.is2.data();
        p.K1[0] = pKF1->fx; p.K1[1] = pKF1->fy; p.K1[2] = pKF1->cx; p.K1[3] = pKF1->cy;   // mK's entries
        p.K2[0] = pKF2->fx; p.K2[1] = pKF2->fy; p.K2[2] = pKF2->cx; p.K2[3] = pKF2->cy;
        std::memcpy(p.S12, cands[k].S12, sizeof p.S12);
        p.th2 = th2;
        p.fix_scale = bFixScale ? 1 : 0;
    }
    std::vector<double> S((size_t) 8 * B);
    std::vector<int> ret(B, 0);
    size_t total = 0;
    for (size_t k = 0; k < B; k++) total += pk[k].index.size();
    if (total < (size_t) ygzf_host_sim3_opt_device_min) {
        for (size_t k = 0; k < B; k++) sim3opt::optimize_host(prob[k], &S[8 * k], removedPtr[k], &ret[k], nullptr);
    } else {
        ygzf_host::Lease lease(ORBextractor::sDevice);
        if (!lease) return;
        if (ygzf_optimize_sim3(lease.get(), (int) B, prob.data(), S.data(), removedPtr.data(), ret.data(), nullptr) != YGZF_OK) {
            ygzf_host::report_failure(who, ygzf_last_error(lease.get()));
            return;
        }
    }
    for (size_t k = 0; k < B; k++) {
        std::vector<MapPoint *> &vpMatches1 = *cands[k].vpMatches1;
        for (size_t j = 0; j < pk[k].index.size(); j++)
            if (pk[k].removed[j]) vpMatches1[pk[k].index[j]] = static_cast<MapPoint *>(nullptr);
        std::memcpy(cands[k].S12, &S[8 * k], 8 * sizeof(double));   // (S12 itself, bit for bit, where :2567 returns before :2591)
        cands[k].nIn = ret[k];
    }
}

}  // namespace ygz
