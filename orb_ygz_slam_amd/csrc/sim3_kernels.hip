// sim3_kernels.hip -- Sim3Solver's RANSAC hypotheses (src/Sim3Solver.cc:132-193: ComputeSim3 + CheckInliers per iteration), every hypothesis of
// every problem of a call in one launch.  Hypotheses are independent of each other: the order in which the solver looks at their inlier counts
// (the best-so-far and return rules of iterate) is replayed on the host from what this kernel leaves behind (host/Sim3Replay.h).
//
// One wave per hypothesis, four waves per workgroup; wave g of the launch takes hypothesis g of the call's concatenated list, so the waves of
// one workgroup may belong to different problems.  Horn's closed form runs wave-uniform (every lane the same few hundred fp32 operations:
// sim3_math.h), then the wave counts the inliers (ransac_device.h).  Nothing is shared between waves: no LDS, no barrier, no atomics.  Every
// loop is bounded by an argument (n, the problem count) or a constant (YGZF_SIM3_JACOBI_SWEEPS).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "ransac_device.h"
#include "sim3_math.h"

namespace ygzf {

namespace {

constexpr int kSim3Waves = 4, kSim3Threads = 64 * kSim3Waves;

__global__ __launch_bounds__(kSim3Threads) void k_sim3_ransac(Sim3Args A) {
    const int lane = threadIdx.x & 63;
    const int g = (int) blockIdx.x * kSim3Waves + ((int) threadIdx.x >> 6);   // wave-uniform
    if (g >= A.totalHyp) return;
    const Sim3ProblemDev &P = ransac::problem_of(A.probs, A.nProblems, g);
    const int h = g - P.firstHyp;
    if (h < 0 || h >= P.nHyp) return;   // (cannot happen with the host's table; a wrong table must not turn into a stray write)
    const int n = P.n;
    float p1[3][3], p2[3][3], K1[4], K2[4];
    for (int k = 0; k < 3; k++) {
        const int idx = P.samples[3 * h + k];   // checked by the host: inside [0, n)
        for (int a = 0; a < 3; a++) {
            p1[k][a] = P.X1[3 * idx + a];
            p2[k][a] = P.X2[3 * idx + a];
        }
    }
    for (int k = 0; k < 4; k++) { K1[k] = P.K1[k]; K2[k] = P.K2[k]; }
    sim3::Hyp H;
    sim3::horn(p1, p2, P.fixScale != 0, H);
    const int words = (n + 63) >> 6;
    const int count = ransac::count_inliers(n, lane, P.bits ? P.bits + (size_t) h * words : nullptr, [&](int i) {
        const float X1[3] = {P.X1[3 * i], P.X1[3 * i + 1], P.X1[3 * i + 2]}, X2[3] = {P.X2[3 * i], P.X2[3 * i + 1], P.X2[3 * i + 2]};
        return sim3::inlier(H, X1, X2, K1, K2, P.maxErr1[i], P.maxErr2[i]);
    });
    if (lane == 0) {
        float *o = P.hyp + (size_t) sim3::kHypFloats * h;
        for (int i = 0; i < 9; i++) o[i] = H.R[i];
        for (int i = 0; i < 3; i++) o[9 + i] = H.t[i];
        o[12] = H.s;
        P.nInliers[h] = count;
    }
}

}  // namespace

void launch_sim3_ransac(hipStream_t st, const Sim3Args &A) {
    if (A.totalHyp <= 0) return;
    hipLaunchKernelGGL(k_sim3_ransac, dim3((A.totalHyp + kSim3Waves - 1) / kSim3Waves), dim3(kSim3Threads), 0, st, A);
}

}  // namespace ygzf
