// sim3_opt_kernels.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:2409-2594): one free VertexSim3Expmap, a pair of projection edges per
// correspondence (e12 through K1 at the estimate, e21 through K2 at its inverse), Huber kernels, g2o's Levenberg over the dense 7 x 7 system,
// optimize(5), the chi2 gate, optimize(nBad > 0 ? 10 : 5), the gate again.  The arithmetic is csrc/sim3_opt_math.h (Sim3, the edges) and
// csrc/lm_math.h (the Levenberg solver, shared with k_pose_opt), compiled here and by the host programs alike; this file is the plan around it.
// Product code.
//
// k_sim3_opt: one workgroup of 256 threads per problem, both rounds x <= 10 iterations x <= 10 trials in one launch.  Every loop is bounded by
// those constants and leaves through them whatever the numbers are (NaN and Inf included); there is no spin wait and no communication between
// workgroups.  Everything is fp64 apart from the one float rounding of project().
//
// Per iteration lanes 0 .. 14 build the 15 forward transforms (S, Sim3(+-delta e_d) S) and their inverses in LDS; a thread then evaluates e12
// at the forward ones and e21 at the inverses for its correspondences and keeps the 36 sums (28 upper entries of H, 7 of b, the robust chi2) in
// registers.  The "device order" of the sums: correspondence c belongs to thread c % 256, ascending c per thread, e12 then e21 of a
// correspondence; lanes by wave_sum_f64 (a balanced tree of neighbours), the four waves in wave order through LDS.  No floating-point atomics:
// the same bits on every run.
//
// What a g2o edge remembers between calls is kept per pair in HBM: its state (`removed`: 0 active, 1 removed after round 0) and the chi2 of both
// edges' _error member as of the last computeError (`stored`) -- computeActiveErrors leaves the errors of the last *trial* there, accepted or
// not (linearizeOplus restores _error after its perturbations), and that is what the gates read.  A pair is read and written by one thread only.
#include "kernels.h"
#include "sim3_opt_math.h"
#include "wave_ops.h"

namespace ygzf {

namespace {

namespace so = sim3opt;

constexpr int kSoThreads = 256;

struct SoShared {
    so::S3 T[2 * so::kTransforms];   // 15 forward transforms, then their 15 inverses
    so::S3 est, backup;
    double red[4][so::kSums];
    double sum[so::kSums];
    lm::Lm<so::kDim, false> lm;            // the one lane's solver state (LDS: indexed dynamically)
    int nBad, nIn, ctl;
};

static_assert(sizeof(so::S3) == 8 * sizeof(double), "k_sim3_opt copies an S3 as 8 doubles");

struct SoPair {
    double p1[3], p2[3], o1[2], o2[2], s1, s2;
};
__device__ __forceinline__ void so_load(const Sim3OptProblemDev &P, int c, SoPair &Q) {
    const size_t i = (size_t) c;
    for (int k = 0; k < 3; k++) { Q.p1[k] = (double) P.P1c[3 * i + k]; Q.p2[k] = (double) P.P2c[3 * i + k]; }
    for (int k = 0; k < 2; k++) { Q.o1[k] = (double) P.obs1[2 * i + k]; Q.o2[k] = (double) P.obs2[2 * i + k]; }
    Q.s1 = (double) P.invSigma2_1[i];
    Q.s2 = (double) P.invSigma2_2[i];
}

// computeActiveErrors + linearizeOplus + constructQuadraticForm + activeRobustChi2 over the active pairs at the 30 transforms of S.T
__device__ void so_pass_system(const Sim3OptProblemDev &P, SoShared &S, const so::Cam &K1, const so::Cam &K2) {
    double acc[so::kSums];
#pragma unroll
    for (int k = 0; k < so::kSums; k++) acc[k] = 0.0;
    for (int c = threadIdx.x; c < P.n; c += kSoThreads) {
        if (P.removed[c]) continue;
        SoPair Q;
        so_load(P, c, Q);
        P.stored[2 * (size_t) c] = so::so_edge_system(S.T, Q.p2, K1, Q.o1, Q.s1, P.delta, acc);
        P.stored[2 * (size_t) c + 1] = so::so_edge_system(S.T + so::kTransforms, Q.p1, K2, Q.o2, Q.s2, P.delta, acc);
    }
    block_sum_f64(acc, S.red, S.sum);
}
// computeActiveErrors + activeRobustChi2 at the trial estimate (S.T[0] and its inverse S.T[15])
__device__ void so_pass_chi2(const Sim3OptProblemDev &P, SoShared &S, const so::Cam &K1, const so::Cam &K2) {
    double acc[1] = {0.0};
    const so::S3 fwd = S.T[0], inv = S.T[so::kTransforms];
    for (int c = threadIdx.x; c < P.n; c += kSoThreads) {
        if (P.removed[c]) continue;
        SoPair Q;
        so_load(P, c, Q);
        double e[2], rho0, rho1;
        so::so_error(fwd, Q.p2, K1, Q.o1, e);
        const double c12 = so::so_chi2(e, Q.s1);
        lm::huber(c12, P.delta, rho0, rho1);
        acc[0] = acc[0] + rho0;
        so::so_error(inv, Q.p1, K2, Q.o2, e);
        const double c21 = so::so_chi2(e, Q.s2);
        lm::huber(c21, P.delta, rho0, rho1);
        acc[0] = acc[0] + rho0;
        P.stored[2 * (size_t) c] = c12;
        P.stored[2 * (size_t) c + 1] = c21;
    }
    block_sum_f64(acc, S.red, S.sum);
}

__global__ __launch_bounds__(kSoThreads) void k_sim3_opt(Sim3OptArgs A) {
    __shared__ SoShared S;
    const Sim3OptProblemDev P = A.probs[blockIdx.x];
    Sim3OptOut &out = A.out[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = P.n;
    const bool fix = P.fixScale != 0;
    const so::Cam K1 = {P.K1[0], P.K1[1], P.K1[2], P.K1[3]}, K2 = {P.K2[0], P.K2[1], P.K2[2], P.K2[3]};
    if (tid == 0) {
        for (int k = 0; k < 8; k++) out.S[k] = P.S12[k];
        for (int r = 0; r < 2; r++) { out.iters[r] = 0; out.trials[r] = 0; out.stop[r] = lm::kStopNotRun; out.lambda[r] = 0; out.chi2[r] = 0; }
        out.ret = 0;
        out.nBad = 0;
        for (int k = 0; k < 4; k++) S.est.q[k] = P.S12[k];
        for (int k = 0; k < 3; k++) S.est.t[k] = P.S12[4 + k];
        S.est.s = P.S12[7];
        lm::init(S.lm);
        S.nBad = 0;
        S.nIn = 0;
    }
    for (int c = tid; c < n; c += kSoThreads) P.removed[c] = 0;
    if (n == 0) return;                               // nothing runs
    int nBad = 0;
    for (int rnd = 0; rnd < 2; rnd++) {
        const int maxIt = rnd == 0 ? 5 : (nBad > 0 ? 10 : 5);
        int reason = lm::kStopMaxIter, iters = 0, trials = 0;   // (thread 0's)
        for (int it = 0; it < maxIt; it++) {
            __syncthreads();
            if (tid < so::kTransforms) so::so_transform(S.est, tid, fix, S.T[tid], S.T[so::kTransforms + tid]);
            __syncthreads();
            so_pass_system(P, S, K1, K2);
            if (tid == 0) lm::iteration_begin(S.lm, S.sum, S.sum + 28, S.sum[35], it == 0);
            for (int trial = 0; trial < 10; trial++) {
                bool ok = false;
                if (tid == 0) {
                    S.backup = S.est;
                    ok = lm::trial_solve(S.lm);
                    so::so_oplus(S.lm.x, fix, S.est);
                    S.T[0] = S.est;
                    so::so_inverse(S.est, S.T[so::kTransforms]);
                }
                __syncthreads();
                so_pass_chi2(P, S, K1, K2);
                if (tid == 0) {
                    double backup[8];                 // (read before trial_end's LDS writes, not behind them)
                    lds_read_now(reinterpret_cast<const double *>(&S.backup), backup);
                    bool restore;
                    S.ctl = lm::trial_end(S.lm, ok, S.sum[0], restore) ? 1 : 0;
                    if (restore)
                        for (int k = 0; k < 8; k++) reinterpret_cast<double *>(&S.est)[k] = backup[k];
                }
                __syncthreads();
                if (!S.ctl) break;
            }
            __syncthreads();                          // (S.ctl is read by all before thread 0 writes it again)
            if (tid == 0) {
                iters++;
                trials += S.lm.qmax;
                const int stop = lm::iteration_end(S.lm);
                if (stop >= 0) reason = stop;
                S.ctl = stop >= 0 ? 1 : 0;
            }
            __syncthreads();
            const int ended = S.ctl;
            __syncthreads();
            if (ended) break;
        }
        if (tid == 0) {
            out.iters[rnd] = iters; out.trials[rnd] = trials; out.stop[rnd] = reason;
            out.lambda[rnd] = S.lm.lambda; out.chi2[rnd] = S.lm.currentChi;
        }
        {   // :2542-2559 / :2575-2587: both edges keep the error of the last trial; `chi2() > th2`, a double against the float th2
            int bad = 0, in = 0;
            for (int c = tid; c < n; c += kSoThreads) {
                if (P.removed[c]) continue;
                const bool isBad = P.stored[2 * (size_t) c] > P.th2 || P.stored[2 * (size_t) c + 1] > P.th2;
                if (isBad) { P.removed[c] = rnd == 0 ? 1 : 2; bad++; }
                else in++;
            }
            if (rnd == 0 && bad) atomicAdd(&S.nBad, bad);
            if (rnd == 1 && in) atomicAdd(&S.nIn, in);
        }
        __syncthreads();
        if (rnd == 0) {
            nBad = S.nBad;
            if (tid == 0) out.nBad = nBad;
            if (n - nBad < 10) return;                // :2567 -- ret = 0 and g2oS12 is not written
        }
    }
    if (tid == 0) {
        for (int k = 0; k < 4; k++) out.S[k] = S.est.q[k];
        for (int k = 0; k < 3; k++) out.S[4 + k] = S.est.t[k];
        out.S[7] = S.est.s;
        out.ret = S.nIn;
    }
}

}  // namespace

void launch_sim3_opt(hipStream_t st, const Sim3OptArgs &A, int nProblems) {
    hipLaunchKernelGGL(k_sim3_opt, dim3(nProblems), dim3(kSoThreads), 0, st, A);
}

}  // namespace ygzf
