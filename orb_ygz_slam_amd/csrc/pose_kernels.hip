// pose_kernels.hip -- Optimizer::PoseOptimization(Frame *) (src/Optimizer.cc:1656-1842): the single-vertex, motion-only problem with exactly the
// g2o and Sophus arithmetic it runs, in fp64.  Here: the two ...OnlyPose edges of types_six_dof_expmap with their analytic Jacobian (unary
// edges with a Huber kernel, weight rho[1] only), SE3d::exp and `*`, and the plan of the rounds.  g2o's Levenberg over the dense 6 x 6 system,
// its pivoted LDLT, Huber's robustify and the quaternion products are csrc/lm_math.h, shared with k_sim3_opt.  Product code.
//
// k_pose_opt: one workgroup of 256 threads per problem, all four rounds x <= 10 iterations x <= 10 trials in one launch.  Every loop is bounded by
// those constants and leaves through them whatever the numbers are (NaN and Inf included); there is no spin wait and no communication between
// workgroups.  tests/pose_opt_cases.py restates every formula below in numpy, term by term and in the same order (this file is compiled with
// -ffp-contract=off like the rest of the library: products and sums round as written).
//
// The "device order" of the sums H (21 upper entries), g (6) and chi2: frame index i belongs to thread i % 256, ascending i per thread; lanes by
// wave_sum_f64 (a balanced tree of neighbours), the four waves in wave order through LDS.  No floating-point atomics: the same bits on every run.
//
// What a g2o edge remembers between calls is kept per edge in HBM: its level is the outlier flag itself (level 1 == outlier, set together at
// :1795-1802), and the chi2 of its _error member as of the last computeError lives in `stored` -- computeActiveErrors leaves the errors of the
// last *trial* there, accepted or not, and that is what the classification at the end of a round reads for level-0 edges (:1793).
#include "kernels.h"
#include "lm_math.h"
#include "wave_ops.h"

namespace ygzf {

namespace {

constexpr int kPoseThreads = 256;
constexpr int kPoseSums = 28;   // 21 + 6 + 1

struct PoseShared {
    double pose[7];             // the vertex estimate: q (x y z w), t
    double backup[7];
    double T0[7];               // pFrame->mTcw.cast<double>()
    double red[4][kPoseSums];
    double sum[kPoseSums];
    lm::Lm<6, true> lm;               // the one lane's solver state (LDS: indexed dynamically)
    int nInitial, nBad, ctl;
};

__device__ __forceinline__ void d_quat_to_R(const double q[4], double R[9]) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
// Sophus SE3d::exp of (upsilon, omega) (se3.hpp:406-428, so3.hpp:425-456; epsilon 1e-10)
__device__ void d_se3_exp(const double a[6], double q[4], double t[3]) {
    const double *om = a + 3;
    const double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    const double theta = sqrt(theta_sq);
    const double half_theta = 0.5 * theta;
    const bool small = theta < 1e-10;
    double imag_factor, real_factor;
    if (small) {
        const double theta_po4 = theta_sq * theta_sq;
        imag_factor = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
        real_factor = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * theta_po4;
    } else {
        imag_factor = sin(half_theta) / theta;
        real_factor = cos(half_theta);
    }
    q[0] = imag_factor * om[0]; q[1] = imag_factor * om[1]; q[2] = imag_factor * om[2]; q[3] = real_factor;
    lm::quat_normalize(q);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double V[9];
    if (small) {
        d_quat_to_R(q, V);
    } else {
        const double theta_sq2 = theta * theta;
        const double c1 = (1.0 - cos(theta)) / theta_sq2;
        const double c2 = (theta - sin(theta)) / (theta_sq2 * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double o2 = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
                V[3 * i + j] = ((i == j) ? 1.0 : 0.0) + c1 * O[3 * i + j] + c2 * o2;
            }
    }
    for (int i = 0; i < 3; i++) t[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2];
}

struct PoseEdge {
    double p[3], e[3], s, chi2;
    bool stereo;
};
// computeError + chi2() of edge i at the pose (q, t): EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
__device__ __forceinline__ void pose_edge(const PoseArgs &A, const PoseProblemDev &P, int i, const double q[4], const double t[3], PoseEdge &E) {
    const ygzf_kp kp = P.keys[i];
    const float ur = P.uRight ? P.uRight[i] : -1.f;
    E.stereo = !(ur < 0);
    const double X[3] = {(double) P.world[3 * (size_t) i], (double) P.world[3 * (size_t) i + 1], (double) P.world[3 * (size_t) i + 2]};
    double r[3];
    lm::quat_rotate(q, X, r);
    E.p[0] = r[0] + t[0]; E.p[1] = r[1] + t[1]; E.p[2] = r[2] + t[2];
    E.s = (double) A.invSigma2[kp.octave];
    const double ox = (double) kp.x, oy = (double) kp.y;
    if (E.stereo) {
        const double invz = (double) (float) (1.0 / E.p[2]);   // cam_project: `const float invz = 1.0f / trans_xyz[2]`
        const double r0 = E.p[0] * invz * A.fx + A.cx;
        E.e[0] = ox - r0;
        E.e[1] = oy - (E.p[1] * invz * A.fy + A.cy);
        E.e[2] = (double) ur - (r0 - A.bf * invz);
        E.chi2 = E.e[0] * (E.s * E.e[0]) + E.e[1] * (E.s * E.e[1]) + E.e[2] * (E.s * E.e[2]);
    } else {
        E.e[0] = ox - (E.p[0] / E.p[2] * A.fx + A.cx);
        E.e[1] = oy - (E.p[1] / E.p[2] * A.fy + A.cy);
        E.e[2] = 0.0;
        E.chi2 = E.e[0] * (E.s * E.e[0]) + E.e[1] * (E.s * E.e[1]);
    }
}
// robustify with the edge's kernel; setRobustKernel(0) in round 3: rho = (chi2, 1)
__device__ __forceinline__ void pose_robustify(double chi2, double delta, bool kernel, double &rho0, double &rho1) {
    if (kernel) lm::huber(chi2, delta, rho0, rho1);
    else { rho0 = chi2; rho1 = 1.0; }
}

// One pass over the problem's active edges at S.pose: computeActiveErrors, and either the whole system (linearizeOplus + constructQuadraticForm +
// activeRobustChi2: 28 sums) or activeRobustChi2 alone.  Result in S.sum (valid for thread 0 after the pass).
template <bool kSystem>
__device__ void pose_pass(const PoseArgs &A, const PoseProblemDev &P, PoseShared &S, bool kernel) {
    const int tid = threadIdx.x;
    double q[4], t[3];
    for (int k = 0; k < 4; k++) q[k] = S.pose[k];
    for (int k = 0; k < 3; k++) t[k] = S.pose[4 + k];
    constexpr int kN = kSystem ? kPoseSums : 1;
    double acc[kN];
#pragma unroll
    for (int k = 0; k < kN; k++) acc[k] = 0.0;
    for (int i = tid; i < P.n; i += kPoseThreads) {
        if (!P.mpValid[i] || P.outlier[i]) continue;   // not an edge / level 1
        PoseEdge E;
        pose_edge(A, P, i, q, t, E);
        P.stored[i] = E.chi2;
        double rho0, rho1;
        pose_robustify(E.chi2, E.stereo ? A.deltaStereo : A.deltaMono, kernel, rho0, rho1);
        if (!kSystem) {
            acc[0] = acc[0] + rho0;
            continue;
        }
        const double x = E.p[0], y = E.p[1];
        const double invz = 1.0 / E.p[2];
        const double invz_2 = invz * invz;
        double J[3][6];
        J[0][0] = x * y * invz_2 * A.fx;
        J[0][1] = -(1 + (x * x * invz_2)) * A.fx;
        J[0][2] = y * invz * A.fx;
        J[0][3] = -invz * A.fx;
        J[0][4] = 0;
        J[0][5] = x * invz_2 * A.fx;
        J[1][0] = (1 + y * y * invz_2) * A.fy;
        J[1][1] = -x * y * invz_2 * A.fy;
        J[1][2] = -x * invz * A.fy;
        J[1][3] = 0;
        J[1][4] = -invz * A.fy;
        J[1][5] = y * invz_2 * A.fy;
        J[2][0] = J[0][0] - A.bf * y * invz_2;
        J[2][1] = J[0][1] + A.bf * x * invz_2;
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0;
        J[2][5] = J[0][5] - A.bf * invz_2;
        const double w = rho1 * E.s;
        int c = 0;
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int k = j; k < 6; k++) {
                double a = J[0][j] * (w * J[0][k]) + J[1][j] * (w * J[1][k]);
                if (E.stereo) a = a + J[2][j] * (w * J[2][k]);
                acc[c] = acc[c] + a;
                c++;
            }
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double a = J[0][j] * (E.s * E.e[0]) + J[1][j] * (E.s * E.e[1]);
            if (E.stereo) a = a + J[2][j] * (E.s * E.e[2]);
            acc[21 + j] = acc[21 + j] + rho1 * a;
        }
        acc[27] = acc[27] + rho0;
    }
    block_sum_f64(acc, S.red, S.sum);
}

// the update of a trial, VertexSE3Expmap::oplusImpl: estimate = SE3d::exp(x[3..5], x[0..2]) * estimate
__device__ void pose_oplus(const double x[6], double pose[7]) {
    const double u[6] = {x[3], x[4], x[5], x[0], x[1], x[2]};
    double qe[4], te[3], q[4], r[3];
    d_se3_exp(u, qe, te);
    lm::quat_rotate(qe, pose + 4, r);            // SE3d::operator*: fastMultiply + normalize
    lm::quat_mul(qe, pose, q);
    lm::quat_normalize(q);
    for (int k = 0; k < 4; k++) pose[k] = q[k];
    for (int k = 0; k < 3; k++) pose[4 + k] = te[k] + r[k];
}

__global__ __launch_bounds__(kPoseThreads) void k_pose_opt(PoseArgs A) {
    __shared__ PoseShared S;
    const PoseProblemDev P = A.probs[blockIdx.x];
    PoseOut &out = A.out[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) { S.nInitial = 0; S.nBad = 0; }
    __syncthreads();
    {   // :1696-1763: every correspondence starts as an inlier
        int cnt = 0;
        for (int i = tid; i < P.n; i += kPoseThreads)
            if (P.mpValid[i]) { P.outlier[i] = 0; cnt++; }
        if (cnt) atomicAdd(&S.nInitial, cnt);
    }
    __syncthreads();
    const int nInitial = S.nInitial;
    if (tid == 0) {
        out.nInitial = nInitial;
        for (int r = 0; r < 4; r++) { out.iters[r] = 0; out.trials[r] = 0; out.stop[r] = lm::kStopNotRun; out.lambda[r] = 0; out.chi2[r] = 0; }
        double q[4] = {(double) P.Tcw[0], (double) P.Tcw[1], (double) P.Tcw[2], (double) P.Tcw[3]};
        lm::quat_normalize(q);                      // SE3f::cast<double>()
        for (int k = 0; k < 4; k++) S.T0[k] = q[k];
        for (int k = 0; k < 3; k++) S.T0[4 + k] = (double) P.Tcw[4 + k];
        lm::init(S.lm);
    }
    if (nInitial < 3) {                           // :1767 -- the pose stays as it is
        if (tid == 0) out.ret = 0;
        return;
    }
    bool kernel = true;
    for (int rnd = 0; rnd < 4; rnd++) {
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < 7; k++) S.pose[k] = S.T0[k];   // :1779, every round
        __syncthreads();
        int reason = lm::kStopMaxIter, iters = 0, trials = 0;      // (thread 0's)
        for (int it = 0; it < 10; it++) {
            pose_pass<true>(A, P, S, kernel);
            if (tid == 0) {
                double b[6];
                for (int j = 0; j < 6; j++) b[j] = -S.sum[21 + j];   // b = -g
                lm::iteration_begin(S.lm, S.sum, b, S.sum[27], it == 0);
            }
            for (int trial = 0; trial < 10; trial++) {
                bool ok = false;
                if (tid == 0) {
                    for (int k = 0; k < 7; k++) S.backup[k] = S.pose[k];
                    ok = lm::trial_solve(S.lm);
                    pose_oplus(S.lm.x, S.pose);
                }
                __syncthreads();
                pose_pass<false>(A, P, S, kernel);
                if (tid == 0) {
                    double backup[7];                 // (read before trial_end's LDS writes, not behind them)
                    lds_read_now(S.backup, backup);
                    bool restore;
                    S.ctl = lm::trial_end(S.lm, ok, S.sum[0], restore) ? 1 : 0;
                    if (restore)
                        for (int k = 0; k < 7; k++) S.pose[k] = backup[k];
                }
                __syncthreads();
                if (!S.ctl) break;
            }
            __syncthreads();                      // (S.ctl is read by all before thread 0 writes it again)
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
            S.nBad = 0;
        }
        __syncthreads();
        {   // :1783-1830: outliers are evaluated at the round's pose, inliers keep the error of the last trial; raw chi2 as a float against the gate
            double q[4], t[3];
            for (int k = 0; k < 4; k++) q[k] = S.pose[k];
            for (int k = 0; k < 3; k++) t[k] = S.pose[4 + k];
            int bad = 0;
            for (int i = tid; i < P.n; i += kPoseThreads) {
                if (!P.mpValid[i]) continue;
                PoseEdge E;
                pose_edge(A, P, i, q, t, E);
                double chi2 = P.stored[i];
                if (P.outlier[i]) { chi2 = E.chi2; P.stored[i] = chi2; }
                const bool isBad = (float) chi2 > (E.stereo ? 7.815f : 5.991f);
                P.outlier[i] = isBad ? 1 : 0;
                bad += isBad ? 1 : 0;
            }
            if (bad) atomicAdd(&S.nBad, bad);
        }
        if (rnd == 2) kernel = false;             // e->setRobustKernel(0)
        if (nInitial < 10) break;                 // optimizer.edges().size() < 10
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 7; k++) out.T[k] = S.pose[k];
        out.ret = nInitial - S.nBad;
    }
}

}  // namespace

void launch_pose_opt(hipStream_t st, const PoseArgs &A, int nProblems) {
    hipLaunchKernelGGL(k_pose_opt, dim3(nProblems), dim3(kPoseThreads), 0, st, A);
}

}  // namespace ygzf
