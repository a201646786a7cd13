// lm_math.h -- what g2o does around one dense N x N vertex, stated once for every optimiser of this library: Eigen's unblocked pivoted LDLT and
// its solve, the Levenberg bookkeeping of optimization_algorithm_levenberg.cpp:61-189 (computeLambdaInit, a trial's push / setLambda / solve,
// rho and the lambda / ni rules, the three stop rules), RobustKernelHuber::robustify and Eigen's fp64 quaternion pieces.  k_pose_opt
// (pose_kernels.hip, N = 6) and k_sim3_opt (sim3_opt_kernels.hip with sim3_opt_math.h, N = 7) call it from their thread-0 slots; plain host
// programs compile this same text with g++ (tests/cpp/lm_host.cc, host/Sim3OptHost.h): nothing of HIP is needed to read it.
//
// Every floating-point operation is + - * / or sqrt on double in the order written, without contraction (-ffp-contract=off), so each is correctly
// rounded and numpy repeats it bit for bit: tests/pose_opt_cases.py holds the one size-generic restatement (ldlt, ldlt_solve, and the
// bookkeeping inside its Levenberg loop), tests/test_lm_host_progs.py holds this file to it for both sizes.  These lines decide whether a step is
// accepted and when a round stops: an optimiser that needs them includes this file, it does not restate them.
//
// What stays with each caller: its edges and their association of J^T W J, the sign of b, the update of its estimate (oplusImpl) and the
// backup / restore of that estimate around a trial (the estimate's type is the caller's).
#ifndef YGZF_LM_MATH_H
#define YGZF_LM_MATH_H
#include <math.h>

// the one set of host-and-device markers of the scalar headers (lm_math.h, sim3_opt_math.h, sim3_math.h)
#if defined(__HIPCC__)
#define YGZF_HD __host__ __device__
#define YGZF_UNROLL _Pragma("unroll")
#define YGZF_ROLLED _Pragma("nounroll")
// a loop of ldlt / ldlt_solve, unrolled in full or not at all.  It reads the N and kUnrolled of the `template <int N, bool kUnrolled>` function it
// stands in, so it is of use in this file only: both macros are undefined again at its end.
#define YGZF_PRAGMA(x) _Pragma(#x)
#define YGZF_LM_LOOP YGZF_PRAGMA(clang loop unroll_count(kUnrolled ? N : 1))
#else
#define YGZF_HD
#define YGZF_UNROLL
#define YGZF_ROLLED
#define YGZF_LM_LOOP
#endif

namespace ygzf {
namespace lm {

constexpr double kDblMax = 1.7976931348623157e308;
enum Stop { kStopMaxIter = 0, kStopTrials = 1, kStopRhoZero = 2, kStopNBad = 3, kStopNotRun = 4 };   // the values of ygzf_pose_stop (include/ygzf.h)

// ---- Eigen's quaternion pieces (x y z w): q * q' = w w' - x x' - y y' - z z' ..; q * v = (v + w uv) + qv x uv, uv = 2 (qv x v) ----------------
YGZF_HD inline void quat_normalize(double q[4]) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
YGZF_HD inline void quat_mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
YGZF_HD inline void quat_rotate(const double q[4], const double v[3], double o[3]) {   // _transformVector
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}

// RobustKernelHuber::robustify: rho[0], rho[1]
YGZF_HD inline void huber(double chi2, double delta, double &rho0, double &rho1) {
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) { rho0 = chi2; rho1 = 1.0; }
    else {
        const double sq = sqrt(chi2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}

// ---- the solver ----------------------------------------------------------------------------------------------------------------------------------
// One vertex's solver state.  x persists across trials, iterations and rounds: a failed solve leaves it as it was.
// kUnrolled says how the device compiles the loops of ldlt and ldlt_solve (the arithmetic is the same either way; a host compiler does not look).
// On the device the state lives in LDS and one lane works on it while 255 wait.  Rolled, every step is an LDS round trip behind a computed
// address; unrolled, the factor stays in registers.  k_pose_opt has the registers and needs them unrolled: 454 / 529 / 842 us per call of 200 /
// 1000 / 2000 correspondences against 781 / 774 / 1117 us rolled.  k_sim3_opt sits at the 256-register ceiling and keeps them rolled, or it
// spills (profiles/lm_math_ab.txt has both sets of figures).
template <int N, bool kUnrolled> struct Lm {
    double H[N * N], Hd[N * N], b[N], x[N], temp[N];
    double lambda, ni, currentChi, iniChi, rho;
    int tr[N];
    int nBadRule, qmax;
};

// Eigen's unblocked lower pivoted LDLT of L.Hd in place (largest |diagonal| first, the first on a tie; the transpositions in L.tr); true: every pivot > 0
template <int N, bool kUnrolled> YGZF_HD inline bool ldlt(Lm<N, kUnrolled> &L) {
    double *m = L.Hd;
YGZF_LM_LOOP
    for (int k = 0; k < N; k++) {
        double big = -1.0;
        int idx = k;
YGZF_LM_LOOP
        for (int j = k; j < N; j++) {
            const double v = fabs(m[(N + 1) * j]);
            if (v > big) { big = v; idx = j; }
        }
        L.tr[k] = idx;
        if (idx != k) {
YGZF_LM_LOOP
            for (int j = 0; j < k; j++) { const double a = m[N * k + j]; m[N * k + j] = m[N * idx + j]; m[N * idx + j] = a; }
YGZF_LM_LOOP
            for (int i = idx + 1; i < N; i++) { const double a = m[N * i + k]; m[N * i + k] = m[N * i + idx]; m[N * i + idx] = a; }
            { const double a = m[(N + 1) * k]; m[(N + 1) * k] = m[(N + 1) * idx]; m[(N + 1) * idx] = a; }
YGZF_LM_LOOP
            for (int i = k + 1; i < idx; i++) { const double a = m[N * i + k]; m[N * i + k] = m[N * idx + i]; m[N * idx + i] = a; }
        }
        if (k > 0) {
YGZF_LM_LOOP
            for (int j = 0; j < k; j++) L.temp[j] = m[(N + 1) * j] * m[N * k + j];
            double s = m[N * k] * L.temp[0];
YGZF_LM_LOOP
            for (int j = 1; j < k; j++) s = s + m[N * k + j] * L.temp[j];
            m[(N + 1) * k] = m[(N + 1) * k] - s;
YGZF_LM_LOOP
            for (int i = k + 1; i < N; i++) {
                double s2 = m[N * i] * L.temp[0];
YGZF_LM_LOOP
                for (int j = 1; j < k; j++) s2 = s2 + m[N * i + j] * L.temp[j];
                m[N * i + k] = m[N * i + k] - s2;
            }
        }
YGZF_LM_LOOP
        for (int i = k + 1; i < N; i++) m[N * i + k] = m[N * i + k] / m[(N + 1) * k];
    }
    bool positive = true;
YGZF_LM_LOOP
    for (int k = 0; k < N; k++) positive = positive && (m[(N + 1) * k] > 0);
    return positive;
}
template <int N, bool kUnrolled> YGZF_HD inline void ldlt_solve(Lm<N, kUnrolled> &L) {   // x = P^T L^-T D^-1 L^-1 P b
    const double *m = L.Hd;
    double *x = L.x;
YGZF_LM_LOOP
    for (int k = 0; k < N; k++) x[k] = L.b[k];
YGZF_LM_LOOP
    for (int k = 0; k < N; k++) { const double a = x[k]; x[k] = x[L.tr[k]]; x[L.tr[k]] = a; }
YGZF_LM_LOOP
    for (int i = 0; i < N; i++)
YGZF_LM_LOOP
        for (int j = 0; j < i; j++) x[i] = x[i] - m[N * i + j] * x[j];
YGZF_LM_LOOP
    for (int i = 0; i < N; i++) x[i] = x[i] / m[(N + 1) * i];
YGZF_LM_LOOP
    for (int i = N - 1; i >= 0; i--)
YGZF_LM_LOOP
        for (int j = i + 1; j < N; j++) x[i] = x[i] - m[N * j + i] * x[j];
YGZF_LM_LOOP
    for (int k = N - 1; k >= 0; k--) { const double a = x[k]; x[k] = x[L.tr[k]]; x[L.tr[k]] = a; }
}
// a solver before its first optimize() call (x: the reference never initialises it in a release build, this library starts it at zero)
template <int N, bool kUnrolled> YGZF_HD inline void init(Lm<N, kUnrolled> &L) {
    for (int k = 0; k < N; k++) L.x[k] = 0.0;
    L.lambda = -1.0;
    L.ni = 2;
}
// a fresh linearisation: the N (N + 1) / 2 upper sums of H (row-major, j <= k), b and the active robust chi2; computeLambdaInit at iteration 0 of
// an optimize() call
template <int N, bool kUnrolled> YGZF_HD inline void iteration_begin(Lm<N, kUnrolled> &L, const double *upper, const double *b, double chi2, bool first) {
    int c = 0;
    for (int j = 0; j < N; j++)
        for (int k = j; k < N; k++) { L.H[N * j + k] = upper[c]; L.H[N * k + j] = upper[c]; c++; }
    for (int j = 0; j < N; j++) L.b[j] = b[j];
    L.currentChi = chi2;
    L.iniChi = L.currentChi;
    if (first) {
        double maxDiagonal = 0.;
        for (int j = 0; j < N; j++) { const double v = fabs(L.H[(N + 1) * j]); maxDiagonal = (v < maxDiagonal) ? maxDiagonal : v; }   // std::max(fabs(H_jj), maxDiagonal)
        L.lambda = 1e-5 * maxDiagonal;
        L.ni = 2;
        L.nBadRule = 0;
    }
    L.rho = 0;
    L.qmax = 0;
}
// the head of a Levenberg trial (:103-113): push, setLambda, solve.  A failed solve (false) leaves x as it was, and the caller's update()
// applies it all the same.
template <int N, bool kUnrolled> YGZF_HD inline bool trial_solve(Lm<N, kUnrolled> &L) {
    for (int k = 0; k < N * N; k++) L.Hd[k] = L.H[k];
    for (int j = 0; j < N; j++) L.Hd[(N + 1) * j] = L.H[(N + 1) * j] + L.lambda;
    const bool ok = ldlt(L);
    if (ok) ldlt_solve(L);
    return ok;
}
// the tail of the trial (:123-149), tempChi the active robust chi2 at the updated estimate; true: another trial follows.  restore: the step is
// rejected, the caller puts its estimate back (discardTop of the accepted one is nothing to do).
template <int N, bool kUnrolled> YGZF_HD inline bool trial_end(Lm<N, kUnrolled> &L, bool ok, double tempChi, bool &restore) {
    if (!ok) tempChi = kDblMax;
    double scale = 0.0;
    for (int j = 0; j < N; j++) scale = scale + L.x[j] * (L.lambda * L.x[j] + L.b[j]);
    scale = scale + 1e-3;
    L.rho = (L.currentChi - tempChi) / scale;
    restore = !(L.rho > 0 && tempChi - tempChi == 0.0);   // g2o_isfinite(tempChi)
    if (!restore) {
        const double c = 2 * L.rho - 1;
        double alpha = 1.0 - c * c * c;
        alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;
        const double scaleFactor = (1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0;
        L.lambda = L.lambda * scaleFactor;
        L.ni = 2;
        L.currentChi = tempChi;
    } else {
        L.lambda = L.lambda * L.ni;
        L.ni = L.ni * 2;
    }
    L.qmax++;
    return L.rho < 0 && L.qmax < 10;
}
// after the trials of an iteration: -1 to go on, else the Stop that ends the optimize() call
template <int N, bool kUnrolled> YGZF_HD inline int iteration_end(Lm<N, kUnrolled> &L) {
    if (L.qmax == 10 || L.rho == 0) return L.qmax == 10 ? kStopTrials : kStopRhoZero;
    if ((L.iniChi - L.currentChi) * 1e3 < L.iniChi) L.nBadRule++;
    else L.nBadRule = 0;
    return L.nBadRule >= 3 ? kStopNBad : -1;
}

}  // namespace lm
}  // namespace ygzf
#undef YGZF_LM_LOOP
#undef YGZF_PRAGMA
#endif
