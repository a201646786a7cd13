// sim3_opt_math.h -- the arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:2409-2594) as scalar fp64 code: g2o's Sim3 (types/sim3.h),
// the two projection edges of types_seven_dof_expmap.h with their numeric Jacobian (core/base_binary_edge.hpp:131-205: this fork comments the
// analytic linearizeOplus out), Huber's robustify, Eigen's 7 x 7 pivoted LDLT and the Levenberg bookkeeping of
// optimization_algorithm_levenberg.cpp:61-189.  k_sim3_opt (sim3_opt_kernels.hip) and plain host programs (tests/cpp/sim3_opt_host.cc, the
// one-thread yardstick of tools/sim3_opt_rate.py) compile this same text: nothing of HIP is needed to read it.  tests/sim3_opt_cases.py
// restates it operation by operation.
//
// Every floating-point operation is + - * / or sqrt on double without contraction (-ffp-contract=off), so each is correctly rounded and numpy
// repeats it bit for bit -- with ONE rounding to float: project() returns a Vector2f (se3_ops.hpp:49-55), so x / z and y / z are rounded to
// float before cam_map widens them again.  A +-1e-9 perturbation moves the quotient by ~1e-9 and a float ulp there is ~3e-8: the numeric
// Jacobian is a dither (mostly 0, else multiples of ulp fx / 2e-9).  That is what the reference runs, so every operation below has to round
// exactly as written; "close in fp64" is not a contract for this file.
//
// Where the reference leaves an evaluation order to Eigen's expression templates this file states one:
//   Quaterniond(R)      Eigen's QuaternionBase::operator=(MatrixBase): trace (m00 + m11) + m22, the four branches, no normalisation
//   q * q', q * v       as csrc/pose_kernels.hip: w w' - x x' - y y' - z z' ..; uv = 2 (qv x v), (v + w uv) + qv x uv
//   R                   (I + a Omega) + b Omega2 entry by entry; Omega2 = Omega Omega with each dot from its first term on
//   W                   (A Omega + B Omega2) + C I; t = W upsilon, each dot from its first term on
//   chi2                e0 (s e0) + e1 (s e1)
//   per edge            H_jk += (J_0j w) J_0k + (J_1j w) J_1k, w = rho1 s;   b_j += J_0j r0 + J_1j r1, r_i = (-(s e_i)) rho1   (weight rho[1] only)
// The reference's g2o needs Eigen, which this repository cannot build against: parity with a compiled g2o is unpinned.
//
// sin, cos and exp are written out below from the same five operations (so_sincos, so_exp): a bounded argument reduction and a fixed-length
// polynomial, defined and deterministic for every input.  Largest distance from libm, measured on the CPU by tests/test_sim3_opt_cases.py over
// 20 001 even steps of |theta| <= pi and of |sigma| <= 1:  sin 2.3e-16, cos 1.2e-16 (absolute), exp 2.3e-16 (relative) -- each below the bound
// YGZF_SIM3_OPT_LIBM_EPS.  exp(+-1e-9) of the Jacobian's seventh column goes through so_exp as well.
#ifndef YGZF_SIM3_OPT_MATH_H
#define YGZF_SIM3_OPT_MATH_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define YGZF_SO_HD __host__ __device__
#define YGZF_SO_UNROLL _Pragma("unroll")
#define YGZF_SO_ROLLED _Pragma("nounroll")
#else
#define YGZF_SO_HD
#define YGZF_SO_UNROLL
#define YGZF_SO_ROLLED
#endif

// the recorded bound on |so_sin - sin|, |so_cos - cos| (absolute, |theta| <= pi) and |so_exp / exp - 1| (|sigma| <= 1); tests/sim3_opt_cases.py
// carries the same figure
#define YGZF_SIM3_OPT_LIBM_EPS 5e-16

namespace ygzf {
namespace sim3opt {

constexpr int kDim = 7;
constexpr int kSums = 36;            // 28 upper entries of H (row-major, j <= k), 7 of b, the robust chi2
constexpr int kTransforms = 15;      // S, then Sim3(+delta e_d) S and Sim3(-delta e_d) S for d = 0 .. 6
constexpr double kDelta = 1e-9;      // base_binary_edge.hpp:147
constexpr double kDblMax = 1.7976931348623157e308;
enum Stop { kStopMaxIter = 0, kStopTrials = 1, kStopRhoZero = 2, kStopNBad = 3, kStopNotRun = 4 };   // the values of ygzf_pose_stop

struct S3 { double q[4], t[3], s; };    // r.x r.y r.z r.w, t, s: 8 doubles
struct Cam { double fx, fy, cx, cy; };

// ---- sin, cos, exp ----------------------------------------------------------------------------------------------------------------------------
// round to the nearest integer for |x| < 2^51, by two additions
YGZF_SO_HD inline double so_nearest(double x) { return (x + 6755399441055744.0) - 6755399441055744.0; }

// |x| <= 2^20: k = nearest(x 2 / pi), r = x - k pi / 2 in three 33-bit pieces (k times each of the first two is exact), then the degree-13 / 14
// polynomials of fdlibm's kernels on |r| <= pi / 4.  Outside that range (NaN and Inf included) the result is defined as sin = x - x,
// cos = 1 + (x - x): 0 and 1 for a finite x, NaN otherwise.
YGZF_SO_HD inline void so_sincos(double x, double &sn, double &cs) {
    if (!(x >= -1048576.0 && x <= 1048576.0)) { sn = x - x; cs = 1.0 + (x - x); return; }
    const double k = so_nearest(x * 6.36619772367581382433e-01);
    const double r = ((x - k * 1.57079632673412561417e+00) - k * 6.07710050630396597660e-11) - k * 2.02226624871116645580e-21;
    const double z = r * r;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double s0 = r + r * (z * ps);
    const double c0 = (1.0 - 0.5 * z) + (z * z) * pc;
    const int n = ((int) k) & 3;
    sn = n == 0 ? s0 : n == 1 ? c0 : n == 2 ? -s0 : -c0;
    cs = n == 0 ? c0 : n == 1 ? -s0 : n == 2 ? -c0 : s0;
}

// x > 709: +Inf; x < -745: 0; NaN: NaN.  Otherwise k = nearest(x / ln 2), r = x - k ln 2 in two pieces (k ln2_hi is exact), the Taylor
// polynomial of degree 13 on |r| <= 0.35 by Horner, and 2^k by eleven squarings.
YGZF_SO_HD inline double so_exp(double x) {
    if (!(x <= 709.0)) return x > 709.0 ? HUGE_VAL : x;
    if (x < -745.0) return 0.0;
    const double k = so_nearest(x * 1.44269504088896338700e+00);
    const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const int ki = (int) k;
    int m = ki < 0 ? -ki : ki;
    double f = ki < 0 ? 0.5 : 2.0, sc = 1.0;
    for (int bit = 0; bit < 11; bit++) {
        if (m & 1) sc = sc * f;
        f = f * f;
        m >>= 1;
    }
    return p * sc;
}

// ---- Eigen's quaternion pieces ----------------------------------------------------------------------------------------------------------------
template <int I> YGZF_SO_HD inline void so_quat_from_R_branch(const double m[9], double q[4]) {   // the largest diagonal entry is m_II
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(m[4 * I] - m[4 * J] - m[4 * K] + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3 * K + J] - m[3 * J + K]) * t;
    q[J] = (m[3 * J + I] + m[3 * I + J]) * t;
    q[K] = (m[3 * K + I] + m[3 * I + K]) * t;
}
YGZF_SO_HD inline void so_quat_from_R(const double m[9], double q[4]) {   // QuaternionBase::operator=(MatrixBase), row-major m
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > (i ? m[4] : m[0])) i = 2;
        if (i == 0) so_quat_from_R_branch<0>(m, q);
        else if (i == 1) so_quat_from_R_branch<1>(m, q);
        else so_quat_from_R_branch<2>(m, q);
    }
}
YGZF_SO_HD inline void so_quat_mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
YGZF_SO_HD inline void so_quat_rotate(const double q[4], const double v[3], double o[3]) {   // _transformVector
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}

// ---- g2o::Sim3 ---------------------------------------------------------------------------------------------------------------------------------
// Sim3(const Vector7d &update) (sim3.h:66-130): omega, upsilon, sigma; all four branches
YGZF_SO_HD inline void so_sim3_exp(const double u[7], S3 &o) {
    const double om[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    const double s = so_exp(sigma);
    double O2[9], R[9];
YGZF_SO_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_SO_UNROLL
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    const double eps = 0.00001;
    const bool smallTheta = theta < eps;
    double A, B, C, ra = 1.0, rb = 1.0, sn = 0.0, cs = 1.0;
    if (!smallTheta) {
        so_sincos(theta, sn, cs);
        ra = sn / theta;
        rb = (1.0 - cs) / (theta * theta);
    }
YGZF_SO_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_SO_UNROLL
        for (int j = 0; j < 3; j++) {
            const double I = i == j ? 1.0 : 0.0;
            R[3 * i + j] = smallTheta ? (I + O[3 * i + j]) + O2[3 * i + j] : (I + ra * O[3 * i + j]) + rb * O2[3 * i + j];
        }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (smallTheta) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (smallTheta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn;
            const double b = s * cs;
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    so_quat_from_R(R, o.q);
    double W[9];
YGZF_SO_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_SO_UNROLL
        for (int j = 0; j < 3; j++) W[3 * i + j] = (A * O[3 * i + j] + B * O2[3 * i + j]) + C * (i == j ? 1.0 : 0.0);
YGZF_SO_UNROLL
    for (int i = 0; i < 3; i++) o.t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o.s = s;
}
YGZF_SO_HD inline void so_map(const S3 &T, const double v[3], double o[3]) {   // s (r xyz) + t
    double r[3];
    so_quat_rotate(T.q, v, r);
    o[0] = T.s * r[0] + T.t[0]; o[1] = T.s * r[1] + T.t[1]; o[2] = T.s * r[2] + T.t[2];
}
YGZF_SO_HD inline void so_inverse(const S3 &T, S3 &o) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    const double f = -1.0 / T.s;
    const double v[3] = {f * T.t[0], f * T.t[1], f * T.t[2]};
    o.q[0] = -T.q[0]; o.q[1] = -T.q[1]; o.q[2] = -T.q[2]; o.q[3] = T.q[3];
    so_quat_rotate(o.q, v, o.t);
    o.s = 1.0 / T.s;
}
YGZF_SO_HD inline void so_mul(const S3 &a, const S3 &b, S3 &o) {   // r r', s (r t') + t, s s'
    double r[3];
    so_quat_mul(a.q, b.q, o.q);
    so_quat_rotate(a.q, b.t, r);
    o.t[0] = a.s * r[0] + a.t[0]; o.t[1] = a.s * r[1] + a.t[1]; o.t[2] = a.s * r[2] + a.t[2];
    o.s = a.s * b.s;
}
// transform j of an iteration and its inverse: j == 0 the estimate, j == 1 + 2 d / 2 + 2 d the estimate after oplusImpl(+delta e_d / -delta e_d)
// (with _fix_scale, oplusImpl zeroes update[6]: both transforms of d == 6 are Sim3(0) * S and the Jacobian's column is exactly zero)
YGZF_SO_HD inline void so_transform(const S3 &S, int j, bool fixScale, S3 &fwd, S3 &inv) {
    if (j == 0) fwd = S;
    else {
        double u[7];
        const int d = (j - 1) >> 1;
YGZF_SO_UNROLL
        for (int k = 0; k < 7; k++) u[k] = k == d ? ((j & 1) ? kDelta : -kDelta) : 0.0;
        if (fixScale) u[6] = 0.0;
        S3 E;
        so_sim3_exp(u, E);
        so_mul(E, S, fwd);
    }
    so_inverse(fwd, inv);
}

// ---- the edges ---------------------------------------------------------------------------------------------------------------------------------
// computeError of EdgeSim3ProjectXYZ (T the estimate, K = K1) and of EdgeInverseSim3ProjectXYZ (T its inverse, K = K2):
// obs - cam_map(project(T.map(X))), project rounding x / z and y / z to float.  There is no depth gate.
YGZF_SO_HD inline void so_error(const S3 &T, const double X[3], const Cam &K, const double obs[2], double e[2]) {
    double p[3];
    so_map(T, X, p);
    const float u = (float) (p[0] / p[2]), v = (float) (p[1] / p[2]);
    e[0] = obs[0] - ((double) u * K.fx + K.cx);
    e[1] = obs[1] - ((double) v * K.fy + K.cy);
}
YGZF_SO_HD inline double so_chi2(const double e[2], double s) { return e[0] * (s * e[0]) + e[1] * (s * e[1]); }
// RobustKernelHuber::robustify: rho[0], rho[1]
YGZF_SO_HD inline void so_huber(double chi2, double delta, double &rho0, double &rho1) {
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) { rho0 = chi2; rho1 = 1.0; }
    else {
        const double sq = sqrt(chi2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}
// One edge at the 15 transforms T (stride in S3s): computeError at T[0], the numeric linearizeOplus (central differences, scalar 1 / (2 delta)),
// the robust constructQuadraticForm added to acc[36].  -> chi2() of the error at T[0].
YGZF_SO_HD inline double so_edge_system(const S3 *T, const double X[3], const Cam &K, const double obs[2], double s, double delta, double acc[kSums]) {
    const double scalar = 1.0 / (2 * kDelta);
    double e[2], J[2][kDim];
    so_error(T[0], X, K, obs, e);
    // (on the device d runs as a real loop and the column is put into J by selects: unrolled, the compiler loads all 15 transforms up front --
    // 240 registers -- and the kernel spills; the arithmetic is the same either way)
YGZF_SO_UNROLL
    for (int k = 0; k < kDim; k++) { J[0][k] = 0.0; J[1][k] = 0.0; }
YGZF_SO_ROLLED
    for (int d = 0; d < kDim; d++) {
        double ep[2], em[2];
        so_error(T[1 + 2 * d], X, K, obs, ep);
        so_error(T[2 + 2 * d], X, K, obs, em);
        const double j0 = scalar * (ep[0] - em[0]), j1 = scalar * (ep[1] - em[1]);
YGZF_SO_UNROLL
        for (int k = 0; k < kDim; k++) { J[0][k] = k == d ? j0 : J[0][k]; J[1][k] = k == d ? j1 : J[1][k]; }
    }
    const double chi2 = so_chi2(e, s);
    double rho0, rho1;
    so_huber(chi2, delta, rho0, rho1);
    const double w = rho1 * s;
    const double r0 = (-(s * e[0])) * rho1, r1 = (-(s * e[1])) * rho1;
    int c = 0;
YGZF_SO_UNROLL
    for (int j = 0; j < kDim; j++)
YGZF_SO_UNROLL
        for (int k = j; k < kDim; k++) {
            acc[c] = acc[c] + ((J[0][j] * w) * J[0][k] + (J[1][j] * w) * J[1][k]);
            c++;
        }
YGZF_SO_UNROLL
    for (int j = 0; j < kDim; j++) acc[28 + j] = acc[28 + j] + (J[0][j] * r0 + J[1][j] * r1);
    acc[35] = acc[35] + rho0;
    return chi2;
}

// ---- the solver: Eigen's unblocked lower pivoted LDLT, 7 x 7, and the Levenberg bookkeeping -----------------------------------------------------
struct Lm {
    double H[49], Hd[49], b[7], x[7], temp[7];
    double lambda, ni, currentChi, iniChi, rho;
    int tr[7];
    int nBadRule, qmax;
};
YGZF_SO_HD inline bool so_ldlt(Lm &L) {   // in place on L.Hd; true: every pivot > 0
    constexpr int N = kDim;
    double *m = L.Hd;
YGZF_SO_ROLLED
    for (int k = 0; k < N; k++) {
        double big = -1.0;
        int idx = k;
YGZF_SO_ROLLED
        for (int j = k; j < N; j++) {
            const double v = fabs(m[(N + 1) * j]);
            if (v > big) { big = v; idx = j; }
        }
        L.tr[k] = idx;
        if (idx != k) {
YGZF_SO_ROLLED
            for (int j = 0; j < k; j++) { const double a = m[N * k + j]; m[N * k + j] = m[N * idx + j]; m[N * idx + j] = a; }
YGZF_SO_ROLLED
            for (int i = idx + 1; i < N; i++) { const double a = m[N * i + k]; m[N * i + k] = m[N * i + idx]; m[N * i + idx] = a; }
            { const double a = m[(N + 1) * k]; m[(N + 1) * k] = m[(N + 1) * idx]; m[(N + 1) * idx] = a; }
YGZF_SO_ROLLED
            for (int i = k + 1; i < idx; i++) { const double a = m[N * i + k]; m[N * i + k] = m[N * idx + i]; m[N * idx + i] = a; }
        }
        if (k > 0) {
YGZF_SO_ROLLED
            for (int j = 0; j < k; j++) L.temp[j] = m[(N + 1) * j] * m[N * k + j];
            double s = m[N * k] * L.temp[0];
YGZF_SO_ROLLED
            for (int j = 1; j < k; j++) s = s + m[N * k + j] * L.temp[j];
            m[(N + 1) * k] = m[(N + 1) * k] - s;
YGZF_SO_ROLLED
            for (int i = k + 1; i < N; i++) {
                double s2 = m[N * i] * L.temp[0];
YGZF_SO_ROLLED
                for (int j = 1; j < k; j++) s2 = s2 + m[N * i + j] * L.temp[j];
                m[N * i + k] = m[N * i + k] - s2;
            }
        }
YGZF_SO_ROLLED
        for (int i = k + 1; i < N; i++) m[N * i + k] = m[N * i + k] / m[(N + 1) * k];
    }
    bool positive = true;
YGZF_SO_ROLLED
    for (int k = 0; k < N; k++) positive = positive && (m[(N + 1) * k] > 0);
    return positive;
}
YGZF_SO_HD inline void so_ldlt_solve(Lm &L) {   // x = P^T L^-T D^-1 L^-1 P b
    constexpr int N = kDim;
    const double *m = L.Hd;
    double *x = L.x;
YGZF_SO_ROLLED
    for (int k = 0; k < N; k++) x[k] = L.b[k];
YGZF_SO_ROLLED
    for (int k = 0; k < N; k++) { const double a = x[k]; x[k] = x[L.tr[k]]; x[L.tr[k]] = a; }
YGZF_SO_ROLLED
    for (int i = 0; i < N; i++)
YGZF_SO_ROLLED
        for (int j = 0; j < i; j++) x[i] = x[i] - m[N * i + j] * x[j];
YGZF_SO_ROLLED
    for (int i = 0; i < N; i++) x[i] = x[i] / m[(N + 1) * i];
YGZF_SO_ROLLED
    for (int i = N - 1; i >= 0; i--)
YGZF_SO_ROLLED
        for (int j = i + 1; j < N; j++) x[i] = x[i] - m[N * j + i] * x[j];
YGZF_SO_ROLLED
    for (int k = N - 1; k >= 0; k--) { const double a = x[k]; x[k] = x[L.tr[k]]; x[L.tr[k]] = a; }
}
// a fresh linearisation: sums -> H, b, currentChi; computeLambdaInit at iteration 0 of an optimize() call
YGZF_SO_HD inline void so_iteration_begin(Lm &L, const double sum[kSums], bool first) {
    int c = 0;
    for (int j = 0; j < kDim; j++)
        for (int k = j; k < kDim; k++) { L.H[kDim * j + k] = sum[c]; L.H[kDim * k + j] = sum[c]; c++; }
    for (int j = 0; j < kDim; j++) L.b[j] = sum[28 + j];
    L.currentChi = sum[35];
    L.iniChi = L.currentChi;
    if (first) {
        double maxDiagonal = 0.;
        for (int j = 0; j < kDim; j++) { const double v = fabs(L.H[(kDim + 1) * j]); maxDiagonal = (v < maxDiagonal) ? maxDiagonal : v; }   // std::max(fabs(H_jj), maxDiagonal)
        L.lambda = 1e-5 * maxDiagonal;
        L.ni = 2;
        L.nBadRule = 0;
    }
    L.rho = 0;
    L.qmax = 0;
}
// the head of a Levenberg trial (:103-115): push, setLambda, solve, update.  A failed solve leaves x as it was, and update() applies it all the
// same.  VertexSim3Expmap::oplusImpl zeroes update[6] in the solver's own x under _fix_scale, then estimate = Sim3(update) * estimate.
YGZF_SO_HD inline bool so_trial_begin(Lm &L, S3 &est, S3 &backup, bool fixScale) {
    backup = est;
    for (int k = 0; k < kDim * kDim; k++) L.Hd[k] = L.H[k];
    for (int j = 0; j < kDim; j++) L.Hd[(kDim + 1) * j] = L.H[(kDim + 1) * j] + L.lambda;
    const bool ok = so_ldlt(L);
    if (ok) so_ldlt_solve(L);
    if (fixScale) L.x[6] = 0.0;
    S3 E, n;
    so_sim3_exp(L.x, E);
    so_mul(E, est, n);
    est = n;
    return ok;
}
// the tail of the trial (:123-149); true: another trial follows
YGZF_SO_HD inline bool so_trial_end(Lm &L, S3 &est, const S3 &backup, bool ok, double tempChi) {
    if (!ok) tempChi = kDblMax;
    double scale = 0.0;
    for (int j = 0; j < kDim; j++) scale = scale + L.x[j] * (L.lambda * L.x[j] + L.b[j]);
    scale = scale + 1e-3;
    L.rho = (L.currentChi - tempChi) / scale;
    if (L.rho > 0 && tempChi - tempChi == 0.0) {   // g2o_isfinite(tempChi)
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
        est = backup;
    }
    L.qmax++;
    return L.rho < 0 && L.qmax < 10;
}
// after the trials of an iteration: -1 to go on, else the Stop that ends the optimize() call
YGZF_SO_HD inline int so_iteration_end(Lm &L) {
    if (L.qmax == 10 || L.rho == 0) return L.qmax == 10 ? kStopTrials : kStopRhoZero;
    if ((L.iniChi - L.currentChi) * 1e3 < L.iniChi) L.nBadRule++;
    else L.nBadRule = 0;
    return L.nBadRule >= 3 ? kStopNBad : -1;
}

}  // namespace sim3opt
}  // namespace ygzf
#endif
