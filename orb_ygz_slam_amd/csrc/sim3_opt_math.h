// sim3_opt_math.h -- the arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:2409-2594) as scalar fp64 code: g2o's Sim3 (types/sim3.h),
// the two projection edges of types_seven_dof_expmap.h with their numeric Jacobian (core/base_binary_edge.hpp:131-205: this fork comments the
// analytic linearizeOplus out) and the vertex's oplusImpl.  Huber's robustify, the quaternion products, Eigen's pivoted LDLT and g2o's Levenberg
// bookkeeping are csrc/lm_math.h (N = 7 here), shared with k_pose_opt.  k_sim3_opt (sim3_opt_kernels.hip) and plain host programs
// (tests/cpp/sim3_opt_host.cc, the one-thread yardstick of tools/sim3_opt_rate.py) compile this same text: nothing of HIP is needed to read it.
// tests/sim3_opt_cases.py restates it operation by operation.
//
// Every floating-point operation is + - * / or sqrt on double without contraction (-ffp-contract=off), so each is correctly rounded and numpy
// repeats it bit for bit -- with ONE rounding to float: project() returns a Vector2f (se3_ops.hpp:49-55), so x / z and y / z are rounded to
// float before cam_map widens them again.  A +-1e-9 perturbation moves the quotient by ~1e-9 and a float ulp there is ~3e-8: the numeric
// Jacobian is a dither (mostly 0, else multiples of ulp fx / 2e-9).  That is what the reference runs, so every operation below has to round
// exactly as written; "close in fp64" is not a contract for this file.
//
// Where the reference leaves an evaluation order to Eigen's expression templates this file states one:
//   Quaterniond(R)      Eigen's QuaternionBase::operator=(MatrixBase): trace (m00 + m11) + m22, the four branches, no normalisation
//   q * q', q * v       lm::quat_mul, lm::quat_rotate (csrc/lm_math.h)
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

#include "lm_math.h"

// the recorded bound on |so_sin - sin|, |so_cos - cos| (absolute, |theta| <= pi) and |so_exp / exp - 1| (|sigma| <= 1); tests/sim3_opt_cases.py
// carries the same figure
#define YGZF_SIM3_OPT_LIBM_EPS 5e-16

namespace ygzf {
namespace sim3opt {

constexpr int kDim = 7;
constexpr int kSums = 36;            // 28 upper entries of H (row-major, j <= k), 7 of b, the robust chi2
constexpr int kTransforms = 15;      // S, then Sim3(+delta e_d) S and Sim3(-delta e_d) S for d = 0 .. 6
constexpr double kDelta = 1e-9;      // base_binary_edge.hpp:147
using lm::Stop; using lm::kStopMaxIter; using lm::kStopTrials; using lm::kStopRhoZero; using lm::kStopNBad; using lm::kStopNotRun;   // lm's one enum, also under this namespace for the host programs

struct S3 { double q[4], t[3], s; };    // r.x r.y r.z r.w, t, s: 8 doubles
struct Cam { double fx, fy, cx, cy; };

// ---- sin, cos, exp ----------------------------------------------------------------------------------------------------------------------------
// round to the nearest integer for |x| < 2^51, by two additions
YGZF_HD inline double so_nearest(double x) { return (x + 6755399441055744.0) - 6755399441055744.0; }

// |x| <= 2^20: k = nearest(x 2 / pi), r = x - k pi / 2 in three 33-bit pieces (k times each of the first two is exact), then the degree-13 / 14
// polynomials of fdlibm's kernels on |r| <= pi / 4.  Outside that range (NaN and Inf included) the result is defined as sin = x - x,
// cos = 1 + (x - x): 0 and 1 for a finite x, NaN otherwise.
YGZF_HD inline void so_sincos(double x, double &sn, double &cs) {
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
YGZF_HD inline double so_exp(double x) {
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
template <int I> YGZF_HD inline void so_quat_from_R_branch(const double m[9], double q[4]) {   // the largest diagonal entry is m_II
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(m[4 * I] - m[4 * J] - m[4 * K] + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3 * K + J] - m[3 * J + K]) * t;
    q[J] = (m[3 * J + I] + m[3 * I + J]) * t;
    q[K] = (m[3 * K + I] + m[3 * I + K]) * t;
}
YGZF_HD inline void so_quat_from_R(const double m[9], double q[4]) {   // QuaternionBase::operator=(MatrixBase), row-major m
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

// ---- g2o::Sim3 ---------------------------------------------------------------------------------------------------------------------------------
// Sim3(const Vector7d &update) (sim3.h:66-130): omega, upsilon, sigma; all four branches
YGZF_HD inline void so_sim3_exp(const double u[7], S3 &o) {
    const double om[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    const double s = so_exp(sigma);
    double O2[9], R[9];
YGZF_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_UNROLL
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    const double eps = 0.00001;
    const bool smallTheta = theta < eps;
    double A, B, C, ra = 1.0, rb = 1.0, sn = 0.0, cs = 1.0;
    if (!smallTheta) {
        so_sincos(theta, sn, cs);
        ra = sn / theta;
        rb = (1.0 - cs) / (theta * theta);
    }
YGZF_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_UNROLL
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
YGZF_UNROLL
    for (int i = 0; i < 3; i++)
YGZF_UNROLL
        for (int j = 0; j < 3; j++) W[3 * i + j] = (A * O[3 * i + j] + B * O2[3 * i + j]) + C * (i == j ? 1.0 : 0.0);
YGZF_UNROLL
    for (int i = 0; i < 3; i++) o.t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o.s = s;
}
YGZF_HD inline void so_map(const S3 &T, const double v[3], double o[3]) {   // s (r xyz) + t
    double r[3];
    lm::quat_rotate(T.q, v, r);
    o[0] = T.s * r[0] + T.t[0]; o[1] = T.s * r[1] + T.t[1]; o[2] = T.s * r[2] + T.t[2];
}
YGZF_HD inline void so_inverse(const S3 &T, S3 &o) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    const double f = -1.0 / T.s;
    const double v[3] = {f * T.t[0], f * T.t[1], f * T.t[2]};
    o.q[0] = -T.q[0]; o.q[1] = -T.q[1]; o.q[2] = -T.q[2]; o.q[3] = T.q[3];
    lm::quat_rotate(o.q, v, o.t);
    o.s = 1.0 / T.s;
}
YGZF_HD inline void so_mul(const S3 &a, const S3 &b, S3 &o) {   // r r', s (r t') + t, s s'
    double r[3];
    lm::quat_mul(a.q, b.q, o.q);
    lm::quat_rotate(a.q, b.t, r);
    o.t[0] = a.s * r[0] + a.t[0]; o.t[1] = a.s * r[1] + a.t[1]; o.t[2] = a.s * r[2] + a.t[2];
    o.s = a.s * b.s;
}
// transform j of an iteration and its inverse: j == 0 the estimate, j == 1 + 2 d / 2 + 2 d the estimate after oplusImpl(+delta e_d / -delta e_d)
// (with _fix_scale, oplusImpl zeroes update[6]: both transforms of d == 6 are Sim3(0) * S and the Jacobian's column is exactly zero)
YGZF_HD inline void so_transform(const S3 &S, int j, bool fixScale, S3 &fwd, S3 &inv) {
    if (j == 0) fwd = S;
    else {
        double u[7];
        const int d = (j - 1) >> 1;
YGZF_UNROLL
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
YGZF_HD inline void so_error(const S3 &T, const double X[3], const Cam &K, const double obs[2], double e[2]) {
    double p[3];
    so_map(T, X, p);
    const float u = (float) (p[0] / p[2]), v = (float) (p[1] / p[2]);
    e[0] = obs[0] - ((double) u * K.fx + K.cx);
    e[1] = obs[1] - ((double) v * K.fy + K.cy);
}
YGZF_HD inline double so_chi2(const double e[2], double s) { return e[0] * (s * e[0]) + e[1] * (s * e[1]); }
// One edge at the 15 transforms T (stride in S3s): computeError at T[0], the numeric linearizeOplus (central differences, scalar 1 / (2 delta)),
// the robust constructQuadraticForm added to acc[36].  -> chi2() of the error at T[0].
YGZF_HD inline double so_edge_system(const S3 *T, const double X[3], const Cam &K, const double obs[2], double s, double delta, double acc[kSums]) {
    const double scalar = 1.0 / (2 * kDelta);
    double e[2], J[2][kDim];
    so_error(T[0], X, K, obs, e);
    // (on the device d runs as a real loop and the column is put into J by selects: unrolled, the compiler loads all 15 transforms up front --
    // 240 registers -- and the kernel spills; the arithmetic is the same either way)
YGZF_UNROLL
    for (int k = 0; k < kDim; k++) { J[0][k] = 0.0; J[1][k] = 0.0; }
YGZF_ROLLED
    for (int d = 0; d < kDim; d++) {
        double ep[2], em[2];
        so_error(T[1 + 2 * d], X, K, obs, ep);
        so_error(T[2 + 2 * d], X, K, obs, em);
        const double j0 = scalar * (ep[0] - em[0]), j1 = scalar * (ep[1] - em[1]);
YGZF_UNROLL
        for (int k = 0; k < kDim; k++) { J[0][k] = k == d ? j0 : J[0][k]; J[1][k] = k == d ? j1 : J[1][k]; }
    }
    const double chi2 = so_chi2(e, s);
    double rho0, rho1;
    lm::huber(chi2, delta, rho0, rho1);
    const double w = rho1 * s;
    const double r0 = (-(s * e[0])) * rho1, r1 = (-(s * e[1])) * rho1;
    int c = 0;
YGZF_UNROLL
    for (int j = 0; j < kDim; j++)
YGZF_UNROLL
        for (int k = j; k < kDim; k++) {
            acc[c] = acc[c] + ((J[0][j] * w) * J[0][k] + (J[1][j] * w) * J[1][k]);
            c++;
        }
YGZF_UNROLL
    for (int j = 0; j < kDim; j++) acc[28 + j] = acc[28 + j] + (J[0][j] * r0 + J[1][j] * r1);
    acc[35] = acc[35] + rho0;
    return chi2;
}

// the update of a trial, VertexSim3Expmap::oplusImpl: under _fix_scale it zeroes update[6] in the solver's own x, then estimate = Sim3(update) * estimate
YGZF_HD inline void so_oplus(double x[kDim], bool fixScale, S3 &est) {
    if (fixScale) x[6] = 0.0;
    S3 E, n;
    so_sim3_exp(x, E);
    so_mul(E, est, n);
    est = n;
}

}  // namespace sim3opt
}  // namespace ygzf
#endif
