// pnp_math.h -- PnPsolver's arithmetic (src/PnPsolver.cc:282-308 CheckInliers, :341-894 EPnP), stated once for k_pnp_hyp / k_pnp_refine
// (pnp_kernels.hip) and for plain host programs (host/PnPHost.h, tests/cpp/pnp_host.cc): nothing of HIP is needed to read it.  Every operation
// is + - * / or sqrt on doubles (floats where the source has floats) in the order written, without contraction (-ffp-contract=off), so each is
// correctly rounded and tests/pnp_cases.py repeats it bit for bit.  With four correspondences M is 8 x 12 and the four vectors EPnP takes from
// the SVD of MtM span a null space whose basis rounding decides: a sum in another order is another pose, so there is one order, the source's.
//
// The text is written for a team of L.nl lanes that run it together (a wave: nl = 64; a host thread: lane 0 of 1).  Lanes own *elements*: each
// long sum is one chain, added in row order by the one lane that owns it, and YGZF_PNP_SYNC() separates a phase that writes the work area from
// the phase that reads it.  What is short runs on lane 0.  A value every lane needs (the Jacobi dot products) every lane sums itself, in index
// order, from the shared work area.  So the number of lanes changes who adds, never what is added to what.
//
// The reference calls four OpenCV routines; this project fixes them as the text below (parity with a compiled OpenCV is unpinned):
//   cvMulTransposed(A, order 1)   AtA[i][j] for j >= i the sum over rows r = 0, 1, .. of A[r][i] * A[r][j] from 0.0; mirrored below the diagonal
//   cvSVD                         OpenCV 2.4 / 3.x's one-sided Jacobi on At (the rows of At are the columns of A): squared row norms in W; cyclic
//                                 (i, j) sweeps; p = the dot of rows i and j; skipped when |p| <= 10 eps sqrt(a b); p *= 2, beta = a - b,
//                                 gamma = sqrt(p p + beta beta) -- NOT libm hypot, which is not correctly rounded --; beta < 0:
//                                 s = sqrt(((gamma - beta) 0.5) / gamma), c = p / (gamma s 2), else c = sqrt((gamma + beta) / (gamma 2)),
//                                 s = p / (gamma c 2); rows i, j and the same rows of Vt become c x + s y and -s x + c y; a, b re-summed; at most
//                                 max(m, 30) sweeps, ending after one that rotated nothing; W = sqrt of the re-summed norms; selection sort by
//                                 descending W (strict <, rows of At and Vt swapped along); row i of At scaled by 1 / W[i].
//                                 Where OpenCV refills a row whose W <= DBL_MIN with a pseudo-random orthogonal vector, the row is scaled by 0.0
//                                 here: bounded, deterministic, and no case of EPnP reads such a row of a finite problem for more than a zero.
//                                 The rotations of At do not depend on Vt, so Vt is left out where the caller does not read it.
//   cvSolve(CV_SVD)               that SVD of At = A', then x = 0 and for i = 0 .. n-1 with |W[i]| > threshold: s = (sum_j At[i][j] b[j]) (1 / W[i]),
//                                 x[j] = x[j] + s Vt[i][j]; threshold = (0 + W[0] + W[1] + ..) * 2 DBL_EPSILON
//   cvInvert(CV_SVD)              the same with b absent: buffer[k] = At[i][k] (1 / W[i]), x[j][k] = x[j][k] + Vt[i][j] buffer[k]
// The reference's uninitialised read has a value here: qr_solve returns on a singular column without writing x, and on the first Gauss-Newton
// step x was never written: x starts as 0 (a later singular step adds the previous step's x again, as the source does).
// Non-finite input ends through the bounded loops: a NaN never passes a `<=` skip test, so the Jacobi runs its max(m, 30) sweeps and stops.
#ifndef YGZF_PNP_MATH_H
#define YGZF_PNP_MATH_H
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "lm_math.h"   // for YGZF_HD, the one set of these macros; nothing else of it is used here

#define YGZF_PNP_MAX_MIN_SET 8     // the largest mRansacMinSet a problem may ask for (the reference's callers use 4)
#define YGZF_PNP_SVD_MIN_SWEEPS 30 // the Jacobi SVD runs at most max(m, this) sweeps
#define YGZF_PNP_GN_STEPS 5        // gauss_newton's iterations_number

#if defined(__HIP_DEVICE_COMPILE__)
// the lanes of one wave run in lockstep and the LDS serves one wave's accesses in order: what is needed is that the compiler keeps them in order
#define YGZF_PNP_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#else
#define YGZF_PNP_SYNC() do { } while (0)
#endif

namespace ygzf {
namespace pnp {

constexpr int kHypDoubles = 12;   // R row-major, t

struct Lanes { int lane, nl; };

struct Points {                    // one solver's correspondences
    const float *P3D, *P2D;        // mvP3Dw n x 3, mvP2D n x 2
    double fu, fv, uc, vc;
};

// the correspondences one EPnP runs over: `list` (count indices, in the order drawn) or, with list null, the set bits of `mask` in ascending
// order (count = their number), n the size of the mask in bits
struct Subset {
    const int *list;
    const uint64_t *mask;
    int count, n;
};

template <typename F> YGZF_HD inline void for_each(const Subset &S, F &&f) {
    if (S.list) {
        for (int k = 0; k < S.count; k++) f(S.list[k]);
    } else {
        for (int i = 0; i < S.n; i++)
            if ((S.mask[i >> 6] >> (i & 63)) & 1ull) f(i);
    }
}

YGZF_HD inline int first_of(const Subset &S) {
    if (S.list) return S.list[0];
    for (int i = 0; i < S.n; i++)
        if ((S.mask[i >> 6] >> (i & 63)) & 1ull) return i;
    return 0;
}

struct Work {                      // one team's work area (LDS on the device)
    double cws[4][3], ccs[4][3], ci[9];
    double mtm[144], d12[12];      // MtM, after the SVD ut
    double l[60], rho[6];
    double sa[30], sw[5], sv[25];  // the small SVDs: At (at most 5 x 6), W, Vt
    double sq[9];                  // PW0tPW0 / CC / ABt
    double pc0[3], pw0[3];
    double betas[4];
    double Rs[3][9], ts[3][3], err[3];
    double R[9], t[3];             // the result
};

// ---------------------------------------------------------------- the fixed linear algebra ----------------------------------------------------------------

// At: n rows of m, W[n], Vt n x n or null.  Run by the whole team.
YGZF_HD inline void jacobi_svd(double *At, int lda, double *W, double *Vt, int ldv, int m, int n, Lanes L) {
    const double eps = DBL_EPSILON * 10, minval = DBL_MIN;
    for (int i = L.lane; i < n; i += L.nl) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * lda + k];
            sd += t * t;
        }
        W[i] = sd;
        if (Vt)
            for (int k = 0; k < n; k++) Vt[i * ldv + k] = k == i ? 1.0 : 0.0;
    }
    YGZF_PNP_SYNC();
    const int max_iter = m > YGZF_PNP_SVD_MIN_SWEEPS ? m : YGZF_PNP_SVD_MIN_SWEEPS;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double *Ai = At + i * lda, *Aj = At + j * lda;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;   // the same for every lane: all of them summed the same numbers
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                YGZF_PNP_SYNC();
                for (int e = L.lane; e < m + (Vt ? n : 0); e += L.nl) {   // elements 0 .. m-1 of the rows of At, then 0 .. n-1 of the rows of Vt
                    double *x = e < m ? Ai + e : Vt + i * ldv + (e - m), *y = e < m ? Aj + e : Vt + j * ldv + (e - m);
                    const double t0 = c * *x + s * *y;
                    const double t1 = -s * *x + c * *y;
                    *x = t0;
                    *y = t1;
                }
                YGZF_PNP_SYNC();
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    a += Ai[k] * Ai[k];
                    b += Aj[k] * Aj[k];
                }
                YGZF_PNP_SYNC();
                if (L.lane == 0) {
                    W[i] = a;
                    W[j] = b;
                }
                YGZF_PNP_SYNC();
                changed = true;
            }
        if (!changed) break;
    }
    for (int i = L.lane; i < n; i += L.nl) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * lda + k];
            sd += t * t;
        }
        W[i] = sqrt(sd);
    }
    YGZF_PNP_SYNC();
    if (L.lane == 0) {
        for (int i = 0; i < n - 1; i++) {
            int j = i;
            for (int k = i + 1; k < n; k++)
                if (W[j] < W[k]) j = k;
            if (i != j) {
                double t = W[i]; W[i] = W[j]; W[j] = t;
                for (int k = 0; k < m; k++) { t = At[i * lda + k]; At[i * lda + k] = At[j * lda + k]; At[j * lda + k] = t; }
                if (Vt)
                    for (int k = 0; k < n; k++) { t = Vt[i * ldv + k]; Vt[i * ldv + k] = Vt[j * ldv + k]; Vt[j * ldv + k] = t; }
            }
        }
    }
    YGZF_PNP_SYNC();
    for (int e = L.lane; e < n * m; e += L.nl) {
        const int i = e / m, k = e - i * m;
        const double sd = W[i];
        const double s = sd > minval ? 1 / sd : 0.0;
        At[i * lda + k] *= s;
    }
    YGZF_PNP_SYNC();
}

// the singular-value threshold of the back-substitution
YGZF_HD inline double svd_threshold(const double *W, int n) {
    double threshold = 0;
    for (int i = 0; i < n; i++) threshold += W[i];
    return threshold * (DBL_EPSILON * 2);
}

// cvSolve(A, b, x, CV_SVD) for A m x n (m >= n), whose transpose the caller has put into At (n x m, lda = m).  Run by the whole team; x by lane 0.
YGZF_HD inline void solve_svd(double *At, double *W, double *Vt, int m, int n, const double *b, double *x, Lanes L) {
    jacobi_svd(At, m, W, Vt, n, m, n, L);
    if (L.lane == 0) {
        for (int j = 0; j < n; j++) x[j] = 0;
        const double threshold = svd_threshold(W, n);
        for (int i = 0; i < n; i++) {
            double wi = W[i];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double s = 0;
            for (int j = 0; j < m; j++) s += At[i * m + j] * b[j];
            s *= wi;
            for (int j = 0; j < n; j++) x[j] = x[j] + s * Vt[i * n + j];
        }
    }
    YGZF_PNP_SYNC();
}

// cvInvert(A, inv, CV_SVD) for A 3 x 3, whose transpose the caller has put into At.  Run by the whole team; inv by lane 0.
YGZF_HD inline void invert3_svd(double *At, double *W, double *Vt, double *inv, Lanes L) {
    jacobi_svd(At, 3, W, Vt, 3, 3, 3, L);
    if (L.lane == 0) {
        for (int j = 0; j < 9; j++) inv[j] = 0;
        const double threshold = svd_threshold(W, 3);
        for (int i = 0; i < 3; i++) {
            double wi = W[i];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double buffer[3];
            for (int k = 0; k < 3; k++) buffer[k] = At[i * 3 + k] * wi;
            for (int j = 0; j < 3; j++)
                for (int k = 0; k < 3; k++) inv[3 * j + k] = inv[3 * j + k] + Vt[i * 3 + j] * buffer[k];
        }
    }
    YGZF_PNP_SYNC();
}

// qr_solve (:805-894) for the 6 x 4 system of a Gauss-Newton step: Householder by columns.  The pivot search reads rows k .. nr-2 (the source
// steps its pointer after the comparison), never the last row.  Returns without writing x on a column whose searched entries are all zero.
YGZF_HD inline void qr_solve_6x4(double *A, double *b, double *x) {
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; i++) {
            const double elt = fabs(A[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) return;
        const double inv_eta = 1. / eta;
        double sum = 0.0;
        for (int i = k; i < nr; i++) {
            A[i * nc + k] *= inv_eta;
            sum += A[i * nc + k] * A[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            for (int i = k; i < nr; i++) s2 += A[i * nc + k] * A[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {   // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    x[nc - 1] = b[nc - 1] / A2[nc - 1];   // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

// ---------------------------------------------------------------- EPnP ----------------------------------------------------------------

YGZF_HD inline double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
YGZF_HD inline double dist2(const double *p1, const double *p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// one correspondence's world point (add_correspondence widens the floats) and barycentric coordinates (:386-396)
YGZF_HD inline void world_point(const Points &P, int i, double pw[3]) {
    pw[0] = (double) P.P3D[3 * (size_t) i];
    pw[1] = (double) P.P3D[3 * (size_t) i + 1];
    pw[2] = (double) P.P3D[3 * (size_t) i + 2];
}
YGZF_HD inline void alphas_of(const Work &w, const double pw[3], double &a0, double &a1, double &a2, double &a3) {
    const double d0 = pw[0] - w.cws[0][0], d1 = pw[1] - w.cws[0][1], d2 = pw[2] - w.cws[0][2];
    a1 = w.ci[0] * d0 + w.ci[1] * d1 + w.ci[2] * d2;
    a2 = w.ci[3] * d0 + w.ci[4] * d1 + w.ci[5] * d2;
    a3 = w.ci[6] * d0 + w.ci[7] * d1 + w.ci[8] * d2;
    a0 = 1.0 - a1 - a2 - a3;
}
// compute_pcs for one correspondence
YGZF_HD inline void camera_point(const Work &w, const double pw[3], double pc[3]) {
    double a0, a1, a2, a3;
    alphas_of(w, pw, a0, a1, a2, a3);
    for (int j = 0; j < 3; j++) pc[j] = a0 * w.ccs[0][j] + a1 * w.ccs[1][j] + a2 * w.ccs[2][j] + a3 * w.ccs[3][j];
}
// fill_M: entry `col` of row 0 / 1 of the correspondence's two rows of M
YGZF_HD inline double m_entry(const Points &P, int row, int col, double a0, double a1, double a2, double a3, double u, double v) {
    const int j = col / 3, t = col - 3 * j;
    const double a = j == 0 ? a0 : j == 1 ? a1 : j == 2 ? a2 : a3;
    if (row == 0) return t == 0 ? a * P.fu : t == 1 ? 0.0 : a * (P.uc - u);
    return t == 0 ? 0.0 : t == 1 ? a * P.fv : a * (P.vc - v);
}

YGZF_HD inline void compute_L_6x10(const double *ut, double *l_6x10) {
    const double *v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
    for (int i = 0; i < 6; i++) {
        // pair i of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int a = i < 3 ? 0 : i < 5 ? 1 : 2, b = i < 3 ? i + 1 : i < 5 ? i - 1 : 3;
        double dv[4][3];
        for (int q = 0; q < 4; q++)
            for (int k = 0; k < 3; k++) dv[q][k] = v[q][3 * a + k] - v[q][3 * b + k];
        double *row = l_6x10 + 10 * i;
        row[0] = dot3(dv[0], dv[0]);
        row[1] = 2.0 * dot3(dv[0], dv[1]);
        row[2] = dot3(dv[1], dv[1]);
        row[3] = 2.0 * dot3(dv[0], dv[2]);
        row[4] = 2.0 * dot3(dv[1], dv[2]);
        row[5] = dot3(dv[2], dv[2]);
        row[6] = 2.0 * dot3(dv[0], dv[3]);
        row[7] = 2.0 * dot3(dv[1], dv[3]);
        row[8] = 2.0 * dot3(dv[2], dv[3]);
        row[9] = dot3(dv[3], dv[3]);
    }
}

YGZF_HD inline void gauss_newton(const double *l_6x10, const double *rho, double betas[4]) {
    double x[4] = {0, 0, 0, 0};   // (the value this file gives the reference's uninitialised x)
    for (int k = 0; k < YGZF_PNP_GN_STEPS; k++) {
        double A[24], b[6];
        for (int i = 0; i < 6; i++) {
            const double *rowL = l_6x10 + i * 10;
            double *rowA = A + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                             rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                             rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                             rowL[9] * betas[3] * betas[3]);
        }
        qr_solve_6x4(A, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// find_betas_approx_1 / 2 / 3 from the solution b of the reduced system (:634-644, :664-675, :697-706)
YGZF_HD inline void betas_from(int approx, const double *b, double *betas) {
    if (approx == 1) {
        if (b[0] < 0) {
            betas[0] = sqrt(-b[0]);
            betas[1] = -b[1] / betas[0];
            betas[2] = -b[2] / betas[0];
            betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = sqrt(b[0]);
            betas[1] = b[1] / betas[0];
            betas[2] = b[2] / betas[0];
            betas[3] = b[3] / betas[0];
        }
        return;
    }
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = approx == 3 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

// compute_pose (:438-485) over the correspondences S of P: the pose into w.R / w.t.  Run by the whole team.
YGZF_HD inline void epnp(const Points &P, const Subset &S, Work &w, Lanes L) {
    const int nc = S.count;
    // choose_control_points
    for (int j = L.lane; j < 3; j += L.nl) {
        double s = 0;
        for_each(S, [&](int i) { s += (double) P.P3D[3 * (size_t) i + j]; });
        w.cws[0][j] = s / nc;
    }
    YGZF_PNP_SYNC();
    for (int e = L.lane; e < 6; e += L.nl) {   // PW0tPW0 (r, c), c >= r
        const int r = e < 3 ? 0 : e < 5 ? 1 : 2, c = e < 3 ? e : e < 5 ? e - 2 : 2;
        const double cr = w.cws[0][r], cc = w.cws[0][c];
        double s = 0;
        for_each(S, [&](int i) { s += ((double) P.P3D[3 * (size_t) i + r] - cr) * ((double) P.P3D[3 * (size_t) i + c] - cc); });
        w.sq[3 * r + c] = s;
        w.sq[3 * c + r] = s;
    }
    YGZF_PNP_SYNC();
    jacobi_svd(w.sq, 3, w.sw, w.sv, 3, 3, 3, L);   // (symmetric: At = A); uct = the rows of At, dc = W
    if (L.lane == 0) {
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(w.sw[i - 1] / nc);
            for (int j = 0; j < 3; j++) w.cws[i][j] = w.cws[0][j] + k * w.sq[3 * (i - 1) + j];
        }
        // compute_barycentric_coordinates: cc[3 i + j - 1] = cws[j][i] - cws[0][i]; its transpose for the SVD
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) w.sa[3 * (j - 1) + i] = w.cws[j][i] - w.cws[0][i];
    }
    YGZF_PNP_SYNC();
    invert3_svd(w.sa, w.sw, w.sv, w.ci, L);
    // MtM = cvMulTransposed(M, order 1): entry (p, q), q >= p, over the 2 nc rows of M in row order
    for (int e = L.lane; e < 78; e += L.nl) {
        int p = 0, rest = e;
        for (int k = 0; k < 12 && rest >= 12 - p; k++) { rest -= 12 - p; p++; }
        const int q = p + rest;
        double s = 0;
        for_each(S, [&](int i) {
            double pw[3], a0, a1, a2, a3;
            world_point(P, i, pw);
            alphas_of(w, pw, a0, a1, a2, a3);
            const double u = (double) P.P2D[2 * (size_t) i], v = (double) P.P2D[2 * (size_t) i + 1];
            s += m_entry(P, 0, p, a0, a1, a2, a3, u, v) * m_entry(P, 0, q, a0, a1, a2, a3, u, v);
            s += m_entry(P, 1, p, a0, a1, a2, a3, u, v) * m_entry(P, 1, q, a0, a1, a2, a3, u, v);
        });
        w.mtm[12 * p + q] = s;
        w.mtm[12 * q + p] = s;
    }
    YGZF_PNP_SYNC();
    jacobi_svd(w.mtm, 12, w.d12, nullptr, 0, 12, 12, L);   // ut = the rows of At
    if (L.lane == 0) {
        compute_L_6x10(w.mtm, w.l);
        w.rho[0] = dist2(w.cws[0], w.cws[1]);
        w.rho[1] = dist2(w.cws[0], w.cws[2]);
        w.rho[2] = dist2(w.cws[0], w.cws[3]);
        w.rho[3] = dist2(w.cws[1], w.cws[2]);
        w.rho[4] = dist2(w.cws[1], w.cws[3]);
        w.rho[5] = dist2(w.cws[2], w.cws[3]);
    }
    YGZF_PNP_SYNC();
    const int i0 = first_of(S);
    for (int approx = 1; approx <= 3; approx++) {
        // the columns of L_6x10 the approximation keeps: [0 1 3 6], [0 1 2], [0 1 2 3 4]
        const int k = approx == 1 ? 4 : approx == 2 ? 3 : 5;
        if (L.lane == 0)
            for (int c = 0; c < k; c++) {
                const int col = approx == 1 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c;
                for (int r = 0; r < 6; r++) w.sa[6 * c + r] = w.l[10 * r + col];
            }
        YGZF_PNP_SYNC();
        double bk[5];
        solve_svd(w.sa, w.sw, w.sv, 6, k, w.rho, bk, L);   // (bk is lane 0's)
        if (L.lane == 0) {
            betas_from(approx, bk, w.betas);
            gauss_newton(w.l, w.rho, w.betas);
            // compute_ccs
            for (int i = 0; i < 4; i++) w.ccs[i][0] = w.ccs[i][1] = w.ccs[i][2] = 0.0;
            for (int i = 0; i < 4; i++) {
                const double *v = w.mtm + 12 * (11 - i);
                for (int j = 0; j < 4; j++)
                    for (int c = 0; c < 3; c++) w.ccs[j][c] += w.betas[i] * v[3 * j + c];
            }
            // solve_for_sign on pcs[2], the depth of the first correspondence.  The source negates ccs and every pc; negating ccs and
            // computing the pcs from them afterwards gives the same numbers (rounding is symmetric in the sign).
            double pw[3], pc[3];
            world_point(P, i0, pw);
            camera_point(w, pw, pc);
            if (pc[2] < 0.0)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 3; j++) w.ccs[i][j] = -w.ccs[i][j];
        }
        YGZF_PNP_SYNC();
        // estimate_R_and_t: the centroids, six chains
        for (int e = L.lane; e < 6; e += L.nl) {
            const int j = e < 3 ? e : e - 3;
            double s = 0;
            for_each(S, [&](int i) {
                double pw[3], pc[3];
                world_point(P, i, pw);
                if (e < 3) {
                    camera_point(w, pw, pc);
                    s += pc[j];
                } else
                    s += pw[j];
            });
            (e < 3 ? w.pc0 : w.pw0)[j] = s / nc;
        }
        YGZF_PNP_SYNC();
        for (int e = L.lane; e < 9; e += L.nl) {   // abt (r, c); its transpose for the SVD
            const int r = e / 3, c = e - 3 * r;
            const double pcr = w.pc0[r], pwc = w.pw0[c];
            double s = 0;
            for_each(S, [&](int i) {
                double pw[3], pc[3];
                world_point(P, i, pw);
                camera_point(w, pw, pc);
                s += (pc[r] - pcr) * (pw[c] - pwc);
            });
            w.sa[3 * c + r] = s;
        }
        YGZF_PNP_SYNC();
        jacobi_svd(w.sa, 3, w.sw, w.sv, 3, 3, 3, L);   // U[i][k] = At[k][i], V[j][k] = Vt[k][j]
        if (L.lane == 0) {
            double *R = w.Rs[approx - 1], *t = w.ts[approx - 1];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[3 * i + j] = w.sa[i] * w.sv[j] + w.sa[3 + i] * w.sv[3 + j] + w.sa[6 + i] * w.sv[6 + j];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) {
                R[6] = -R[6];
                R[7] = -R[7];
                R[8] = -R[8];
            }
            t[0] = w.pc0[0] - dot3(R, w.pw0);
            t[1] = w.pc0[1] - dot3(R + 3, w.pw0);
            t[2] = w.pc0[2] - dot3(R + 6, w.pw0);
            // reprojection_error
            double sum2 = 0.0;
            for_each(S, [&](int i) {
                double pw[3];
                world_point(P, i, pw);
                const double Xc = dot3(R, pw) + t[0];
                const double Yc = dot3(R + 3, pw) + t[1];
                const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
                const double ue = P.uc + P.fu * Xc * inv_Zc;
                const double ve = P.vc + P.fv * Yc * inv_Zc;
                const double u = (double) P.P2D[2 * (size_t) i], v = (double) P.P2D[2 * (size_t) i + 1];
                sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            });
            w.err[approx - 1] = sum2 / nc;
        }
        YGZF_PNP_SYNC();
    }
    if (L.lane == 0) {
        int N = 0;
        if (w.err[1] < w.err[0]) N = 1;
        if (w.err[2] < w.err[N]) N = 2;
        for (int i = 0; i < 9; i++) w.R[i] = w.Rs[N][i];
        for (int i = 0; i < 3; i++) w.t[i] = w.ts[N][i];
    }
    YGZF_PNP_SYNC();
}

// CheckInliers (:282-308) for one correspondence: double products rounded to float Xc, Yc, invZc; ue, ve doubles; distX, distY, error2 floats;
// the gate strict, no depth gate
YGZF_HD inline bool inlier(const double R[9], const double t[3], const Points &P, int i, float maxError) {
    const float X = P.P3D[3 * (size_t) i], Y = P.P3D[3 * (size_t) i + 1], Z = P.P3D[3 * (size_t) i + 2];
    const float Xc = (float) (R[0] * X + R[1] * Y + R[2] * Z + t[0]);
    const float Yc = (float) (R[3] * X + R[4] * Y + R[5] * Z + t[1]);
    const float invZc = (float) (1 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
    const double ue = P.uc + P.fu * Xc * invZc;
    const double ve = P.vc + P.fv * Yc * invZc;
    const float distX = (float) (P.P2D[2 * (size_t) i] - ue);
    const float distY = (float) (P.P2D[2 * (size_t) i + 1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < maxError;
}

// mBestTcw / mRefinedTcw: the double pose converted entry by entry into a float 4 x 4, row-major
inline void pose_to_float(const double *hyp12, float T[16]) {
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float) hyp12[3 * r + c];
        T[4 * r + 3] = (float) hyp12[9 + r];
    }
}

}  // namespace pnp
}  // namespace ygzf
#endif
