// sim3_math.h -- one RANSAC hypothesis of Sim3Solver (src/Sim3Solver.cc:209-338: ComputeSim3 and the per-correspondence test of CheckInliers)
// as scalar fp32 code in the order tests/sim3_cases.py restates as mode "device".  k_sim3_ransac (sim3_kernels.hip) and plain host programs
// (tests/cpp/sim3_host.cc, tools/sim3_rate.py's one-thread yardstick) compile this same text: nothing of HIP is needed to read it.  Every
// operation is + - * / or sqrt on float or double without contraction (-ffp-contract=off), so each is correctly rounded and numpy repeats it
// bit for bit.
//
// The cv::Mat arithmetic is OpenCV 2.4 / 3.2's as host/ORBmatcherLoop.h and tests/loop_cases.py fix it for this project, reused here:
//   small gemm             a float dot, left to right: (a0 b0 + a1 b1) + a2 b2
//   scalar * Mat, Mat / n  a double factor, each entry rounded to float once
//   Mat::dot, norm         double accumulation in index order
// and, new with this file:
//   cv::reduce(SUM)        a float sum, left to right
//   cv::eigen              cyclic Jacobi in fp32 (below); the reference's own solver is OpenCV's, so parity with it is unpinned
//   the rotation           straight from the quaternion q = (w, x, y, z) (row 0 of cv::eigen's eigenvectors), R = I + (2 / |q|^2) [..]: what
//                          atan2 -> angle-axis -> cv::Rodrigues compute, without the trigonometry.  x = y = z = 0 exactly gives the reference's
//                          0 / 0: every entry of R is NaN and the hypothesis has no inliers.
#ifndef YGZF_SIM3_MATH_H
#define YGZF_SIM3_MATH_H
#include <math.h>
#include <stdint.h>

#include "lm_math.h"   // for YGZF_HD and YGZF_UNROLL, the one set of these macros; nothing else of it is used here

// The most sweeps of the Jacobi eigen-solver, for the kernel and the restatement alike (tests/sim3_cases.py reads this line).  A sweep is
// the six rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the solver stops before a sweep only when all six off-diagonal entries are exactly zero.
#define YGZF_SIM3_JACOBI_SWEEPS 8

namespace ygzf {
namespace sim3 {

constexpr int kHypFloats = 13;   // R12 row-major, t12, s12

struct Hyp {
    float R[9], t[3], s;          // mR12i, mt12i, ms12i
    float sR12[9];                // T12 = [sR12 | t]
    float sR21[9], t21[3];        // T21 = [(1.0 / s) R' | -sR21 t]
};

// symmetric 4 x 4, eigenvectors in the columns of V
YGZF_HD inline void jacobi4(float A[4][4], float V[4][4]) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.f : 0.f;
    for (int sweep = 0; sweep < YGZF_SIM3_JACOBI_SWEEPS; sweep++) {
        if (A[0][1] == 0.f && A[0][2] == 0.f && A[0][3] == 0.f && A[1][2] == 0.f && A[1][3] == 0.f && A[2][3] == 0.f) break;
YGZF_UNROLL
        for (int p = 0; p < 3; p++) {
YGZF_UNROLL
            for (int q = p + 1; q < 4; q++) {
                const float apq = A[p][q];
                if (apq == 0.f) continue;
                const float theta = (A[q][q] - A[p][p]) / (2.f * apq);
                const float tt = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));
                const float t = theta < 0.f ? -tt : tt;
                const float c = 1.f / sqrtf(t * t + 1.f);
                const float s = t * c;
                const float h = t * apq;
                A[p][p] = A[p][p] - h;
                A[q][q] = A[q][q] + h;
                A[p][q] = 0.f;
                A[q][p] = 0.f;
YGZF_UNROLL
                for (int r = 0; r < 4; r++) {
                    if (r != p && r != q) {
                        const float arp = A[r][p], arq = A[r][q];
                        const float np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                        A[r][p] = np_; A[p][r] = np_;
                        A[r][q] = nq_; A[q][r] = nq_;
                    }
                    const float vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        }
    }
}

// ComputeSim3 on the three correspondences p1[k] / p2[k] (camera-1 / camera-2 coordinates of sample k)
YGZF_HD inline void horn(const float p1[3][3], const float p2[3][3], bool fixScale, Hyp &H) {
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];   // Pr[k][axis]
    const double third = 1.0 / 3.0;
    for (int a = 0; a < 3; a++) {
        O1[a] = (float) ((double) ((p1[0][a] + p1[1][a]) + p1[2][a]) * third);
        O2[a] = (float) ((double) ((p2[0][a] + p2[1][a]) + p2[2][a]) * third);
    }
    for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++) {
            Pr1[k][a] = p1[k][a] - O1[a];
            Pr2[k][a] = p2[k][a] - O2[a];
        }
    float M[3][3];   // Pr2 * Pr1.t()
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[r][c] = (Pr2[0][r] * Pr1[0][c] + Pr2[1][r] * Pr1[1][c]) + Pr2[2][r] * Pr1[2][c];
    float N[4][4], V[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    for (int r = 1; r < 4; r++)
        for (int c = 0; c < r; c++) N[r][c] = N[c][r];
    jacobi4(N, V);
    // the largest eigenvalue, the first of equals (a NaN never wins)
    float best = N[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
YGZF_UNROLL
    for (int k = 1; k < 4; k++)
        if (N[k][k] > best) { best = N[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
    if (x == 0.f && y == 0.f && z == 0.f) {
        const float nan = __builtin_nanf("");
        for (int i = 0; i < 9; i++) H.R[i] = nan;
    } else {
        const float n2 = ((w * w + x * x) + y * y) + z * z;
        const float s2 = 2.f / n2;
        const float xs = x * s2, ys = y * s2, zs = z * s2;
        const float wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
        H.R[0] = 1.f - (yy + zz); H.R[1] = xy - wz;         H.R[2] = xz + wy;
        H.R[3] = xy + wz;         H.R[4] = 1.f - (xx + zz); H.R[5] = yz - wx;
        H.R[6] = xz - wy;         H.R[7] = yz + wx;         H.R[8] = 1.f - (xx + yy);
    }
    if (!fixScale) {
        // P3 = R * Pr2; nom = Pr1.dot(P3); den = the double sum of the float squares of P3, both over the 3 x 3 matrices in row-major order
        double nom = 0.0, den = 0.0;
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) {
                const float p3 = (H.R[3 * r] * Pr2[k][0] + H.R[3 * r + 1] * Pr2[k][1]) + H.R[3 * r + 2] * Pr2[k][2];
                nom += (double) Pr1[k][r] * (double) p3;
                den += (double) (p3 * p3);
            }
        H.s = (float) (nom / den);
    } else
        H.s = 1.f;
    const double sd = (double) H.s, inv = 1.0 / sd;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            H.sR12[3 * r + c] = (float) (sd * (double) H.R[3 * r + c]);
            H.sR21[3 * r + c] = (float) (inv * (double) H.R[3 * c + r]);
        }
    for (int r = 0; r < 3; r++) H.t[r] = O1[r] - ((H.sR12[3 * r] * O2[0] + H.sR12[3 * r + 1] * O2[1]) + H.sR12[3 * r + 2] * O2[2]);
    for (int r = 0; r < 3; r++) H.t21[r] = -((H.sR21[3 * r] * H.t[0] + H.sR21[3 * r + 1] * H.t[1]) + H.sR21[3 * r + 2] * H.t[2]);
}

// FromCameraToImage: no depth gate, invz may be infinite
YGZF_HD inline void to_image(const float X[3], const float K[4], float uv[2]) {
    const float invz = 1.f / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}

// Project: sR X + t, then FromCameraToImage
YGZF_HD inline void project(const float sR[9], const float t[3], const float X[3], const float K[4], float uv[2]) {
    float P[3];
    for (int r = 0; r < 3; r++) P[r] = ((sR[3 * r] * X[0] + sR[3 * r + 1] * X[1]) + sR[3 * r + 2] * X[2]) + t[r];
    to_image(P, K, uv);
}

// dist.dot(dist) of a 2-vector: double accumulation, the result cast to float
YGZF_HD inline float err2(const float a[2], const float b[2]) {
    const float d0 = a[0] - b[0], d1 = a[1] - b[1];
    double s = (double) d0 * (double) d0;
    s += (double) d1 * (double) d1;
    return (float) s;
}

// one correspondence under one hypothesis (CheckInliers, :325-336): both errors below their gates with `<`, so a NaN fails
YGZF_HD inline bool inlier(const Hyp &H, const float X1[3], const float X2[3], const float K1[4], const float K2[4], float max1, float max2,
                                float *e1 = nullptr, float *e2 = nullptr) {
    float p1im1[2], p2im2[2], p2im1[2], p1im2[2];
    to_image(X1, K1, p1im1);
    to_image(X2, K2, p2im2);
    project(H.sR12, H.t, X2, K1, p2im1);
    project(H.sR21, H.t21, X1, K2, p1im2);
    const float err1 = err2(p1im1, p2im1), err2_ = err2(p1im2, p2im2);
    if (e1) *e1 = err1;
    if (e2) *e2 = err2_;
    return err1 < max1 && err2_ < max2;
}

}  // namespace sim3
}  // namespace ygzf
#endif
