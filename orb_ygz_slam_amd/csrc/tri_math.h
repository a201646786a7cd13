// tri_math.h -- one matched pair of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1078-1194: the two rays and the parallax test, the
// linear triangulation through Eigen::JacobiSVD<Matrix4f> or KeyFrame::UnprojectStereo (src/KeyFrame.cc:815-828), the two depth signs, the two
// reprojection gates and the scale-consistency gate) as scalar fp32 code in the source's order of operations.  k_triangulate
// (tri_kernels.hip) and plain host programs (tests/cpp/tri_host.cc) compile this same text: nothing of HIP is needed to read it.  Every
// operation is + - * / or sqrt on float (the gates: one product and one comparison on double, as the source's double literals make them)
// without contraction (-ffp-contract=off), so each is correctly rounded and numpy repeats it bit for bit (tests/triangulate_cases.py).
//
// What is read as the reference reads it:
//   keys                   the DISTORTED mvKeys (:1068, :1073), for the rays and for the reprojection errors alike
//   KF2's right-eye term   u2_r = u2 - mpCurrentKeyFrame->mbf * invz2 (:1168): KF1's mbf, not KF2's
//   1.0 / z                a double quotient rounded to float (:1134); for float z that is the float quotient (a double rounding of a
//                          quotient of two floats is innocuous: 53 >= 2 * 24 + 2), and the float quotient is what stands here
//   3-term Eigen sums      Matrix3f * Vector3f, dot and norm as (a0 b0 + a1 b1) + a2 b2, the order this library gives Eigen's small products
//                          everywhere (match_kernels.hip: k_frustum, k_fuse)
//   Twc * x3Dc             Sophus SE3f: unit quaternion (x y z w) through Eigen's _transformVector, v + w uv + qv x uv with uv = 2 (qv x v),
//                          then + translation (se3_device.h states the same product for the aligner)
//
// The stereo parallax cos(2 * atan2(mb / 2, mvDepth[idx])) (:1090, :1092) is a pure function of one feature of one keyframe: the caller
// computes it once per keyframe and passes it per feature (Feat::cosStereo).  In LocalMapping.cc `using namespace std` (include/Common.h:19)
// is in force and every operand is float (mb, mvDepth; 2 * float is float), so overload resolution picks std::atan2(float, float) and
// std::cos(float): the expression is cosf(2 * atan2f(mb / 2, depth)) in fp32, and the shell writes exactly that.  No trigonometric function
// is left for this text; there is one restatement, not a "device mode" beside a "reference mode".
//
// Eigen::JacobiSVD<Matrix4f>(A, ComputeFullU | ComputeFullV) is FIXED HERE as Eigen 3.3's two-sided Jacobi for a real square matrix
// (Eigen/src/SVD/JacobiSVD.h: compute(); Eigen/src/Jacobi/Jacobi.h: makeJacobi, apply_rotation_in_the_plane; RealSvd2x2.h), written down from
// knowledge of that text; Eigen is not available to hold it against, so parity with a compiled Eigen is unpinned:
//   scale = max |a_ij| (1 if 0); W = A / scale; V = I; maxDiag = max |W_ii|
//   sweep until a sweep rotates nothing: for p = 1..3, for q = 0..p-1:
//     threshold = max(FLT_MIN, 2 eps maxDiag);  if |W_pq| > threshold or |W_qp| > threshold:
//       real_2x2_jacobi_svd of [W_pp W_pq; W_qp W_qq]:
//         t = m00 + m11, d = m10 - m01;  rot1 = (c 1, s 0) if |d| < FLT_MIN, else u = t / d, tmp = sqrt(1 + u^2), s = 1 / tmp, c = u / tmp
//         m = rot1 applied on the left: row0' = c row0 + s row1, row1' = -s row0 + c row1
//         j_right = makeJacobi(m00, m01, m11): deno = 2 |y|; (c 1, s 0) if deno < FLT_MIN, else tau = (x - z) / deno, w = sqrt(tau^2 + 1),
//           t = 1 / (tau + w) if tau > 0 else 1 / (tau - w), n = 1 / sqrt(t^2 + 1), s = -sign(t) (y / |y|) |t| n, c = n
//         j_left = rot1 * j_right^T: c = c1 cr - s1 (-sr), s = c1 (-sr) + s1 cr
//       W.applyOnTheLeft(p, q, j_left):   row_p' = c row_p + s row_q,  row_q' = -s row_p + c row_q   (skipped when c == 1 and s == 0)
//       W.applyOnTheRight(p, q, j_right), V likewise: col_p' = c col_p + (-s) col_q, col_q' = s col_p + c col_q
//       maxDiag = max(maxDiag, max(|W_pp|, |W_qq|))
//   singular values |W_ii| * scale (the sign goes into U, which :1107-1110 never reads and which does not feed W: U is left out)
//   descending selection sort: the first largest of the tail, columns of V swapped with it
// One deviation: Eigen's loop has no iteration cap and a kernel's must.  kMaxSweeps rotating sweeps without a clean one end the pair with
// status kSweepCap (rejected).  DESIGN.md records the largest count met and why the cap is far from it.
#ifndef YGZF_TRI_MATH_H
#define YGZF_TRI_MATH_H
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "lm_math.h"   // for YGZF_HD and YGZF_UNROLL, the one set of these macros; nothing else of it is used here

// The most rotating sweeps of the Jacobi SVD, for the kernel and the restatement alike (tests/triangulate_cases.py reads this line).  A host
// program may be built with a lower cap (-DYGZF_TRI_MAX_SWEEPS=n) to drive the kSweepCap exit; the library is never built that way.
#ifndef YGZF_TRI_MAX_SWEEPS
#define YGZF_TRI_MAX_SWEEPS 16
#endif

namespace ygzf {
namespace tri {

constexpr int kMaxSweeps = YGZF_TRI_MAX_SWEEPS;

// status byte: low 4 bits = 0 accepted, else the `continue` of the source that took the pair, in the source's order; bits 6-7 = where x3D came from
enum Status : uint8_t {
    kAccepted = 0,
    kLowParallax = 1,   // :1117 no stereo and very low parallax
    kV33Zero = 2,       // :1108
    kZ1 = 3,            // :1123
    kZ2 = 4,            // :1127
    kReproj1 = 5,       // :1141 / :1150
    kReproj2 = 6,       // :1164 / :1173
    kZeroDist = 7,      // :1184
    kScaleRatio = 8,    // :1193
    kSweepCap = 9,      // this text's own: the SVD met kMaxSweeps
    kStatusMask = 15,
    kFromNone = 0 << 6, kFromSvd = 1 << 6, kFromKf1 = 2 << 6, kFromKf2 = 3 << 6, kFromMask = 3 << 6
};

struct Kf {                       // what the pair reads of one keyframe
    float fx, fy, cx, cy, invfx, invfy, mbf;
    float Rcw[9], tcw[3], Ow[3];  // GetRotation (row-major) / GetTranslation / GetCameraCenter
    float q[4], t[3];             // Twc as the keyframe holds it: unit quaternion x y z w, translation
};
struct Feat {                     // what the pair reads of one feature
    float x, y;                   // mvKeys[idx].pt
    float uR;                     // mvuRight[idx] (monocular: -1)
    float depth, cosStereo;       // mvDepth[idx], cos(2 * atan2(mb / 2, mvDepth[idx])); read only where uR >= 0
    float sigma2, scale;          // mvLevelSigma2 / mvScaleFactors at mvKeys[idx].octave
};

YGZF_HD inline float max_f(float a, float b) { return a < b ? b : a; }   // std::max / numext::maxi

// One (p, q) step of a sweep on the registers of W and V; P and Q are constants, so no array is indexed by a run-time value.
template <int P, int Q> YGZF_HD inline void svd_step(float W[4][4], float V[4][4], float &maxDiag, bool &rotated) {
    const float threshold = max_f(FLT_MIN, (2.f * FLT_EPSILON) * maxDiag);
    if (!(fabsf(W[P][Q]) > threshold || fabsf(W[Q][P]) > threshold)) return;
    rotated = true;
    // real_2x2_jacobi_svd
    float m00 = W[P][P], m01 = W[P][Q], m10 = W[Q][P], m11 = W[Q][Q];
    const float t = m00 + m11, d = m10 - m01;
    float c1, s1;
    if (fabsf(d) < FLT_MIN) {
        s1 = 0.f;
        c1 = 1.f;
    } else {
        const float u = t / d;
        const float tmp = sqrtf(1.f + u * u);
        s1 = 1.f / tmp;
        c1 = u / tmp;
    }
    if (!(c1 == 1.f && s1 == 0.f)) {   // m.applyOnTheLeft(0, 1, rot1)
        const float a00 = c1 * m00 + s1 * m10, a10 = -s1 * m00 + c1 * m10;
        const float a01 = c1 * m01 + s1 * m11, a11 = -s1 * m01 + c1 * m11;
        m00 = a00; m10 = a10; m01 = a01; m11 = a11;
    }
    float cr, sr;   // j_right = makeJacobi(m00, m01, m11)
    const float deno = 2.f * fabsf(m01);
    if (deno < FLT_MIN) {
        cr = 1.f;
        sr = 0.f;
    } else {
        const float tau = (m00 - m11) / deno;
        const float w = sqrtf(tau * tau + 1.f);
        const float tt = tau > 0.f ? 1.f / (tau + w) : 1.f / (tau - w);
        const float sign_t = tt > 0.f ? 1.f : -1.f;
        const float n = 1.f / sqrtf(tt * tt + 1.f);
        sr = -sign_t * (m01 / fabsf(m01)) * fabsf(tt) * n;
        cr = n;
    }
    // j_left = rot1 * j_right.transpose(), the transpose being (cr, -sr)
    const float nsr = -sr;
    const float cl = c1 * cr - s1 * nsr, sl = c1 * nsr + s1 * cr;
    if (!(cl == 1.f && sl == 0.f)) {   // W.applyOnTheLeft(p, q, j_left)
YGZF_UNROLL
        for (int i = 0; i < 4; i++) {
            const float x = W[P][i], y = W[Q][i];
            W[P][i] = cl * x + sl * y;
            W[Q][i] = -sl * x + cl * y;
        }
    }
    if (!(cr == 1.f && nsr == 0.f)) {   // W.applyOnTheRight(p, q, j_right); V.applyOnTheRight(p, q, j_right): the rotation applied is the transpose
YGZF_UNROLL
        for (int i = 0; i < 4; i++) {
            const float x = W[i][P], y = W[i][Q];
            W[i][P] = cr * x + nsr * y;
            W[i][Q] = -nsr * x + cr * y;
        }
YGZF_UNROLL
        for (int i = 0; i < 4; i++) {
            const float x = V[i][P], y = V[i][Q];
            V[i][P] = cr * x + nsr * y;
            V[i][Q] = -nsr * x + cr * y;
        }
    }
    maxDiag = max_f(maxDiag, max_f(fabsf(W[P][P]), fabsf(W[Q][Q])));
}

// swap the tail's first largest singular value (and its column of V) into place I
template <int I> YGZF_HD inline void svd_sort_step(float sv[4], float V[4][4]) {
    float best = sv[I];
    int pos = I;
YGZF_UNROLL
    for (int j = I + 1; j < 4; j++)
        if (sv[j] > best) { best = sv[j]; pos = j; }
YGZF_UNROLL
    for (int j = I + 1; j < 4; j++) {
        if (pos == j) {   // j is a constant of the unrolled loop
            const float s = sv[I]; sv[I] = sv[j]; sv[j] = s;
YGZF_UNROLL
            for (int r = 0; r < 4; r++) { const float v = V[r][I]; V[r][I] = V[r][j]; V[r][j] = v; }
        }
    }
}

// JacobiSVD<Matrix4f>: V (columns = right singular vectors, descending singular values sv) of A.  -> the rotating sweeps used;
// kMaxSweeps: the cap was met and V / sv are not to be used.
YGZF_HD inline int jacobi_svd4(const float A[4][4], float V[4][4], float sv[4]) {
    float W[4][4];
    float scale = 0.f;
YGZF_UNROLL
    for (int r = 0; r < 4; r++)
YGZF_UNROLL
        for (int c = 0; c < 4; c++) {
            const float a = fabsf(A[r][c]);
            if (r == 0 && c == 0) scale = a; else if (a > scale) scale = a;   // maxCoeff: the first, replaced by what is greater
        }
    if (scale == 0.f) scale = 1.f;
YGZF_UNROLL
    for (int r = 0; r < 4; r++)
YGZF_UNROLL
        for (int c = 0; c < 4; c++) {
            W[r][c] = A[r][c] / scale;
            V[r][c] = r == c ? 1.f : 0.f;
        }
    float maxDiag = fabsf(W[0][0]);
YGZF_UNROLL
    for (int i = 1; i < 4; i++)
        if (fabsf(W[i][i]) > maxDiag) maxDiag = fabsf(W[i][i]);
    int sweeps = 0;
    for (int s = 0; s < kMaxSweeps; s++) {
        bool rotated = false;
        svd_step<1, 0>(W, V, maxDiag, rotated);
        svd_step<2, 0>(W, V, maxDiag, rotated);
        svd_step<2, 1>(W, V, maxDiag, rotated);
        svd_step<3, 0>(W, V, maxDiag, rotated);
        svd_step<3, 1>(W, V, maxDiag, rotated);
        svd_step<3, 2>(W, V, maxDiag, rotated);
        if (!rotated) break;
        sweeps++;
    }
YGZF_UNROLL
    for (int i = 0; i < 4; i++) sv[i] = fabsf(W[i][i]) * scale;
    svd_sort_step<0>(sv, V);
    svd_sort_step<1>(sv, V);
    svd_sort_step<2>(sv, V);
    return sweeps;
}

YGZF_HD inline void unproject_stereo(const Kf &K, const Feat &f, float o[3]) {   // KeyFrame::UnprojectStereo
    const float z = f.depth;
    if (z > 0.f) {
        const float v[3] = {(f.x - K.cx) * z * K.invfx, (f.y - K.cy) * z * K.invfy, z};
        const float *q = K.q;
        float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
        uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
        const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
YGZF_UNROLL
        for (int i = 0; i < 3; i++) o[i] = ((v[i] + q[3] * uv[i]) + c[i]) + K.t[i];
    } else {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    }
}

YGZF_HD inline float row_dot(const float *R, const float x[3]) { return (R[0] * x[0] + R[1] * x[1]) + R[2] * x[2]; }

// the chi-square gate of one keyframe (:1130-1152 / :1154-1175); mbf is KF1's on both sides.  true: the pair goes on
YGZF_HD inline bool reprojects(const Kf &K, const Feat &f, float mbf, const float X[3], float z) {
    const float x = row_dot(K.Rcw, X) + K.tcw[0];
    const float y = row_dot(K.Rcw + 3, X) + K.tcw[1];
    const float invz = 1.f / z;
    const float u = K.fx * x * invz + K.cx;
    if (!(f.uR >= 0.f)) {
        const float v = K.fy * y * invz + K.cy;
        const float eX = u - f.x, eY = v - f.y;
        return !((double) (eX * eX + eY * eY) > 5.991 * (double) f.sigma2);
    }
    const float u_r = u - mbf * invz;
    const float v = K.fy * y * invz + K.cy;
    const float eX = u - f.x, eY = v - f.y, eR = u_r - f.uR;
    return !((double) (eX * eX + eY * eY + eR * eR) > 7.8 * (double) f.sigma2);
}

// One pair.  -> the status byte; x3D is written for every pair (0 0 0 where no source gave one); *sweeps (nullable) = the SVD's sweeps (0 without SVD)
YGZF_HD inline uint8_t triangulate_pair(const Kf &K1, const Kf &K2, const Feat &f1, const Feat &f2, float ratioFactor, float x3D[3], int *sweeps) {
    if (sweeps) *sweeps = 0;
    x3D[0] = 0.f; x3D[1] = 0.f; x3D[2] = 0.f;
    const bool stereo1 = f1.uR >= 0.f, stereo2 = f2.uR >= 0.f;
    const float xn1[3] = {(f1.x - K1.cx) * K1.invfx, (f1.y - K1.cy) * K1.invfy, 1.f};
    const float xn2[3] = {(f2.x - K2.cx) * K2.invfx, (f2.y - K2.cy) * K2.invfy, 1.f};
    float ray1[3], ray2[3];   // Rwc * xn, Rwc = Rcw'
YGZF_UNROLL
    for (int i = 0; i < 3; i++) {
        ray1[i] = (K1.Rcw[i] * xn1[0] + K1.Rcw[3 + i] * xn1[1]) + K1.Rcw[6 + i] * xn1[2];
        ray2[i] = (K2.Rcw[i] * xn2[0] + K2.Rcw[3 + i] * xn2[1]) + K2.Rcw[6 + i] * xn2[2];
    }
    const float cosRays = row_dot(ray1, ray2) / (sqrtf(row_dot(ray1, ray1)) * sqrtf(row_dot(ray2, ray2)));
    float cosStereo = cosRays + 1.f;
    float cosStereo1 = cosStereo, cosStereo2 = cosStereo;
    if (stereo1) cosStereo1 = f1.cosStereo;
    else if (stereo2) cosStereo2 = f2.cosStereo;
    cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;   // std::min(cosStereo1, cosStereo2)
    uint8_t from;
    if (cosRays < cosStereo && cosRays > 0.f && (stereo1 || stereo2 || (double) cosRays < 0.9998)) {
        float A[4][4], V[4][4], sv[4];
YGZF_UNROLL
        for (int j = 0; j < 4; j++) {
            const float a0 = j < 3 ? K1.Rcw[j] : K1.tcw[0], a1 = j < 3 ? K1.Rcw[3 + j] : K1.tcw[1], a2 = j < 3 ? K1.Rcw[6 + j] : K1.tcw[2];
            const float b0 = j < 3 ? K2.Rcw[j] : K2.tcw[0], b1 = j < 3 ? K2.Rcw[3 + j] : K2.tcw[1], b2 = j < 3 ? K2.Rcw[6 + j] : K2.tcw[2];
            A[0][j] = xn1[0] * a2 - a0;
            A[1][j] = xn1[1] * a2 - a1;
            A[2][j] = xn2[0] * b2 - b0;
            A[3][j] = xn2[1] * b2 - b1;
        }
        const int n = jacobi_svd4(A, V, sv);
        if (sweeps) *sweeps = n;
        from = kFromSvd;
        if (n >= kMaxSweeps) return from | kSweepCap;
        if (V[3][3] == 0.f) return from | kV33Zero;
        x3D[0] = V[0][3] / V[3][3]; x3D[1] = V[1][3] / V[3][3]; x3D[2] = V[2][3] / V[3][3];
    } else if (stereo1 && cosStereo1 < cosStereo2) {
        from = kFromKf1;
        unproject_stereo(K1, f1, x3D);
    } else if (stereo2 && cosStereo2 < cosStereo1) {
        from = kFromKf2;
        unproject_stereo(K2, f2, x3D);
    } else {
        return kFromNone | kLowParallax;
    }
    const float z1 = row_dot(K1.Rcw + 6, x3D) + K1.tcw[2];
    if (z1 <= 0.f) return from | kZ1;
    const float z2 = row_dot(K2.Rcw + 6, x3D) + K2.tcw[2];
    if (z2 <= 0.f) return from | kZ2;
    if (!reprojects(K1, f1, K1.mbf, x3D, z1)) return from | kReproj1;
    if (!reprojects(K2, f2, K1.mbf, x3D, z2)) return from | kReproj2;
    const float n1[3] = {x3D[0] - K1.Ow[0], x3D[1] - K1.Ow[1], x3D[2] - K1.Ow[2]};
    const float n2[3] = {x3D[0] - K2.Ow[0], x3D[1] - K2.Ow[1], x3D[2] - K2.Ow[2]};
    const float dist1 = sqrtf(row_dot(n1, n1)), dist2 = sqrtf(row_dot(n2, n2));
    if (dist1 == 0.f || dist2 == 0.f) return from | kZeroDist;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = f1.scale / f2.scale;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return from | kScaleRatio;
    return from | kAccepted;
}

}  // namespace tri
}  // namespace ygzf
#endif
