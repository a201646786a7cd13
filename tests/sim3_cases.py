"""Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) restated in numpy, its plausible wrong forms behind a switch each, and constructed cases
with a reach predicate each.  No device and no library: tests/test_sim3_cases.py holds the cases to their claims, tests/test_sim3_host_progs.py
runs host/Sim3Replay.h against `sim3_iterate`, tests/test_gpu_sim3.py runs the cases on the GPU against mode "device", bit for bit.

The reference's file needs cv::eigen, cv::Rodrigues, cv::reduce and cv::pow, which the stand-in OpenCV of oracle/ref_shim does not have: this row is
*parity unpinned*  and the arithmetic below is what fixes it.  The cv::Mat roundings are OpenCV 2.4 / 3.2's as
host/ORBmatcherLoop.h and tests/loop_cases.py already fix them for this project, reused here:

    small gemm             a float dot, left to right: (a0 b0 + a1 b1) + a2 b2          (M = Pr2 Pr1', P3 = R Pr2, sR O2, sRinv t, R X + t)
    scalar * Mat, Mat / n  a double factor, each entry rounded to float once           (C / 3 = C * (1.0 / 3), s R, (1.0 / s) R')
    Mat::dot, norm         double accumulation in index order                          (nom, dist.dot(dist), norm(vec))
and new with this module:
    cv::reduce(SUM)        a float sum, left to right
    N11 .. N44             float sums left to right (they are assigned to doubles and stored into a float matrix: no rounding is added)
    cv::eigen              cyclic Jacobi in fp32, both modes: rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per sweep, at most JACOBI_SWEEPS sweeps
                           (csrc/sim3_math.h holds the constant), a pair with an exactly zero entry is passed over -- so the solver stops
                           exactly when all six are zero --; theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
                           c = 1 / sqrt(t^2 + 1), s = t c; the eigenvector of the largest eigenvalue, the first of equals
    den                    the double sum, row-major, of the float squares of P3
    t12                    O1 - (sR) O2 with sR = s R as above: the gemm's alpha is applied first

Two modes of the step from the eigenvector q = (w, x, y, z) to R:
    reference  the source text: ang = atan2(norm(vec), w) in double, vec = vec * (2 ang / norm(vec)) rounded to float, cv::Rodrigues in double
               (theta = norm(vec), R = cos I + (1 - cos) r r' + sin [r]x), cast to float
    device     the kernel's: R = I + (2 / |q|^2) [..] with + - * / only, every operation correctly rounded, so numpy repeats the device bit for
               bit.  Both keep the reference's 0 / 0: x = y = z = 0 exactly makes every entry of R NaN.
"""
import collections
import math
import os
import re

import numpy as np

f32, f64 = np.float32, np.float64
_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER = os.path.join(os.path.dirname(_HERE), "orb_ygz_slam_amd", "csrc", "sim3_math.h")
JACOBI_SWEEPS = int(re.search(r"^#define YGZF_SIM3_JACOBI_SWEEPS (\d+)", open(_HEADER).read(), re.M).group(1))

WRONG_FORMS = ("float_gates", "gate_le", "best_gt", "return_ge", "best_reset", "depth_gate", "identity_ok", "scale_when_fixed", "t21_inverse",
               "sample_replace", "niter_no_n_rule", "nomore_on_return")
# float_gates        the gates are 9.21 sigma^2 as floats (the reference: truncated to size_t)
# gate_le            err <= gate
# best_gt            the best hypothesis is replaced on > only (the reference: >=, a tie takes the later one)
# return_ge          iterate returns on mnInliersi >= mRansacMinInliers (the reference: >)
# best_reset         the best-so-far count starts at 0 in every iterate call
# depth_gate         a correspondence needs z > 0 in all four projections
# identity_ok        a zero imaginary part gives R = I
# scale_when_fixed   the scale is computed although mbFixScale is set
# t21_inverse        T21 is the inverse of the rounded T12 (the reference: (1.0 / s) R' and -sRinv t)
# sample_replace     the three draws of a triple do not remove what they drew
# niter_no_n_rule    nIterations is always the logarithm formula
# nomore_on_return   bNoMore is also set on a call that returns a hypothesis at mnIterations == mRansacMaxIts

# ---- tolerances ----------------------------------------------------------------------------------------------------------------------------------
# EPS_MODE: the largest difference of any finite hyp entry (R, t, s) between the two modes over the constructed cases, whose samples are well
# conditioned -- what evaluating the rotation through atan2 / Rodrigues instead of straight from the quaternion does.  tests/test_sim3_cases.py
# measures it and holds it against this constant (at most the constant, which is at most twice the measurement).
EPS_MODE = 1.5e-6   # measured 9.54e-7 (eight units in the last place of a translation entry near 1), at all_n64 and the two-group cases; the
# constant leaves room for a libm whose atan2 / sin / cos round the reference mode one unit further
# MARGIN_MIN: the decision margin every constructed case must keep, in both modes: the smallest |err - gate| / gate over all finite errors (an
# error exactly equal to its gate is a tie that both modes reproduce, not a decision, and is left out).  What EPS_MODE does to an error: an
# entry of R or t off by eps moves a projected pixel by at most about f (|X| / z) eps with f <= 520 and |X| / z <= 1.5 in the cases below, i.e.
# 780 eps px; an error near its gate g >= 9 is e = d^2 with d = sqrt(g) >= 3, so de / g = 2 d dd / g <= 2 * 780 eps / 3 = 520 eps = 7.8e-4.
# MARGIN_MIN is ten times that (the tightest case, gate13_between, sits 1e-2 from both 13 and 13.26 by construction).
MARGIN_MIN = 8.0e-3

Problem = collections.namedtuple("Problem", "X1 X2 sigma2_1 sigma2_2 K1 K2 fix_scale samples prob min_inliers max_its calls mN1 indices1")
# X1 / X2: mvX3Dc1 / mvX3Dc2 (n x 3 float32); sigma2_*: mvLevelSigma2 of each correspondence's octave; K: fx fy cx cy; samples: H x 3 (the triples
# in the order iterate draws them); prob / min_inliers / max_its: SetRansacParameters' arguments; calls: the nIterations of successive iterate
# calls ("find" = find()); mN1 / indices1: vpMatched12.size() and mvnIndices1
Hyps = collections.namedtuple("Hyps", "hyp err1 err2 bits count margin")
Call = collections.namedtuple("Call", "returned hyp_index n_inliers no_more inliers12 best_index best_inliers iterations")
Case = collections.namedtuple("Case", "name problem moved_by reach seeded")


# ---- the gates and SetRansacParameters -----------------------------------------------------------------------------------------------------------
def gates(sigma2, wrong=None):
    g = 9.210 * np.asarray(sigma2, f32).astype(f64)
    if wrong == "float_gates":
        return g.astype(f32)
    with np.errstate(invalid="ignore"):
        return np.floor(g).astype(f32)


def ransac_max_its(N, prob, min_inliers, max_its, wrong=None):
    """mRansacMaxIts (:107-130).  epsilon is a float quotient, the rest double.  The reference converts the quotient of logarithms to int, which
    is undefined beyond INT_MAX and for a NaN (N < minInliers gives log of a negative number): the restatement, like host/Sim3Replay.h, compares
    in double and takes maxIterations there -- iterate never runs an iteration when N < minInliers, and a count beyond INT_MAX is beyond
    maxIterations."""
    with np.errstate(all="ignore"):
        if min_inliers == N and wrong != "niter_no_n_rule":
            n_it = f64(1)
        else:
            eps = f32(min_inliers) / f32(N)
            n_it = np.ceil(np.log(f64(1) - f64(prob)) / np.log(f64(1) - f64(math.pow(float(eps), 3)) if np.isfinite(eps) else f64(-np.inf)))
        if np.isnan(n_it) or n_it > max_its:
            n_it = f64(max_its)
        if n_it < 1:
            n_it = f64(1)
    return int(n_it)


# (N, minInliers, probability, maxIterations) -> mRansacMaxIts, worked out by hand from the formula: e.g. N = 40, minInliers = 20: epsilon = 0.5,
# log(0.01) / log(0.875) = 34.49 -> 35; N = 21: epsilon^3 = 0.8638, log(0.01) / log(0.1362) = 2.31 -> 3; N = 25: log(0.01) / log(0.488) = 6.42 -> 7
MAX_ITS_TABLE = ((100, 20, 0.99, 300, 300), (40, 20, 0.99, 300, 35), (25, 20, 0.99, 300, 7), (20, 20, 0.99, 300, 1), (21, 20, 0.99, 300, 3),
                 (10, 20, 0.99, 300, 300), (5000, 6, 0.99, 300, 300), (40, 20, 0.5, 300, 6), (40, 20, 0.99, 2, 2), (0, 6, 0.99, 300, 300), (3, 3, 0.99, 300, 1),
                 (3, 2, 0.99, 300, 14), (40, 20, 1.0, 300, 300), (40, 0, 0.99, 300, 1))


# ---- sampling (:152-165) -------------------------------------------------------------------------------------------------------------------------
class Lcg:
    """a stand-in for rand() with RAND_MAX = 2^31 - 1, so that a host program can repeat the draws: DUtils::Random::RandomInt on top of it"""

    def __init__(self, seed):
        self.state = seed & 0x7FFFFFFF

    def rand(self):
        self.state = (self.state * 1103515245 + 12345) & 0x7FFFFFFF
        return self.state

    def random_int(self, lo, hi):
        d = hi - lo + 1
        return int((float(self.rand()) / (2147483647.0 + 1.0)) * d) + lo


def draw_triples(n, count, random_int, wrong=None):
    """`count` iterations' worth of draws in the reference's order: a fresh copy of mvAllIndices per iteration, three draws, each swapped with the
    back and popped"""
    out = np.zeros((count, 3), np.int32)
    for h in range(count):
        avail = list(range(n))
        for i in range(3):
            r = random_int(0, len(avail) - 1)
            out[h, i] = avail[r]
            if wrong != "sample_replace":
                avail[r] = avail[-1]
                avail.pop()
    return out


# ---- one batch of hypotheses, vectorised over the hypotheses (every array op below is one correctly rounded operation per element) --------------------
def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _jacobi(A):
    """A: H x 4 x 4 float32 symmetric -> (eigenvalues on the diagonal of A, V with the eigenvectors in its columns)"""
    H = A.shape[0]
    A = A.copy()
    V = np.zeros((H, 4, 4), f32)
    for i in range(4):
        V[:, i, i] = 1
    one, two = f32(1), f32(2)
    for _ in range(JACOBI_SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[:, p, q].copy()
                on = ~(apq == 0)   # (a NaN is rotated like any other entry)
                if not on.any():
                    continue
                theta = (A[:, q, q] - A[:, p, p]) / (two * apq)
                tt = one / (np.abs(theta) + np.sqrt(theta * theta + one))
                t = np.where(theta < 0, -tt, tt)
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                A[:, p, p] = np.where(on, A[:, p, p] - h, A[:, p, p])
                A[:, q, q] = np.where(on, A[:, q, q] + h, A[:, q, q])
                A[:, p, q] = np.where(on, 0, A[:, p, q])
                A[:, q, p] = np.where(on, 0, A[:, q, p])
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        n_p, n_q = c * arp - s * arq, s * arp + c * arq
                        A[:, r, p] = A[:, p, r] = np.where(on, n_p, arp)
                        A[:, r, q] = A[:, q, r] = np.where(on, n_q, arq)
                    vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p] = np.where(on, c * vrp - s * vrq, vrp)
                    V[:, r, q] = np.where(on, s * vrp + c * vrq, vrq)
    return A, V


def _rotation_device(w, x, y, z):
    one, two = f32(1), f32(2)
    n2 = ((w * w + x * x) + y * y) + z * z
    s2 = two / n2
    xs, ys, zs = x * s2, y * s2, z * s2
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    return np.stack([one - (yy + zz), xy - wz, xz + wy, xy + wz, one - (xx + zz), yz - wx, xz - wy, yz + wx, one - (xx + yy)], axis=1)


def _rotation_reference(w, x, y, z):
    v = np.stack([x, y, z], axis=1).astype(f64)
    nrm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])   # norm(vec): double accumulation
    ang = np.arctan2(nrm, w.astype(f64))
    vec = (v * ((2.0 * ang) / nrm)[:, None]).astype(f32).astype(f64)   # MatExpr: one double factor, rounded to float
    theta = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
    c, s = np.cos(theta), np.sin(theta)
    r = vec / theta[:, None]
    R = np.zeros((len(w), 3, 3))
    for i in range(3):
        for j in range(3):
            R[:, i, j] = (1 - c) * r[:, i] * r[:, j] + (c if i == j else 0)
    R[:, 0, 1] -= s * r[:, 2]; R[:, 0, 2] += s * r[:, 1]
    R[:, 1, 0] += s * r[:, 2]; R[:, 1, 2] -= s * r[:, 0]
    R[:, 2, 0] -= s * r[:, 1]; R[:, 2, 1] += s * r[:, 0]
    small = theta < np.finfo(f64).eps   # cvRodrigues2's identity branch (a NaN does not take it)
    R[small] = np.eye(3)
    return R.reshape(-1, 9).astype(f32)


def _to_image(X, K):
    """FromCameraToImage on (..., 3) arrays"""
    invz = f32(1) / X[..., 2]
    x, y = X[..., 0] * invz, X[..., 1] * invz
    return f32(K[0]) * x + f32(K[2]), f32(K[1]) * y + f32(K[3])


def _project(sR, t, X, K):
    """Project: sR (H x 9), t (H x 3) on X (n x 3) -> u, v (H x n), and the depth"""
    P = []
    for r in range(3):
        P.append(_dot3(sR[:, 3 * r, None], X[None, :, 0], sR[:, 3 * r + 1, None], X[None, :, 1], sR[:, 3 * r + 2, None], X[None, :, 2]) + t[:, r, None])
    P = np.stack(P, axis=-1)
    u, v = _to_image(P, K)
    return u, v, P[..., 2]


def _err(ua, va, ub, vb):
    d0, d1 = (ua - ub).astype(f64), (va - vb).astype(f64)
    s = d0 * d0
    s = s + d1 * d1
    return s.astype(f32)


def sim3_hypotheses(P, mode="device", wrong=None):
    """every hypothesis of P.samples: hyp (H x 13: R12 row-major, t12, s12), err1 / err2 (H x n), the inlier bits (H x ceil(n / 64) uint64), the
    counts, and the decision margin"""
    assert mode in ("reference", "device")
    with np.errstate(all="ignore"):
        return _hypotheses(P, mode, wrong)


def _hypotheses(P, mode, wrong):
    X1, X2 = np.asarray(P.X1, f32).reshape(-1, 3), np.asarray(P.X2, f32).reshape(-1, 3)
    n = len(X1)
    S = np.asarray(P.samples, np.int64).reshape(-1, 3)
    H = len(S)
    words = (n + 63) // 64
    if H == 0:
        return Hyps(np.zeros((0, 13), f32), np.zeros((0, n), f32), np.zeros((0, n), f32), np.zeros((0, words), np.uint64), np.zeros(0, np.int32), np.inf)
    p1, p2 = X1[S], X2[S]   # H x 3 (sample) x 3 (axis)
    third = 1.0 / 3.0
    O1 = (((p1[:, 0] + p1[:, 1]) + p1[:, 2]).astype(f64) * third).astype(f32)
    O2 = (((p2[:, 0] + p2[:, 1]) + p2[:, 2]).astype(f64) * third).astype(f32)
    Pr1, Pr2 = p1 - O1[:, None, :], p2 - O2[:, None, :]
    M = np.zeros((H, 3, 3), f32)
    for r in range(3):
        for c in range(3):
            M[:, r, c] = _dot3(Pr2[:, 0, r], Pr1[:, 0, c], Pr2[:, 1, r], Pr1[:, 1, c], Pr2[:, 2, r], Pr1[:, 2, c])
    N = np.zeros((H, 4, 4), f32)
    N[:, 0, 0] = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    N[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = (M[:, 0, 0] - M[:, 1, 1]) - M[:, 2, 2]
    N[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = (-M[:, 0, 0] + M[:, 1, 1]) - M[:, 2, 2]
    N[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = (-M[:, 0, 0] - M[:, 1, 1]) + M[:, 2, 2]
    for r in range(1, 4):
        for c in range(r):
            N[:, r, c] = N[:, c, r]
    D, V = _jacobi(N)
    best = D[:, 0, 0].copy()
    q = V[:, :, 0].copy()
    for k in range(1, 4):
        win = D[:, k, k] > best
        best = np.where(win, D[:, k, k], best)
        q = np.where(win[:, None], V[:, :, k], q)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = _rotation_device(w, x, y, z) if mode == "device" else _rotation_reference(w, x, y, z)
    zero_im = (x == 0) & (y == 0) & (z == 0)
    if wrong == "identity_ok":
        R[zero_im] = np.eye(3, dtype=f32).reshape(9)
    else:
        R[zero_im] = np.nan
    if P.fix_scale and wrong != "scale_when_fixed":
        s = np.ones(H, f32)
    else:
        nom, den = np.zeros(H), np.zeros(H)
        for r in range(3):
            for k in range(3):
                p3 = _dot3(R[:, 3 * r], Pr2[:, k, 0], R[:, 3 * r + 1], Pr2[:, k, 1], R[:, 3 * r + 2], Pr2[:, k, 2])
                nom = nom + Pr1[:, k, r].astype(f64) * p3.astype(f64)
                den = den + (p3 * p3).astype(f64)
        s = (nom / den).astype(f32)
    sd = s.astype(f64)
    inv = 1.0 / sd
    sR12 = (sd[:, None] * R.astype(f64)).astype(f32)
    Rt = R.reshape(H, 3, 3).transpose(0, 2, 1).reshape(H, 9)
    sR21 = (inv[:, None] * Rt.astype(f64)).astype(f32)
    t = np.stack([O1[:, r] - _dot3(sR12[:, 3 * r], O2[:, 0], sR12[:, 3 * r + 1], O2[:, 1], sR12[:, 3 * r + 2], O2[:, 2]) for r in range(3)], axis=1)
    t21 = np.stack([-_dot3(sR21[:, 3 * r], t[:, 0], sR21[:, 3 * r + 1], t[:, 1], sR21[:, 3 * r + 2], t[:, 2]) for r in range(3)], axis=1)
    if wrong == "t21_inverse":
        for h in range(H):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = sR12[h].reshape(3, 3), t[h]
            if np.all(np.isfinite(T)) and abs(np.linalg.det(T)) > 0:
                Ti = np.linalg.inv(T)
                sR21[h], t21[h] = Ti[:3, :3].reshape(9).astype(f32), Ti[:3, 3].astype(f32)
    u11, v11 = _to_image(X1, P.K1)
    u22, v22 = _to_image(X2, P.K2)
    u21, v21, z21 = _project(sR12, t, X2, P.K1)
    u12, v12, z12 = _project(sR21, t21, X1, P.K2)
    err1 = _err(u11[None, :], v11[None, :], u21, v21)
    err2 = _err(u12, v12, u22[None, :], v22[None, :])
    g1, g2 = gates(P.sigma2_1, wrong), gates(P.sigma2_2, wrong)
    if wrong == "gate_le":
        ok = (err1 <= g1[None, :]) & (err2 <= g2[None, :])
    else:
        ok = (err1 < g1[None, :]) & (err2 < g2[None, :])
    if wrong == "depth_gate":
        ok &= (X1[None, :, 2] > 0) & (X2[None, :, 2] > 0) & (z21 > 0) & (z12 > 0)
    count = ok.sum(axis=1).astype(np.int32)
    padded = np.zeros((H, words * 64), bool)
    padded[:, :n] = ok
    bits = np.packbits(padded.reshape(H, words, 64), axis=2, bitorder="little").view(np.uint64).reshape(H, words)
    margin = np.inf
    for e, g in ((err1, g1), (err2, g2)):
        G = np.broadcast_to(g[None, :], e.shape)
        m = np.isfinite(e) & (e != G) & (G > 0)
        if m.any():
            margin = min(margin, float(np.min(np.abs(e[m].astype(f64) - G[m]) / G[m])))
    hyp = np.concatenate([R, t, s[:, None]], axis=1).astype(f32)
    return Hyps(hyp, err1, err2, bits, count, margin)


# ---- iterate / find replayed from the counts and bits (:132-198) --------------------------------------------------------------------------------
def bit(bits_row, i):
    return bool((int(bits_row[i >> 6]) >> (i & 63)) & 1)


def sim3_iterate(count, bits, P, wrong=None):
    """SetRansacParameters(P.prob, P.min_inliers, P.max_its), then one iterate call per entry of P.calls on one solver: what each call returns and
    the solver's state behind it.  Hypothesis h of `count` / `bits` is the solver's iteration h + 1."""
    N = len(np.asarray(P.X1).reshape(-1, 3))
    max_its = ransac_max_its(N, P.prob, P.min_inliers, P.max_its, wrong)
    it, best, best_idx = 0, 0, -1
    out = []
    for nIterations in P.calls:
        if nIterations == "find":
            nIterations = max_its
        if wrong == "best_reset":
            best = 0
        inl = np.zeros(P.mN1, bool)
        if N < P.min_inliers:
            out.append(Call(False, -1, 0, True, inl, best_idx, best, it))
            continue
        cur, res = 0, None
        while it < max_its and cur < nIterations:
            cur += 1
            it += 1
            c = int(count[it - 1])
            if (c > best) if wrong == "best_gt" else (c >= best):
                best, best_idx = c, it - 1
                if (c >= P.min_inliers) if wrong == "return_ge" else (c > P.min_inliers):
                    for i in range(N):
                        if bit(bits[it - 1], i):
                            inl[P.indices1[i]] = True
                    res = Call(True, it - 1, c, wrong == "nomore_on_return" and it >= max_its, inl, best_idx, best, it)
                    break
        if res is None:
            res = Call(False, -1, 0, it >= max_its, inl, best_idx, best, it)
        out.append(res)
    return out


def budget(P, wrong=None):
    """the iterations the solver can ever run: what ygz::Sim3Solver draws triples for"""
    return ransac_max_its(len(np.asarray(P.X1).reshape(-1, 3)), P.prob, P.min_inliers, P.max_its, wrong)


# ---- results -------------------------------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "hyps calls")
_RESULTS = {}


def run(P, mode="device", wrong=None):
    Hy = sim3_hypotheses(P, mode, wrong)
    return Result(Hy, sim3_iterate(Hy.count, Hy.bits, P, wrong))


def expected(case, mode="device", wrong=None):
    key = (case.name, mode, wrong)
    if key not in _RESULTS:
        P = case.problem
        if wrong == "sample_replace" and case.seeded:
            P = P._replace(samples=_seeded_samples(case.name, len(P.X1), len(P.samples), wrong))
        _RESULTS[key] = run(P, mode, wrong)
    return _RESULTS[key]


def same_calls(a, b):
    return len(a) == len(b) and all(x[:4] == y[:4] and np.array_equal(x.inliers12, y.inliers12) and x[5:] == y[5:] for x, y in zip(a, b))


def same_result(a, b):
    A, B = a.hyps, b.hyps
    return (A.hyp.shape == B.hyp.shape and np.array_equal(A.hyp, B.hyp, equal_nan=True) and np.array_equal(A.err1, B.err1, equal_nan=True) and
            np.array_equal(A.err2, B.err2, equal_nan=True) and np.array_equal(A.bits, B.bits) and np.array_equal(A.count, B.count) and same_calls(a.calls, b.calls))


def same_decisions(a, b):
    return np.array_equal(a.hyps.bits, b.hyps.bits) and np.array_equal(a.hyps.count, b.hyps.count) and same_calls(a.calls, b.calls)


# ---- scene builders ------------------------------------------------------------------------------------------------------------------------------
EUROC4 = (458.654, 457.296, 367.215, 248.375)
CAM_B = (435.2, 435.2, 367.4, 252.2)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)]).astype(f32)   # mvLevelSigma2 at scale factor 1.2


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _triangle_ok(X, tri, min_area=1.0):
    a, b, c = X[tri[0]].astype(f64), X[tri[1]].astype(f64), X[tri[2]].astype(f64)
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a)) >= min_area


def good_triples(X, members, count, rs):
    """`count` triples of distinct indices out of `members` whose triangle in X has at least a square unit of area: well conditioned samples"""
    out = []
    members = np.asarray(members)
    for _ in range(200 * count):
        tri = rs.choice(members, 3, replace=False)
        if _triangle_ok(X, tri):
            out.append(tri)
            if len(out) == count:
                return np.asarray(out, np.int32)
    raise AssertionError("no well conditioned triples")


def build(groups, n_junk, seed, octaves=(0, 4), shuffle=True):
    """correspondences in groups, each consistent with its own Sim3 (s, R, t): X1 = s R X2 + t rounded to float; junk correspondences pair
    unrelated points.  -> X1, X2, sigma2_1, sigma2_2, members (the index lists of the groups, then of the junk)"""
    rs = np.random.RandomState(seed)
    X1, X2, mem = [], [], []
    at = 0
    for cnt, (s, R, t) in groups:
        x2 = rs.uniform([-2.5, -1.8, 3.0], [2.5, 1.8, 9.0], (cnt, 3))
        X2.append(x2)
        X1.append(s * x2 @ np.asarray(R).T + np.asarray(t))
        mem.append(list(range(at, at + cnt)))
        at += cnt
    if n_junk:
        X2.append(rs.uniform([-2.5, -1.8, 3.0], [2.5, 1.8, 9.0], (n_junk, 3)))
        X1.append(rs.uniform([-2.5, -1.8, 3.0], [2.5, 1.8, 9.0], (n_junk, 3)))
        mem.append(list(range(at, at + n_junk)))
        at += n_junk
    X1, X2 = np.concatenate(X1).astype(f32), np.concatenate(X2).astype(f32)
    perm = rs.permutation(at) if shuffle else np.arange(at)
    where = np.argsort(perm)
    mem = [sorted(int(where[i]) for i in m) for m in mem]
    o1, o2 = rs.randint(octaves[0], octaves[1], at), rs.randint(octaves[0], octaves[1], at)
    return X1[perm], X2[perm], SIGMA2[o1], SIGMA2[o2], mem


def problem(X1, X2, s1, s2, samples, K1=EUROC4, K2=CAM_B, fix_scale=False, prob=0.99, min_inliers=20, max_its=None, calls=(5, 5, "find"), holes=2):
    """mvnIndices1: the correspondences sit in vpMatched12 with `holes` unmatched entries in front of each third one"""
    n = len(X1)
    samples = np.asarray(samples, np.int32).reshape(-1, 3)
    max_its = len(samples) if max_its is None else max_its   # (explicit triples: the solver's budget ends with them)
    idx, at = [], 0
    for i in range(n):
        at += holes if i % 3 == 0 else 0
        idx.append(at)
        at += 1
    return Problem(np.ascontiguousarray(X1, f32), np.ascontiguousarray(X2, f32), np.asarray(s1, f32), np.asarray(s2, f32), tuple(K1), tuple(K2), bool(fix_scale),
                   np.asarray(samples, np.int32).reshape(-1, 3), prob, min_inliers, max_its, tuple(calls), at + 1, tuple(idx))


TA = (1.0, rot([0.2, 1.0, 0.1], 0.35), [0.4, -0.1, 0.3])
TB = (1.0, rot([1.0, -0.3, 0.2], -0.6), [-1.2, 0.5, 0.8])
TS = (1.7, rot([0.1, 0.9, -0.3], 0.25), [0.3, 0.2, -0.4])


def _all_inliers(n, seed):
    X1, X2, s1, s2, mem = build([(n, TS)], 0, seed)
    rs = np.random.RandomState(seed + 1)
    tri = good_triples(X2, mem[0], 4, rs) if n > 3 else np.array([[0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]], np.int32)
    return problem(X1, X2, s1, s2, tri, min_inliers=min(20, n) - 1 if n > 3 else 2, calls=(5,))


def _two_groups(nA, nB, n_junk, order, seed, **kw):
    """order: a string over A, B, J (junk: a triple that mixes the groups)"""
    X1, X2, s1, s2, mem = build([(nA, TA), (nB, TB)], n_junk, seed)
    rs = np.random.RandomState(seed + 1)
    tri = []
    for ch in order:
        if ch == "A":
            tri.append(good_triples(X2, mem[0], 1, rs)[0])
        elif ch == "B":
            tri.append(good_triples(X2, mem[1], 1, rs)[0])
        else:
            a = good_triples(X2, mem[0], 1, rs)[0]
            b = good_triples(X2, mem[1], 1, rs)[0]
            j = good_triples(X2, mem[2], 1, rs)[0]
            tri.append(np.array([a[0], b[0], j[0]], np.int32))
    return problem(X1, X2, s1, s2, np.asarray(tri), **kw), mem


def _shift_px(P, i, px):
    """moves correspondence i of camera 1 sideways by px pixels of its own image"""
    X1 = P.X1.copy()
    X1[i, 0] = f32(float(X1[i, 0]) + px * float(X1[i, 2]) / P.K1[0])
    return P._replace(X1=X1)


def _gate13(px2, seed=41):
    """all correspondences exact but one, whose error in image 1 is about px2 square pixels at octave 1 (gate 13 truncated, 13.26 as a float); its
    gate in image 2 is octave 7's"""
    X1, X2, s1, s2, mem = build([(30, TA)], 0, seed)
    rs = np.random.RandomState(seed + 1)
    i = 7
    others = [m for m in mem[0] if m != i]
    tri = good_triples(X2, others, 3, rs)
    s1, s2 = s1.copy(), s2.copy()
    s1[i], s2[i] = SIGMA2[1], SIGMA2[7]
    P = problem(X1, X2, s1, s2, tri, K2=EUROC4, min_inliers=20, calls=(5,))
    return _shift_px(P, i, math.sqrt(px2))


def _gate_exact():
    """a half turn about z with dyadic coordinates: N is diagonal, the quaternion (0, 0, 0, 1), R = diag(-1, -1, 1) and s = 1 exactly, every
    projection exact; correspondence 3 is moved by exactly 3 px in image 1: err1 == 9 == its gate at octave 0 (the gate in image 2 is octave 1's)"""
    K = (512.0, 512.0, 320.0, 240.0)
    X2 = np.array([[3.0, 0.25, 4.0], [-3.0, 0.5, 4.0], [0.0, -0.75, 4.0], [1.0, 0.125, 4.0], [2.0, -0.25, 2.0], [-1.0, 0.25, 8.0]], f32)
    t = np.array([0.5, 0.25, 0.0])
    X1 = (X2.astype(f64) * np.array([-1.0, -1.0, 1.0]) + t).astype(f32)
    X1[3, 0] += f32(3.0 * 4.0 / 512.0)
    s1 = np.full(6, SIGMA2[0], f32)
    s2 = np.full(6, SIGMA2[1], f32)
    return problem(X1, X2, s1, s2, [[0, 1, 2]], K1=K, K2=K, min_inliers=4, calls=(5,))


def _degenerate(kind, seed=51):
    X1, X2, s1, s2, mem = build([(24, TA)], 0, seed, shuffle=False)
    X1, X2 = X1.copy(), X2.copy()
    if kind == "collinear":
        X2[1] = X2[0] * f32(0.5) + X2[2] * f32(0.5)
        X1[1] = X1[0] * f32(0.5) + X1[2] * f32(0.5)
        tri = [[0, 1, 2]]
    else:   # coincident: three correspondences of one and the same point pair
        X1[1], X1[2], X2[1], X2[2] = X1[0], X1[0], X2[0], X2[0]
        tri = [[0, 1, 2], [2, 1, 0]]
    return problem(X1, X2, s1, s2, tri, min_inliers=20, calls=(5,))


def _identity(seed=61):
    X1, X2, s1, s2, mem = build([(24, (1.0, np.eye(3), [0.0, 0.0, 0.0]))], 0, seed)
    rs = np.random.RandomState(seed + 1)
    return problem(X2.copy(), X2, s1, s2, good_triples(X2, mem[0], 2, rs), min_inliers=20, calls=(5,))


def _behind(seed=71):
    """correspondence 5 lies behind camera 2 (and, moved by TA, behind camera 1): the reference projects it like any other"""
    X1, X2, s1, s2, mem = build([(24, TA)], 0, seed, shuffle=False)
    X1, X2 = X1.copy(), X2.copy()
    X2[5] = np.array([0.7, -0.4, -5.0], f32)
    X1[5] = (TA[0] * TA[1] @ X2[5].astype(f64) + np.asarray(TA[2])).astype(f32)
    rs = np.random.RandomState(seed + 1)
    tri = good_triples(X2, [m for m in mem[0] if m != 5], 2, rs)
    return problem(X1, X2, s1, s2, tri, min_inliers=20, calls=(5,))


def _z_zero(seed=81):
    X1, X2, s1, s2, mem = build([(24, TA)], 0, seed, shuffle=False)
    X1, X2 = X1.copy(), X2.copy()
    X2[5, 2] = 0.0
    X1[5] = (TA[0] * TA[1] @ X2[5].astype(f64) + np.asarray(TA[2])).astype(f32)
    X1[9, 2] = 0.0
    rs = np.random.RandomState(seed + 1)
    tri = good_triples(X2, [m for m in mem[0] if m not in (5, 9)], 2, rs)
    return problem(X1, X2, s1, s2, tri, min_inliers=20, calls=(5,))


def _fix_scale(seed=91):
    X1, X2, s1, s2, mem = build([(24, TS)], 0, seed)
    rs = np.random.RandomState(seed + 1)
    return problem(X1, X2, s1, s2, good_triples(X2, mem[0], 3, rs), fix_scale=True, min_inliers=20, calls=(5,))


def _nonfinite(seed=101):
    """a NaN and an infinity in correspondences that no triple samples (plain outliers), then a triple that samples the infinity"""
    X1, X2, s1, s2, mem = build([(24, TA)], 0, seed, shuffle=False)
    X1, X2 = X1.copy(), X2.copy()
    X1[4, 1] = np.nan
    X2[11, 0] = np.inf
    rs = np.random.RandomState(seed + 1)
    tri = list(good_triples(X2, [m for m in mem[0] if m not in (4, 11)], 2, rs)) + [np.array([11, 0, 1], np.int32), np.array([4, 2, 3], np.int32)]
    return problem(X1, X2, s1, s2, np.asarray(tri), min_inliers=20, calls=(5,))


def _seeded_samples(name, n, count, wrong=None):
    seed = int.from_bytes(name.encode(), "little") % 2147483647
    return draw_triples(n, count, Lcg(seed).random_int, wrong)


def _seeded(name, n, frac_out, seed):
    n_out = int(round(frac_out * n))
    X1, X2, s1, s2, mem = build([(n - n_out, TS if seed % 2 else TA)], n_out, seed, octaves=(0, 8))
    return problem(X1, X2, s1, s2, _seeded_samples(name, n, 300), min_inliers=max(3, min(20, (n - n_out) // 2)), max_its=300, calls=(5, 5, 5, "find"))


# ---- reach predicates: (problem, result) -> bool -------------------------------------------------------------------------------------------------
def r_all_inliers(P, r):
    return len(r.hyps.count) > 0 and all(int(c) == len(P.X1) for c in r.hyps.count) and r.calls[0].returned and r.calls[0].n_inliers == len(P.X1)


def r_counts(*want):
    def reach(P, r):
        return [int(c) for c in r.hyps.count] == list(want)
    return reach


def r_calls(*want):
    """want: per call (returned, hyp_index, no_more)"""
    def reach(P, r):
        return [(c.returned, c.hyp_index, c.no_more) for c in r.calls] == list(want)
    return reach


def r_both(*fs):
    return lambda P, r: all(f(P, r) for f in fs)


def r_bit(i, want, h=0):
    return lambda P, r: bit(r.hyps.bits[h], i) == want


def r_nan_hyp(*hs):
    return lambda P, r: all(np.all(np.isnan(r.hyps.hyp[h, :9])) and int(r.hyps.count[h]) == 0 for h in hs)


def r_no_inliers(P, r):
    return all(int(c) == 0 for c in r.hyps.count)


def r_best(idx):
    return lambda P, r: r.calls[-1].best_index == idx


def r_scene(P, r):
    n = len(P.X1)
    return 20 <= n <= 500 and len(P.samples) == 300 and int(r.hyps.count.max()) > P.min_inliers and any(c.returned for c in r.calls)


def _specs():
    S = []
    for n in (3, 20, 63, 64, 65, 128, 129):
        S.append(("all_n%d" % n, (lambda n: lambda: _all_inliers(n, 1000 + n))(n), r_all_inliers))
    S.append(("gate13_inside", lambda: _gate13(12.0), r_both(r_bit(7, True), r_counts(30, 30, 30))))
    S.append(("gate13_between", lambda: _gate13(13.13), r_both(r_bit(7, False), r_counts(29, 29, 29))))
    S.append(("gate_exact", _gate_exact, r_both(r_bit(3, False), r_counts(5), lambda P, r: float(r.hyps.err1[0, 3]) == 9.0)))
    S.append(("count_min", lambda: _two_groups(20, 6, 4, "JA", 201, min_inliers=20, max_its=2, calls=(5, 5))[0], r_both(r_counts(0, 20), r_calls((False, -1, True), (False, -1, True)))))
    S.append(("count_min_plus1", lambda: _two_groups(21, 6, 4, "JA", 211, min_inliers=20, max_its=2, calls=(5, 5))[0], r_both(r_counts(0, 21), r_calls((True, 1, False), (False, -1, True)))))
    S.append(("tie", lambda: _two_groups(24, 24, 6, "ABJ", 221, min_inliers=30, max_its=3, calls=(5,))[0], r_both(r_counts(24, 24, 0), r_best(1), r_calls((False, -1, True)))))
    S.append(("return_then_beat", lambda: _two_groups(25, 22, 6, "JJABBBBBBB", 231, min_inliers=20, max_its=300, calls=(5, 5))[0],
              r_both(r_counts(0, 0, 25, 22, 22, 22, 22, 22, 22, 22), r_calls((True, 2, False), (False, -1, False)), r_best(2))))
    S.append(("return_then_beaten", lambda: _two_groups(22, 25, 6, "JAJBAAAAAAAA", 241, min_inliers=20, max_its=300, calls=(2, 5, 5))[0],
              r_both(r_counts(0, 22, 0, 25, 22, 22, 22, 22, 22, 22, 22, 22), r_calls((True, 1, False), (True, 3, False), (False, -1, False)))))
    S.append(("ends_on_max", lambda: _two_groups(12, 8, 6, "JABJABJ", 251, min_inliers=20, max_its=7, calls=(5, 5, 5))[0],
              r_both(r_calls((False, -1, False), (False, -1, True), (False, -1, True)), r_best(4))))
    S.append(("returns_on_max", lambda: _two_groups(25, 8, 6, "JJJJJJA", 261, min_inliers=20, max_its=7, calls=(5, 5, 5))[0],
              r_calls((False, -1, False), (True, 6, False), (False, -1, True))))
    S.append(("n_below_min", lambda: _two_groups(8, 4, 0, "AB", 271, min_inliers=20, calls=(5, "find"))[0], r_calls((False, -1, True), (False, -1, True))))
    S.append(("min_equals_n", lambda: _two_groups(12, 0, 0, "AAA", 281, min_inliers=12, max_its=300, calls=(5, 5))[0],
              r_both(lambda P, r: budget(P) == 1, r_calls((False, -1, True), (False, -1, True)), r_best(0))))
    # (three collinear points still fit themselves -- the rotation about their line is arbitrary --: a garbage hypothesis that explains its own sample only)
    S.append(("collinear", lambda: _degenerate("collinear"), r_both(r_counts(3), r_calls((False, -1, True)))))
    S.append(("coincident", lambda: _degenerate("coincident"), r_both(r_no_inliers, r_nan_hyp(0, 1))))
    S.append(("identity", _identity, r_both(r_nan_hyp(0, 1), r_calls((False, -1, True)))))
    S.append(("behind_camera2", _behind, r_both(r_bit(5, True), r_counts(24, 24), lambda P, r: P.X2[5, 2] < 0)))
    S.append(("z_zero", _z_zero, r_both(r_bit(5, False), r_bit(9, False), r_counts(22, 22))))
    S.append(("fix_scale_17", _fix_scale, lambda P, r: bool(np.all(r.hyps.hyp[:, 12] == 1)) and int(r.hyps.count.max()) < 20))
    S.append(("nonfinite", _nonfinite, r_both(r_counts(22, 22, 0, 0), r_nan_hyp(2, 3))))
    return S


_SCENES = [("scene0", 3, 7001), ("scene1", 5, 7101), ("scene2", 10, 7201), ("scene3", 4, 7301)]   # name, candidates, seed


def _scene_specs():
    S = []
    for name, cands, seed in _SCENES:
        rs = np.random.RandomState(seed)
        for k in range(cands):
            n = int(rs.randint(20, 501))
            frac = float(rs.uniform(0.10, 0.60))
            nm = "%s_c%d_n%d" % (name, k, n)
            S.append((nm, (lambda nm, n, frac, sd: lambda: _seeded(nm, n, frac, sd))(nm, n, frac, seed + 1 + k), r_scene))
    return S


SPECS = _specs()
SCENE_SPECS = _scene_specs()
NAMES = [s[0] for s in SPECS]
SCENE_NAMES = [s[0] for s in SCENE_SPECS]

# name -> the wrong forms that change the case's result (hyp, errors, bits, counts or any iterate call), as tests/test_sim3_cases.py finds them.
# t21_inverse moves every case with a finite hypothesis: the inverse of the rounded T12 differs from (1.0 / s) R' in the last bits of err2.
# niter_no_n_rule moves no case, and cannot: minInliers == N makes epsilon exactly 1, the formula log(1 - p) / log(0) = 0, ceil 0, and
# max(1, min(0, maxIterations)) is the 1 the rule sets.  The rule is kept in the restatement and the host code because the source has it.
MOVED_BY = {
    "all_n3": ("t21_inverse",),
    "all_n20": ("t21_inverse",),
    "all_n63": ("t21_inverse",),
    "all_n64": ("t21_inverse",),
    "all_n65": ("t21_inverse",),
    "all_n128": ("t21_inverse",),
    "all_n129": ("t21_inverse",),
    "gate13_inside": ("t21_inverse",),
    "gate13_between": ("float_gates", "t21_inverse",),
    "gate_exact": ("float_gates", "gate_le", "nomore_on_return",),
    "count_min": ("return_ge", "best_reset", "t21_inverse",),
    "count_min_plus1": ("best_reset", "t21_inverse", "nomore_on_return",),
    "tie": ("best_gt", "t21_inverse",),
    "return_then_beat": ("best_reset", "t21_inverse",),
    "return_then_beaten": ("best_reset", "t21_inverse",),
    "ends_on_max": ("best_gt", "best_reset", "t21_inverse",),
    "returns_on_max": ("best_gt", "best_reset", "t21_inverse", "nomore_on_return",),
    "n_below_min": ("t21_inverse",),
    "min_equals_n": ("return_ge", "best_reset", "t21_inverse",),
    "collinear": ("t21_inverse",),
    "coincident": ("best_gt", "identity_ok",),
    "identity": ("best_gt", "identity_ok",),
    "behind_camera2": ("depth_gate", "t21_inverse",),
    "z_zero": ("t21_inverse",),
    "fix_scale_17": ("best_gt", "scale_when_fixed", "t21_inverse",),
    "nonfinite": ("t21_inverse",),
    "scene0_c0_n412": ("best_gt", "t21_inverse", "sample_replace",),
    "scene0_c1_n172": ("float_gates", "best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene0_c2_n360": ("best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene1_c0_n158": ("best_gt", "t21_inverse", "sample_replace",),
    "scene1_c1_n420": ("float_gates", "best_gt", "t21_inverse", "sample_replace",),
    "scene1_c2_n474": ("best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene1_c3_n268": ("float_gates", "best_gt", "t21_inverse", "sample_replace",),
    "scene1_c4_n470": ("float_gates", "best_gt", "t21_inverse", "sample_replace",),
    "scene2_c0_n240": ("best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene2_c1_n169": ("best_gt", "t21_inverse", "sample_replace",),
    "scene2_c2_n56": ("best_gt", "t21_inverse", "sample_replace",),
    "scene2_c3_n49": ("best_gt", "t21_inverse", "sample_replace",),
    "scene2_c4_n159": ("float_gates", "best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene2_c5_n302": ("best_gt", "t21_inverse", "sample_replace",),
    "scene2_c6_n300": ("best_gt", "t21_inverse", "sample_replace",),
    "scene2_c7_n140": ("float_gates", "best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene2_c8_n103": ("float_gates", "best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene2_c9_n131": ("float_gates", "best_gt", "t21_inverse", "sample_replace",),
    "scene3_c0_n443": ("best_gt", "t21_inverse", "sample_replace",),
    "scene3_c1_n452": ("best_gt", "best_reset", "t21_inverse", "sample_replace",),
    "scene3_c2_n231": ("best_gt", "t21_inverse", "sample_replace",),
    "scene3_c3_n211": ("float_gates", "best_gt", "t21_inverse", "sample_replace",),
}

_CASES = []


def cases():
    if not _CASES:
        for name, mk, reach in SPECS:
            _CASES.append(Case(name, mk(), MOVED_BY.get(name, ()), reach, False))
        for name, mk, reach in SCENE_SPECS:
            _CASES.append(Case(name, mk(), MOVED_BY.get(name, ()), reach, True))
    return _CASES


def constructed():
    return [c for c in cases() if not c.seeded]


def scene(name):
    """the candidates of one seeded scene, as ComputeSim3 holds them"""
    return [c for c in cases() if c.seeded and c.name.startswith(name + "_")]


def case_by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- the cases as files, for the host programs (tests/cpp/sim3_host.cc, tests/cpp/sim3_shell.cc) ---------------------------------------------------
def write_case(P, path):
    """int32 n mN1 H fix minInliers maxIterations nCalls | double probability | float K1[4] K2[4] | int32 calls (-1 = find) | int32 indices1[n] |
    float X1[3n] X2[3n] maxErr1[n] maxErr2[n] | int32 samples[3H]"""
    with open(path, "wb") as f:
        np.array([len(P.X1), P.mN1, len(P.samples), int(P.fix_scale), P.min_inliers, P.max_its, len(P.calls)], np.int32).tofile(f)
        np.array([P.prob], f64).tofile(f)
        np.asarray(P.K1, f32).tofile(f)
        np.asarray(P.K2, f32).tofile(f)
        np.array([-1 if c == "find" else c for c in P.calls], np.int32).tofile(f)
        np.asarray(P.indices1, np.int32).tofile(f)
        for a in (P.X1, P.X2, gates(P.sigma2_1), gates(P.sigma2_2)):
            np.ascontiguousarray(a, f32).tofile(f)
        np.ascontiguousarray(P.samples, np.int32).tofile(f)


def read_result(P, path):
    """what the host programs write back: Hyps (errors and margin unset) and the calls"""
    n, H = len(P.X1), len(P.samples)
    words = (n + 63) // 64
    with open(path, "rb") as f:
        hyp = np.fromfile(f, f32, 13 * H).reshape(H, 13)
        count = np.fromfile(f, np.int32, H)
        bits = np.fromfile(f, np.uint64, H * words).reshape(H, words)
        calls = []
        for _ in P.calls:
            h, n_inl, no_more, best_idx, best, it = (int(v) for v in np.fromfile(f, np.int32, 6))
            inl = np.fromfile(f, np.uint8, P.mN1).astype(bool)
            calls.append(Call(h >= 0, h, n_inl, bool(no_more), inl, best_idx, best, it))
    return Result(Hyps(hyp, None, None, bits, count, None), calls)
