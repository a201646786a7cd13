"""PnPsolver (src/PnPsolver.cc, include/PnPsolver.h) restated in Python floats and numpy, independently of csrc/pnp_math.h: the RANSAC of
iterate / find / Refine / CheckInliers with its mixed widths, EPnP as the file writes it (stored pws / us / alphas / pcs arrays), and the four
OpenCV routines it calls as this project fixes them (include/ygzf.h: cvMulTransposed as ordered sums, cvSVD as OpenCV 2.4 / 3.x's one-sided
Jacobi with gamma = sqrt(p p + beta beta), cvSolve / cvInvert(CV_SVD) as that SVD and a thresholded back-substitution).  Every operation is a
correctly rounded + - * / or sqrt in the source's order, so the header on one host thread (tests/cpp/pnp_host.cc) and the kernels
(tests/test_gpu_pnp.py) are held to it bit for bit.

WRONG lists plausible misreadings; every constructed case names the ones that change what it returns, and tests/test_pnp_cases.py checks
that each wrong form moves exactly those cases and that every case reaches what it claims."""
import math
import struct
from collections import namedtuple

import numpy as np

NAN, INF = float("nan"), float("inf")
DBL_EPSILON, DBL_MIN = 2.220446049250313e-16, 2.2250738585072014e-308
SVD_MIN_SWEEPS, GN_STEPS, MAX_MIN_SET = 30, 5, 8
TH2 = np.float32(5.991)

WRONG = ("loop_and", "refine_current", "refine_gate_ge", "qualify_gt", "best_ge", "check_le", "check_float_ue", "check_all_double", "depth_gate",
         "draw_replace", "sign_mean_depth", "no_det_flip", "reperr_le", "inliers_sized_n")
_CHECK_FORMS = {"check_le", "check_float_ue", "check_all_double", "depth_gate"}
_TAIL_FORMS = {"sign_mean_depth", "no_det_flip", "reperr_le"}

Problem = namedtuple("Problem", "name P3D P2D max_err K min_set min_inliers max_its samples key_indices n_matches calls")
Hyps = namedtuple("Hyps", "hyp count bits refined_n refined_hyp refined_bits")
Call = namedtuple("Call", "kind index n_inliers no_more best_index best_inliers iterations T inliers")
EMPTY, REFINED, BEST = 0, 1, 2


# ---------------------------------------------------------------- scalar helpers ----------------------------------------------------------------

def div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def sqrt(x):
    return math.sqrt(x) if x >= 0 else NAN   # (a NaN fails the comparison)


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(p, q):
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2])


# ---------------------------------------------------------------- the fixed linear algebra ----------------------------------------------------------------

def mul_transposed(A):
    """cvMulTransposed(A, dst, 1): A' A, each entry of the upper triangle summed over the rows in order, mirrored"""
    n = len(A[0])
    out = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            s = 0.0
            for row in A:
                s += row[i] * row[j]
            out[i][j] = out[j][i] = s
    return out


def jacobi_svd(At, want_v=True):
    """At: n rows of m -> (At scaled: the rows are the left singular vectors, W descending, Vt)"""
    At = [list(r) for r in At]
    n, m = len(At), len(At[0])
    eps = DBL_EPSILON * 10
    Vt = [[1.0 if k == i else 0.0 for k in range(n)] for i in range(n)] if want_v else None
    W = []
    for row in At:
        sd = 0.0
        for t in row:
            sd += t * t
        W.append(sd)
    for _ in range(max(m, SVD_MIN_SWEEPS)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b, p = W[i], W[j], 0.0
                for k in range(m):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = sqrt(div(delta, gamma))
                    c = div(p, gamma * s * 2)
                else:
                    c = sqrt(div(gamma + beta, gamma * 2))
                    s = div(p, gamma * c * 2)
                a = b = 0.0
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = -s * Ai[k] + c * Aj[k]
                    Ai[k], Aj[k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                if Vt is not None:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = -s * Vi[k] + c * Vj[k]
                        Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i, row in enumerate(At):
        sd = 0.0
        for t in row:
            sd += t * t
        W[i] = sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if Vt is not None:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    for i in range(n):
        s = div(1.0, W[i]) if W[i] > DBL_MIN else 0.0   # (OpenCV refills such a row with a pseudo-random vector: fixed as zero here)
        At[i] = [t * s for t in At[i]]
    return At, W, Vt


def _threshold(W):
    t = 0.0
    for w in W:
        t += w
    return t * (DBL_EPSILON * 2)


def solve_svd(A, b):
    """cvSolve(A, b, x, CV_SVD), A m x n"""
    m, n = len(A), len(A[0])
    At, W, Vt = jacobi_svd([[A[r][c] for r in range(m)] for c in range(n)])
    x = [0.0] * n
    th = _threshold(W)
    for i in range(n):
        wi = W[i]
        if abs(wi) <= th:
            continue
        wi = div(1.0, wi)
        s = 0.0
        for j in range(m):
            s += At[i][j] * b[j]
        s *= wi
        for j in range(n):
            x[j] = x[j] + s * Vt[i][j]
    return x


def invert_svd(A):
    """cvInvert(A, inv, CV_SVD), A 3 x 3"""
    At, W, Vt = jacobi_svd([[A[r][c] for r in range(3)] for c in range(3)])
    x = [[0.0] * 3 for _ in range(3)]
    th = _threshold(W)
    for i in range(3):
        wi = W[i]
        if abs(wi) <= th:
            continue
        wi = div(1.0, wi)
        buf = [At[i][k] * wi for k in range(3)]
        for j in range(3):
            for k in range(3):
                x[j][k] = x[j][k] + Vt[i][j] * buf[k]
    return x


def qr_solve(A, b, x):
    """:805-894 on copies of the 6 x 4 A and b; writes x unless a column is singular -> True when solved"""
    nr, nc = len(A), len(A[0])
    A = [list(r) for r in A]
    b = list(b)
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k + 1, nr):
            elt = abs(A[i - 1][k])   # (the source advances its pointer after the comparison: rows k .. nr-2)
            if eta < elt:
                eta = elt
        if eta == 0:
            return False
        inv_eta = div(1.0, eta)
        s = 0.0
        for i in range(k, nr):
            A[i][k] *= inv_eta
            s += A[i][k] * A[i][k]
        sigma = sqrt(s)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] += sigma
        A1[k] = sigma * A[k][k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i][k] * A[i][j]
            tau = div(s, A1[k])
            for i in range(k, nr):
                A[i][j] -= tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i][j] * b[i]
        tau = div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i][j]
    x[nc - 1] = div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i][j] * x[j]
        x[i] = div(b[i] - s, A2[i])
    return True


# ---------------------------------------------------------------- EPnP ----------------------------------------------------------------

class Front:
    """compute_pose up to the three betas (what no wrong form touches), kept per (problem, subset)"""
    __slots__ = "pws us alphas cws ut l rho betas qr_singular mats".split()


def epnp_front(pws, us, K):
    fu, fv, uc, vc = K
    n = len(pws)
    F = Front()
    F.pws, F.us = pws, us
    # choose_control_points
    c0 = [0.0, 0.0, 0.0]
    for p in pws:
        for j in range(3):
            c0[j] += p[j]
    c0 = [div(c0[j], n) for j in range(3)]
    PW0 = [[p[j] - c0[j] for j in range(3)] for p in pws]
    F.mats = dict(pw0=PW0, pw0tpw0=mul_transposed(PW0))   # (what the OpenCV routines are given: tools/make_golden_pnp_opencv.py)
    uct, dc, _ = jacobi_svd(F.mats["pw0tpw0"])   # (symmetric: its transpose is itself)
    cws = [c0]
    for i in range(1, 4):
        k = sqrt(div(dc[i - 1], n))
        cws.append([c0[j] + k * uct[i - 1][j] for j in range(3)])
    F.cws = cws
    # compute_barycentric_coordinates
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = invert_svd(cc)
    F.mats["cc"] = cc
    alphas = []
    for p in pws:
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = ci[j][0] * (p[0] - cws[0][0]) + ci[j][1] * (p[1] - cws[0][1]) + ci[j][2] * (p[2] - cws[0][2])
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)
    F.alphas = alphas
    # fill_M, MtM, its SVD
    M = []
    for a, (u, v) in zip(alphas, us):
        r1, r2 = [], []
        for i in range(4):
            r1 += [a[i] * fu, 0.0, a[i] * (uc - u)]
            r2 += [0.0, a[i] * fv, a[i] * (vc - v)]
        M += [r1, r2]
    F.mats["M"], F.mats["mtm"] = M, mul_transposed(M)
    ut, _, _ = jacobi_svd(F.mats["mtm"], want_v=False)
    F.ut = ut
    # compute_L_6x10, compute_rho
    v = [ut[11], ut[10], ut[9], ut[8]]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[[v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)] for (a, b) in pairs] for i in range(4)]
    L = []
    for i in range(6):
        d = [dv[q][i] for q in range(4)]
        L.append([dot3(d[0], d[0]), 2.0 * dot3(d[0], d[1]), dot3(d[1], d[1]), 2.0 * dot3(d[0], d[2]), 2.0 * dot3(d[1], d[2]), dot3(d[2], d[2]),
                  2.0 * dot3(d[0], d[3]), 2.0 * dot3(d[1], d[3]), 2.0 * dot3(d[2], d[3]), dot3(d[3], d[3])])
    rho = [dist2(cws[a], cws[b]) for (a, b) in pairs]
    F.l, F.rho = L, rho
    F.mats["l"], F.mats["rho"] = L, rho
    F.betas, F.qr_singular = [], 0
    for cols in ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4)):
        b = solve_svd([[L[r][c] for c in cols] for r in range(6)], rho)
        be = [0.0] * 4
        if len(cols) == 4:
            if b[0] < 0:
                be[0] = sqrt(-b[0])
                be[1], be[2], be[3] = div(-b[1], be[0]), div(-b[2], be[0]), div(-b[3], be[0])
            else:
                be[0] = sqrt(b[0])
                be[1], be[2], be[3] = div(b[1], be[0]), div(b[2], be[0]), div(b[3], be[0])
        else:
            if b[0] < 0:
                be[0] = sqrt(-b[0])
                be[1] = sqrt(-b[2]) if b[2] < 0 else 0.0
            else:
                be[0] = sqrt(b[0])
                be[1] = sqrt(b[2]) if b[2] > 0 else 0.0
            if b[1] < 0:
                be[0] = -be[0]
            be[2] = div(b[3], be[0]) if len(cols) == 5 else 0.0
        # gauss_newton; the x the source never initialised is 0
        x = [0.0] * 4
        for _ in range(GN_STEPS):
            A, rhs = [], []
            for i in range(6):
                r = L[i]
                A.append([2 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3],
                          r[1] * be[0] + 2 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3],
                          r[3] * be[0] + r[4] * be[1] + 2 * r[5] * be[2] + r[8] * be[3],
                          r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2 * r[9] * be[3]])
                rhs.append(rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] +
                                     r[4] * be[1] * be[2] + r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] +
                                     r[8] * be[2] * be[3] + r[9] * be[3] * be[3]))
            if not qr_solve(A, rhs, x):
                F.qr_singular += 1
            for i in range(4):
                be[i] += x[i]
        F.betas.append(be)
    return F


def epnp_tail(F, K, wrong=frozenset()):
    """compute_R_and_t for the three betas and the choice -> (R 3 x 3, t, info)"""
    fu, fv, uc, vc = K
    n = len(F.pws)
    res, info = [], dict(sign_flip=[], det_flip=[], errs=[], abt=[])
    for be in F.betas:
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            v = F.ut[11 - i]
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += be[i] * v[3 * j + k]
        pcs = [[a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)] for a in F.alphas]
        if "sign_mean_depth" in wrong:
            z = 0.0
            for pc in pcs:
                z += pc[2]
            flip = z < 0.0
        else:
            flip = pcs[0][2] < 0.0
        info["sign_flip"].append(flip)
        if flip:
            ccs = [[-c for c in row] for row in ccs]
            pcs = [[-c for c in pc] for pc in pcs]
        # estimate_R_and_t
        pc0, pw0 = [0.0] * 3, [0.0] * 3
        for pc, pw in zip(pcs, F.pws):
            for j in range(3):
                pc0[j] += pc[j]
                pw0[j] += pw[j]
        pc0 = [div(c, n) for c in pc0]
        pw0 = [div(c, n) for c in pw0]
        abt = [[0.0] * 3 for _ in range(3)]
        for pc, pw in zip(pcs, F.pws):
            for j in range(3):
                abt[j][0] += (pc[j] - pc0[j]) * (pw[0] - pw0[0])
                abt[j][1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1])
                abt[j][2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2])
        info["abt"].append([list(r) for r in abt])
        At, _, Vt = jacobi_svd([[abt[r][c] for r in range(3)] for c in range(3)])
        U = [[At[k][i] for k in range(3)] for i in range(3)]
        V = [[Vt[k][j] for k in range(3)] for j in range(3)]
        R = [[dot3(U[i], V[j]) for j in range(3)] for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
               R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        info["det_flip"].append(det < 0)
        if det < 0 and "no_det_flip" not in wrong:
            R[2] = [-c for c in R[2]]
        t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
        sum2 = 0.0
        for pw, (u, v) in zip(F.pws, F.us):
            Xc = dot3(R[0], pw) + t[0]
            Yc = dot3(R[1], pw) + t[1]
            inv_Zc = div(1.0, dot3(R[2], pw) + t[2])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
        err = div(sum2, n)
        info["errs"].append(err)
        res.append((R, t))
    e = info["errs"]
    if "reperr_le" in wrong:
        N = 1 if e[1] <= e[0] else 0
        N = 2 if e[2] <= e[N] else N
    else:
        N = 1 if e[1] < e[0] else 0
        N = 2 if e[2] < e[N] else N
    info["winner"] = N + 1
    info["qr_singular"] = F.qr_singular
    return res[N][0], res[N][1], info


_FRONTS, _POSES = {}, {}


def compute_pose(P, subset, wrong=frozenset()):
    """compute_pose over the correspondences `subset` (a tuple of indices in add_correspondence order) -> (hyp12 float64, info)"""
    tail = frozenset(wrong) & _TAIL_FORMS
    key = (P.name, subset, tail)
    if key not in _POSES:
        fk = (P.name, subset)
        if fk not in _FRONTS:
            pws = [[float(P.P3D[i, 0]), float(P.P3D[i, 1]), float(P.P3D[i, 2])] for i in subset]
            us = [(float(P.P2D[i, 0]), float(P.P2D[i, 1])) for i in subset]
            _FRONTS[fk] = epnp_front(pws, us, [float(k) for k in P.K])
        R, t, info = epnp_tail(_FRONTS[fk], [float(k) for k in P.K], tail)
        _POSES[key] = (np.array([c for row in R for c in row] + list(t), np.float64), info)
    return _POSES[key]


def matrices(P, subset):
    """what compute_pose hands to cvMulTransposed / cvSVD / cvInvert / cvSolve for the correspondences `subset`, as float64 arrays"""
    _, info = compute_pose(P, subset)
    m = dict(_FRONTS[(P.name, subset)].mats)
    m["abt"] = info["abt"]
    return {k: np.array(v, np.float64) for k, v in m.items()}


def check_inliers(P, hyp12, wrong=frozenset(), errors=False):
    """CheckInliers: double products rounded to float Xc, Yc, invZc; ue, ve doubles; distX, distY, error2 floats; strict gate, no depth gate"""
    R, t = hyp12[:9], hyp12[9:]
    fu, fv, uc, vc = (np.float64(k) for k in P.K)
    X, Y, Z = (P.P3D[:, k].astype(np.float64) for k in range(3))
    u, v = P.P2D[:, 0], P.P2D[:, 1]
    with np.errstate(all="ignore"):
        xd = R[0] * X + R[1] * Y + R[2] * Z + t[0]
        yd = R[3] * X + R[4] * Y + R[5] * Z + t[1]
        zd = R[6] * X + R[7] * Y + R[8] * Z + t[2]
        if "check_all_double" in wrong:
            ue, ve = uc + fu * xd * (1 / zd), vc + fv * yd * (1 / zd)
            dx, dy = u.astype(np.float64) - ue, v.astype(np.float64) - ve
            e2 = dx * dx + dy * dy
        else:
            Xc, Yc, invZc = xd.astype(np.float32), yd.astype(np.float32), (1 / zd).astype(np.float32)
            if "check_float_ue" in wrong:
                ue = (uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)).astype(np.float32)
                ve = (vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)).astype(np.float32)
                dx, dy = u - ue, v - ve
            else:
                ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
                ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
                dx, dy = (u.astype(np.float64) - ue).astype(np.float32), (v.astype(np.float64) - ve).astype(np.float32)
            e2 = dx * dx + dy * dy
        ok = (e2 <= P.max_err) if "check_le" in wrong else (e2 < P.max_err)
        if "depth_gate" in wrong:
            ok &= zd > 0
    return (ok, e2, zd) if errors else ok


def pack_bits(ok):
    n = len(ok)
    words = (n + 63) // 64
    b = np.zeros(words * 64, np.uint8)
    b[:n] = ok
    return np.packbits(b.reshape(words, 64), axis=1, bitorder="little").view("<u8").reshape(words).astype(np.uint64)


def hypothesis(P, h, wrong=frozenset()):
    hyp, _ = compute_pose(P, tuple(int(i) for i in P.samples[h]), wrong)
    return hyp, check_inliers(P, hyp, wrong)


def refine_of(P, ok, wrong=frozenset()):
    """Refine on the inlier set `ok` -> (hyp12, inliers)"""
    hyp, _ = compute_pose(P, tuple(int(i) for i in np.nonzero(ok)[0]), wrong)
    return hyp, check_inliers(P, hyp, wrong)


def pnp_hypotheses(P, count=None, wrong=frozenset()):
    """what ygzf_pnp_ransac leaves for the first `count` sample sets (default: the budget, min(len(samples), max_its))"""
    H = min(len(P.samples), P.max_its) if count is None else count
    n = len(P.P3D)
    words = (n + 63) // 64
    out = Hyps(np.zeros((H, 12)), np.zeros(H, np.int32), np.zeros((H, words), np.uint64), np.full(H, -1, np.int32), np.zeros((H, 12)),
               np.zeros((H, words), np.uint64))
    best = -1
    for h in range(H):
        hyp, ok = hypothesis(P, h, wrong)
        out.hyp[h], out.count[h], out.bits[h] = hyp, int(ok.sum()), pack_bits(ok)
        if out.count[h] >= P.min_inliers and out.count[h] > best:   # a record
            rh, rok = refine_of(P, ok, wrong)
            out.refined_n[h], out.refined_hyp[h], out.refined_bits[h] = int(rok.sum()), rh, pack_bits(rok)
        best = max(best, int(out.count[h]))
    return out


def pnp_refine(P, h, wrong=frozenset()):
    """Refine on hypothesis h's own mask -> (count, hyp12, bits)"""
    _, ok = hypothesis(P, h, wrong)
    rh, rok = refine_of(P, ok, wrong)
    return int(rok.sum()), rh, pack_bits(rok)


def pose_to_float(hyp12):
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        T[:3, :3] = hyp12[:9].reshape(3, 3).astype(np.float32)
        T[:3, 3] = hyp12[9:].astype(np.float32)
    return T


def pnp_iterate(P, wrong=frozenset()):
    """every call of P.calls (an iteration count, -1 for find) on one solver -> [Call]; iteration h + 1 uses P.samples[h]"""
    wrong = frozenset(wrong)
    N = len(P.P3D)
    iterations, best_inliers, best_index = 0, 0, -1
    best_ok, best_T = None, np.zeros((4, 4), np.float32)
    calls = []
    size = N if "inliers_sized_n" in wrong else P.n_matches

    def mark(ok):
        vb = np.zeros(size, np.uint8)
        idx = np.asarray(P.key_indices)[np.nonzero(ok)[0]]
        vb[idx[idx < size]] = 1
        return vb

    for nit in P.calls:
        nit = P.max_its if nit < 0 else nit
        if N < P.min_inliers:
            calls.append(Call(EMPTY, -1, 0, 1, best_index, best_inliers, iterations, np.zeros((4, 4), np.float32), np.zeros(0, np.uint8)))
            continue
        cur, ret = 0, None
        while (iterations < P.max_its and cur < nit) if "loop_and" in wrong else (iterations < P.max_its or cur < nit):
            cur += 1
            iterations += 1
            h = iterations - 1
            hyp, ok = hypothesis(P, h, wrong)
            cnt = int(ok.sum())
            if (cnt > P.min_inliers) if "qualify_gt" in wrong else (cnt >= P.min_inliers):
                if (cnt >= best_inliers) if "best_ge" in wrong else (cnt > best_inliers):
                    best_ok, best_inliers, best_index, best_T = ok, cnt, h, pose_to_float(hyp)
                rh, rok = refine_of(P, ok if "refine_current" in wrong else best_ok, wrong)
                rn = int(rok.sum())
                if (rn >= P.min_inliers) if "refine_gate_ge" in wrong else (rn > P.min_inliers):
                    ret = Call(REFINED, h if "refine_current" in wrong else best_index, rn, 0, best_index, best_inliers, iterations, pose_to_float(rh), mark(rok))
                    break
        if ret is None:
            if iterations >= P.max_its:
                if best_inliers >= P.min_inliers:
                    ret = Call(BEST, best_index, best_inliers, 1, best_index, best_inliers, iterations, best_T.copy(), mark(best_ok))
                else:
                    ret = Call(EMPTY, -1, 0, 1, best_index, best_inliers, iterations, np.zeros((4, 4), np.float32), np.zeros(0, np.uint8))
            else:
                ret = Call(EMPTY, -1, 0, 0, best_index, best_inliers, iterations, np.zeros((4, 4), np.float32), np.zeros(0, np.uint8))
        calls.append(ret)
    return calls


def iterations_reached(P):
    """how many sample sets the calls of P consume"""
    calls = pnp_iterate(P)
    return max([c.iterations for c in calls] + [0])


def same_calls(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if (x.kind, x.index, x.n_inliers, x.no_more, x.best_index, x.best_inliers, x.iterations) != (y.kind, y.index, y.n_inliers, y.no_more, y.best_index, y.best_inliers, y.iterations):
            return False
        if x.kind != EMPTY and (x.T.view(np.uint32) != y.T.view(np.uint32)).any() and not (np.isnan(x.T) == np.isnan(y.T)).all():
            return False
        if x.kind != EMPTY:
            nan = np.isnan(x.T)
            if not np.array_equal(nan, np.isnan(y.T)) or not np.array_equal(x.T.view(np.uint32)[~nan], y.T.view(np.uint32)[~nan]):
                return False
        if len(x.inliers) != len(y.inliers) or not np.array_equal(x.inliers, y.inliers):
            return False
    return True


# ---------------------------------------------------------------- the draws, SetRansacParameters ----------------------------------------------------------------

class Lcg:
    """a scripted rand(): RAND_MAX = 2^31 - 1; random_int is DUtils::Random::RandomInt on it"""
    def __init__(self, seed):
        self.state = seed & 0x7FFFFFFF

    def random_int(self, lo, hi):
        self.state = (self.state * 1103515245 + 12345) & 0x7FFFFFFF
        d = hi - lo + 1
        return int((self.state / (2147483647.0 + 1.0)) * d) + lo


def draw_quads(n, min_set, count, random_int, wrong=frozenset()):
    """the sample sets of `count` iterations in the reference's draw order: each draw swapped with the back of the available list and popped"""
    out = []
    if n < min_set:
        return np.zeros((0, min_set), np.int32)
    for _ in range(count):
        avail = list(range(n))
        s = []
        for _ in range(min_set):
            r = random_int(0, len(avail) - 1)
            s.append(avail[r])
            if "draw_replace" not in wrong:
                avail[r] = avail[-1]
                avail.pop()
        out.append(s)
    return np.array(out, np.int32).reshape(-1, min_set)


def ransac_parameters(N, probability, min_inliers, max_iterations, min_set, epsilon):
    """SetRansacParameters (:111-143) -> (mRansacMinInliers, mRansacMaxIts)"""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)
    n_min = max(n_min, min_inliers, min_set)
    with np.errstate(all="ignore"):
        q = np.float32(n_min) / np.float32(N) if N else np.float32(INF)
    if eps < q:
        eps = q
    if n_min == N:
        nit = 1.0
    else:
        try:
            nit = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
        except (ValueError, ZeroDivisionError, OverflowError):
            nit = NAN
    if nit != nit or nit > max_iterations:
        nit = max_iterations
    return n_min, int(max(1, nit))


PARAMETER_TABLE = [(N, p, mi, mx, ms, e) for N in (0, 3, 4, 10, 11, 20, 50, 150, 500, 2000) for (p, mi, mx, ms, e) in
                   ((0.99, 10, 300, 4, 0.5), (0.99, 4, 300, 4, 0.3), (0.999, 10, 50, 5, 0.1), (0.5, 1, 300, 4, 0.9))]


# ---------------------------------------------------------------- cases ----------------------------------------------------------------

Case = namedtuple("Case", "name problem moved_by reach")
K_EUROC = (458.654, 457.296, 367.215, 248.375)


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _project(R, t, X, K):
    Xc = X @ R.T + t
    return np.stack([K[2] + K[0] * Xc[:, 0] / Xc[:, 2], K[3] + K[1] * Xc[:, 1] / Xc[:, 2]], axis=1)


def _scene(rng, n, n_out, pose=None, noise=0.3):
    """n correspondences of one camera pose, the last n_out of them with random image points"""
    R, t = pose if pose is not None else (_rot(*rng.uniform(-0.3, 0.3, 3)), rng.uniform(-0.5, 0.5, 3))
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], axis=1)
    X = _f32((Xc - t) @ R)   # world = R' (Xc - t)
    uv = _project(R, t, X.astype(np.float64), K_EUROC) + rng.normal(0, noise, (n, 2))
    if n_out:
        uv[n - n_out:] = np.stack([rng.uniform(0, 752, n_out), rng.uniform(0, 480, n_out)], axis=1)
    return X, _f32(uv), (R, t)


def _gates(rng, n):
    sigma2 = _f32(1.2 ** (2 * rng.integers(0, 4, n)))
    return sigma2 * TH2   # mvMaxError: the float product


def _problem(name, X, uv, max_err, samples, min_inliers, max_its, calls, min_set=4, gaps=3):
    n = len(X)
    key = np.arange(n) + np.minimum(np.arange(n), gaps) if n else np.zeros(0, np.int64)   # a few matches without MapPoint before the kept ones
    return Problem(name, _f32(X), _f32(uv), _f32(max_err), tuple(np.float64(np.float32(k)) for k in K_EUROC), min_set, min_inliers, max_its,
                   np.ascontiguousarray(samples, np.int32).reshape(-1, min_set), key.astype(np.int64), int(n + gaps + 2), tuple(calls))


def _sets_from(rng, pool, count, min_set=4):
    return np.array([rng.choice(pool, min_set, replace=False) for _ in range(count)], np.int32)


def _rows(max_its, calls):
    """sample sets enough for every iteration the calls can reach, the `||` overrun included"""
    return max_its + sum(c if c >= 0 else max_its for c in calls)


def _info(P, h):
    return compute_pose(P, tuple(int(i) for i in P.samples[h]))[1]


def _build():
    cases = []

    def add(P, moved_by, reach):
        cases.append(Case(P.name, P, frozenset(moved_by or ()), reach))

    # every correspondence an inlier, sizes around the 64-lane word
    for n in (4, 5, 63, 64, 65, 129):
        rng = np.random.default_rng(100 + n)
        X, uv, _ = _scene(rng, n, 0, noise=0.05)
        P = _problem("all_n%d" % n, X, uv, _gates(rng, n), _sets_from(rng, n, _rows(6, (5, 5, -1))), 4, 6, (5, 5, -1))
        add(P, (), lambda P=P: pnp_hypotheses(P).count.max() >= min(len(P.P3D), 4))
    return cases


# ---------------------------------------------------------------- the host program's files ----------------------------------------------------------------

Result = namedtuple("Result", "hyps calls")


def write_case(P, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", len(P.P3D), P.n_matches, len(P.samples), P.min_set, P.min_inliers, P.max_its, len(P.calls)))
        f.write(np.array(P.K, "<f8").tobytes())
        f.write(np.array(P.calls, "<i4").tobytes())
        f.write(np.asarray(P.key_indices).astype("<i4").tobytes())
        for a in (P.P3D, P.P2D, P.max_err):
            f.write(np.ascontiguousarray(a, "<f4").tobytes())
        f.write(np.ascontiguousarray(P.samples, "<i4").tobytes())


def read_result(P, path):
    buf = open(path, "rb").read()
    n = len(P.P3D)
    words = (n + 63) // 64
    pos = [0]

    def take(dtype, count):
        a = np.frombuffer(buf, dtype, count, pos[0]).copy()
        pos[0] += a.nbytes
        return a
    H = int(take("<i4", 1)[0])
    hyp, count, bits = take("<f8", 12 * H).reshape(H, 12), take("<i4", H), take("<u8", H * words).reshape(H, words)
    rn, rh, rb = take("<i4", H), take("<f8", 12 * H).reshape(H, 12), take("<u8", H * words).reshape(H, words)
    calls = []
    for _ in P.calls:
        v = take("<i4", 8)
        T = take("<f4", 16).reshape(4, 4)
        calls.append(Call(int(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4]), int(v[5]), int(v[6]), T, take("u1", int(v[7]))))
    assert pos[0] == len(buf)
    return Result(Hyps(hyp, count, bits, rn, rh, rb), calls)


_EXPECTED = {}


def expected(c):
    """the calls of the case, and what is known of its hypotheses afterwards: the budget, and the iterations the calls reached beyond it"""
    if c.name not in _EXPECTED:
        P = c.problem
        calls = pnp_iterate(P)
        budget = min(len(P.samples), P.max_its) if len(P.P3D) >= P.min_set else 0
        H = max([budget] + [k.iterations for k in calls]) if len(P.P3D) >= P.min_inliers else budget
        _EXPECTED[c.name] = Result(pnp_hypotheses(P, H), calls)
    return _EXPECTED[c.name]


def same_hyps(a, b):
    for x, y in ((a.hyp, b.hyp), (a.refined_hyp, b.refined_hyp)):
        nan = np.isnan(x)
        if x.shape != y.shape or not np.array_equal(nan, np.isnan(y)) or not np.array_equal(x.view(np.uint64)[~nan], y.view(np.uint64)[~nan]):
            return False
    return (np.array_equal(a.count, b.count) and np.array_equal(a.bits, b.bits) and np.array_equal(a.refined_n, b.refined_n) and
            np.array_equal(a.refined_bits, b.refined_bits))


def _errors(P, h):
    """(inlier, error2, Zc) of every correspondence under hypothesis h"""
    return check_inliers(P, hypothesis(P, h)[0], errors=True)


def _infos(P, count=None):
    return [_info(P, h) for h in range(min(len(P.samples), P.max_its) if count is None else count)]


def _mixed(rng, n, n_out, good, total, max_its, calls, name, min_inliers, noise=0.05, min_set=4, bad_first=0):
    """n correspondences, the last n_out outliers; `good` sample sets from the inliers at rows bad_first .., every other row holds two outliers"""
    X, uv, pose = _scene(rng, n, n_out, noise=noise)
    rows = _rows(max_its, calls) if total is None else total
    inl, out = np.arange(n - n_out), np.arange(n - n_out, n)
    sets = []
    for r in range(rows):
        if bad_first <= r < bad_first + good or n_out < 2:
            sets.append(rng.choice(inl, min_set, replace=False))
        else:
            sets.append(np.concatenate([rng.choice(inl, min_set - 2, replace=False), rng.choice(out, 2, replace=False)]))
    return _problem(name, X, uv, _gates(rng, n), np.array(sets), min_inliers, max_its, calls, min_set=min_set), pose


def _build_more():
    cases = []

    def add(P, moved_by, reach):
        cases.append(Case(P.name, P, frozenset(moved_by or ()), reach))

    # an error exactly on the gate, and one float either side: correspondences 15 .. 19 are in no sample set; the gate of one of them is set
    # from its own error under hypothesis 0.  gate_all_double / gate_float_ue: the gate stands between the error and what the all-double
    # and the float-ue misreadings of CheckInliers make of it.
    rng = np.random.default_rng(7)
    X, uv, _ = _scene(rng, 20, 0, noise=0.3)
    base = _problem("gate", X, uv, _gates(rng, 20), _sets_from(rng, 15, _rows(4, (5, -1))), 10, 4, (5, -1))
    h0 = hypothesis(base, 0)[0]
    e2 = check_inliers(base, h0, errors=True)[1]
    e2d = check_inliers(base, h0, frozenset(["check_all_double"]), errors=True)[1]
    e2f = check_inliers(base, h0, frozenset(["check_float_ue"]), errors=True)[1]

    def gate_case(name, j, g, moved, want):
        me = base.max_err.copy()
        me[j] = g
        P = base._replace(name=name, max_err=me)
        add(P, moved, lambda: _errors(P, 0)[1][j] == e2[j] and bool(_errors(P, 0)[0][j]) == want)
    gate_case("gate_on", 19, e2[19], ("check_le",), False)
    gate_case("gate_above", 19, np.nextafter(e2[19], np.float32(INF)), (), True)
    gate_case("gate_below", 19, np.nextafter(e2[19], np.float32(0)), (), False)
    j = next(k for k in range(15, 20) if e2d[k] < np.float64(e2[k]))       # the double error is below its float rounding: the gate at the float
    gate_case("gate_all_double", j, e2[j], ("check_all_double", "check_le"), False)
    j = next(k for k in range(15, 20) if e2f[k] != e2[k])
    gate_case("gate_float_ue", j, max(e2f[j], e2[j]), ("check_float_ue",), bool(e2[j] < e2f[j]))

    # a point behind the camera whose image point is where the formula puts it: an inlier, there is no depth gate
    rng = np.random.default_rng(8)
    X, uv, (R, t) = _scene(rng, 20, 0, noise=0.05)
    X[19] = _f32((np.array([0.3, -0.2, -5.0]) - t) @ R)
    uv[19] = _f32(_project(R, t, X[19:20].astype(np.float64), K_EUROC)[0])
    P = _problem("behind_camera", X, uv, _gates(rng, 20), _sets_from(rng, 19, _rows(4, (5, -1))), 10, 4, (5, -1))
    add(P, ("depth_gate", "inliers_sized_n"), lambda P=P: any(_errors(P, h)[0][19] and _errors(P, h)[2][19] < 0 for h in range(6)))

    # Zc == 0 exactly under hypothesis 0: X and Y of correspondence 19 take up what Z leaves of R2 . X + t2, so invZc is infinite
    rng = np.random.default_rng(9)
    X, uv, _ = _scene(rng, 20, 0, noise=0.05)
    base = _problem("zc_zero", X, uv, _gates(rng, 20), _sets_from(rng, 19, _rows(4, (5, -1))), 10, 4, (5, -1))
    h0 = hypothesis(base, 0)[0]
    r6, r7, r8, t2 = (float(v) for v in (h0[6], h0[7], h0[8], h0[11]))
    z = float(np.float32(-t2 / r8))
    y = float(np.float32((-t2 - r8 * z) / r7))
    x = float(np.float32((-t2 - r8 * z - r7 * y) / r6))
    X = X.copy()
    X[19] = (x, y, z)
    P = base._replace(P3D=X)
    add(P, ("inliers_sized_n",), lambda P=P: _errors(P, 0)[2][19] == 0 and not _errors(P, 0)[0][19])

    # two consensus groups, in both orders: 12 correspondences of one pose, 20 of another, 4 of neither
    rng = np.random.default_rng(10)
    XA, uvA, _ = _scene(rng, 12, 0, noise=0.05)
    XB, uvB, _ = _scene(rng, 24, 4, noise=0.05)
    X, uv, me = np.concatenate([XA, XB]), np.concatenate([uvA, uvB]), _gates(rng, 36)
    A = [rng.choice(np.arange(12), 4, replace=False) for _ in range(3)]
    B = [rng.choice(np.arange(12, 32), 4, replace=False) for _ in range(3)]
    bad = [np.array([0, 1, 33, 34]), np.array([13, 14, 34, 35])]
    fill = [bad[k % 2] for k in range(16)]
    P = _problem("groups_a_then_b", X, uv, me, np.array([A[0], bad[0], A[1], B[0], A[2], B[1]] + fill), 8, 6, (1, 1, 1, 1, 1, -1))
    add(P, ("refine_current", "loop_and"), lambda P=P: sorted(set(int(c.best_index) for c in pnp_iterate(P))) == [0, 3])
    P = _problem("groups_b_then_a", X, uv, me, np.array([B[0], bad[0], A[0], B[1], A[1], bad[1]] + fill), 8, 6, (1, 1, 1, 1, 1, -1))
    add(P, ("refine_current",), lambda P=P: [c.best_index for c in pnp_iterate(P)] == [0] * 6 and pnp_hypotheses(P).count[2] >= 8)

    # Refine fails with exactly min_inliers inliers and succeeds with one more
    for name, mi in (("refine_exact_min", 10), ("refine_one_more", 9)):
        rng = np.random.default_rng(11)
        P, _ = _mixed(rng, 16, 6, 3, None, 5, (5, -1), name, mi, bad_first=1)
        add(P, ("refine_gate_ge", "qualify_gt", "best_ge") if mi == 10 else (), lambda P=P, mi=mi: pnp_hypotheses(P).refined_n.max() == 10 and pnp_hypotheses(P).count.max() == 10 and
            (pnp_iterate(P)[0].kind == (BEST if mi == 10 else REFINED)))

    # a success followed by further calls; a call that starts near the end of the budget and runs past it
    rng = np.random.default_rng(12)
    P, _ = _mixed(rng, 30, 9, 6, None, 8, (5, 5, 5, -1), "success_then_calls", 10, bad_first=2)
    add(P, None, lambda P=P: [c.kind for c in pnp_iterate(P)][:2] == [REFINED, REFINED])
    rng = np.random.default_rng(13)
    P, _ = _mixed(rng, 30, 12, 1, None, 8, (5, 5), "overrun", 10, bad_first=5)
    add(P, ("loop_and",), lambda P=P: [c.iterations for c in pnp_iterate(P)] == [6, 11] and P.max_its == 8)

    # N < min_inliers; min_inliers == N (one iteration of budget)
    rng = np.random.default_rng(14)
    X, uv, _ = _scene(rng, 6, 0)
    P = _problem("n_below_min", X, uv, _gates(rng, 6), _sets_from(rng, 6, 4), 10, 4, (5, -1))
    add(P, None, lambda P=P: all(c.no_more and c.kind == EMPTY and c.iterations == 0 for c in pnp_iterate(P)))
    rng = np.random.default_rng(15)
    X, uv, _ = _scene(rng, 8, 0, noise=0.02)
    P = _problem("min_inliers_eq_n", X, uv, _gates(rng, 8), _sets_from(rng, 8, _rows(1, (5, 1))), 8, ransac_parameters(8, 0.99, 8, 300, 4, 0.5)[1], (5, 1))
    add(P, ("loop_and",), lambda P=P: P.max_its == 1 and pnp_iterate(P)[0].iterations == 5)

    # degenerate sample sets: coplanar, collinear, a repeated 3D point, four times the same point
    rng = np.random.default_rng(16)
    X, uv, (R, t) = _scene(rng, 16, 0, noise=0.05)
    Xc = X.astype(np.float64) @ R.T + t
    Xc[:4, 2] = 5.0                                                   # coplanar in the camera frame
    Xc[4:8] = Xc[4] + np.outer(np.arange(4), [0.4, 0.25, 0.3])        # collinear
    Xc[9] = Xc[8]                                                     # repeated
    X = _f32((Xc - t) @ R)
    X[9] = X[8]
    uv = _f32(_project(R, t, X.astype(np.float64), K_EUROC))
    uv[9] = uv[8]
    sets = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]] + [[12, 13, 14, 15]] * 8)
    P = _problem("degenerate_sets", X, uv, _gates(rng, 16), sets, 8, 4, (5, -1))
    add(P, None, lambda P=P: len(pnp_hypotheses(P).count) == 4)
    X2, uv2 = X.copy(), uv.copy()
    X2[1:4], uv2[1:4] = X2[0], uv2[0]
    P = _problem("same_point_four_times", X2, uv2, _gates(rng, 16), sets, 8, 4, (5, -1))
    add(P, None, lambda P=P: _info(P, 0)["qr_singular"] > 0)

    # every beta approximation wins somewhere; both sign decisions and the det < 0 flip are taken somewhere
    rng = np.random.default_rng(17)
    P, _ = _mixed(rng, 40, 14, 8, 24, 24, (-1,), "winners_and_flips", 12, noise=0.4)
    add(P, ("sign_mean_depth", "no_det_flip"), lambda P=P: {i["winner"] for i in _infos(P)} == {1, 2, 3} and any(any(i["sign_flip"]) for i in _infos(P)) and
        any(not all(i["sign_flip"]) for i in _infos(P)) and any(any(i["det_flip"]) for i in _infos(P)))

    # non-finite input: a NaN in a correspondence no set samples, an infinity in one that the second set samples
    rng = np.random.default_rng(18)
    X, uv, _ = _scene(rng, 20, 0, noise=0.05)
    X[19, 1] = NAN
    X[18, 0] = INF
    uv[17, 0] = NAN
    sets = np.concatenate([_sets_from(rng, 17, 1), [[0, 1, 2, 18]], [[3, 4, 5, 17]], _sets_from(rng, 17, _rows(4, (5, -1)))])
    P = _problem("nonfinite", X, uv, _gates(rng, 20), sets, 10, 4, (5, -1))
    add(P, None, lambda P=P: np.isnan(pnp_hypotheses(P).hyp[1]).any() and pnp_hypotheses(P).count[1] == 0 and pnp_hypotheses(P).count[0] == 17)

    # min_set 5
    rng = np.random.default_rng(19)
    P, _ = _mixed(rng, 24, 6, 4, None, 6, (5, -1), "min_set5", 10, min_set=5, bad_first=1)
    add(P, None, lambda P=P: P.samples.shape[1] == 5 and pnp_iterate(P)[0].kind == REFINED)

    # Refine sets of 11, 64 and 65 inliers
    for k, n in ((11, 20), (64, 80), (65, 129)):
        rng = np.random.default_rng(200 + k)
        P, _ = _mixed(rng, n, n - k, 2, None, 4, (5, -1), "refine_%d" % k, 10, noise=0.02, bad_first=1)
        add(P, None, lambda P=P, k=k: k in [int(c) for c, r in zip(pnp_hypotheses(P).count, pnp_hypotheses(P).refined_n) if r >= 0])
    return cases


# seeded candidates of a relocalisation: n correspondences, a share of outliers, sets drawn as the solver draws them
SCENE_NAMES = ["scene_n60", "scene_n100", "scene_n150"]


def scene(name):
    n = int(name.split("_n")[1])
    rng = np.random.default_rng(300 + n)
    n_out = int(n * {60: 0.3, 100: 0.4, 150: 0.5}[n])
    X, uv, _ = _scene(rng, n, n_out, noise=0.5)
    perm = rng.permutation(n)
    X, uv = X[perm], uv[perm]
    calls = (5, 5, 5, -1)
    sets = draw_quads(n, 4, _rows(16, calls), Lcg(n + {60: 11000, 100: 3000, 150: 5000}[n]).random_int)   # (seeds with two or three records in the budget)
    P = _problem(name, X, uv, _gates(rng, n), sets, 10, 16, calls, gaps=7)
    return Case(name, P, None, lambda: True)


NAMES = ["all_n4", "all_n5", "all_n63", "all_n64", "all_n65", "all_n129", "gate_on", "gate_above", "gate_below", "gate_all_double", "gate_float_ue", "behind_camera", "zc_zero",
         "groups_a_then_b", "groups_b_then_a", "refine_exact_min", "refine_one_more", "success_then_calls", "overrun", "n_below_min",
         "min_inliers_eq_n", "degenerate_sets", "same_point_four_times", "winners_and_flips", "nonfinite", "min_set5", "refine_11", "refine_64",
         "refine_65"]


_CASES = None


def case_by_name(name):
    if name in SCENE_NAMES:
        return scene(name)
    return next(c for c in constructed() if c.name == name)


def moved(c, form):
    """does the wrong form change what the case's calls return, or what its hypotheses evaluate to?"""
    want = expected(c)
    P = c.problem
    w = frozenset([form])
    if not same_calls(pnp_iterate(P, w), want.calls):
        return True
    return form in (_CHECK_FORMS | _TAIL_FORMS) and not same_hyps(pnp_hypotheses(P, len(want.hyps.count), w), want.hyps)


def constructed():
    global _CASES
    if _CASES is None:
        _CASES = _build() + _build_more()
    return _CASES


# Which constructed cases each wrong form moves (tests/test_pnp_cases.py recomputes this table).  The cases built FOR a form name it in their
# own moved_by; the rest of a row is what the form also changes on the way: no_det_flip and sign_mean_depth change the garbage poses of sample
# sets that hold outliers, best_ge and refine_current change which record a call reports wherever two hypotheses tie, inliers_sized_n changes
# every returned vector, loop_and every first call that does not succeed within its own count.
# Finding: reperr_le can move no case short of two approximations with bit-equal reprojection errors, which none of these inputs produces
# (a NaN error compares false under both forms); draw_replace changes draw_quads, which no case calls (tests/test_pnp_cases.py tests the draws).
MOVES = {
    "loop_and": ("all_n4", "behind_camera", "zc_zero", "groups_a_then_b", "groups_b_then_a", "refine_exact_min", "overrun",
        "min_inliers_eq_n", "degenerate_sets", "same_point_four_times", "refine_11", "refine_64"),
    "refine_current": ("all_n5", "all_n63", "all_n64", "all_n65", "all_n129", "gate_on", "gate_above", "gate_below", "gate_all_double",
        "gate_float_ue", "zc_zero", "groups_a_then_b", "groups_b_then_a", "refine_one_more", "success_then_calls",
        "degenerate_sets", "same_point_four_times", "nonfinite", "min_set5", "refine_65"),
    "refine_gate_ge": ("refine_exact_min", "min_inliers_eq_n"),
    "qualify_gt": ("all_n4", "refine_exact_min", "min_inliers_eq_n"),
    "best_ge": ("all_n4", "all_n5", "all_n63", "all_n64", "all_n129", "zc_zero", "groups_a_then_b", "groups_b_then_a",
        "refine_exact_min", "refine_one_more", "success_then_calls", "min_inliers_eq_n", "degenerate_sets",
        "same_point_four_times", "nonfinite", "min_set5"),
    "check_le": ("gate_on", "gate_all_double"),
    "check_float_ue": ("gate_above", "gate_float_ue"),
    "check_all_double": ("gate_above", "gate_all_double"),
    "depth_gate": ("behind_camera", "refine_64"),
    "draw_replace": (),
    "sign_mean_depth": ("overrun", "winners_and_flips", "refine_64"),
    "no_det_flip": ("all_n4", "all_n64", "all_n129", "gate_on", "gate_above", "gate_below", "gate_all_double", "gate_float_ue",
        "behind_camera", "zc_zero", "refine_exact_min", "success_then_calls", "overrun", "n_below_min", "min_inliers_eq_n",
        "winners_and_flips", "refine_11", "refine_64", "refine_65"),
    "reperr_le": (),
    "inliers_sized_n": ("all_n4", "all_n5", "all_n63", "all_n64", "all_n65", "all_n129", "gate_on", "gate_above", "gate_below",
        "gate_all_double", "gate_float_ue", "behind_camera", "zc_zero", "groups_a_then_b", "groups_b_then_a",
        "refine_exact_min", "refine_one_more", "success_then_calls", "overrun", "min_inliers_eq_n", "degenerate_sets",
        "same_point_four_times", "winners_and_flips", "nonfinite", "min_set5", "refine_11", "refine_64", "refine_65"),
}
