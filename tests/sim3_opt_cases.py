"""Optimizer::OptimizeSim3 (src/Optimizer.cc:2409-2594) restated in fp64 numpy together with exactly the g2o code it runs, its plausible wrong
forms behind a switch each, and constructed cases with a reach predicate each.  No device and no library: tests/test_sim3_opt_cases.py holds
the cases to their claims, tests/test_sim3_opt_host_progs.py runs csrc/sim3_opt_math.h on the host against mode "reference" and
tests/test_gpu_sim3_opt.py runs the kernel against mode "device", both bit for bit.

The restatement mirrors orb_ygz_slam_amd/csrc/sim3_opt_math.h operation for operation (the header's opening comment states the evaluation
orders this project fixes where the reference leaves them to Eigen): scalars are numpy.float64, the per-edge code is the same expressions on
float64 arrays over the correspondences, and the ONE float rounding -- project() returns a Vector2f -- goes through numpy.float32.  The
header's own sin / cos / exp (argument reduction + fixed polynomial from + - * / only) are restated too; LIBM_EPS is the recorded bound on
their distance from libm, measured by test_sim3_opt_cases.py::test_transcendentals_against_libm over 20 001 even steps each: sin 2.3e-16,
cos 1.2e-16 (absolute, |theta| <= pi), exp 2.3e-16 (relative, |sigma| <= 1).  The reference's g2o needs Eigen, which is not available to this repository: this row
is *parity unpinned* (DESIGN.md section 2), as k_pose_opt's is.  The LDLT, the margin record and `_rel` are tests/pose_opt_cases.py's.

The numeric Jacobian (central differences of 1e-9 through a projection that is rounded to float) is a dither: most entries are exactly 0, the
others multiples of ulp f / 2e-9.  One different last bit in a quotient moves an entry by thousands, so a case is admitted only if the two
summation modes never round a projection quotient to different floats (Result.qhash is the digest of every rounded quotient of a run; the
seeds below were searched on the CPU until every listed case qualifies, and the test asserts it -- no case is skipped).

Two summation modes for H, b and the active robust chi2:
    reference  edges in insertion order: e12(i0), e21(i0), e12(i1), .. one after the other
    device     correspondence c belongs to thread c % 256, ascending c per thread, e12 then e21; 64 lanes combined as a balanced tree of
               neighbours, the four waves in wave order: ((w0 + w1) + w2) + w3   (wave_sum_f64, as k_pose_opt)
"""
import collections
import hashlib
import math
import struct

import numpy as np

from tests import pose_opt_cases as PC

F = np.float64
WRONG_FORMS = ("proj_double", "analytic_jacobian", "delta_1e6", "classify_accepted", "more_always_10", "more_always_5", "gate_and", "huber_th2",
               "scale_free", "inverse_forward", "early_writes_s12", "lt10_before_removal")
# proj_double          the projection quotients stay double (the reference: project() returns Vector2f)
# analytic_jacobian    the analytic Jacobian of the two edges (the reference: this fork comments linearizeOplus out -- central differences)
# delta_1e6            central differences with delta = 1e-6 (the reference: 1e-9)
# classify_accepted    the gates read the error at the accepted estimate (the reference: _error of the last trial, accepted or not).
#                      FINDING: it can move no case that keeps its margin.  The trial loop ends on an accepted trial (rho > 0) unless ten
#                      trials failed, rho == 0 or an operand is non-finite.  After ten failures lambda has grown by 2^45 and the last step
#                      is far below a float ulp of any quotient, rho == 0 means no error changed at all, and a non-finite system fails its
#                      factorisation, which leaves x stale and the estimate finite: in each the last trial's errors ARE the accepted ones
#                      (stop_trials, stop_rho_zero and nan_point reach the three routes; test_last_trial_errors_equal_the_accepted_ones)
# more_always_10 / _5  optimize(10) / optimize(5) after the first gate whatever nBad is (the reference: nBad > 0 ? 10 : 5)
# gate_and             e12->chi2() > th2 && e21->chi2() > th2 (the reference: ||)
# huber_th2            Huber delta th2 (the reference: float sqrt(th2))
# scale_free           update[6] is applied under _fix_scale (the reference: oplusImpl zeroes it, in the solver's own x)
# inverse_forward      e21 maps its point through the estimate (the reference: through estimate().inverse())
# early_writes_s12     the early return writes g2oS12 (the reference returns before `g2oS12 = estimate`)
# lt10_before_removal  nCorrespondences < 10 is tested (the reference: nCorrespondences - nBad < 10)

STOP_MAX_ITER, STOP_TRIALS, STOP_RHO_ZERO, STOP_NBAD, STOP_NOT_RUN = 0, 1, 2, 3, 4
STOP_NAMES = ("max_iter", "trials", "rho_zero", "nbad", "not_run")
DBL_MAX = float(np.finfo(np.float64).max)
MARGIN_MIN = PC.MARGIN_MIN
LIBM_EPS = 5e-16   # YGZF_SIM3_OPT_LIBM_EPS of the header

# The largest difference between the Sim3s (8 numbers) of the two summation modes over all cases below, as tests/test_sim3_opt_cases.py
# measures it on the CPU: what reordering the sums alone does to the reference's algorithm under the admission rule above.  (The test asserts
# that the measured value does not exceed the constant and is within a factor 4 of it.)
EPS_ORDER = 1.4e-15   # measured 1.33e-15, at scene_1 (a translation component of ~0.3: a few units in its last place); 0 on 13 of the cases

Problem = collections.namedtuple("Problem", "P1c P2c obs1 obs2 is1 is2 K1 K2 S12 th2 fix_scale")
Result = collections.namedtuple("Result", "S12 removed ret n_bad iters trials stop lam chi2 margin where pivot_margin trace qhash")
# margin: the smallest relative distance of a chi2 gate, a rho sign or a stop rule from its branch point (>= MARGIN_MIN on every case);
# pivot_margin: the smallest |pivot| / largest |diagonal| of a factorisation.  The pivots decide `every pivot > 0`, and the dithered
# Jacobian leaves the system badly conditioned, so their floor is set from the arithmetic instead: a pivot's rounding error is a few
# eps x the largest diagonal (~1e-15), PIVOT_MARGIN_MIN keeps three orders of magnitude above that.  Not counted: the scale's pivot under
# _fix_scale, whose row of H is exactly zero in any order and whose pivot is lambda itself.
PIVOT_MARGIN_MIN = 1e-12
Case = collections.namedtuple("Case", "name problem reach")


# ---- the header's sin, cos, exp -----------------------------------------------------------------------------------------------------------------
def so_nearest(x):
    return (x + F(6755399441055744.0)) - F(6755399441055744.0)


def so_sincos(x):
    x = F(x)
    if not (x >= -1048576.0 and x <= 1048576.0):
        with np.errstate(all="ignore"):
            return x - x, F(1.0) + (x - x)
    k = so_nearest(x * F(6.36619772367581382433e-01))
    r = ((x - k * F(1.57079632673412561417e+00)) - k * F(6.07710050630396597660e-11)) - k * F(2.02226624871116645580e-21)
    z = r * r
    ps = F(-1.66666666666666324348e-01) + z * (F(8.33333333332248946124e-03) + z * (F(-1.98412698298579493134e-04) + z * (F(2.75573137070700676789e-06) + z * (F(-2.50507602534068634195e-08) + z * F(1.58969099521155010221e-10)))))
    pc = F(4.16666666666666019037e-02) + z * (F(-1.38888888888741095749e-03) + z * (F(2.48015872894767294178e-05) + z * (F(-2.75573143513906633035e-07) + z * (F(2.08757232129817482790e-09) + z * F(-1.13596475577881948265e-11)))))
    s0 = r + r * (z * ps)
    c0 = (F(1.0) - F(0.5) * z) + (z * z) * pc
    n = int(k) & 3
    return (s0, c0, -s0, -c0)[n], (c0, -s0, -c0, s0)[n]


_EXP_COEF = [F(1.0) / F(v) for v in (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0)] + [F(0.5), F(1.0), F(1.0)]


def so_exp(x):
    x = F(x)
    if not (x <= 709.0):
        return F(np.inf) if x > 709.0 else x
    if x < -745.0:
        return F(0.0)
    k = so_nearest(x * F(1.44269504088896338700e+00))
    r = (x - k * F(6.93147180369123816490e-01)) - k * F(1.90821492927058770002e-10)
    p = _EXP_COEF[0]
    for c in _EXP_COEF[1:]:
        p = p * r + c
    ki = int(k)
    m = -ki if ki < 0 else ki
    f, sc = (F(0.5) if ki < 0 else F(2.0)), F(1.0)
    with np.errstate(all="ignore"):   # (the last squarings overflow or underflow, unused, as in the header)
        for _ in range(11):
            if m & 1:
                sc = sc * f
            f = f * f
            m >>= 1
        return p * sc


# ---- Eigen's quaternion pieces and g2o::Sim3; a transform is (q [4], t [3], s) of float64 scalars ------------------------------------------------
def quat_from_R(m):
    q = [None] * 4
    t = (m[0] + m[4]) + m[8]
    if t > 0.0:
        t = np.sqrt(t + F(1.0))
        q[3] = F(0.5) * t
        t = F(0.5) / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + F(1.0))
        q[i] = F(0.5) * t
        t = F(0.5) / t
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_rotate(q, v):
    """_transformVector; v: three scalars or three arrays"""
    ux, uy, uz = q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = q[1] * uz - q[2] * uy, q[2] * ux - q[0] * uz, q[0] * uy - q[1] * ux
    return [v[0] + q[3] * ux + cx, v[1] + q[3] * uy + cy, v[2] + q[3] * uz + cz]


def sim3_exp(u):
    u = [F(v) for v in u]
    om = u[0:3]
    sigma = u[6]
    theta = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    z = F(0.0)
    O = [z, -om[2], om[1], om[2], z, -om[0], -om[1], om[0], z]
    s = so_exp(sigma)
    O2 = [O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j] for i in range(3) for j in range(3)]
    eps = F(0.00001)
    small = bool(theta < eps)
    one = F(1.0)
    if not small:
        sn, cs = so_sincos(theta)
        ra = sn / theta
        rb = (one - cs) / (theta * theta)
    R = []
    for i in range(3):
        for j in range(3):
            I = one if i == j else z
            R.append((I + O[3 * i + j]) + O2[3 * i + j] if small else (I + ra * O[3 * i + j]) + rb * O2[3 * i + j])
    if abs(sigma) < eps:
        C = one
        if small:
            A = one / F(2.0)
            B = one / F(6.0)
        else:
            theta2 = theta * theta
            A = (one - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - one) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - one) * s + one) / sigma2
            B = ((F(0.5) * sigma2 - sigma + one) * s) / (sigma2 * sigma)
        else:
            a = s * sn
            b = s * cs
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (one - b) * theta) / (theta * c)
            B = (C - ((b - one) * sigma + a * theta) / c) * one / theta2
    q = quat_from_R(R)
    W = [(A * O[3 * i + j] + B * O2[3 * i + j]) + C * (one if i == j else z) for i in range(3) for j in range(3)]
    t = [W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5] for i in range(3)]
    return (q, t, s)


def s3_map(T, v):
    r = quat_rotate(T[0], v)
    return [T[2] * r[0] + T[1][0], T[2] * r[1] + T[1][1], T[2] * r[2] + T[1][2]]


def s3_inverse(T):
    q, t, s = T
    f = F(-1.0) / s
    v = [f * t[0], f * t[1], f * t[2]]
    qi = [-q[0], -q[1], -q[2], q[3]]
    return (qi, quat_rotate(qi, v), F(1.0) / s)


def s3_mul(a, b):
    r = quat_rotate(a[0], b[1])
    return (quat_mul(a[0], b[0]), [a[2] * r[0] + a[1][0], a[2] * r[1] + a[1][1], a[2] * r[2] + a[1][2]], a[2] * b[2])


def s3_from8(S):
    S = [F(v) for v in S]
    return (S[0:4], S[4:7], S[7])


def s3_to8(T):
    return np.array(list(T[0]) + list(T[1]) + [T[2]], np.float64)


def transform(S, j, fix_scale, delta, wrong=None):
    """-> (forward, inverse) of transform j of an iteration"""
    if j == 0:
        fwd = S
    else:
        d = (j - 1) >> 1
        u = [F(0.0)] * 7
        u[d] = F(delta) if (j & 1) else -F(delta)
        if fix_scale and wrong != "scale_free":
            u[6] = F(0.0)
        fwd = s3_mul(sim3_exp(u), S)
    return fwd, s3_inverse(fwd)


# ---- the edges, vectorised over the correspondences ----------------------------------------------------------------------------------------------
class _Edges:
    def __init__(self, P, wrong):
        f32 = np.float32
        self.n = len(np.asarray(P.P1c).reshape(-1, 3))
        X1 = np.asarray(P.P1c, f32).reshape(-1, 3).astype(np.float64)
        X2 = np.asarray(P.P2c, f32).reshape(-1, 3).astype(np.float64)
        o1 = np.asarray(P.obs1, f32).reshape(-1, 2).astype(np.float64)
        o2 = np.asarray(P.obs2, f32).reshape(-1, 2).astype(np.float64)
        self.X = ([X2[:, 0], X2[:, 1], X2[:, 2]], [X1[:, 0], X1[:, 1], X1[:, 2]])   # e12 maps P3D2c, e21 maps P3D1c
        self.obs = ([o1[:, 0], o1[:, 1]], [o2[:, 0], o2[:, 1]])
        self.s = (np.asarray(P.is1, f32).astype(np.float64), np.asarray(P.is2, f32).astype(np.float64))
        self.K = ([F(f32(v)) for v in P.K1], [F(f32(v)) for v in P.K2])
        th2 = f32(P.th2)
        self.th2 = F(th2)
        self.delta = self.th2 if wrong == "huber_th2" else F(f32(np.sqrt(F(th2))))   # `const float deltaHuber = sqrt(th2)`
        self.wrong = wrong
        self.hash = hashlib.sha1()

    def error(self, T, which):
        """computeError of e12 (which = 0, T the estimate) / e21 (which = 1, T its inverse) -> e0, e1, p"""
        K = self.K[which]
        p = s3_map(T, self.X[which])
        u, v = p[0] / p[2], p[1] / p[2]
        if self.wrong != "proj_double":
            u, v = u.astype(np.float32), v.astype(np.float32)
            self.hash.update(u.tobytes())
            self.hash.update(v.tobytes())
            u, v = u.astype(np.float64), v.astype(np.float64)
        return self.obs[which][0] - (u * K[0] + K[2]), self.obs[which][1] - (v * K[1] + K[3]), p

    def chi2(self, e0, e1, which):
        s = self.s[which]
        return e0 * (s * e0) + e1 * (s * e1)

    def huber(self, chi2):
        dsqr = self.delta * self.delta
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, 2 * sq * self.delta - dsqr), np.where(inl, 1.0, self.delta / sq)

    def analytic(self, T, which, fix_scale):
        """the analytic Jacobian (wrong form): d e / d (omega, upsilon, sigma) of a left update"""
        K = self.K[which]
        X = self.X[which]
        p = s3_map(T, X)
        x, y, z = p
        a = [[-K[0] / z, 0 * z, K[0] * x / (z * z)], [0 * z, -K[1] / z, K[1] * y / (z * z)]]      # -d cam(proj(p)) / d p
        if which == 0:
            D = [[0 * x, z, -y, 1 + 0 * x, 0 * x, 0 * x, x], [-z, 0 * x, x, 0 * x, 1 + 0 * x, 0 * x, y], [y, -x, 0 * x, 0 * x, 0 * x, 1 + 0 * x, z]]
        else:   # p = S^-1 (exp(-u) X): d p / d u = -(s^-1 R^-1) [-X^ | I | X]
            R = PC.quat_to_R(np.array(T[0], np.float64)) * T[2]
            x0, y0, z0 = X
            E = [[0 * x, z0, -y0, 1 + 0 * x, 0 * x, 0 * x, x0], [-z0, 0 * x, x0, 0 * x, 1 + 0 * x, 0 * x, y0], [y0, -x0, 0 * x, 0 * x, 0 * x, 1 + 0 * x, z0]]
            D = [[-(R[i, 0] * E[0][k] + R[i, 1] * E[1][k] + R[i, 2] * E[2][k]) for k in range(7)] for i in range(3)]
        J = [[a[r][0] * D[0][k] + a[r][1] * D[1][k] + a[r][2] * D[2][k] for k in range(7)] for r in range(2)]
        if fix_scale and self.wrong != "scale_free":
            J[0][6], J[1][6] = 0 * x, 0 * x
        return J

    def edge_terms(self, Ts, which, fix_scale, jdelta):
        """one edge kind at the 15 transforms Ts -> terms [n, 36] (28 of H, 7 of b, rho0), chi2 [n]"""
        e0, e1, _ = self.error(Ts[0], which)
        if self.wrong == "analytic_jacobian":
            J = self.analytic(Ts[0], which, fix_scale)
        else:
            scalar = F(1.0) / (2 * F(jdelta))
            J = [[None] * 7, [None] * 7]
            for d in range(7):
                p0, p1, _ = self.error(Ts[1 + 2 * d], which)
                m0, m1, _ = self.error(Ts[2 + 2 * d], which)
                J[0][d] = scalar * (p0 - m0)
                J[1][d] = scalar * (p1 - m1)
        s = self.s[which]
        chi2 = self.chi2(e0, e1, which)
        rho0, rho1 = self.huber(chi2)
        w = rho1 * s
        r0, r1 = (-(s * e0)) * rho1, (-(s * e1)) * rho1
        cols = []
        for j in range(7):
            for k in range(j, 7):
                cols.append((J[0][j] * w) * J[0][k] + (J[1][j] * w) * J[1][k])
        for j in range(7):
            cols.append(J[0][j] * r0 + J[1][j] * r1)
        cols.append(rho0)
        return np.stack(cols, -1), chi2

    def ordered_sum(self, t12, t21, active, mode):
        """the rows of t12 / t21 [n, k] of the active pairs summed in the mode's order, from 0.0 on"""
        k = t12.shape[1]
        if mode == "reference":
            rows = np.empty((2 * self.n + 1, k))
            rows[0] = 0.0
            rows[1::2] = t12
            rows[2::2] = t21
            keep = np.concatenate([[True], np.repeat(active, 2)])
            return np.cumsum(rows[keep], axis=0)[-1]
        assert mode == "device"
        nrow = max((self.n + 255) // 256, 1)
        a12, a21 = np.zeros((nrow * 256, k)), np.zeros((nrow * 256, k))
        act = np.zeros(nrow * 256, bool)
        a12[:self.n], a21[:self.n], act[:self.n] = t12, t21, active
        a12, a21, act = a12.reshape(-1, 256, k), a21.reshape(-1, 256, k), act.reshape(-1, 256)
        acc = np.zeros((256, k))
        for r in range(nrow):
            acc = np.where(act[r][:, None], (acc + a12[r]) + a21[r], acc)
        v = acc.reshape(4, 4, 16, k)
        for _ in range(4):
            v = v[:, :, 0::2] + v[:, :, 1::2]
        v = v[:, :, 0]
        w = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
        return ((w[0] + w[1]) + w[2]) + w[3]


def optimize_sim3(P, mode="reference", wrong=None):
    """The restatement.  -> Result; trace: per round its trials (iteration, trial, rho, lambda, ..) and its gate, for the reach predicates.
    (Inf and NaN are values here, as they are on the device: no warnings.)"""
    with np.errstate(all="ignore"):
        return _optimize_sim3(P, mode, wrong)


def _optimize_sim3(P, mode, wrong):
    assert mode in ("reference", "device") and (wrong is None or wrong in WRONG_FORMS)
    E = _Edges(P, wrong)
    n = E.n
    fix = bool(P.fix_scale)
    S_in = np.asarray(P.S12, np.float64).copy()
    removed = np.zeros(n, np.uint8)
    iters, trials, stop = [0, 0], [0, 0], [STOP_NOT_RUN] * 2
    lam_out, chi_out = [0.0, 0.0], [0.0, 0.0]
    M, MP = PC._Margin(), PC._Margin()
    trace = []

    def result(S, ret, nBad):
        return Result(S, removed, ret, nBad, iters, trials, stop, lam_out, chi_out, M.v, M.where, MP.v, trace, E.hash.hexdigest())
    if n == 0:
        return result(S_in, 0, 0)
    est = s3_from8(S_in)
    jdelta = 1e-6 if wrong == "delta_1e6" else 1e-9
    stored12, stored21 = np.full(n, np.nan), np.full(n, np.nan)
    x = [F(0.0)] * 7
    lam, ni = F(-1.0), F(2.0)
    nBad = 0
    ret = 0
    for rnd in range(2):
        active = removed == 0
        if rnd == 0:
            max_it = 5
        else:
            max_it = 10 if wrong == "more_always_10" else 5 if wrong == "more_always_5" else (10 if nBad > 0 else 5)
        rtrace = []
        reason = STOP_MAX_ITER
        nbad_rule = 0
        acc12, acc21 = stored12, stored21          # the errors at the accepted estimate (wrong form classify_accepted)
        for it in range(max_it):
            pairs = [transform(est, j, fix, jdelta, wrong) for j in range(15)]
            Tf = [p[0] for p in pairs]
            Ti = Tf if wrong == "inverse_forward" else [p[1] for p in pairs]
            t12, c12 = E.edge_terms(Tf, 0, fix, jdelta)
            t21, c21 = E.edge_terms(Ti, 1, fix, jdelta)
            stored12, stored21 = np.where(active, c12, stored12), np.where(active, c21, stored21)
            acc12, acc21 = stored12, stored21
            S = E.ordered_sum(t12, t21, active, mode)
            H = np.zeros((7, 7))
            c = 0
            for j in range(7):
                for k in range(j, 7):
                    H[j, k] = H[k, j] = S[c]
                    c += 1
            b = [F(v) for v in S[28:35]]
            currentChi = F(S[35])
            iniChi = currentChi
            if it == 0:
                md = F(0.0)
                for j in range(7):          # std::max(fabs(H_jj), maxDiagonal): (a < b) ? b : a
                    v = abs(H[j, j])
                    md = md if v < md else v
                lam = F(1e-5) * md
                ni = F(2.0)
                nbad_rule = 0
            rho = F(0.0)
            qmax = 0
            while True:
                backup = est
                Hd = H.copy()
                for j in range(7):
                    Hd[j, j] = H[j, j] + lam
                ok, Lm, tr, piv = PC.ldlt(Hd)
                dmax = max(abs(Hd[j, j]) for j in range(7))
                if dmax > 0 and np.all(np.isfinite(Hd)):   # (an all-zero or non-finite matrix fails in any summation order)
                    exact = fix and wrong is None and not np.any(H[6])          # the scale's pivot is lambda itself
                    MP.note(min(abs(v) for v in (sorted(piv, key=abs)[1:] if exact else piv)) / dmax, ("pivot", rnd, it, qmax))
                if ok:
                    x = [F(v) for v in PC.ldlt_solve(Lm, tr, b)]
                if fix and wrong != "scale_free":
                    x[6] = F(0.0)
                est = s3_mul(sim3_exp(x), est)
                inv = est if wrong == "inverse_forward" else s3_inverse(est)
                e0, e1, _ = E.error(est, 0)
                d12 = E.chi2(e0, e1, 0)
                e0, e1, _ = E.error(inv, 1)
                d21 = E.chi2(e0, e1, 1)
                stored12, stored21 = np.where(active, d12, stored12), np.where(active, d21, stored21)
                r12, r21 = E.huber(d12)[0], E.huber(d21)[0]
                tempChi = F(E.ordered_sum(r12[:, None], r21[:, None], active, mode)[0])
                if not ok:
                    tempChi = F(DBL_MAX)
                scale = F(0.0)
                for j in range(7):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + F(1e-3)
                rho = (currentChi - tempChi) / scale
                # as tests/pose_opt_cases.py: rho is a ratio already, its distance from 0 is |rho|; not counted: an update that leaves every
                # edge's error as it was -- the estimate itself, or every float quotient under a step too small to move one: the same terms
                # in the same order give tempChi == currentChi and rho == 0 by construction in any order -- and non-finite operands (they
                # propagate through every order alike)
                moved = not (np.array_equal(d12[active], acc12[active], equal_nan=True) and np.array_equal(d21[active], acc21[active], equal_nan=True))
                if (moved or not ok) and math.isfinite(currentChi) and math.isfinite(rho):
                    M.note(abs(float(rho)), ("rho", rnd, it, qmax))
                good = bool(rho > 0) and math.isfinite(tempChi)
                rtrace.append(dict(it=it, trial=qmax, ok=ok, rho=float(rho), lam=float(lam), good=good, chi=float(currentChi), temp=float(tempChi),
                                   nactive=int(active.sum()), scale=float(est[2])))
                if good:
                    c3 = 2 * rho - 1
                    alpha = F(1.0) - c3 * c3 * c3
                    alpha = F(2.0) / F(3.0) if F(2.0) / F(3.0) < alpha else alpha
                    lam = lam * (alpha if F(1.0) / F(3.0) < alpha else F(1.0) / F(3.0))
                    ni = F(2.0)
                    currentChi = tempChi
                    acc12, acc21 = stored12, stored21
                else:
                    lam = lam * ni
                    ni = ni * 2
                    est = backup
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            iters[rnd] += 1
            trials[rnd] += qmax
            if qmax == 10 or rho == 0:
                reason = STOP_TRIALS if qmax == 10 else STOP_RHO_ZERO
                break
            lhs = (iniChi - currentChi) * F(1e3)
            if math.isfinite(lhs) and math.isfinite(iniChi):
                M.note(PC._rel(float(lhs), float(iniChi)), ("stop", rnd, it))
            if lhs < iniChi:
                nbad_rule += 1
            else:
                nbad_rule = 0
            if nbad_rule >= 3:
                reason = STOP_NBAD
                break
        stop[rnd] = reason
        lam_out[rnd], chi_out[rnd] = float(lam), float(currentChi)
        g12, g21 = (acc12, acc21) if wrong == "classify_accepted" else (stored12, stored21)
        for g in (g12, g21):
            gm = np.abs(g - E.th2) / E.th2
            gm = np.where(active & np.isfinite(g), gm, np.inf)
            if len(gm):
                M.note(float(np.min(gm)), ("gate", rnd))
        b12, b21 = g12 > E.th2, g21 > E.th2
        bad = active & ((b12 & b21) if wrong == "gate_and" else (b12 | b21))
        rtr = dict(trials=rtrace, bad12=active & b12, bad21=active & b21, bad=bad, est=s3_to8(est),
                   bad_accepted=active & ((acc12 > E.th2) | (acc21 > E.th2)))   # (what the gate would say at the accepted estimate)
        trace.append(rtr)
        if rnd == 0:
            removed[bad] = 1
            nBad = int(bad.sum())
            if (n if wrong == "lt10_before_removal" else n - nBad) < 10:
                return result(s3_to8(est) if wrong == "early_writes_s12" else S_in, 0, nBad)
        else:
            removed[bad] = 2
            ret = int((active & ~bad).sum())
    return result(s3_to8(est), ret, nBad)


def same(a, b, info=True):
    """two Results agree in every output (NaN equals NaN)"""
    ok = (np.array_equal(a.S12.view(np.uint64), b.S12.view(np.uint64)) or (np.array_equal(np.isnan(a.S12), np.isnan(b.S12)) and
          np.array_equal(a.S12[~np.isnan(a.S12)], b.S12[~np.isnan(b.S12)])))
    ok = ok and np.array_equal(a.removed, b.removed) and a.ret == b.ret and a.n_bad == b.n_bad
    if info:
        ok = ok and list(a.iters) == list(b.iters) and list(a.trials) == list(b.trials) and list(a.stop) == list(b.stop)
        ok = ok and np.array_equal(np.array(a.lam), np.array(b.lam), equal_nan=True) and np.array_equal(np.array(a.chi2), np.array(b.chi2), equal_nan=True)
    return bool(ok)


def same_decisions(a, b):
    return (np.array_equal(a.removed, b.removed) and a.ret == b.ret and a.n_bad == b.n_bad and list(a.iters) == list(b.iters) and
            list(a.trials) == list(b.trials) and list(a.stop) == list(b.stop))


# ---- the exchange with tests/cpp/sim3_opt_host.cc ---------------------------------------------------------------------------------------------
def write_case(P, path):
    f32 = np.float32
    n = len(np.asarray(P.P1c).reshape(-1, 3))
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n, int(bool(P.fix_scale))))
        f.write(np.asarray([P.th2], f32).tobytes())
        f.write(np.asarray(P.K1, f32).tobytes())
        f.write(np.asarray(P.K2, f32).tobytes())
        f.write(np.asarray(P.S12, np.float64).tobytes())
        for a in (P.P1c, P.P2c, P.obs1, P.obs2, P.is1, P.is2):
            f.write(np.ascontiguousarray(a, f32).tobytes())


def read_result(P, path):
    n = len(np.asarray(P.P1c).reshape(-1, 3))
    raw = open(path, "rb").read()
    S = np.frombuffer(raw, np.float64, 8, 0).copy()
    ret, nBad = struct.unpack_from("<ii", raw, 64)
    at = 72
    iters, trials, stop, lam, chi = [], [], [], [], []
    for _ in range(2):
        a, b, c = struct.unpack_from("<iii", raw, at)
        d, e = struct.unpack_from("<dd", raw, at + 12)
        at += 28
        iters.append(a), trials.append(b), stop.append(c), lam.append(d), chi.append(e)
    removed = np.frombuffer(raw, np.uint8, n, at).copy()
    return Result(S, removed, ret, nBad, iters, trials, stop, lam, chi, None, None, None, None, None)


def as_api(P):
    """the problem as Context.optimize_sim3 takes it"""
    return dict(P1c=P.P1c, P2c=P.P2c, obs1=P.obs1, obs2=P.obs2, inv_sigma2_1=P.is1, inv_sigma2_2=P.is2, K1=P.K1, K2=P.K2, S12=P.S12, th2=P.th2,
                fix_scale=P.fix_scale)


def from_api(r):
    return Result(np.asarray(r["S12"], np.float64), np.asarray(r["removed"], np.uint8), r["ret"], r["n_bad"], r["iterations"], r["trials"], r["stop"],
                  r["lam"], r["chi2"], None, None, None, None, None)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
K_A = (458.654, 457.296, 367.215, 248.375)      # EuRoC cam0
K_B = (520.9, 521.0, 325.1, 249.7)              # TUM fr1
K_POW2 = (512.0, 512.0, 0.0, 0.0)


def _axis_angle_q(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return list(a * math.sin(angle / 2)) + [math.cos(angle / 2)]


def scene(seed, n, out1=0, out2=0, fix_scale=True, K1=K_A, K2=K_A, th2=10.0, octaves=False, noise=0.4, start=(0.004, 0.02, 0.0), scale=1.0,
          spoil=None):
    """n correspondences of a true S12 (a rotation of 0.15 rad, a translation, `scale`), observations with `noise` pixels of error per level
    sigma, the first out1 pairs with a gross error (25 .. 80 pixels) in KF1's observation, the next out2 in KF2's; the start is the truth
    perturbed by `start` = (rotation, translation, log scale).  spoil(arrays dict): last edits."""
    rng = np.random.RandomState(seed)
    f32 = np.float32
    P2c = rng.uniform([-2.0, -1.5, 3.0], [2.0, 1.5, 9.0], (n, 3)).astype(f32)
    true = s3_from8(_axis_angle_q(rng.normal(size=3), 0.15) + [0.3, -0.1, 0.2] + [scale])
    m = s3_map(true, [P2c[:, k].astype(np.float64) for k in range(3)])
    P1c = np.stack(m, -1).astype(f32)
    oct1 = rng.randint(0, 8, n) if octaves else np.zeros(n, int)
    oct2 = rng.randint(0, 8, n) if octaves else np.zeros(n, int)
    sig = 1.2 ** np.arange(8)
    is_tab = (1.0 / (sig * sig)).astype(f32)

    def proj(X, K, o):
        X = X.astype(np.float64)
        uv = np.stack([X[:, 0] / X[:, 2] * K[0] + K[2], X[:, 1] / X[:, 2] * K[1] + K[3]], -1)
        return uv + rng.normal(size=(len(X), 2)) * noise * sig[o][:, None]
    obs1, obs2 = proj(P1c, K1, oct1), proj(P2c, K2, oct2)
    gross = rng.uniform(25.0, 80.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    obs1[:out1] += gross[:out1] * sig[oct1[:out1]][:, None]
    obs2[out1:out1 + out2] += gross[out1:out1 + out2] * sig[oct2[out1:out1 + out2]][:, None]
    pert = sim3_exp(list(rng.normal(size=3) * start[0]) + list(rng.normal(size=3) * start[1]) + [0.0 if fix_scale else start[2]])
    S12 = s3_to8(s3_mul(pert, true))
    a = dict(P1c=P1c, P2c=P2c, obs1=obs1.astype(f32), obs2=obs2.astype(f32), is1=is_tab[oct1], is2=is_tab[oct2], S12=S12)
    if spoil:
        spoil(a)
    return Problem(a["P1c"], a["P2c"], a["obs1"], a["obs2"], a["is1"], a["is2"], tuple(K1), tuple(K2), a["S12"], th2, fix_scale)


def exact_fit(seed, n):
    """observations that equal the projections at the start bit for bit (f = 512, c = 0: float(u) * 512 is a float): every error is 0, b = 0,
    the update is Sim3(0) and leaves the estimate as it was -- rho == 0"""
    P = scene(seed, n, K1=K_POW2, K2=K_POW2, noise=0.0)
    E = _Edges(P, None)
    S = s3_from8(P.S12)
    with np.errstate(all="ignore"):
        e0, e1, _ = E.error(S, 0)
        o1 = np.stack([E.obs[0][0] - e0, E.obs[0][1] - e1], -1)
        e0, e1, _ = E.error(s3_inverse(S), 1)
        o2 = np.stack([E.obs[1][0] - e0, E.obs[1][1] - e1], -1)
    assert np.array_equal(o1.astype(np.float32).astype(np.float64), o1) and np.array_equal(o2.astype(np.float32).astype(np.float64), o2)
    return P._replace(obs1=o1.astype(np.float32), obs2=o2.astype(np.float32))


def _set(key, idx, val):
    def f(a):
        a[key] = a[key].copy()
        a[key][idx] = val
    return f


# reach predicates: r = the Result of either mode
def _survivors(k):
    return lambda r: len(r.removed) - r.n_bad == k and (r.ret == 0 and r.stop[1] == STOP_NOT_RUN if k < 10 else r.stop[1] != STOP_NOT_RUN)


def _rejected(r):
    return any(not t["good"] for rt in r.trace for t in rt["trials"])


def _stops(*names):
    return lambda r: all(STOP_NAMES[s] in names for s in r.stop) and all(nm in [STOP_NAMES[s] for s in r.stop] for nm in names)


CASES = []


def _case(name, build, seed, reach):
    """seed: the first of 1, 2, .. at which the case qualifies (reach and margins in both modes, equal decisions, equal quotient digests)"""
    CASES.append(Case(name, build(seed), reach))


# -- the survivors of round 0: 20 correspondences, 20 - k gross outliers (the < 10 rule, the early return, S12 untouched)
for _k in (0, 1, 9, 10, 11):
    _case("survive_%d" % _k, (lambda k: lambda seed: scene(seed, 20, out1=(20 - k + 1) // 2, out2=(20 - k) // 2, noise=0.2, start=(0.0005, 0.002, 0.0)))(_k),
          1, _survivors(_k))
# -- nBad == 0: five further iterations; nBad > 0: ten
_case("nbad_zero", lambda seed: scene(seed, 40, noise=0.2, start=(0.0005, 0.002, 0.0)), 1, lambda r: r.n_bad == 0 and r.iters[1] <= 5 and r.ret == 40)
_case("nbad_some", lambda seed: scene(seed, 40, out1=3, out2=3), 3, lambda r: r.n_bad == 6 and r.ret > 0)
# -- a pair removed by e12 alone and one by e21 alone
_case("one_side_each", lambda seed: scene(seed, 30, out1=1, out2=1), 1,
      lambda r: bool(r.trace[0]["bad12"][0] and not r.trace[0]["bad21"][0] and r.trace[0]["bad21"][1] and not r.trace[0]["bad12"][1]))
# -- scale free / fixed, two cameras, mixed octaves
_case("scale_free", lambda seed: scene(seed, 50, out1=4, out2=4, fix_scale=False, scale=1.15, start=(0.004, 0.02, 0.03)), 1,
      lambda r: r.ret > 0 and r.S12[7] != r.trace[0]["trials"][0]["scale"] and abs(r.S12[7] - 1.15) < 0.05)
_case("scale_fixed", lambda seed: scene(seed, 50, out1=4, out2=4, fix_scale=True), 1, lambda r: r.ret > 0 and r.S12[7] == 1.0)
_case("two_cameras", lambda seed: scene(seed, 50, out1=3, out2=3, K1=K_A, K2=K_B), 1, lambda r: r.ret > 0)
_case("mixed_octaves", lambda seed: scene(seed, 60, out1=4, out2=4, octaves=True), 1, lambda r: r.ret > 0)
# -- a rejected trial; the stop reasons
_case("rejected_trial", lambda seed: scene(seed, 40, out1=4, out2=4, start=(0.02, 0.1, 0.0)), 1, _rejected)
_case("stop_rho_zero", lambda seed: exact_fit(seed, 24), 1, _stops("rho_zero"))
_case("stop_max_iter", lambda seed: scene(seed, 40, out1=2, out2=2, start=(0.03, 0.2, 0.0)), 1, lambda r: STOP_MAX_ITER in r.stop)
_case("stop_nbad", lambda seed: scene(seed, 40, out1=2, out2=2), 3, lambda r: STOP_NBAD in r.stop and r.ret > 0)
_case("stop_trials", lambda seed: scene(seed, 40, out1=3, out2=3), 1, lambda r: STOP_TRIALS in r.stop and r.ret > 0)
# -- no depth gate; z == 0; NaN
_case("behind_camera", lambda seed: scene(seed, 30, spoil=_set("P2c", (0, 2), -4.0)), 1, lambda r: r.removed[0] == 1 and r.ret > 0)
_case("z_zero", lambda seed: scene(seed, 30, spoil=_set("P2c", (0, 2), 0.0)), 1, lambda r: True)
_case("nan_point", lambda seed: scene(seed, 30, spoil=_set("P1c", (3, 1), np.nan)), 1, lambda r: bool(np.isnan(r.chi2[0])))
# -- sizes around the wave and the workgroup
for _n in (63, 64, 65, 255, 256, 257, 600):
    _case("n_%d" % _n, (lambda n: lambda seed: scene(seed, n, out1=n // 20, out2=n // 20))(_n), 1, lambda r: r.ret > 0 and r.n_bad > 0)
# -- seeded scenes: n in 30 .. 300, 10 .. 40 % gross outliers
for _i, (_n, _frac) in enumerate([(30, 0.1), (75, 0.4), (120, 0.25), (200, 0.3), (300, 0.15)]):
    _case("scene_%d" % _i, (lambda n, fr, i: lambda seed: scene(seed, n, out1=int(n * fr / 2), out2=int(n * fr / 2), octaves=bool(i & 1),
                                                                 fix_scale=bool(i & 2), scale=1.0 if i & 2 else 0.9))(_n, _frac, _i), 1,
          lambda r: r.ret > 0 and r.n_bad > 0)
_case("n_zero", lambda seed: scene(seed, 0), 1, lambda r: r.ret == 0 and r.stop == [STOP_NOT_RUN] * 2)
_case("n_one", lambda seed: scene(seed, 1), 1, lambda r: r.ret == 0 and r.stop[1] == STOP_NOT_RUN and r.stop[0] != STOP_NOT_RUN)

NAMES = [c.name for c in CASES]


def _all_but(*names):
    assert all(n in NAMES for n in names)
    return [n for n in NAMES if n not in names]


# The cases each wrong form moves (any output differs from the restatement's: S12, removed, ret, nBad or a round's counts, lambda, chi2), in
# both summation modes alike, as measured on the CPU; tests/test_sim3_opt_cases.py holds every form to exactly its list.  The dithered Jacobian
# makes every run sensitive to the last bit, so a form that touches the per-edge arithmetic moves nearly everything it can reach: n_zero runs
# nothing, nan_point is NaN either way, stop_rho_zero and nbad_zero have no outlier for a gate or a kernel to treat differently.
MOVED = {
    'proj_double': _all_but('nan_point', 'n_zero'),
    'analytic_jacobian': _all_but('nan_point', 'n_zero'),
    'delta_1e6': _all_but('nan_point', 'n_zero'),
    'classify_accepted': [],
    'more_always_10': ['nbad_zero'],
    'more_always_5': _all_but('survive_0', 'survive_1', 'survive_9', 'nbad_zero', 'stop_rho_zero', 'stop_max_iter', 'n_65', 'n_zero', 'n_one'),
    'gate_and': _all_but('nbad_zero', 'stop_rho_zero', 'n_zero'),
    'huber_th2': _all_but('nbad_zero', 'stop_rho_zero', 'nan_point', 'n_zero'),
    'scale_free': _all_but('survive_0', 'survive_1', 'scale_free', 'stop_rho_zero', 'nan_point', 'scene_0', 'scene_1', 'scene_4', 'n_zero', 'n_one'),
    'inverse_forward': _all_but('n_zero'),
    'early_writes_s12': ['survive_0', 'survive_1', 'survive_9', 'stop_max_iter', 'n_one'],
    'lt10_before_removal': ['survive_0', 'survive_1', 'survive_9', 'stop_max_iter'],
}


def case_by_name(name):
    return CASES[NAMES.index(name)]


_CACHE = {}


def expected(case, mode):
    """computed once per case and mode, shared by the tests, never modified"""
    key = (case.name, mode)
    if key not in _CACHE:
        _CACHE[key] = optimize_sim3(case.problem, mode)
    return _CACHE[key]
