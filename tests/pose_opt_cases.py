"""Optimizer::PoseOptimization(Frame *) (src/Optimizer.cc:1656-1842) restated in fp64 numpy together with exactly the g2o and Sophus code it
runs, its plausible wrong forms behind a switch each, and constructed cases with a reach predicate each.  No device and no library:
tests/test_pose_opt_cases.py holds the cases to their claims, tests/test_gpu_pose_opt.py runs them on the GPU.

The reference's g2o needs Eigen, which is not available to this repository: this row is *parity unpinned*  and the
arithmetic below is what fixes it.  Where the reference leaves an evaluation order to Eigen's expression templates the restatement states one:

    p        = R(q) Xw + t as Eigen's Quaternion::_transformVector: uv = 2 (qv x Xw), p = (Xw + w uv) + qv x uv, then + t
    mono     e = obs - (p.xy / p.z * f + c)                              (project2d divides)
    stereo   e = obs - (p.x invz fx + cx, p.y invz fy + cy, u - bf invz), invz = float(1 / p.z)          (cam_project: `const float invz`)
    chi2     = sum_i e_i (s e_i), s = double(mvInvLevelSigma2[octave])
    Huber    delta = double(float(sqrt(5.991))) / double(float(sqrt(7.815))), dsqr = delta delta; e <= dsqr: (e, 1) else (2 sqrt(e) delta - dsqr, delta / sqrt(e))
    J        types_six_dof_expmap.cpp:347-377 term by term (invz = 1.0 / p.z, a double)
    per edge H_jk += sum_i J_ij ((rho1 s) J_ik),  g_j += rho1 (sum_i J_ij (s e_i)),  b = -g          (weight rho[1] only; rho1 = 1 without a kernel)
    LM       optimization_algorithm_levenberg.cpp:61-189 as written out in `_pose_opt`; the solver's x persists across trials, iterations and rounds
             (a failed solve leaves it stale; the reference never initialises it in a release build, the restatement starts it at zero)
    LDLT     Eigen's unblocked lower pivoted LDLT (largest |diagonal| first, the first on a tie; symmetric swap; t = D L_k^T, a_kk -= L_k t,
             column -= L t, column /= a_kk; dot products summed from their first term on); positive = every pivot > 0 (an all-zero matrix is
             not: Eigen 3.2's sign test); solve = P^T L^-T D^-1 L^-1 P b, each row's terms subtracted one after the other
    exp      Sophus SE3d::exp (epsilon 1e-10), `*` = fastMultiply + normalize, cast<double> / cast<float> normalise in the target type
    update   oplusImpl: exp(u[3..5], u[0..2]) * estimate

Two summation modes for H, g and the active chi2:
    reference  edges one after the other, the monocular list and then the stereo list (as the issue states g2o walks its active edges)
    device     frame index i belongs to thread i % 256, ascending i per thread; 64 lanes combined as a balanced tree of neighbours (lanes 2k, 2k+1,
               then pairs, quads, half rows, rows 0+1 and 2+3), the four waves in wave order: ((w0 + w1) + w2) + w3
"""
import collections
import math

import numpy as np

WRONG_FORMS = ("restart_prev_round", "no_outlier_reeval", "huber_round3", "gate_robust", "stereo_invz_double", "delta_double", "update_right",
               "update_no_swap", "lambda_carried", "break_counts_active", "few_writes_pose", "no_nbad_rule", "level1_in_system", "skip_behind")
# restart_prev_round    a round restarts from the previous round's pose (the reference: from pFrame->mTcw, every round)
# no_outlier_reeval     outlier edges keep the error of their last evaluation at the end of a round (the reference: computeError at the round's pose)
# huber_round3          the Huber kernel is kept in round 3 (the reference drops it for every edge after round index 2)
# gate_robust           the chi2 gate uses the robustified value (the reference: raw chi2() cast to float, `>` against float 5.991 / 7.815)
# stereo_invz_double    the stereo projection uses a double 1 / z
# delta_double          delta is a double sqrt(5.991) / sqrt(7.815)
# update_right          estimate * exp(u)
# update_no_swap        exp(u[0..5]) * estimate
# lambda_carried        lambda is not recomputed at iteration 0 of rounds 1..3
# break_counts_active   the `edges().size() < 10` break counts level-0 edges
# few_writes_pose       nInitialCorrespondences < 3 still writes the pose (through cast<double> and cast<float>: normalised)
# no_nbad_rule          the vendored stop rule is missing
# level1_in_system      level-1 edges still enter H, g and the active chi2
# skip_behind           points with z <= 0 are left out of the sums and count as outliers

STOP_MAX_ITER, STOP_TRIALS, STOP_RHO_ZERO, STOP_NBAD, STOP_NOT_RUN = 0, 1, 2, 3, 4
DBL_MAX = float(np.finfo(np.float64).max)
CHI2_MONO, CHI2_STEREO = np.float32(5.991), np.float32(7.815)
TAU, GOOD_UP, GOOD_LOW = 1e-5, 2.0 / 3.0, 1.0 / 3.0
MARGIN_MIN = 1e-6

# The largest difference between the double poses (7 numbers, quaternion sign aligned) of the two summation modes over all cases below, as
# tests/test_pose_opt_cases.py measures it on the CPU: what reordering the sums alone does to the reference's algorithm.  The GPU test allows
# the device 4 x this against the device-order restatement.  (The test asserts that the measured value does not exceed the constant and is
# within a factor 4 of it, so the constant cannot drift into a loose bound.)
EPS_ORDER = 1.6e-13   # measured 1.563e-13, at far_pose (a translation of ~150: five units in its last place); ~3e-16 on the ordinary scenes

Problem = collections.namedtuple("Problem", "xy octave u_right mp_valid world Tcw outlier_in cam inv_sigma2")
# cam: (fx, fy, cx, cy, bf) floats; u_right: None = all monocular; outlier_in: mvbOutlier before the call
Result = collections.namedtuple("Result", "Tcw Tcw64 outlier ret iters trials stop lam chi2 margin rounds")
Case = collections.namedtuple("Case", "name problem moved_by reach")


# ---- Sophus / Eigen pieces, fp64 (scalar code on 4- and 3-vectors) ------------------------------------------------------------------------------
def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_normalize(q):
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / n


def quat_rotate(q, v):
    """Eigen _transformVector; v: [..., 3]"""
    v = np.asarray(v)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    ux, uy, uz = q[1] * z - q[2] * y, q[2] * x - q[0] * z, q[0] * y - q[1] * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = q[1] * uz - q[2] * uy, q[2] * ux - q[0] * uz, q[0] * uy - q[1] * ux
    return np.stack([x + q[3] * ux + cx, y + q[3] * uy + cy, z + q[3] * uz + cz], -1)


def quat_to_R(q):
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def se3_exp(a, eps=1e-10):
    """Sophus SE3::exp of (upsilon, omega) -> (q, t) (se3.hpp:406-428, so3.hpp:425-456)"""
    a = np.asarray(a, np.float64)
    om = a[3:]
    theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    theta = np.sqrt(theta_sq)
    half = 0.5 * theta
    small = bool(theta < eps)
    if small:
        po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4
        real = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * po4
    else:
        imag = np.sin(half) / theta
        real = np.cos(half)
    q = quat_normalize(np.array([imag * om[0], imag * om[1], imag * om[2], real]))
    O = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]], np.float64)
    O2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            O2[i, j] = O[i, 0] * O[0, j] + O[i, 1] * O[1, j] + O[i, 2] * O[2, j]
    if small:
        V = quat_to_R(q)
    else:
        tsq = theta * theta
        c1 = (1.0 - np.cos(theta)) / tsq
        c2 = (theta - np.sin(theta)) / (tsq * theta)
        V = np.eye(3) + c1 * O + c2 * O2
    t = np.array([V[i, 0] * a[0] + V[i, 1] * a[1] + V[i, 2] * a[2] for i in range(3)])
    return q, t


def se3_mul(qa, ta, qb, tb):
    t = ta + quat_rotate(qa, tb)
    return quat_normalize(quat_mul(qa, qb)), t


def cast_double(T7):
    T = np.asarray(T7, np.float32).astype(np.float64)
    return quat_normalize(T[:4]), T[4:].copy()


def cast_float(q, t):
    qf = np.asarray(q, np.float64).astype(np.float32)
    n = np.sqrt(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3])
    return np.concatenate([qf / n, np.asarray(t, np.float64).astype(np.float32)]).astype(np.float32)


# ---- Eigen's pivoted LDLT, 6 x 6 -----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    s = None
    for x, y in zip(a, b):
        s = x * y if s is None else s + x * y
    return s


def ldlt(A):
    """-> (positive, L\\D in place (lower), transpositions, pivots)"""
    m = np.array(A, np.float64)
    n = m.shape[0]
    tr = list(range(n))
    for k in range(n):
        big, idx = -1.0, k
        for j in range(k, n):
            v = abs(m[j, j])
            if v > big:
                big, idx = v, j
        tr[k] = idx
        if idx != k:
            m[[k, idx], :k] = m[[idx, k], :k]
            for i in range(idx + 1, n):
                m[i, k], m[i, idx] = m[i, idx], m[i, k]
            m[k, k], m[idx, idx] = m[idx, idx], m[k, k]
            for i in range(k + 1, idx):
                m[i, k], m[idx, i] = m[idx, i], m[i, k]
        if k > 0:
            temp = [m[j, j] * m[k, j] for j in range(k)]
            m[k, k] = m[k, k] - _dot(m[k, :k], temp)
            for i in range(k + 1, n):
                m[i, k] = m[i, k] - _dot(m[i, :k], temp)
        for i in range(k + 1, n):
            m[i, k] = m[i, k] / m[k, k]
    piv = [float(m[k, k]) for k in range(n)]
    return all(p > 0 for p in piv), m, tr, piv


def ldlt_solve(m, tr, b):
    n = len(tr)
    x = [float(v) for v in b]
    for k in range(n):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(n):
        for j in range(i):
            x[i] = x[i] - m[i, j] * x[j]
    for i in range(n):
        x[i] = x[i] / m[i, i]
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            x[i] = x[i] - m[j, i] * x[j]
    for k in range(n - 1, -1, -1):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    return np.array(x)


# ---- the edges, vectorised over the correspondences ----------------------------------------------------------------------------------------------
class _Edges:
    def __init__(self, P, wrong):
        valid = np.asarray(P.mp_valid).astype(bool)
        self.idx = np.nonzero(valid)[0]
        self.n = len(valid)
        ur = np.full(self.n, -1.0, np.float32) if P.u_right is None else np.asarray(P.u_right, np.float32)
        self.stereo = ~(ur[self.idx] < 0)
        self.obs = np.stack([np.asarray(P.xy, np.float32)[self.idx, 0], np.asarray(P.xy, np.float32)[self.idx, 1], ur[self.idx]], -1).astype(np.float64)
        self.s = np.asarray(P.inv_sigma2, np.float32)[np.asarray(P.octave)[self.idx]].astype(np.float64)
        self.X = np.asarray(P.world, np.float32)[self.idx].astype(np.float64)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(np.float32(v)) for v in P.cam)
        dm, ds = (math.sqrt(5.991), math.sqrt(7.815)) if wrong == "delta_double" else (float(np.float32(math.sqrt(5.991))), float(np.float32(math.sqrt(7.815))))
        self.delta = np.where(self.stereo, ds, dm)
        self.dsqr = self.delta * self.delta
        self.gate = np.where(self.stereo, float(CHI2_STEREO), float(CHI2_MONO))
        self.wrong = wrong
        self.order_ref = np.concatenate([np.nonzero(~self.stereo)[0], np.nonzero(self.stereo)[0]])

    def errors(self, q, t):
        """-> p [m, 3], e [m, 3] (e[:, 2] = 0 for monocular edges), chi2 [m]"""
        p = quat_rotate(q, self.X) + t
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        with np.errstate(all="ignore"):
            m0 = self.obs[:, 0] - (x / z * self.fx + self.cx)
            m1 = self.obs[:, 1] - (y / z * self.fy + self.cy)
            invz = 1.0 / z if self.wrong == "stereo_invz_double" else (1.0 / z).astype(np.float32).astype(np.float64)
            r0 = x * invz * self.fx + self.cx
            s0 = self.obs[:, 0] - r0
            s1 = self.obs[:, 1] - (y * invz * self.fy + self.cy)
            s2 = self.obs[:, 2] - (r0 - self.bf * invz)
            e = np.stack([np.where(self.stereo, s0, m0), np.where(self.stereo, s1, m1), np.where(self.stereo, s2, 0.0)], -1)
            c01 = e[:, 0] * (self.s * e[:, 0]) + e[:, 1] * (self.s * e[:, 1])
            chi2 = np.where(self.stereo, c01 + e[:, 2] * (self.s * e[:, 2]), c01)
        return p, e, chi2

    def huber(self, chi2, kernel):
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            inl = chi2 <= self.dsqr
            rho0 = np.where(inl, chi2, 2 * sq * self.delta - self.dsqr)
            rho1 = np.where(inl, 1.0, self.delta / sq)
        if not kernel:
            return chi2, np.ones_like(chi2)
        return rho0, rho1

    def system_terms(self, p, e, chi2, kernel):
        """-> [m, 28]: the 21 upper entries of the edge's J^T W J (row-major, j <= k), its 6 entries of g, its robust chi2"""
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        fx, fy, bf = self.fx, self.fy, self.bf
        with np.errstate(all="ignore"):
            invz = 1.0 / z
            invz2 = invz * invz
            zero = np.zeros_like(x)
            J0 = [x * y * invz2 * fx, -(1 + (x * x * invz2)) * fx, y * invz * fx, -invz * fx, zero, x * invz2 * fx]
            J1 = [(1 + y * y * invz2) * fy, -x * y * invz2 * fy, -x * invz * fy, zero, -invz * fy, y * invz2 * fy]
            J2 = [J0[0] - bf * y * invz2, J0[1] + bf * x * invz2, J0[2], J0[3], zero, J0[5] - bf * invz2]
            rho0, rho1 = self.huber(chi2, kernel)
            w = rho1 * self.s
            cols = []
            for j in range(6):
                for k in range(j, 6):
                    a = J0[j] * (w * J0[k]) + J1[j] * (w * J1[k])
                    cols.append(np.where(self.stereo, a + J2[j] * (w * J2[k]), a))
            for j in range(6):
                a = J0[j] * (self.s * e[:, 0]) + J1[j] * (self.s * e[:, 1])
                cols.append(rho1 * np.where(self.stereo, a + J2[j] * (self.s * e[:, 2]), a))
            cols.append(rho0)
        return np.stack(cols, -1)

    def ordered_sum(self, vals, active, mode):
        """vals [m, k] summed over the active edges in the mode's order"""
        k = vals.shape[1]
        if mode == "reference":
            o = self.order_ref[active[self.order_ref]]
            if len(o) == 0:
                return np.zeros(k)
            with np.errstate(all="ignore"):
                return np.cumsum(vals[o], axis=0)[-1]
        assert mode == "device"
        rows = (self.n + 255) // 256
        arr = np.zeros((max(rows, 1) * 256, k))
        act = np.zeros(max(rows, 1) * 256, bool)
        arr[self.idx] = vals
        act[self.idx] = active
        arr, act = arr.reshape(-1, 256, k), act.reshape(-1, 256)
        acc = np.zeros((256, k))
        with np.errstate(all="ignore"):
            for r in range(arr.shape[0]):
                acc = np.where(act[r][:, None], acc + arr[r], acc)
            v = acc.reshape(4, 4, 16, k)
            for _ in range(4):
                v = v[:, :, 0::2] + v[:, :, 1::2]
            v = v[:, :, 0]
            w = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
            return ((w[0] + w[1]) + w[2]) + w[3]


def _rel(a, b):
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else math.inf


class _Margin:
    """the smallest relative distance of a branch operand from its branch point over a run (module docstring of the test: what counts)"""
    def __init__(self):
        self.v = math.inf
        self.where = None

    def note(self, v, where):
        if not (v >= self.v):   # NaN counts as no margin
            self.v = float(v) if v == v else 0.0
            self.where = where


def pose_opt(P, mode="reference", wrong=None):
    """The restatement.  -> Result; rounds: per round its trials (iteration, trial, rho, lambda, ...), its classification and its pose, for the
    reach predicates.  (Inf and NaN are values here, as they are on the device: no warnings.)"""
    with np.errstate(all="ignore"):
        return _pose_opt(P, mode, wrong)


def _pose_opt(P, mode, wrong):
    assert mode in ("reference", "device") and (wrong is None or wrong in WRONG_FORMS)
    E = _Edges(P, wrong)
    m = len(E.idx)
    outlier = np.asarray(P.outlier_in).astype(np.uint8).copy()
    outlier[E.idx] = 0
    Tin = np.asarray(P.Tcw, np.float32)
    iters, trials, stop = [0] * 4, [0] * 4, [STOP_NOT_RUN] * 4
    lam_out, chi_out = [0.0] * 4, [0.0] * 4
    M = _Margin()
    trace = []
    if m < 3:
        T32, T64 = Tin.copy(), Tin.astype(np.float64)
        if wrong == "few_writes_pose":
            q, t = cast_double(Tin)
            T32, T64 = cast_float(q, t), np.concatenate([q, t])
        return Result(T32, T64, outlier, 0, iters, trials, stop, lam_out, chi_out, math.inf, trace)
    q0, t0 = cast_double(Tin)
    q, t = q0, t0
    level1 = np.zeros(m, bool)         # e->level() == 1
    kernel = True
    stored = np.full(m, np.nan)        # chi2 of every edge's _error member: written by round 0 before anything reads it
    x = np.zeros(6)
    lam, ni = -1.0, 2.0
    nBad = 0
    for rnd in range(4):
        if not (wrong == "restart_prev_round" and rnd > 0):
            q, t = q0, t0
        active = np.ones(m, bool) if wrong == "level1_in_system" else ~level1
        rtrace = []

        def behind_mask(p):
            return active & (p[:, 2] > 0) if wrong == "skip_behind" else active
        nbad_rule = 0
        reason = STOP_MAX_ITER
        for it in range(10):
            p, e, chi2 = E.errors(q, t)
            stored = np.where(active, chi2, stored)
            act = behind_mask(p)
            S = E.ordered_sum(E.system_terms(p, e, chi2, kernel), act, mode)
            H = np.zeros((6, 6))
            c = 0
            for j in range(6):
                for k in range(j, 6):
                    H[j, k] = H[k, j] = S[c]
                    c += 1
            b = -S[21:27]
            currentChi = float(S[27])
            iniChi = currentChi
            if it == 0:
                if not (wrong == "lambda_carried" and rnd > 0):
                    md = 0.0
                    for j in range(6):          # std::max(fabs(H_jj), maxDiagonal): (a < b) ? b : a
                        v = abs(H[j, j])
                        md = md if v < md else v
                    lam = TAU * md
                ni = 2.0
                nbad_rule = 0
            rho = 0.0
            qmax = 0
            while True:
                qb, tb = q, t
                Hd = H.copy()
                for j in range(6):
                    Hd[j, j] = H[j, j] + lam
                ok, Lm, tr, piv = ldlt(Hd)
                dmax = max(abs(Hd[j, j]) for j in range(6))
                if dmax > 0 and np.all(np.isfinite(Hd)):   # (an all-zero or non-finite matrix fails in any summation order)
                    M.note(min(abs(v) for v in piv) / dmax, ("pivot", rnd, it, qmax))
                if ok:
                    x = ldlt_solve(Lm, tr, b)
                u = x if wrong == "update_no_swap" else np.concatenate([x[3:], x[:3]])
                qe, te = se3_exp(u)
                q, t = se3_mul(q, t, qe, te) if wrong == "update_right" else se3_mul(qe, te, q, t)
                p2, e2, chi2b = E.errors(q, t)
                stored = np.where(active, chi2b, stored)
                r0, _ = E.huber(chi2b, kernel)
                tempChi = float(E.ordered_sum(r0[:, None], behind_mask(p2), mode)[0])
                if not ok:
                    tempChi = DBL_MAX
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                with np.errstate(all="ignore"):
                    rho = float(np.float64(currentChi - tempChi) / np.float64(scale))
                moved = not (np.array_equal(q, qb) and np.array_equal(t, tb))
                # rho is a ratio already -- the decrease over the predicted decrease + 1e-3 -- so its distance from 0 is |rho|.  Not counted: an
                # update that leaves the pose as it was (tempChi == currentChi in any order: rho == 0 by construction) and non-finite operands
                # (Inf and NaN propagate through every order alike)
                if (moved or not ok) and math.isfinite(currentChi) and math.isfinite(rho):
                    M.note(abs(rho), ("rho", rnd, it, qmax))
                good = rho > 0 and math.isfinite(tempChi)
                rtrace.append(dict(it=it, trial=qmax, ok=ok, rho=rho, lam=lam, ni=ni, good=good, chi=currentChi, temp=tempChi, nactive=int(act.sum())))
                if good:
                    with np.errstate(all="ignore"):
                        alpha = 1.0 - float(np.power(np.float64(2 * rho - 1), 3.0))   # pow(2 rho - 1, 3)
                    alpha = min(alpha, GOOD_UP)
                    lam *= max(GOOD_LOW, alpha)
                    ni = 2.0
                    currentChi = tempChi
                else:
                    lam *= ni
                    ni *= 2
                    q, t = qb, tb
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            iters[rnd] += 1
            trials[rnd] += qmax
            if qmax == 10 or rho == 0:
                reason = STOP_TRIALS if qmax == 10 else STOP_RHO_ZERO
                break
            lhs = (iniChi - currentChi) * 1e3
            if math.isfinite(lhs) and math.isfinite(iniChi):
                M.note(_rel(lhs, iniChi), ("stop", rnd, it))
            if lhs < iniChi:
                nbad_rule += 1
            else:
                nbad_rule = 0
            if nbad_rule >= 3 and wrong != "no_nbad_rule":
                reason = STOP_NBAD
                break
        stop[rnd] = reason
        lam_out[rnd], chi_out[rnd] = lam, currentChi
        # the classification (Optimizer.cc:1783-1830)
        pf, ef, chif = E.errors(q, t)
        if wrong != "no_outlier_reeval":
            stored = np.where(level1, chif, stored)
        gate_val = stored
        if wrong == "gate_robust":
            gate_val = E.huber(stored, kernel)[0]
        with np.errstate(all="ignore"):
            gm = np.abs(gate_val - E.gate) / E.gate
            M.note(float(np.min(np.where(np.isfinite(gate_val), gm, np.inf))), ("gate", rnd))
            bad = gate_val.astype(np.float32) > E.gate.astype(np.float32)
        if wrong == "skip_behind":
            bad = bad | ~(pf[:, 2] > 0)
        level1 = bad.copy()
        outlier[E.idx] = bad
        nBad = int(bad.sum())
        if rnd == 2 and wrong != "huber_round3":
            kernel = False
        trace.append(dict(trials=rtrace, bad=bad.copy(), q=q, t=t))
        if (int((~level1).sum()) if wrong == "break_counts_active" else m) < 10:
            break
    return Result(cast_float(q, t), np.concatenate([q, t]), outlier, m - nBad, iters, trials, stop, lam_out, chi_out, M.v, trace)


def pose_diff(a, b):
    """largest difference of two 7-number poses, the quaternions' signs aligned"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sgn = -1.0 if float(np.dot(a[:4], b[:4])) < 0 else 1.0
    return float(max(np.max(np.abs(a[:4] - sgn * b[:4])), np.max(np.abs(a[4:] - b[4:]))))


def decisions(r):
    return (r.outlier.tobytes(), r.ret, tuple(r.iters), tuple(r.trials), tuple(r.stop))


def same_result(a, b):
    return decisions(a) == decisions(b) and np.array_equal(a.Tcw64, b.Tcw64) and np.array_equal(a.Tcw, b.Tcw)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
# moved_by: the wrong forms under which the restatement gives another result for this case (every other form must give the same one: flags, ret,
#           per-round counts and both poses, bit for bit).  Recorded from the restatement, as the margins are; tests/test_pose_opt_cases.py holds
#           the table to it in both directions.
# reach:    what the case is there for, as a predicate on (problem, reference-order result).
EUROC = (458.654, 457.296, 367.215, 248.375, 47.90639384423901)
INV_SIGMA2 = (1.0 / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)


def scene(seed, n, frac_out=0.0, stereo=0.5, noise=1.0, dpose=0.05, zlo=2.0, zhi=10.0, octaves=(0, 8), rot=0.3, trans=1.0, valid=1.0, cam=EUROC):
    """n keypoints seen from a seeded pose: observations = projections + noise (in pixels of the keypoint's level), a fraction replaced by
    gross outliers, a fraction `stereo` with a right coordinate, the frame's pose the true one moved by a seeded twist of size dpose."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy, bf = cam
    q, t = se3_exp(np.concatenate([rs.uniform(-trans, trans, 3), rs.uniform(-rot, rot, 3)]))
    u, v, z = rs.uniform(20, 732, n), rs.uniform(20, 460, n), rs.uniform(zlo, zhi, n)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    world = quat_rotate(np.array([-q[0], -q[1], -q[2], q[3]]), pc - t).astype(np.float32)
    octave = rs.randint(octaves[0], octaves[1], n)
    sc = 1.2 ** octave
    xy = np.stack([u, v], -1) + rs.normal(0, noise, (n, 2)) * sc[:, None]
    ur = u - bf / z + rs.normal(0, noise, n) * sc
    out = rs.rand(n) < frac_out
    xy[out] = np.stack([rs.uniform(0, 752, int(out.sum())), rs.uniform(0, 480, int(out.sum()))], -1)
    ur = np.where(rs.rand(n) < stereo, ur, -1.0)
    d = rs.normal(0, dpose, 6)
    d[3:] *= 0.3
    qe, te = se3_exp(d)
    q1, t1 = se3_mul(qe, te, q, t)
    mp_valid = (rs.rand(n) < valid).astype(np.uint8)
    return Problem(xy.astype(np.float32), octave.astype(np.int32), None if stereo == 0 else ur.astype(np.float32), mp_valid, world, cast_float(q1, t1),
                   (rs.rand(n) < 0.5).astype(np.uint8), cam, INV_SIGMA2)


def _edges_of(P):
    return _Edges(P, None)


def _count(P):
    return int(np.asarray(P.mp_valid).astype(bool).sum())


def r_count(k):
    def reach(P, r):
        if _count(P) != k:
            return False
        if k < 3:
            return r.ret == 0 and r.stop == [STOP_NOT_RUN] * 4 and np.array_equal(r.Tcw, np.asarray(P.Tcw, np.float32))
        if k < 10:
            return r.stop[0] != STOP_NOT_RUN and r.stop[1:] == [STOP_NOT_RUN] * 3
        return STOP_NOT_RUN not in r.stop
    return reach


def r_kinds(mono, stereo):
    def reach(P, r):
        E = _edges_of(P)
        ok = bool((~E.stereo).any()) == mono and bool(E.stereo.any()) == stereo
        if mono and stereo:   # interleaved in index order: both kinds on both sides of the middle
            h = len(E.stereo) // 2
            ok = ok and E.stereo[:h].any() and (~E.stereo[:h]).any() and E.stereo[h:].any() and (~E.stereo[h:]).any()
        return ok
    return reach


def r_round0_rejects(P, r):
    b = [x["bad"] for x in r.rounds]
    return len(b) == 4 and b[0].sum() >= 5 and all(np.array_equal(b[0], x) for x in b[1:])


def r_readmitted(P, r):
    b = [x["bad"] for x in r.rounds]
    return any((b[i] & ~b[j]).any() for i in range(len(b)) for j in range(i + 1, len(b)))


def r_side_change_23(P, r):
    b = [x["bad"] for x in r.rounds]
    return len(b) == 4 and bool((b[2] != b[3]).any())


def r_empty_round(P, r):
    for x in r.rounds[1:]:
        tr = x["trials"]
        if len(tr) == 10 and all(e["nactive"] == 0 and not e["ok"] and e["temp"] == DBL_MAX for e in tr) and tr[-1]["trial"] == 9:
            return STOP_TRIALS in r.stop
    return False


def r_reject_then_accept(P, r):
    """a rejected trial, a second one and an accepted one in one iteration: lambda x 2, x 4, then ni back at 2"""
    for x in r.rounds:
        tr = x["trials"]
        for i in range(len(tr) - 3):
            a, b, c, d = tr[i:i + 4]
            if a["trial"] == 0 and not a["good"] and a["ok"] and not b["good"] and c["good"] and c["it"] == a["it"] and b["lam"] == a["lam"] * 2 and c["lam"] == b["lam"] * 4 \
                    and (a["ni"], b["ni"], c["ni"], d["ni"]) == (2, 4, 8, 2):
                return True
    return False


def r_stop(reason):
    return lambda P, r: reason in r.stop


def r_rho_zero(P, r):
    return r.stop[0] == STOP_RHO_ZERO and r.trials[0] == 1 and r.ret == _count(P)


def r_behind(P, r):
    E = _edges_of(P)
    z = (quat_rotate(r.Tcw64[:4], E.X) + r.Tcw64[4:])[:, 2]
    return bool(((z < 0) & (r.outlier[E.idx] == 0)).any())


def r_nonfinite(P, r):
    tr = r.rounds[0]["trials"]
    return any(not math.isfinite(e["chi"]) for e in tr) and np.all(np.isfinite(r.Tcw64)) and r.rounds[0]["bad"].sum() >= 1 and r.stop[0] == STOP_MAX_ITER


def r_octave(o):
    return lambda P, r: bool((np.asarray(P.octave) == o).all()) and STOP_NOT_RUN not in r.stop


def r_far(P, r):
    T = r.Tcw64
    return abs(T[3]) < 0.5 and np.max(np.abs(T[4:])) > 50 and r.ret > 0.7 * _count(P)


def r_scene(lo, hi):
    def reach(P, r):
        n = _count(P)
        return 100 <= n <= 1500 and lo <= 1 - r.ret / n <= hi + 0.1
    return reach


def _few(n_valid, seed):
    """n_valid correspondences among 40 keypoints; the pose's quaternion is 0.1 % off unit length (a call that returns early leaves it so)"""
    P = scene(seed, 40, stereo=0.5, valid=0.0)
    v = np.zeros(40, np.uint8)
    v[np.random.RandomState(seed).permutation(40)[:n_valid]] = 1
    T = np.asarray(P.Tcw, np.float32).copy()
    T[:4] *= np.float32(1.001)
    return P._replace(mp_valid=v, Tcw=T)


def _exact(n=12):
    """identity pose, power-of-two camera, points whose projections are integers: every error is exactly 0, the first update is exactly 0"""
    cam = (512.0, 512.0, 256.0, 256.0, 64.0)
    k = np.arange(n)
    z = np.where(k % 2 == 0, 4.0, 8.0)
    world = np.stack([((k % 5) - 2) / 8.0 * z, ((k % 3) - 1) / 8.0 * z + (k // 6) / 16.0 * z, z], -1).astype(np.float32)
    u, v = world[:, 0] / world[:, 2] * 512 + 256, world[:, 1] / world[:, 2] * 512 + 256
    ur = np.where(k % 3 == 0, u - 64.0 / world[:, 2], -1.0)
    return Problem(np.stack([u, v], -1).astype(np.float32), (k % 8).astype(np.int32), ur.astype(np.float32), np.ones(n, np.uint8), world,
                   np.array([0, 0, 0, 1, 0, 0, 0], np.float32), np.ones(n, np.uint8), cam, INV_SIGMA2)


def _behind(seed):
    """a clean scene plus one monocular point mirrored through the camera centre: z < 0, and its projection still falls on its keypoint"""
    P = scene(seed, 30, stereo=0.5, noise=0.3, dpose=0.01)
    ur = np.asarray(P.u_right, np.float32).copy()
    ur[0] = -1.0
    P = P._replace(u_right=ur)
    E = _edges_of(P)
    q, t = cast_double(P.Tcw)
    pc = quat_rotate(q, E.X[0]) + t
    w = np.asarray(P.world, np.float32).copy()
    w[0] = quat_rotate(np.array([-q[0], -q[1], -q[2], q[3]]), -pc - t).astype(np.float32)
    return P._replace(world=w)


def _in_camera_plane(seed):
    """a clean scene at the identity pose plus one point with z == 0 exactly: an infinite chi2 from finite inputs"""
    P = scene(seed, 24, stereo=0.5, noise=0.5, dpose=0.0, rot=0.0, trans=0.0)
    w = np.asarray(P.world, np.float32).copy()
    w[5] = (1.0, 0.5, 0.0)
    return P._replace(world=w, Tcw=np.array([0, 0, 0, 1, 0, 0, 0], np.float32))


def _garbage(seed, n=12):
    P = scene(seed, n, frac_out=1.0, stereo=0.5)
    return P


def _far(seed):
    P = scene(seed, 200, frac_out=0.1, rot=0.0, trans=0.0)
    # the same scene seen from a pose far from the identity: world' = A^-1 world, Tcw' = Tcw A
    qa, ta = se3_exp(np.array([80.0, -60.0, 120.0, 1.9, -1.4, 0.9]))
    q, t = cast_double(P.Tcw)
    q2, t2 = se3_mul(q, t, qa, ta)
    qi = np.array([-qa[0], -qa[1], -qa[2], qa[3]])
    w = quat_rotate(qi, np.asarray(P.world, np.float64) - ta).astype(np.float32)
    return P._replace(world=w, Tcw=cast_float(q2, t2))


SPECS = [   # name, builder(seed), seed, reach
    ("n2", lambda s: _few(2, s), 1, r_count(2)),
    ("n3", lambda s: _few(3, s), 1001, r_count(3)),
    ("n9", lambda s: _few(9, s), 2008, r_count(9)),
    ("n10", lambda s: scene(s, 10, stereo=0.5), 3001, r_count(10)),
    ("n63", lambda s: scene(s, 63, frac_out=0.1), 4001, r_count(63)),
    ("n64", lambda s: scene(s, 64, frac_out=0.1), 5001, r_count(64)),
    ("n65", lambda s: scene(s, 65, frac_out=0.1), 6043, r_count(65)),
    ("n255", lambda s: scene(s, 255, frac_out=0.1), 7008, r_count(255)),
    ("n256", lambda s: scene(s, 256, frac_out=0.1), 8001, r_count(256)),
    ("n257", lambda s: scene(s, 257, frac_out=0.1), 9001, r_count(257)),
    ("n2049", lambda s: scene(s, 2049, frac_out=0.15), 10057, r_count(2049)),
    # (monocular residuals are smooth down to rounding: a run that converges takes its last decisions inside the noise, so this one starts far away
    # and every round ends at the iteration limit instead)
    ("mono_only", lambda s: scene(s, 150, frac_out=0.1, stereo=0.0, dpose=1.0), 9, r_kinds(True, False)),
    ("stereo_only", lambda s: scene(s, 150, frac_out=0.1, stereo=1.0), 12001, r_kinds(False, True)),
    ("interleaved", lambda s: scene(s, 150, frac_out=0.1, stereo=0.5, valid=0.7), 13015, r_kinds(True, True)),
    ("round0_rejects", lambda s: scene(s, 120, frac_out=0.15, noise=0.3, dpose=0.01), 14001, r_round0_rejects),
    ("readmitted", lambda s: scene(s, 300, frac_out=0.3, dpose=0.15), 15022, r_readmitted),
    ("side_change_23", lambda s: scene(s, 600, frac_out=0.2, noise=1.3), 16043, r_side_change_23),
    ("empty_round", lambda s: _garbage(s), 17001, r_empty_round),
    ("reject_then_accept", lambda s: scene(s, 200, frac_out=0.2, dpose=0.25, zlo=1.0, zhi=4.0), 18890, r_reject_then_accept),
    ("nbad_stop", lambda s: scene(s, 100, frac_out=0.2), 19015, r_stop(STOP_NBAD)),
    ("rho_zero", lambda s: _exact(), 0, r_rho_zero),
    ("behind_camera", _behind, 21001, r_behind),
    ("in_camera_plane", _in_camera_plane, 22008, r_nonfinite),
    ("octave0", lambda s: scene(s, 100, frac_out=0.1, octaves=(0, 1)), 23015, r_octave(0)),
    ("octave7", lambda s: scene(s, 100, frac_out=0.1, octaves=(7, 8)), 24001, r_octave(7)),
    ("far_pose", _far, 25022, r_far),
]
# a dozen seeded scenes: correspondences, outlier fraction, seed (the seeds: the first of a fixed sequence whose scene keeps the margin)
_SCENES = [(117, 0.10, 26008), (342, 0.25, 27008), (611, 0.40, 28008), (905, 0.15, 29036), (1203, 0.30, 30015), (1500, 0.20, 31001), (100, 0.35, 32001), (480, 0.12, 33015), (760, 0.22, 34001),
           (1050, 0.38, 35001), (1333, 0.17, 36015), (222, 0.28, 37015)]
for _i, (_n, _f, _s) in enumerate(_SCENES):
    SPECS.append(("scene%02d_n%d" % (_i, _n), (lambda n, f: lambda s: scene(s, n, frac_out=f))(_n, _f), _s, r_scene(0.10, 0.40)))

# gate_robust moves no case, and cannot: Huber's rho(e) = 2 sqrt(e) delta - delta^2 crosses delta^2 exactly where e does, and delta^2 is the gate
# (5.991 / 7.815) up to float rounding -- the two forms differ only inside a band of 1e-7 around the gate, which the decision margin excludes.
MOVED_BY = {
    "n2": ("few_writes_pose",),
    "n3": ("stereo_invz_double", "delta_double", "update_right", "update_no_swap", "no_nbad_rule",),
    "n9": ("stereo_invz_double", "delta_double", "update_right", "update_no_swap", "no_nbad_rule",),
    "n10": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule",),
    "n63": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n64": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n65": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n255": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n256": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n257": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "n2049": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "delta_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "mono_only": ("restart_prev_round", "huber_round3", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "stereo_only": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "interleaved": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "round0_rejects": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "readmitted": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "side_change_23": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "empty_round": ("restart_prev_round", "update_right", "update_no_swap", "lambda_carried", "break_counts_active", "no_nbad_rule", "level1_in_system",),
    "reject_then_accept": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "nbad_stop": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "rho_zero": (),
    "behind_camera": ("restart_prev_round", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "skip_behind",),
    "in_camera_plane": ("restart_prev_round", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system", "skip_behind",),
    "octave0": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "octave7": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "far_pose": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene00_n117": ("restart_prev_round", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene01_n342": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene02_n611": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene03_n905": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene04_n1203": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene05_n1500": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene06_n100": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene07_n480": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene08_n760": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene09_n1050": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene10_n1333": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
    "scene11_n222": ("restart_prev_round", "no_outlier_reeval", "huber_round3", "stereo_invz_double", "update_right", "update_no_swap", "lambda_carried", "no_nbad_rule", "level1_in_system",),
}

_CASES, _RESULTS = [], {}


def cases():
    if not _CASES:
        for name, build, seed, reach in SPECS:
            _CASES.append(Case(name, build(seed), MOVED_BY.get(name, ()), reach))
    return _CASES


def case_by_name(name):
    return next(c for c in cases() if c.name == name)


def expected(case, mode="reference", wrong=None):
    """the restatement's result for a case, computed once per (case, mode, wrong form) and shared"""
    key = (case.name, mode, wrong)
    if key not in _RESULTS:
        _RESULTS[key] = pose_opt(case.problem, mode, wrong)
    return _RESULTS[key]
