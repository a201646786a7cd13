"""csrc/lm_math.h -- the Levenberg solver k_pose_opt (N = 6) and k_sim3_opt (N = 7) share -- as a plain host program (tests/cpp/lm_host.cc), built
with -fsanitize=address,undefined and -ffp-contract=off.  For both sizes: the pivoted LDLT and its solve on constructed matrices equal
tests/pose_opt_cases.ldlt / ldlt_solve bit for bit (NaN equal to NaN), each matrix first held in numpy to the property it is named after; the
bookkeeping (iteration_begin, trial_end, iteration_end) on scripted sequences equals `lm_script` below, the arithmetic both case modules spell
inside their Levenberg loops (alpha as tests/sim3_opt_cases.py and the kernels write it: 1 - c c c)."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import pose_opt_cases as PC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")
F = np.float64
SIZES = (6, 7)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_host") / "lm_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lm_host.cc"), "-o", exe])
    return exe


def bits(v):
    return " ".join("%016x" % int(x) for x in np.atleast_1d(np.asarray(v, F)).ravel().view(np.uint64))


def unbits(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(F)


def same_bits(a, b):
    a, b = np.asarray(a, F).ravel(), np.asarray(b, F).ravel()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def run(prog, mode, n, text):
    r = subprocess.run([prog, mode, str(n)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


# ---- the factorisation and the solve --------------------------------------------------------------------------------------------------------------
def spd(n, seed):
    m = np.random.RandomState(seed).uniform(-1, 1, (n, n))
    return m @ m.T + n * np.eye(n)


def _with_diag(A, places):
    A = A.copy()
    for j, v in places:
        A[j, j] = v
    return A


def _swap_loops(n, k, idx):
    """how often each of ldlt's four swap loops runs at step k with pivot idx: the row heads, the column tails, the diagonal, the part between"""
    return (k, n - 1 - idx, 1, idx - k - 1) if idx != k else (0, 0, 0, 0)


# name -> (matrix(n), lambda, the property of (n, H, lambda, ok, factor, transpositions) the input is named after)
SOLVE_CASES = {
    "a_spd": (lambda n: spd(n, 10 + n), 0.0, lambda n, H, lam, ok, m, tr: ok and np.all(np.linalg.eigvalsh(H) > 0)),
    "b_largest_last": (lambda n: _with_diag(spd(n, 20 + n), [(n - 1, 100.0)]), 0.0,
                       lambda n, H, lam, ok, m, tr: tr[0] == n - 1 and _swap_loops(n, 0, tr[0]) == (0, 0, 1, n - 2)),
    "c_largest_next": (lambda n: _with_diag(spd(n, 30 + n), [(1, 100.0)]), 0.0, lambda n, H, lam, ok, m, tr: tr[0] == 1 and _swap_loops(n, 0, 1)[3] == 0),
    "d_tie_first_wins": (lambda n: _with_diag(spd(n, 40 + n), [(2, 100.0), (4, -100.0)]), 0.0, lambda n, H, lam, ok, m, tr: abs(H[2, 2]) == abs(H[4, 4]) == np.max(np.abs(np.diag(H))) and tr[0] == 2),
    "e_indefinite": (lambda n: _with_diag(spd(n, 50 + n), [(3, -5.0)]), 0.0, lambda n, H, lam, ok, m, tr: not ok and np.all(np.isfinite(m)) and np.min(np.linalg.eigvalsh(H)) < 0),
    "f_zero": (lambda n: np.zeros((n, n)), 0.0, lambda n, H, lam, ok, m, tr: not ok and np.all(np.isnan(m[np.tril_indices(n, -1)]))),
    "g_nan_inf": (lambda n: _with_diag(spd(n, 60 + n), [(1, np.nan), (4, np.inf)]), 0.0, lambda n, H, lam, ok, m, tr: not ok and tr[0] == 4 and np.isnan(H[1, 1])),
    "h_huge_lambda": (lambda n: spd(n, 70 + n), 1e30,
                      lambda n, H, lam, ok, m, tr: ok and all(H[j, j] + lam == lam for j in range(n)) and list(tr) == list(range(n)) and np.max(np.abs(m[np.tril_indices(n, -1)])) < 1e-28),
}


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
@pytest.mark.parametrize("n", SIZES)
def test_ldlt_and_solve(prog, n, name):
    build, lam, prop = SOLVE_CASES[name]
    H = np.asarray(build(n), F)
    rs = np.random.RandomState(n)
    b, x0 = rs.uniform(-1, 1, n), rs.uniform(1, 2, n)
    with np.errstate(all="ignore"):
        Hd = H.copy()
        for j in range(n):
            Hd[j, j] = H[j, j] + F(lam)
        ok, m, tr, _ = PC.ldlt(Hd)
        x_any = PC.ldlt_solve(m, tr, b)
        assert prop(n, H, F(lam), ok, m, tr), "the input does not have the property it is named after"
    x_trial = x_any if ok else x0          # a failed solve leaves x as it was
    out = run(prog, "solve", n, " ".join([bits(H), bits(b), bits(lam), bits(x0)])).split("|")
    assert len(out) == 5
    assert int(out[0]) == int(ok)
    assert [int(v) for v in out[1].split()] == list(tr)
    assert same_bits(unbits(out[2].split()), m), "the factor differs from tests/pose_opt_cases.ldlt in some bit"
    assert same_bits(unbits(out[3].split()), x_trial), "x after trial_solve differs in some bit"
    assert same_bits(unbits(out[4].split()), x_any), "ldlt_solve differs from tests/pose_opt_cases.ldlt_solve in some bit"


# ---- the bookkeeping ------------------------------------------------------------------------------------------------------------------------------
def lm_script(n, script):
    """optimization_algorithm_levenberg.cpp:61-189 around the solve.  -> (the program's output lines, what each trial / end was)"""
    lam, ni, cur, ini, rho, qmax, nbad, b = F(-1.0), F(2.0), F(0.0), F(0.0), F(0.0), 0, 0, None
    lines, seen = [], []
    with np.errstate(all="ignore"):
        for cmd in script:
            if cmd[0] == "begin":
                _, first, chi2, upper, b = cmd
                H = np.zeros((n, n))
                H[np.triu_indices(n)] = upper
                H = np.triu(H) + np.triu(H, 1).T
                cur = ini = F(chi2)
                if first:
                    md = F(0.0)
                    for j in range(n):      # std::max(fabs(H_jj), maxDiagonal): (a < b) ? b : a
                        v = abs(H[j, j])
                        md = md if v < md else v
                    lam, ni, nbad = F(1e-5) * md, F(2.0), 0
                rho, qmax = F(0.0), 0
                tail = bits(H) + " " + bits(b)
            elif cmd[0] == "trial":
                _, ok, temp, x = cmd
                temp = F(temp) if ok else F(PC.DBL_MAX)
                scale = F(0.0)
                for j in range(n):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + F(1e-3)
                rho = (cur - temp) / scale
                good = bool(rho > 0) and math.isfinite(temp)
                if good:
                    c3 = 2 * rho - 1
                    alpha = F(1.0) - c3 * c3 * c3
                    seen.append("alpha_low" if alpha < F(1.0) / F(3.0) else "alpha_high" if F(2.0) / F(3.0) < alpha else "alpha_mid")
                    alpha = F(2.0) / F(3.0) if F(2.0) / F(3.0) < alpha else alpha
                    lam = lam * (alpha if F(1.0) / F(3.0) < alpha else F(1.0) / F(3.0))
                    ni, cur = F(2.0), temp
                else:
                    seen.append("failed_solve" if not ok else "inf_rho_positive" if (rho > 0 and math.isinf(temp)) else "rho_zero" if rho == 0 else "rejected")
                    lam, ni = lam * ni, ni * 2
                qmax += 1
                tail = "%d %d" % (not good, bool(rho < 0) and qmax < 10)
            else:
                stop = -1
                if qmax == 10 or rho == 0:
                    stop = PC.STOP_TRIALS if qmax == 10 else PC.STOP_RHO_ZERO
                else:
                    nbad = nbad + 1 if (ini - cur) * F(1e3) < ini else 0
                    if nbad >= 3:
                        stop = PC.STOP_NBAD
                seen.append(("stop", stop))
                tail = "%d" % stop
            lines.append("%d %d | %s | %s" % (qmax, nbad, bits([lam, ni, cur, ini, rho]), tail))
    return lines, seen


class _Script:
    """a scripted sequence, built against the restatement's own state: a trial is asked for by the rho it should come out near"""
    def __init__(self, n, seed):
        self.n, self.rs, self.cmds = n, np.random.RandomState(seed), []

    def begin(self, first, chi2=100.0):
        n = self.n
        upper = self.rs.uniform(0.5, 4.0, n * (n + 1) // 2)
        self.b = self.rs.uniform(1.0, 2.0, n)
        self.cur = F(chi2) if not self.cmds else self._state()[2]
        self.cmds.append(("begin", first, self.cur, upper, self.b))
        return self

    def _state(self):
        return unbits(lm_script(self.n, self.cmds)[0][-1].split("|")[1].split())   # lambda ni currentChi iniChi rho

    def trial(self, rho, x=0.5, ok=True, temp=None):
        lam, _, cur = self._state()[:3]
        xs = np.full(self.n, F(x))
        scale = F(0.0)
        for j in range(self.n):
            scale = scale + xs[j] * (lam * xs[j] + self.b[j])
        scale = scale + F(1e-3)
        self.cmds.append(("trial", ok, cur - F(rho) * scale if temp is None else F(temp), xs))
        return self

    def end(self):
        self.cmds.append(("end",))
        return self

    def text(self):
        out = []
        for c in self.cmds:
            if c[0] == "begin":
                out.append("begin %d %s %s %s" % (c[1], bits(c[2]), bits(c[3]), bits(c[4])))
            elif c[0] == "trial":
                out.append("trial %d %s %s" % (c[1], bits(c[2]), bits(c[3])))
            else:
                out.append("end")
        return "\n".join(out) + "\n"


def _sequences(n):
    """name -> (script, what the restatement must have met on the way)"""
    T, R, NB = ("stop", PC.STOP_TRIALS), ("stop", PC.STOP_RHO_ZERO), ("stop", PC.STOP_NBAD)
    go = ("stop", -1)
    s = {}
    # accepted steps, alpha at each clamp: rho near 0.97 (alpha < 1/3), 0.9 (between), 0.5 (alpha = 1 > 2/3)
    s["alpha_clamps"] = (_Script(n, 1).begin(1).trial(0.97).end().begin(0).trial(0.9).end().begin(0).trial(0.5).end(), ["alpha_low", go, "alpha_mid", go, "alpha_high", go])
    # a rejected step (lambda x 2, ni 4), a second one (x 4, ni 8), then an accepted one puts ni back; a new optimize() call recomputes lambda
    s["reject_then_accept"] = (_Script(n, 2).begin(1).trial(-0.3).trial(-2.0).trial(0.6).end().begin(1).trial(0.6).end(), ["rejected", "rejected", "alpha_high", go, "alpha_high", go])
    # tempChi = Inf beside a negative scale (x against b): rho = +Inf > 0 and the step is still rejected, no further trial
    s["inf_rho_positive"] = (_Script(n, 3).begin(1).trial(0.0, x=-0.5, temp=np.inf).end(), ["inf_rho_positive", go])
    # a failed solve: tempChi is DBL_MAX whatever the pass summed, and another trial follows
    s["failed_solve"] = (_Script(n, 4).begin(1).trial(0.0, ok=False, temp=1.0).trial(0.8).end(), ["failed_solve", "alpha_high", go])
    sc = _Script(n, 5).begin(1)
    for _ in range(10):
        sc.trial(-1.0)
    s["ten_rejections"] = (sc.end(), ["rejected"] * 10 + [T])
    s["rho_zero"] = (_Script(n, 6).begin(1).trial(0.0).end(), ["rho_zero", R])
    # (iniChi - currentChi) 1e3 < iniChi twice, a step that clears the count, then three times in a row
    sc = _Script(n, 7).begin(1).trial(0.5, x=0.01).end().begin(0).trial(0.5, x=0.01).end().begin(0).trial(0.97, x=0.5).end()
    for _ in range(3):
        sc.begin(0).trial(0.5, x=0.01).end()
    s["nbad_three_in_a_row"] = (sc, ["alpha_high", go, "alpha_high", go, "alpha_low", go, "alpha_high", go, "alpha_high", go, "alpha_high", NB])
    return s


SEQUENCE_NAMES = sorted(_sequences(6))


@pytest.mark.parametrize("name", SEQUENCE_NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_bookkeeping(prog, n, name):
    script, met = _sequences(n)[name]
    want, seen = lm_script(n, script.cmds)
    assert seen == met, "the sequence does not reach what it is there for"
    got = [" ".join(line.split()) for line in run(prog, "script", n, script.text()).splitlines()]
    assert got == [" ".join(line.split()) for line in want]


def test_sequences_cover_every_rule():
    seen = [x for name in SEQUENCE_NAMES for x in lm_script(6, _sequences(6)[name][0].cmds)[1]]
    assert {"alpha_low", "alpha_mid", "alpha_high", "rejected", "inf_rho_positive", "failed_solve", "rho_zero",
            ("stop", PC.STOP_TRIALS), ("stop", PC.STOP_RHO_ZERO), ("stop", PC.STOP_NBAD), ("stop", -1)} <= set(seen)
