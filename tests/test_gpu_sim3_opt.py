"""GPU tests of ygzf_optimize_sim3 (Optimizer::OptimizeSim3, src/Optimizer.cc:2409-2594) on the constructed cases of tests/sim3_opt_cases.py:
the result equals the device-order restatement BIT FOR BIT -- S12_out, removed, ret, nBad and per round the iterations, Levenberg trials, stop
reason, lambda and chi2.  Everything on that path is a correctly rounded + - * / sqrt or text the kernel shares with the restatement's host
twin (csrc/sim3_opt_math.h), and the numeric Jacobian is a dither of float roundings: a tolerance would be no contract.  Batches against single
calls; the early return leaves S12 untouched; argument errors; a context that extracts and matches around the calls; the class shell
(tests/cpp/sim3_opt_shell.cc) against the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_opt_cases as SC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from orb_ygz_slam_amd import Extractor
    e = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=2)
    yield e
    e.close()


def run(ex, cases):
    return [SC.from_api(r) for r in ex.optimize_sim3([SC.as_api(c.problem) for c in cases])]


def check(case, got):
    want = SC.expected(case, "device")
    with np.errstate(all="ignore"):
        d = np.abs(got.S12 - want.S12)
    print("%s: ret %d / %d, nBad %d / %d, iterations %s trials %s stop %s | lambda %r / %r | chi2 %r / %r | largest Sim3 difference %r" % (
        case.name, got.ret, want.ret, got.n_bad, want.n_bad, got.iters, got.trials, got.stop, got.lam, want.lam, got.chi2, want.chi2,
        float(np.nanmax(d)) if len(d) else 0.0))
    assert np.array_equal(got.removed, want.removed), "removed"
    assert (got.ret, got.n_bad) == (want.ret, want.n_bad)
    assert (list(got.iters), list(got.trials), list(got.stop)) == (list(want.iters), list(want.trials), list(want.stop))
    assert np.array_equal(np.asarray(got.lam), np.asarray(want.lam), equal_nan=True), "lambda differs in some bit"
    assert np.array_equal(np.asarray(got.chi2), np.asarray(want.chi2), equal_nan=True), "chi2 differs in some bit"
    assert SC.same(got, want), "S12 differs from the device-order restatement in some bit"


_SINGLE = {}


def single(ex, name):
    if name not in _SINGLE:
        _SINGLE[name] = run(ex, [SC.case_by_name(name)])[0]
    return _SINGLE[name]


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_single_call_twice(ex, name):
    """the case, a case of another size, the case again on one context: the restatement bit for bit both times"""
    case = SC.case_by_name(name)
    other = SC.case_by_name("n_257" if name != "n_257" else "n_64")
    a = single(ex, name)
    run(ex, [other])
    b = run(ex, [case])[0]
    check(case, a)
    assert SC.same(a, b), "the second call on the same context differs from the first"


def test_all_cases_in_one_batch(ex):
    got = run(ex, SC.CASES)
    for c, g in zip(SC.CASES, got):
        assert SC.same(g, single(ex, c.name)), c.name


@pytest.mark.parametrize("names", [("n_64",), ("n_zero", "n_600"), ("survive_9", "scene_2"), ("n_63", "n_one", "nan_point", "n_65", "z_zero"),
                                   ("n_600", "n_zero", "survive_0", "stop_rho_zero")])
def test_batches(ex, names):
    """n = 0 beside n = 600, an early return beside a full run, non-finite problems between finite ones: every problem as its single call"""
    cases = [SC.case_by_name(n) for n in names]
    for c, g in zip(cases, run(ex, cases)):
        check(c, g)
        assert SC.same(g, single(ex, c.name)), c.name


@pytest.mark.parametrize("name", ["survive_0", "survive_1", "survive_9", "n_one", "n_zero"])
def test_early_return_leaves_s12_untouched(ex, name):
    case = SC.case_by_name(name)
    got = single(ex, name)
    assert got.ret == 0 and got.stop[1] == SC.STOP_NOT_RUN
    assert np.array_equal(got.S12.view(np.uint64), np.asarray(case.problem.S12, np.float64).view(np.uint64))
    assert int((got.removed == 1).sum()) == got.n_bad and not (got.removed == 2).any()   # the round-0 removals are still reported


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import Sim3OptInfo, Sim3OptProblem, YgzfError
    L, h = ex.L, ex.h
    case = SC.case_by_name("n_64")
    P = case.problem
    n = len(P.P1c)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (P.P1c, P.P2c, P.obs1, P.obs2, P.is1, P.is2)]

    def rec(nn=n, drop=None):
        ptrs = [None if k == drop else vp(a) for k, a in enumerate(arrs)]
        return (Sim3OptProblem * 1)(Sim3OptProblem(nn, *ptrs, (C.c_float * 4)(*P.K1), (C.c_float * 4)(*P.K2), (C.c_double * 8)(*P.S12), P.th2, int(P.fix_scale)))
    S, ret, flags = np.zeros(8), np.zeros(1, np.int32), np.zeros(n, np.uint8)
    fl = (C.c_void_p * 1)(flags.ctypes.data)
    call = lambda nprob=1, r=None, s=vp(S), f=fl, rt=vp(ret): L.ygzf_optimize_sim3(h, nprob, rec() if r is None else r, s, f, rt, None)
    assert call() == 0
    for bad in (0, -3):
        assert call(nprob=bad) == -1 and b"n_problems" in L.ygzf_last_error(h)
    assert call(s=None) == -1 and b"null argument" in L.ygzf_last_error(h)
    assert call(rt=None) == -1 and call(f=None) == -1
    assert L.ygzf_optimize_sim3(h, 1, None, vp(S), fl, vp(ret), None) == -1
    assert L.ygzf_optimize_sim3(None, 1, rec(), vp(S), fl, vp(ret), None) == -1
    for drop in range(6):
        assert call(r=rec(drop=drop)) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(f=(C.c_void_p * 1)(None)) == -1 and b"null array" in L.ygzf_last_error(h)
    assert call(r=rec(nn=-1)) == -1 and b"negative count" in L.ygzf_last_error(h)
    with pytest.raises(YgzfError):
        ex.optimize_sim3([])
    # an empty problem is no error: nothing runs, ret 0, S12 as it came
    r0 = (Sim3OptProblem * 1)(Sim3OptProblem(0, None, None, None, None, None, None, (C.c_float * 4)(*P.K1), (C.c_float * 4)(*P.K2), (C.c_double * 8)(*P.S12), P.th2, 1))
    info = (Sim3OptInfo * 1)()
    ret[0] = 7
    assert L.ygzf_optimize_sim3(h, 1, r0, vp(S), (C.c_void_p * 1)(None), vp(ret), info) == 0
    assert ret[0] == 0 and np.array_equal(S, np.asarray(P.S12)) and list(info[0].stop) == [4, 4] and info[0].n == 0
    # and the context still works
    check(case, run(ex, [case])[0])


def test_context_that_extracts_and_matches_around_the_calls(ex):
    from orb_ygz_slam_amd.capi import make_camera
    from orb_ygz_slam_amd.synth import synth_frame
    imgs = np.stack([synth_frame(7, 752, 480), synth_frame(8, 752, 480)])
    cam = make_camera(752, 480)

    def extract_and_match():
        ex.extract_batch_host(imgs)
        ex.match_batch_prev(cam)
        return [ex.match_fetch(f)[0].copy() for f in range(2)], [ex.batch_fetch(f) for f in range(2)]
    m0, k0 = extract_and_match()
    case = SC.case_by_name("scene_3")
    a = run(ex, [case])[0]
    m1, k1 = extract_and_match()
    b = run(ex, [case])[0]
    check(case, a)
    assert SC.same(a, b)
    for f in range(2):
        assert np.array_equal(k0[f][0], k1[f][0]) and np.array_equal(k0[f][1], k1[f][1])
    assert np.array_equal(m0[1], m1[1])   # (pair 0 of the second run matches against the carried frame of the first)


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "sim3_opt_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "sim3_opt_shell.cc")] + [os.path.join(host, f) for f in ("OptimizerSim3.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_shell_against_the_abi(ex, tmp_path):
    """ygz::OptimizeSim3Device / OptimizeSim3Batch over stub KeyFrames and a stand-in Sim3: vpMatches1, g2oS12 and the return values are the
    ABI's results for the same problems with the device forced, mode "reference" with the host forced, each bit for bit; the batch equals the
    single calls; the default threshold sends the small single calls to the host and the batch to the device"""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    names = ["n_65", "survive_9", "two_cameras", "mixed_octaves", "n_257"]   # one KF1: K1, th2 and fix_scale are shared
    tab = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
    d = tmp_path / "data"
    d.mkdir()
    (d / "meta.txt").write_text("%d\n" % len(names))
    for k, name in enumerate(names):
        P = SC.case_by_name(name).problem
        assert P.K1 == SC.K_A and P.th2 == 10.0 and P.fix_scale
        g = single(ex, name)
        h = SC.expected(SC.case_by_name(name), "reference")
        n = len(P.P1c)
        oct1, oct2 = (np.argmin(np.abs(tab[None, :] - np.asarray(a, np.float32)[:, None]), 1).astype(np.int32) for a in (P.is1, P.is2))
        assert np.array_equal(tab[oct1], P.is1) and np.array_equal(tab[oct2], P.is2)
        with open(str(d / ("problem_%d.bin" % k)), "wb") as f:
            np.array([n, int(P.fix_scale)], np.int32).tofile(f)
            for a in (np.array([P.th2], np.float32), np.asarray(P.K1, np.float32), np.asarray(P.K2, np.float32), np.asarray(P.S12, np.float64),
                      np.asarray(P.P1c, np.float32), np.asarray(P.P2c, np.float32), np.asarray(P.obs1, np.float32), np.asarray(P.obs2, np.float32),
                      oct1, oct2, tab, g.S12, g.removed, np.array([g.ret], np.int32), h.S12, h.removed, np.array([h.ret], np.int32)):
                np.ascontiguousarray(a).tofile(f)
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sim3 opt shell ok" in out.stdout, out.stdout + out.stderr
