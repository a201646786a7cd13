"""GPU tests of ygzf_pose_optimization (Optimizer::PoseOptimization(Frame *), src/Optimizer.cc:1656-1842) on the constructed cases of
tests/pose_opt_cases.py: every decision -- outlier flags, return value, and per round the iterations, Levenberg trials and stop reason -- is the
device-order restatement's (the cases' decision margins make that a fair demand), the double pose agrees within 4 x EPS_ORDER (the reordering
error measured on the CPU; the factor covers what the restatement cannot mirror: pow against a cube, division and sqrt sequences, sin / cos),
the float pose is equal or one float ulp away; batches against single calls; argument errors; a context that extracts and matches around the
calls; the class shell (tests/cpp/pose_shell.cc) against the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pose_opt_cases as PC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

NAMES = [s[0] for s in PC.SPECS]


@pytest.fixture(scope="module")
def ex():
    from orb_ygz_slam_amd import Extractor
    e = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=2)
    yield e
    e.close()


def camera(P):
    from orb_ygz_slam_amd.capi import Camera
    fx, fy, cx, cy, bf = P.cam
    return Camera(fx, fy, cx, cy, 0.0, bf, 0.0, 0.0, 752.0, 480.0)


def as_dict(P):
    from orb_ygz_slam_amd.capi import KP_DTYPE
    n = len(P.octave)
    keys = np.zeros(n, KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = P.xy[:, 0], P.xy[:, 1], P.octave
    keys["size"], keys["angle"], keys["class_id"] = 31.0, -1.0, -1
    return dict(keys=keys, u_right=P.u_right, mp_valid=P.mp_valid, world=P.world, Tcw=P.Tcw, outlier=P.outlier_in)


def run(ex, cases):
    """one call over the cases (all cases of this module share one camera per call: grouped by camera)"""
    out = [None] * len(cases)
    cams = sorted({c.problem.cam for c in cases})
    for cam in cams:
        idx = [i for i, c in enumerate(cases) if c.problem.cam == cam]
        res = ex.pose_optimization(camera(cases[idx[0]].problem), [as_dict(cases[i].problem) for i in idx], PC.INV_SIGMA2)
        for i, r in zip(idx, res):
            out[i] = r
    return out


def ulps(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.max(np.abs(ia - ib)))


def check(case, got):
    want = PC.expected(case, "device")
    n = len(case.problem.octave)
    print("%s: ret %d / %d, iterations %s trials %s stop %s | pose diff %.3e (bound %.3e), float ulps %d" % (
        case.name, got["ret"], want.ret, got["iterations"], got["trials"], got["stop"], PC.pose_diff(got["Tcw64"], want.Tcw64), 4 * PC.EPS_ORDER,
        ulps(got["Tcw"], want.Tcw)))
    assert np.array_equal(got["outlier"][:n], want.outlier), "outlier flags"
    assert got["ret"] == want.ret
    assert (got["iterations"], got["trials"], got["stop"]) == (want.iters, want.trials, want.stop)
    if want.ret == 0 and want.stop == [PC.STOP_NOT_RUN] * 4:
        assert np.array_equal(got["Tcw"], np.asarray(case.problem.Tcw, np.float32)) and np.array_equal(got["Tcw64"], np.asarray(case.problem.Tcw, np.float32).astype(np.float64))
        return
    assert PC.pose_diff(got["Tcw64"], want.Tcw64) <= 4 * PC.EPS_ORDER
    assert ulps(got["Tcw"], want.Tcw) <= 1


def same(a, b):
    """bit-equal results (lambda and chi2 of a round that met a non-finite chi2 are NaN or Inf on both sides)"""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("Tcw", "Tcw64", "outlier", "ret", "iterations", "trials", "stop")) and \
        all(np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), equal_nan=True) for k in ("lam", "chi2"))


_SINGLE = {}


def single(ex, name):
    if name not in _SINGLE:
        _SINGLE[name] = run(ex, [PC.case_by_name(name)])[0]
    return _SINGLE[name]


@pytest.mark.parametrize("name", NAMES)
def test_case_single_call_twice(ex, name):
    """the case, a case of another size, the case again on one context: the restatement's decisions and pose both times, bit-equal to each other"""
    case = PC.case_by_name(name)
    other = PC.case_by_name("n257" if name != "n257" else "n64")
    a = single(ex, name)
    run(ex, [other])
    b = run(ex, [case])[0]
    check(case, a)
    assert same(a, b), "the second call on the same context differs from the first"


def test_all_cases_in_one_batch(ex):
    cases = PC.cases()
    got = run(ex, cases)
    for c, g in zip(cases, got):
        assert same(g, single(ex, c.name)), c.name


@pytest.mark.parametrize("names", [("n64",), ("n9", "n256"), ("scene00_n117", "n2", "interleaved", "empty_round", "n10"), ("n63", "n2", "n65"), ("n2049", "n3")])
def test_batches(ex, names):
    """batches of 1, 2 and 5 problems; a problem with n = 2 in the middle (ret 0, pose unchanged, its neighbours undisturbed); 2049 edges beside 3"""
    cases = [PC.case_by_name(n) for n in names]
    got = run(ex, cases)
    for c, g in zip(cases, got):
        check(c, g)
        assert same(g, single(ex, c.name)), c.name


def test_outlier_entries_of_non_correspondences_stay(ex):
    case = PC.case_by_name("interleaved")
    P = case.problem
    got = run(ex, [case])[0]
    off = ~np.asarray(P.mp_valid).astype(bool)
    assert off.any() and np.asarray(P.outlier_in)[off].any()
    assert np.array_equal(got["outlier"][off], np.asarray(P.outlier_in)[off])


def test_context_tables_when_no_sigma_is_given(ex):
    """inv_level_sigma2 == NULL reads the context's tables: the restatement on those tables"""
    case = PC.case_by_name("n65")
    tab = ex.tables()["inv_sigma2"]
    P = case.problem._replace(inv_sigma2=tab)
    want = PC.pose_opt(P, "device")
    got = ex.pose_optimization(camera(P), [as_dict(P)], None)[0]
    assert np.array_equal(got["outlier"], want.outlier) and got["ret"] == want.ret and (got["iterations"], got["trials"], got["stop"]) == (want.iters, want.trials, want.stop)
    assert PC.pose_diff(got["Tcw64"], want.Tcw64) <= 4 * PC.EPS_ORDER


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import PoseInfo, PoseProblem, YgzfError
    L, h = ex.L, ex.h
    case = PC.case_by_name("n10")
    P = case.problem
    d = as_dict(P)
    n = len(d["keys"])
    cam = camera(P)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    valid, world, flags = np.ascontiguousarray(P.mp_valid, np.uint8), np.ascontiguousarray(P.world, np.float32), np.zeros(n, np.uint8)
    T, ret = np.zeros(7, np.float32), np.zeros(1, np.int32)
    fl = (C.c_void_p * 1)(flags.ctypes.data)
    rec = (PoseProblem * 1)(PoseProblem(n, vp(d["keys"]), None, vp(valid), vp(world), (C.c_float * 7)(*P.Tcw)))
    call = lambda nprob=1, r=rec, t=vp(T), f=fl, rt=vp(ret), cm=C.byref(cam): L.ygzf_pose_optimization(h, cm, None, nprob, r, t, None, f, rt, None)
    assert call() == 0
    for bad in (0, -3):
        assert call(nprob=bad) == -1 and b"n_problems" in L.ygzf_last_error(h)
    assert call(t=None) == -1 and b"null argument" in L.ygzf_last_error(h)
    assert call(rt=None) == -1 and call(f=None) == -1 and call(cm=None) == -1 and call(r=None) == -1
    assert L.ygzf_pose_optimization(None, C.byref(cam), None, 1, rec, vp(T), None, fl, vp(ret), None) == -1
    for field in ("keys", "mp_valid", "mp_world"):
        r2 = (PoseProblem * 1)(PoseProblem(n, vp(d["keys"]), None, vp(valid), vp(world), (C.c_float * 7)(*P.Tcw)))
        setattr(r2[0], field, None)
        assert call(r=r2) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(f=(C.c_void_p * 1)(None)) == -1 and b"null array" in L.ygzf_last_error(h)
    r3 = (PoseProblem * 1)(PoseProblem(-1, vp(d["keys"]), None, vp(valid), vp(world), (C.c_float * 7)(*P.Tcw)))
    assert call(r=r3) == -1 and b"negative count" in L.ygzf_last_error(h)
    k2 = d["keys"].copy()
    k2["octave"][int(np.nonzero(valid)[0][0])] = 8
    r4 = (PoseProblem * 1)(PoseProblem(n, vp(k2), None, vp(valid), vp(world), (C.c_float * 7)(*P.Tcw)))
    assert call(r=r4) == -1 and b"octave 8 outside the 8 levels" in L.ygzf_last_error(h)
    k2["octave"][:] = -1
    assert call(r=r4) == -1
    with pytest.raises(YgzfError):
        ex.pose_optimization(cam, [], None)
    # an empty problem is no error: ret 0, the pose unchanged
    r5 = (PoseProblem * 1)(PoseProblem(0, None, None, None, None, (C.c_float * 7)(*P.Tcw)))
    info = (PoseInfo * 1)()
    assert L.ygzf_pose_optimization(h, C.byref(cam), None, 1, r5, vp(T), None, (C.c_void_p * 1)(None), vp(ret), info) == 0
    assert ret[0] == 0 and np.array_equal(T, np.asarray(P.Tcw, np.float32)) and list(info[0].stop) == [4, 4, 4, 4]
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
    case = PC.case_by_name("scene03_n905")
    a = run(ex, [case])[0]
    m1, k1 = extract_and_match()
    b = run(ex, [case])[0]
    check(case, a)
    assert same(a, b)
    for f in range(2):
        assert np.array_equal(k0[f][0], k1[f][0]) and np.array_equal(k0[f][1], k1[f][1])
    assert np.array_equal(m0[1], m1[1])   # (pair 0 of the second run matches against the carried frame of the first)


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "pose_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "pose_shell.cc")] + [os.path.join(host, f) for f in ("OptimizerPose.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_shell_against_the_abi(ex, tmp_path):
    """ygz::PoseOptimizationDevice / PoseOptimizationBatch over stub Frames: mvbOutlier, the return values and the poses SetPose received are the
    ABI's results for the same problems"""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    names = ["n2", "n65", "interleaved", "scene00_n117"]
    d = tmp_path / "data"
    d.mkdir()
    (d / "meta.txt").write_text("%d\n" % len(names))
    for k, name in enumerate(names):
        case = PC.case_by_name(name)
        P = case.problem
        assert P.cam == PC.EUROC
        g = single(ex, name)
        n = len(P.octave)
        ur = np.full(n, -1.0, np.float32) if P.u_right is None else np.asarray(P.u_right, np.float32)
        with open(str(d / ("problem_%d.bin" % k)), "wb") as f:
            np.array([n], np.int32).tofile(f)
            for a in (as_dict(P)["keys"], ur, np.asarray(P.mp_valid, np.uint8), np.asarray(P.world, np.float32), np.asarray(P.Tcw, np.float32),
                      np.asarray(P.outlier_in, np.uint8), np.asarray(PC.INV_SIGMA2, np.float32), np.asarray(PC.EUROC, np.float32),
                      g["Tcw"], g["outlier"][:n], np.array([g["ret"]], np.int32)):
                a.tofile(f)
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pose shell ok" in out.stdout, out.stdout + out.stderr
