"""GPU tests of ygzf_sim3_ransac (Sim3Solver's RANSAC hypotheses, src/Sim3Solver.cc:132-338) against mode "device" of tests/sim3_cases.py: hyp bit
for bit (NaN as NaN), counts and inlier masks exactly, the tail bits of every mask zero -- every constructed case and two seeded scenes, twice on
one context; all cases in one batch against the single calls; batches that mix n = 3 / 64 / 65 / 500 with n_hyp = 0 / 1 / 4 / 5 / 300, so that
the four waves of a workgroup straddle a problem's end; inlier_bits == NULL; argument errors; a context that extracts and matches around the
calls; the class shell (tests/cpp/sim3_shell.cc) against sim3_iterate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_cases as SC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from orb_ygz_slam_amd import Extractor
    e = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=2)
    yield e
    e.close()


def as_dict(P):
    return dict(X1=P.X1, X2=P.X2, max_err1=SC.gates(P.sigma2_1), max_err2=SC.gates(P.sigma2_2), K1=P.K1, K2=P.K2, fix_scale=P.fix_scale, samples=P.samples)


def run(ex, problems, want_bits=True):
    return ex.sim3_ransac([as_dict(P) for P in problems], want_bits)


def check(P, got, want=None, name=""):
    want = SC.sim3_hypotheses(P, "device") if want is None else want
    n = len(P.X1)
    nan = np.isnan(want.hyp)
    print("%s: n %d, %d hypotheses, %d NaN, counts %s" % (name, n, len(want.count), int(nan.any(axis=1).sum()), list(map(int, got["n_inliers"][:8]))))
    assert got["hyp"].shape == want.hyp.shape
    assert np.array_equal(np.isnan(got["hyp"]), nan), "NaN pattern of hyp"
    assert np.array_equal(got["hyp"].view(np.uint32)[~nan], want.hyp.view(np.uint32)[~nan]), "hyp differs from the restatement in some bit"
    assert np.array_equal(got["n_inliers"], want.count)
    if got["bits"] is not None:
        assert np.array_equal(got["bits"], want.bits)
        if n % 64 and len(want.count):
            assert not (got["bits"][:, -1] >> np.uint64(n % 64)).any(), "tail bits"
        assert np.array_equal(np.array([bin(int(w)).count("1") for w in got["bits"].reshape(-1)], np.int64).reshape(got["bits"].shape).sum(axis=1), got["n_inliers"])


def same(a, b):
    return (np.array_equal(a["hyp"].view(np.uint32), b["hyp"].view(np.uint32)) and np.array_equal(a["n_inliers"], b["n_inliers"]) and
            (a["bits"] is None or b["bits"] is None or np.array_equal(a["bits"], b["bits"])))


_SINGLE = {}


def single(ex, name):
    if name not in _SINGLE:
        _SINGLE[name] = run(ex, [SC.case_by_name(name).problem])[0]
    return _SINGLE[name]


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_single_call_twice(ex, name):
    """the case, a case of another size, the case again on one context: the restatement both times, bit-equal to each other"""
    c = SC.case_by_name(name)
    other = SC.case_by_name("all_n129" if name != "all_n129" else "all_n64")
    a = single(ex, name)
    run(ex, [other.problem])
    b = run(ex, [c.problem])[0]
    check(c.problem, a, SC.expected(c, "device").hyps, name)
    assert same(a, b), "the second call on the same context differs from the first"


@pytest.mark.parametrize("scene", ["scene0", "scene3"])
def test_seeded_scene_twice(ex, scene):
    """the candidates of one current keyframe in one call, as ComputeSim3 holds them: 300 random triples each"""
    cs = SC.scene(scene)
    a = run(ex, [c.problem for c in cs])
    b = run(ex, [c.problem for c in cs])
    for c, g, g2 in zip(cs, a, b):
        check(c.problem, g, SC.expected(c, "device").hyps, c.name)
        assert same(g, g2)


def test_all_cases_in_one_batch(ex):
    cs = SC.constructed()
    got = run(ex, [c.problem for c in cs])
    for c, g in zip(cs, got):
        assert same(g, single(ex, c.name)), c.name


def _with_hyps(P, count):
    S = np.asarray(P.samples)
    return P._replace(samples=np.ascontiguousarray(np.concatenate([S] * (count // len(S) + 1))[:count].reshape(-1, 3), np.int32))


@pytest.fixture(scope="module")
def mixed():
    P3, P64, P65 = (SC.case_by_name(n).problem for n in ("all_n3", "all_n64", "all_n65"))
    P500 = SC._seeded("mix_n500", 500, 0.3, 9001)
    assert len(P500.X1) == 500 and len(P500.samples) == 300
    return P3, P64, P65, P500


@pytest.mark.parametrize("plan", [((3, 5), (64, 1), (65, 0), (65, 4), (500, 300)), ((500, 300), (3, 1), (64, 5), (65, 0), (3, 4)), ((65, 0), (64, 4), (3, 0)),
                                  ((3, 1), (3, 1), (3, 1), (64, 1), (65, 1), (65, 0))])
def test_mixed_batches(ex, mixed, plan):
    """the hypotheses of a call are one list of waves, four to a workgroup: a workgroup's waves belong to up to four problems here, and problems
    without hypotheses stand between them"""
    by_n = dict(zip((3, 64, 65, 500), mixed))
    probs = [_with_hyps(by_n[n], h) for n, h in plan]
    got = run(ex, probs)
    for (n, h), P, g in zip(plan, probs, got):
        assert g["hyp"].shape == (h, 13)
        check(P, g, name="n%d x %d" % (n, h))


def test_without_inlier_bits(ex):
    cs = [SC.case_by_name(n) for n in ("all_n65", "return_then_beat", "nonfinite")]
    got = run(ex, [c.problem for c in cs], want_bits=False)
    for c, g in zip(cs, got):
        assert g["bits"] is None
        check(c.problem, g, SC.expected(c, "device").hyps, c.name)
        assert same(g, single(ex, c.name))


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import Sim3Problem, YgzfError
    L, h = ex.L, ex.h
    c = SC.case_by_name("all_n20")
    P = c.problem
    n, nh = len(P.X1), len(P.samples)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    X1, X2 = np.ascontiguousarray(P.X1, np.float32), np.ascontiguousarray(P.X2, np.float32)
    e1, e2 = SC.gates(P.sigma2_1), SC.gates(P.sigma2_2)
    smp = np.ascontiguousarray(P.samples, np.int32)
    hyp, cnt, bits = np.zeros((nh, 13), np.float32), np.zeros(nh, np.int32), np.zeros((nh, 1), np.uint64)

    def rec(n_=n, nh_=nh, s=smp, **null):
        r = Sim3Problem(n_, vp(X1), vp(X2), vp(e1), vp(e2), (C.c_float * 4)(*P.K1), (C.c_float * 4)(*P.K2), 0, nh_, vp(s))
        for k in null:
            setattr(r, k, None)
        return (Sim3Problem * 1)(r)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data if a is not None else None)
    call = lambda r=None, nprob=1, hp=one(hyp), cp=one(cnt), bp=one(bits): L.ygzf_sim3_ransac(h, nprob, rec() if r is None else r, hp, cp, bp)
    assert call() == 0
    check(P, dict(hyp=hyp, n_inliers=cnt, bits=bits), SC.expected(c, "device").hyps, "raw call")
    for bad in (0, -2):
        assert call(nprob=bad) == -1 and b"n_problems" in L.ygzf_last_error(h)
    assert L.ygzf_sim3_ransac(None, 1, rec(), one(hyp), one(cnt), one(bits)) == -1
    assert L.ygzf_sim3_ransac(h, 1, None, one(hyp), one(cnt), one(bits)) == -1 and b"null argument" in L.ygzf_last_error(h)
    assert call(hp=None) == -1 and call(cp=None) == -1
    assert call(hp=one(None)) == -1 and b"null array" in L.ygzf_last_error(h)
    assert call(cp=one(None)) == -1
    for field in ("X3Dc1", "X3Dc2", "max_err1", "max_err2", "samples"):
        assert call(rec(**{field: True})) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(rec(n_=2)) == -1 and b"a hypothesis needs 3" in L.ygzf_last_error(h)
    assert call(rec(nh_=-1)) == -1 and b"negative hypothesis count" in L.ygzf_last_error(h)
    for bad_index in (-1, n):
        s2 = smp.copy()
        s2[1, 2] = bad_index
        assert call(rec(s=s2)) == -1 and b"outside [0, 20)" in L.ygzf_last_error(h)
    s3 = smp.copy()
    s3[2, 1] = s3[2, 0]
    assert call(rec(s=s3)) == -1 and b"hypothesis 2 repeats an index" in L.ygzf_last_error(h)
    with pytest.raises(YgzfError):
        ex.sim3_ransac([])
    # n_hyp == 0 is legal and touches nothing: the pointers may be NULL, the outputs stay as they were
    hyp[:], cnt[:], bits[:] = 7, 7, 7
    assert call(rec(n_=0, nh_=0, X3Dc1=True, X3Dc2=True, max_err1=True, max_err2=True, samples=True), hp=one(None), cp=one(None), bp=None) == 0
    assert call(rec(n_=2, nh_=0)) == 0
    assert (hyp == 7).all() and (cnt == 7).all() and (bits == 7).all()
    # inlier_bits as a whole may be NULL; and the context still works
    assert call(bp=None) == 0 and (bits == 7).all()
    check(P, dict(hyp=hyp, n_inliers=cnt, bits=None), SC.expected(c, "device").hyps, "after the errors")


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
    cs = SC.scene("scene1")
    a = run(ex, [c.problem for c in cs])
    m1, k1 = extract_and_match()
    b = run(ex, [c.problem for c in cs])
    for c, g, g2 in zip(cs, a, b):
        check(c.problem, g, SC.expected(c, "device").hyps, c.name)
        assert same(g, g2)
    for f in range(2):
        assert np.array_equal(k0[f][0], k1[f][0]) and np.array_equal(k0[f][1], k1[f][1])
    assert np.array_equal(m0[1], m1[1])   # (pair 0 of the second run matches against the carried frame of the first)


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "sim3_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "sim3_shell.cc")] + [os.path.join(host, f) for f in ("Sim3Solver.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_shell_round_robin_against_sim3_iterate(ex, tmp_path):
    """Sim3SolverBatch over three solvers (and a fourth that evaluates itself), then their iterate(5) calls round-robin as ComputeSim3 drives its
    candidates: every call's matrix, inlier vector, count and bNoMore, and the final GetEstimated*, are sim3_iterate's on the same triples"""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    names = ["return_then_beat", "ends_on_max", SC.scene("scene0")[1].name, "returns_on_max"]
    files = []
    for k, name in enumerate(names):
        P = SC.case_by_name(name).problem
        path = str(tmp_path / ("case_%d.bin" % k))
        SC.write_case(P, path)
        with open(path, "ab") as f:
            for s in (P.sigma2_1, P.sigma2_2):
                o = np.array([int(np.nonzero(SC.SIGMA2 == v)[0][0]) for v in s], np.int32)
                o.tofile(f)
            SC.SIGMA2.tofile(f)
        files.append(path)
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, out] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sim3 shell ok" in r.stdout, r.stdout + r.stderr
    with open(out, "rb") as f:
        for name in names:
            c = SC.case_by_name(name)
            want = SC.expected(c, "device")
            for j, w in enumerate(want.calls):
                returned, n_inl, no_more = (int(v) for v in np.fromfile(f, np.int32, 3))
                T = np.fromfile(f, np.float32, 16).reshape(4, 4)
                inl = np.fromfile(f, np.uint8, c.problem.mN1).astype(bool)
                is_find = c.problem.calls[j] == "find"
                assert (bool(returned), n_inl) == (w.returned, w.n_inliers), (name, j)
                assert is_find or bool(no_more) == w.no_more, (name, j)
                assert np.array_equal(inl, w.inliers12), (name, j)
                if w.returned:
                    hyp = want.hyps.hyp[w.hyp_index]
                    sR = (np.float64(hyp[12]) * hyp[:9].astype(np.float64)).astype(np.float32).reshape(3, 3)
                    assert np.array_equal(T[:3, :3], sR) and np.array_equal(T[:3, 3], hyp[9:12]) and np.array_equal(T[3], np.array([0, 0, 0, 1], np.float32)), (name, j)
        for name in names:
            c = SC.case_by_name(name)
            want = SC.expected(c, "device")
            have = int(np.fromfile(f, np.int32, 1)[0])
            v = np.fromfile(f, np.float32, 13)
            best = want.calls[-1].best_index
            assert bool(have) == (best >= 0), name
            if have:
                assert np.array_equal(v, want.hyps.hyp[best], equal_nan=True), name
