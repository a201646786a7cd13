"""GPU tests of ygzf_pnp_ransac (PnPsolver's EPnP RANSAC hypotheses and the Refine of their records, src/PnPsolver.cc:155-308 and :341-894)
against tests/pnp_cases.py: poses bit for bit (NaN as NaN), counts, masks, record flags and Refine results exactly, the tail bits of every
mask zero -- every constructed case and the seeded scenes, twice on one context with a case of another size between; all cases in one batch
against the single calls; batches that mix n = 4 / 64 / 65 / 129 with n_hyp = 0 / 1 / 4 / 5 / 24, so that the four waves of a workgroup
straddle a problem's end, with Refine sets of 11, 64 and 65 inliers among them; inlier_bits == NULL; argument errors; a context that extracts
and matches around the calls; the class shell (tests/cpp/pnp_shell.cc) against pnp_iterate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pnp_cases as PC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from orb_ygz_slam_amd import Extractor
    e = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=2)
    yield e
    e.close()


def budget(P):
    return min(len(P.samples), P.max_its) if len(P.P3D) >= P.min_set else 0


def as_dict(P, count=None):
    return dict(P3Dw=P.P3D, P2D=P.P2D, max_err=P.max_err, K=P.K, min_set=P.min_set, min_inliers=P.min_inliers,
                samples=P.samples[:budget(P) if count is None else count])


def run(ex, problems, want_bits=True):
    return ex.pnp_ransac([p if isinstance(p, dict) else as_dict(p) for p in problems], want_bits)


def bits_equal(a, b):
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def check(P, got, want=None, name=""):
    H = len(got["n_inliers"])
    want = PC.pnp_hypotheses(P, H) if want is None else want
    n = len(P.P3D)
    records = want.refined_n[:H] >= 0
    print("%s: n %d, %d hypotheses, %d NaN, %d records, counts %s refined %s" % (name, n, H, int(np.isnan(want.hyp[:H]).any(axis=1).sum()), int(records.sum()),
                                                                                 list(map(int, got["n_inliers"][:8])), list(map(int, got["refined_n"][:8]))))
    assert bits_equal(got["hyp"], want.hyp[:H]), "hyp differs from the restatement in some bit"
    assert np.array_equal(got["n_inliers"], want.count[:H])
    assert np.array_equal(got["refined_n"], want.refined_n[:H]), "record flags / Refine counts"
    assert bits_equal(got["refined_hyp"], want.refined_hyp[:H]), "refined_hyp differs from the restatement in some bit"
    if got["bits"] is not None:
        pop = lambda b: np.array([bin(int(w)).count("1") for w in b.reshape(-1)], np.int64).reshape(b.shape).sum(axis=1)
        assert np.array_equal(got["bits"], want.bits[:H]) and np.array_equal(got["refined_bits"], want.refined_bits[:H])
        if n % 64 and H:
            assert not (got["bits"][:, -1] >> np.uint64(n % 64)).any() and not (got["refined_bits"][:, -1] >> np.uint64(n % 64)).any(), "tail bits"
        assert np.array_equal(pop(got["bits"]), got["n_inliers"])
        assert np.array_equal(pop(got["refined_bits"])[records], got["refined_n"][records]) and not got["refined_bits"][~records].any()


def same(a, b):
    return (np.array_equal(a["hyp"].view(np.uint64), b["hyp"].view(np.uint64)) and np.array_equal(a["n_inliers"], b["n_inliers"]) and
            np.array_equal(a["refined_n"], b["refined_n"]) and np.array_equal(a["refined_hyp"].view(np.uint64), b["refined_hyp"].view(np.uint64)) and
            (a["bits"] is None or b["bits"] is None or (np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["refined_bits"], b["refined_bits"]))))


_SINGLE = {}


def single(ex, name):
    if name not in _SINGLE:
        _SINGLE[name] = run(ex, [PC.case_by_name(name).problem])[0]
    return _SINGLE[name]


@pytest.mark.parametrize("name", PC.NAMES + PC.SCENE_NAMES)
def test_case_single_call_twice(ex, name):
    """the case, a case of another size, the case again on one context: the restatement both times, bit-equal to each other"""
    c = PC.case_by_name(name)
    other = PC.case_by_name("all_n129" if name != "all_n129" else "all_n64")
    a = single(ex, name)
    run(ex, [other.problem])
    b = run(ex, [c.problem])[0]
    check(c.problem, a, name=name)
    assert same(a, b), "the second call on the same context differs from the first"


def test_all_cases_in_one_batch(ex):
    cs = PC.constructed() + [PC.scene(n) for n in PC.SCENE_NAMES]
    got = run(ex, [c.problem for c in cs])
    for c, g in zip(cs, got):
        assert same(g, single(ex, c.name)), c.name


@pytest.mark.parametrize("plan", [(("all_n4", 5), ("all_n64", 1), ("all_n65", 0), ("refine_65", 4), ("winners_and_flips", 24)),
                                  (("winners_and_flips", 24), ("all_n4", 1), ("refine_64", 5), ("all_n65", 0), ("refine_11", 4)),
                                  (("all_n65", 0), ("all_n64", 4), ("all_n4", 0)),
                                  (("all_n4", 1), ("all_n4", 1), ("all_n4", 1), ("refine_64", 4), ("all_n129", 1), ("all_n65", 0), ("refine_11", 5))])
def test_mixed_batches(ex, plan):
    """the hypotheses of a call are one list of waves, four to a workgroup: a workgroup's waves belong to up to four problems here, problems
    without hypotheses stand between them, and the Refine sets have 11, 64 and 65 correspondences"""
    probs = [PC.case_by_name(name).problem for name, _ in plan]
    got = run(ex, [as_dict(P, h) for P, (_, h) in zip(probs, plan)])
    sizes = set()
    for (name, h), P, g in zip(plan, probs, got):
        assert g["hyp"].shape == (h, 12) and len(P.samples) >= h
        check(P, g, name="%s x %d" % (name, h))
        sizes |= {int(c) for c, r in zip(g["n_inliers"], g["refined_n"]) if r >= 0}
    if any(name.startswith("refine_") for name, _ in plan):
        assert sizes & {11, 64, 65}, sizes


def test_without_inlier_bits(ex):
    cs = [PC.case_by_name(n) for n in ("all_n65", "groups_a_then_b", "nonfinite")]
    got = run(ex, [c.problem for c in cs], want_bits=False)
    for c, g in zip(cs, got):
        assert g["bits"] is None and g["refined_bits"] is None
        check(c.problem, g, name=c.name)
        assert same(g, single(ex, c.name))


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import PnpProblem, YgzfError
    L, h = ex.L, ex.h
    P = PC.case_by_name("gate_on").problem
    n, nh = len(P.P3D), budget(P)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    P3, P2, me = (np.ascontiguousarray(a, np.float32) for a in (P.P3D, P.P2D, P.max_err))
    smp = np.ascontiguousarray(P.samples[:nh], np.int32)
    hyp, cnt, bits = np.zeros((nh, 12)), np.zeros(nh, np.int32), np.zeros((nh, 1), np.uint64)
    rn, rh, rb = np.zeros(nh, np.int32), np.zeros((nh, 12)), np.zeros((nh, 1), np.uint64)

    def rec(n_=n, nh_=nh, s=smp, ms=4, **null):
        r = PnpProblem(n_, vp(P3), vp(P2), vp(me), (C.c_double * 4)(*P.K), ms, P.min_inliers, nh_, vp(s))
        for k in null:
            setattr(r, k, None)
        return (PnpProblem * 1)(r)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data if a is not None else None)
    outs = dict(hp=one(hyp), cp=one(cnt), bp=one(bits), rnp=one(rn), rhp=one(rh), rbp=one(rb))

    def call(r=None, nprob=1, **kw):
        o = dict(outs, **kw)
        return L.ygzf_pnp_ransac(h, nprob, rec() if r is None else r, o["hp"], o["cp"], o["bp"], o["rnp"], o["rhp"], o["rbp"])
    got = lambda with_bits=True: dict(hyp=hyp, n_inliers=cnt, bits=bits if with_bits else None, refined_n=rn, refined_hyp=rh, refined_bits=rb if with_bits else None)
    assert call() == 0
    check(P, got(), name="raw call")
    for bad in (0, -2):
        assert call(nprob=bad) == -1 and b"n_problems" in L.ygzf_last_error(h)
    assert L.ygzf_pnp_ransac(None, 1, rec(), *[outs[k] for k in ("hp", "cp", "bp", "rnp", "rhp", "rbp")]) == -1
    assert L.ygzf_pnp_ransac(h, 1, None, *[outs[k] for k in ("hp", "cp", "bp", "rnp", "rhp", "rbp")]) == -1 and b"null argument" in L.ygzf_last_error(h)
    for key in ("hp", "cp", "rnp", "rhp"):
        assert call(**{key: None}) == -1 and b"null argument" in L.ygzf_last_error(h)
        assert call(**{key: one(None)}) == -1 and b"null array" in L.ygzf_last_error(h)
    for field in ("P3Dw", "P2D", "max_err", "samples"):
        assert call(rec(**{field: True})) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(rec(n_=3)) == -1 and b"a hypothesis needs 4" in L.ygzf_last_error(h)
    assert call(rec(nh_=-1)) == -1 and b"negative hypothesis count" in L.ygzf_last_error(h)
    for ms in (3, 0, 9):
        assert call(rec(ms=ms)) == -1 and b"min_set" in L.ygzf_last_error(h)
    for bad_index in (-1, n):
        s2 = smp.copy()
        s2[1, 2] = bad_index
        assert call(rec(s=s2)) == -1 and b"outside [0, 20)" in L.ygzf_last_error(h)
    for a, b in ((1, 0), (3, 0), (3, 2)):
        s3 = smp.copy()
        s3[2, a] = s3[2, b]
        assert call(rec(s=s3)) == -1 and b"hypothesis 2 repeats an index" in L.ygzf_last_error(h)
    with pytest.raises(YgzfError):
        ex.pnp_ransac([])
    # n_hyp == 0 is legal and touches nothing: the pointers may be NULL, the outputs stay as they were
    for a in (hyp, cnt, bits, rn, rh, rb):
        a[:] = 7
    assert call(rec(n_=0, nh_=0, P3Dw=True, P2D=True, max_err=True, samples=True), hp=one(None), cp=one(None), bp=None, rnp=one(None), rhp=one(None), rbp=None) == 0
    assert call(rec(n_=2, nh_=0)) == 0
    assert all((a == 7).all() for a in (hyp, cnt, bits, rn, rh, rb))
    # inlier_bits and refined_bits as a whole may be NULL; and the context still works
    assert call(bp=None, rbp=None) == 0 and (bits == 7).all() and (rb == 7).all()
    check(P, got(False), name="after the errors")
    assert call(bp=None) == 0 and (bits == 7).all()
    assert np.array_equal(rb, PC.pnp_hypotheses(P, nh).refined_bits)


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
    cs = [PC.scene(n) for n in PC.SCENE_NAMES]
    a = run(ex, [c.problem for c in cs])
    m1, k1 = extract_and_match()
    b = run(ex, [c.problem for c in cs])
    for c, g, g2 in zip(cs, a, b):
        check(c.problem, g, name=c.name)
        assert same(g, g2)
    for f in range(2):
        assert np.array_equal(k0[f][0], k1[f][0]) and np.array_equal(k0[f][1], k1[f][1])
    assert np.array_equal(m0[1], m1[1])   # (pair 0 of the second run matches against the carried frame of the first)


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "pnp_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "pnp_shell.cc")] + [os.path.join(host, f) for f in ("PnPsolver.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def _run_shell(tmp_path, names, flags=("--min=0",)):
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    files = []
    for k, name in enumerate(names):
        path = str(tmp_path / ("case_%d.bin" % k))
        PC.write_case(PC.case_by_name(name).problem, path)
        files.append(path)
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe] + list(flags) + [out] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pnp shell ok" in r.stdout, r.stdout + r.stderr
    with open(out, "rb") as f:
        for name in names:
            c = PC.case_by_name(name)
            want = PC.expected(c).calls
            for j, w in enumerate(want):
                returned, n_inl, no_more, size = (int(v) for v in np.fromfile(f, np.int32, 4))
                T = np.fromfile(f, np.float32, 16).reshape(4, 4)
                inl = np.fromfile(f, np.uint8, size)
                print(name, j, (returned, n_inl, no_more, size), (w.kind, w.index, w.n_inliers, w.no_more, w.iterations))
                assert (bool(returned), n_inl, size) == (w.kind != PC.EMPTY, w.n_inliers, len(w.inliers)), (name, j)
                assert c.problem.calls[j] < 0 or bool(no_more) == bool(w.no_more), (name, j)
                assert np.array_equal(inl, w.inliers), (name, j)
                if returned:
                    assert np.array_equal(T.view(np.uint32), w.T.view(np.uint32)), (name, j)
        assert f.read() == b""
    return [PC.expected(PC.case_by_name(n)).calls for n in names]


def test_shell_round_robin_against_pnp_iterate(ex, tmp_path):
    """PnPsolverBatch over three solvers (and a fourth that was never batched and evaluates itself), then their calls round-robin as
    Tracking::Relocalization drives its candidates: every call's matrix, inlier vector, count and bNoMore are pnp_iterate's on the same sets"""
    calls = _run_shell(tmp_path, ["groups_a_then_b", "success_then_calls", "refine_exact_min", "scene_n60"])
    assert {k.kind for cs in calls for k in cs} >= {PC.REFINED, PC.BEST}, "both kinds of return are among the calls"


def test_shell_overrun_path(ex, tmp_path):
    """calls that run past mRansacMaxIts: the iterations beyond the device's budget are evaluated on the calling thread with the same arithmetic"""
    calls = _run_shell(tmp_path, ["overrun", "min_inliers_eq_n", "refine_exact_min"])
    for name, cs in zip(("overrun", "min_inliers_eq_n", "refine_exact_min"), calls):
        assert max(k.iterations for k in cs) > PC.case_by_name(name).problem.max_its, name


def test_shell_below_the_device_threshold(ex, tmp_path):
    """with the default ygzf_host_pnp_device_min a batch of three pre-evaluates nothing: every iteration is evaluated when it is reached, on
    the calling thread, and every return is the same"""
    _run_shell(tmp_path, ["groups_a_then_b", "overrun", "refine_exact_min", "scene_n60"], flags=())


def test_solver_blocks_beyond_packed_max_bypass_the_staging():
    """The four batched solvers lay a call's problems out as one block each way (ProblemBlock, csrc/ygzf_ctx.h).  Beyond kPackedMax the blocks
    cross without the page-locked staging area, one copy each way from / to the block itself (PackedTransfer::direct).  With
    YGZF_FORCE=packed_max=4096 the small batches of the four suites take that path: n = 0, 1, 2, 3, 63, 64, 65, problems without hypotheses,
    a problem above 4096 bytes beside one below, and PnP's masks as a device-only tail (test_without_inlier_bits).  They must hold unchanged.
    The child (20 tests) took 2.4 and 2.8 s in two sessions on an MI355X at the commit before ProblemBlock, interpreter start included; the
    timeout is ten times that and more, a backstop against a hang and no speed assertion."""
    import sys
    from orb_ygz_slam_amd.capi import force_env
    env = dict(os.environ, YGZF_FORCE=force_env(packed_max=4096))
    files = [os.path.join(ROOT, "tests", "test_gpu_%s.py" % s) for s in ("pose_opt", "sim3_opt", "sim3", "pnp")]
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + files +
                         ["-k", "(test_batches or test_mixed_batches or test_without_inlier_bits) and not beyond_packed_max"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=30)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "skipped" not in out.stdout, out.stdout[-1000:]
