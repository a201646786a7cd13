"""GPU tests of ygzf_triangulate_pairs (the per-pair body of LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:1060-1194) against
tests/triangulate_cases.py: x3D equal as uint32 and the status equal as bytes -- every constructed case and both seeded scenes, twice on one
context; the pair counts at which the indexing can go wrong (0, 1, 63, 64, 65, 255, 256, 257) as one problem and as mixed batches whose problems
end inside a wave and inside a workgroup, with empty problems first, in the middle and last, forwards and reversed; a batch against single
calls; one keyframe as kf2 of several problems; a monocular kf2 beside a stereo one in one call; argument errors; a context that extracts and
matches around the calls."""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from orb_ygz_slam_amd import Extractor
    e = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=2)
    yield e
    e.close()


_KF = {}


def api_kf(kf):
    """a keyframe of triangulate_cases as the binding takes it; one keyframe is one dict, so the binding names its arrays once"""
    from orb_ygz_slam_amd.capi import Camera
    if id(kf) not in _KF:
        d = {k: kf.get(k) for k in ("keys", "u_right", "depth", "cos_stereo", "scale_factors", "level_sigma2", "Rcw", "tcw", "Ow", "Twc_q", "Twc_t", "invfx", "invfy")}
        d["cam"] = Camera(*[float(kf[k]) for k in ("fx", "fy", "cx", "cy", "mb", "mbf")], 0, 0, 0, 0)
        _KF[id(kf)] = (kf, d)   # the source is kept alive: its id stays its own
    return _KF[id(kf)][1]


def run(ex, kf1, ratio, problems):
    """problems: (kf2, idx1, idx2)"""
    return ex.triangulate_pairs(api_kf(kf1), ratio, [dict(kf2=api_kf(k2), idx1=i1, idx2=i2) for k2, i1, i2 in problems])


def check(got, want, name=""):
    x3d, status = got
    wx, ws, _ = TC.as_arrays(want)
    print("%s: %d pairs, %d accepted, sources %s" % (name, len(ws), int((ws & 15 == 0).sum()), np.bincount(ws >> 6, minlength=4).tolist()))
    assert x3d.shape == wx.shape and status.shape == ws.shape
    assert np.array_equal(status, ws), "status differs from the restatement"
    assert np.array_equal(x3d.view(np.uint32), wx.view(np.uint32)), "x3D differs from the restatement in some bit"


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_single_call_twice(ex, name):
    """the case, a scene's pairs, the case again on one context: the restatement both times, bit-equal to each other"""
    c = TC.case_by_name(name)
    a = run(ex, c.kf1, c.ratio, [(c.kf2, [c.idx1], [c.idx2])])[0]
    k1, k2, i1, i2, ratio = TC.scene("mono")
    run(ex, k1, ratio, [(k2, i1[:70], i2[:70])])
    b = run(ex, c.kf1, c.ratio, [(c.kf2, [c.idx1], [c.idx2])])[0]
    check(a, [TC.expected(c)], name)
    assert same(a, b)


@pytest.mark.parametrize("name", TC.SCENE_NAMES)
def test_seeded_scene_twice(ex, name):
    k1, k2, i1, i2, ratio = TC.scene(name)
    a = run(ex, k1, ratio, [(k2, i1, i2)])[0]
    c = TC.case_by_name("v33_zero")
    run(ex, c.kf1, c.ratio, [(c.kf2, [c.idx1], [c.idx2])])
    b = run(ex, k1, ratio, [(k2, i1, i2)])[0]
    check(a, TC.scene_expected(name), name)
    assert same(a, b)


# ---- the stereo scene's KF1 against its KF2 and against a monocular copy of that KF2 (NULL stereo arrays) -------------------------------------------
_MONO = {}


def variants():
    """-> kf1, ratio, {"stereo" | "mono": (kf2, idx1, idx2, the restatement's pairs)}"""
    k1, k2, i1, i2, ratio = TC.scene("stereo")
    if not _MONO:
        m = dict(k2)
        m["u_right"] = m["depth"] = m["cos_stereo"] = None
        _MONO["kf"] = m
        _MONO["want"] = [TC.tri_pair(k1, m, int(a), int(b), ratio) for a, b in zip(i1, i2)]
    return k1, ratio, {"stereo": (k2, i1, i2, TC.scene_expected("stereo")), "mono": (_MONO["kf"], i1, i2, _MONO["want"])}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_pair_counts_as_one_problem(ex, n):
    k1, ratio, V = variants()
    k2, i1, i2, want = V["stereo"]
    got = run(ex, k1, ratio, [(k2, i1[:n], i2[:n])])[0]
    if n == 0:
        assert got[0].shape == (0, 3) and got[1].shape == (0,)
    else:
        check(got, want[:n], "n = %d" % n)


PLANS = {"ends_inside_a_wave_and_a_workgroup": [3, 61, 1, 192], "one_past_a_workgroup": [255, 2, 43], "empty_first_middle_last": [0, 3, 61, 0, 0, 1, 192, 0],
         "empty_reversed": [0, 192, 1, 0, 0, 61, 3, 0], "every_problem_one_pair": [1] * 70}


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_mixed_batches_against_single_calls(ex, plan):
    """problems alternate between the stereo KF2 and its monocular copy, so each keyframe is kf2 of several problems and both kinds share a
    launch; every problem takes the next pairs of the scene, so a problem's results cannot be another's"""
    k1, ratio, V = variants()
    problems, wants, at = [], [], 0
    for j, n in enumerate(PLANS[plan]):
        k2, i1, i2, want = V["stereo" if j % 2 == 0 else "mono"]
        problems.append((k2, i1[at:at + n], i2[at:at + n]))
        wants.append(want[at:at + n])
        at += n
    assert at <= TC.SCENE_PAIRS
    got = run(ex, k1, ratio, problems)
    for j, (g, w) in enumerate(zip(got, wants)):
        if len(w):
            check(g, w, "%s[%d]" % (plan, j))
        else:
            assert g[1].shape == (0,)
    for j in (1, len(problems) - 2):
        assert same(got[j], run(ex, k1, ratio, [problems[j]])[0]), "problem %d differs from its single call" % j


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import TriProblem, YgzfError
    L, h = ex.L, ex.h
    k1, ratio, V = variants()
    k2, i1, i2, want = V["stereo"]
    n = 40
    i1, i2 = np.ascontiguousarray(i1[:n]), np.ascontiguousarray(i2[:n])
    keep, cache = [], {}
    K1, K2 = ex._tri_kf(api_kf(k1), keep, cache), ex._tri_kf(api_kf(k2), keep, cache)
    x3d, status = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data if a is not None else None)

    def rec(n_=n, a=i1, b=i2, kf2=K2):
        r = TriProblem()
        r.kf2 = kf2
        r.n_pairs, r.idx1, r.idx2 = n_, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data
        return (TriProblem * 1)(r)

    def edited(K, **fields):
        from orb_ygz_slam_amd.capi import TriKf
        c = TriKf.from_buffer_copy(K)
        for name, v in fields.items():
            if "." in name:
                setattr(getattr(c, name.split(".")[0]), name.split(".")[1], v)
            else:
                setattr(c, name, v)
        return c
    call = lambda r=None, nprob=1, kf1=K1, xp=one(x3d), sp=one(status): L.ygzf_triangulate_pairs(h, C.byref(kf1) if kf1 is not None else None, ratio,
                                                                                                   nprob, rec() if r is None else r, xp, sp)
    assert call() == 0
    check((x3d, status), want[:n], "raw call")
    for bad in (0, -2):
        assert call(nprob=bad) == -1 and b"n_problems" in L.ygzf_last_error(h)
    assert L.ygzf_triangulate_pairs(None, C.byref(K1), ratio, 1, rec(), one(x3d), one(status)) == -1
    assert call(kf1=None) == -1 and b"null argument" in L.ygzf_last_error(h)
    assert L.ygzf_triangulate_pairs(h, C.byref(K1), ratio, 1, None, one(x3d), one(status)) == -1 and b"null argument" in L.ygzf_last_error(h)
    assert call(xp=None) == -1 and call(sp=None) == -1
    assert call(xp=one(None)) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(sp=one(None)) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(rec(a=None)) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(rec(b=None)) == -1 and b"problem 0: null array" in L.ygzf_last_error(h)
    assert call(rec(n_=-1)) == -1 and b"negative pair count" in L.ygzf_last_error(h)
    for bad_index in (-1, TC.SCENE_PAIRS):
        j = i1.copy()
        j[7] = bad_index
        assert call(rec(a=j)) == -1 and b"of kf1 outside [0, 300)" in L.ygzf_last_error(h)
        assert call(rec(b=j)) == -1 and b"of kf2 outside [0, 300)" in L.ygzf_last_error(h)
    keys = np.ascontiguousarray(k2["keys"]).copy()
    for bad_octave in (-1, 8):
        keys["octave"][11] = bad_octave
        assert call(rec(kf2=edited(K2, **{"view.keys": keys.ctypes.data}))) == -1 and b"kf2: keypoint octave" in L.ygzf_last_error(h)
        assert call(kf1=edited(K1, **{"view.keys": keys.ctypes.data})) == -1 and b"kf1: keypoint octave" in L.ygzf_last_error(h)
    assert call(rec(kf2=edited(K2, **{"view.keys": None}))) == -1 and b"kf2: null keys" in L.ygzf_last_error(h)
    assert call(kf1=edited(K1, **{"view.n": -1})) == -1
    assert call(rec(kf2=edited(K2, depth=None))) == -1 and b"u_right without depth or cos_stereo" in L.ygzf_last_error(h)
    assert call(kf1=edited(K1, cos_stereo=None)) == -1 and b"u_right without depth or cos_stereo" in L.ygzf_last_error(h)
    with pytest.raises(YgzfError):
        ex.triangulate_pairs(api_kf(k1), ratio, [])
    # n_pairs == 0 is legal and touches nothing: the pointers may be NULL, the outputs stay as they were
    x3d[:], status[:] = 7, 7
    assert call(rec(n_=0, a=None, b=None, kf2=edited(K2, **{"view.keys": None})), xp=one(None), sp=one(None)) == 0
    assert (x3d == 7).all() and (status == 7).all()
    # and the context still works
    assert call() == 0
    check((x3d, status), want[:n], "after the errors")


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
    k1, k2, i1, i2, ratio = TC.scene("stereo")
    a = run(ex, k1, ratio, [(k2, i1, i2)])[0]
    m1, kk1 = extract_and_match()
    b = run(ex, k1, ratio, [(k2, i1, i2)])[0]
    check(a, TC.scene_expected("stereo"), "between the batches")
    assert same(a, b)
    for f in range(2):
        assert np.array_equal(k0[f][0], kk1[f][0]) and np.array_equal(k0[f][1], kk1[f][1])
    assert np.array_equal(m0[1], m1[1])   # (pair 0 of the second run matches against the carried frame of the first)


# ---- the shells of host/LocalMappingTriangulate.cc (tests/cpp/tri_shell.cc) ---------------------------------------------------------------------------
import ctypes.util
import os
import subprocess

from tests.conftest import ROOT

HOST_FORCED, DEVICE_FORCED, DEFAULT_MIN = 1 << 30, 0, -1


@pytest.fixture(scope="module")
def shell(tmp_path_factory):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = str(tmp_path_factory.mktemp("tri_shell") / "tri_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "tri_shell.cc")] + [os.path.join(host, f) for f in ("LocalMappingTriangulate.cc", "ORBmatcher.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def shell_kf(kf):
    """the keyframe with the stereo cosine the shell computes: the reference's cos(2 * atan2(mb / 2, depth)) in float, by this host's libm"""
    if kf.get("u_right") is None:
        return kf
    m = C.CDLL(ctypes.util.find_library("m"))
    m.cosf.restype = m.atan2f.restype = C.c_float
    m.cosf.argtypes, m.atan2f.argtypes = [C.c_float], [C.c_float, C.c_float]
    half = float(np.float32(kf["mb"]) / np.float32(2))
    out = dict(kf)
    out["cos_stereo"] = np.array([m.cosf(float(np.float32(2) * np.float32(m.atan2f(half, float(d))))) for d in kf["depth"]], np.float32)
    return out


_SHELL_WANT = {}


def shell_scene(name):
    if name not in _SHELL_WANT:
        k1, k2, i1, i2, ratio = TC.scene(name)
        k1, k2 = shell_kf(k1), shell_kf(k2)
        _SHELL_WANT[name] = (k1, k2, i1, i2, ratio, TC.as_arrays([TC.tri_pair(k1, k2, int(a), int(b), ratio) for a, b in zip(i1, i2)]))
    return _SHELL_WANT[name]


@pytest.mark.parametrize("n", [40, TC.SCENE_PAIRS])
@pytest.mark.parametrize("minimum", [DEVICE_FORCED, HOST_FORCED, DEFAULT_MIN])
@pytest.mark.parametrize("name", TC.SCENE_NAMES)
def test_shell_one_neighbour(ex, shell, tmp_path, name, minimum, n):
    """ygz::TriangulatePairsDevice with the device forced, the host forced and the default threshold (64: 40 pairs stay on the host, 300 go to
    the device): the restatement bit for bit every time, over the cosines the shell computes itself"""
    k1, k2, i1, i2, ratio, want = shell_scene(name)
    TC.write_pairs(str(tmp_path / "in.bin"), k1, k2, i1[:n], i2[:n], ratio)
    r = subprocess.run([shell, "pairs", str(minimum), repr(float(k1["mb"])), repr(float(k2["mb"])), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(str(tmp_path / "out.bin"), "rb") as f:
        x3d, status = np.fromfile(f, np.float32, 3 * n).reshape(n, 3), np.fromfile(f, np.uint8, n)
    assert np.array_equal(status, want[1][:n]) and np.array_equal(x3d.view(np.uint32), want[0][:n].view(np.uint32))


@pytest.mark.parametrize("minimum,stop,mono,n,neighbours", [(DEVICE_FORCED, -1, 0, 120, 3), (HOST_FORCED, -1, 0, 120, 3), (DEFAULT_MIN, -1, 0, 120, 3),
                                                            (DEFAULT_MIN, -1, 0, 40, 1), (DEFAULT_MIN, 2, 0, 120, 3), (DEVICE_FORCED, 1, 1, 120, 3),
                                                            (DEVICE_FORCED, -1, 1, 120, 3)])
def test_shell_create_new_map_points_batch(ex, shell, tmp_path, minimum, stop, mono, n, neighbours):
    """ygz::CreateNewMapPointsBatch -- real SearchForTriangulation, one ygzf_triangulate_pairs, TriangulateApply -- against the neighbour loop as
    the reference runs it (the program compares points, slots, normals and distances), and every created point against the restatement.  Every
    neighbour matches the same KF1 features, so the drop rule decides most pairs; the poll stops the loop before neighbour 1 or 2."""
    k1, problems, ratio = TC.make_scene(8100 + n, n, not mono, neighbours)
    k1 = shell_kf(k1)
    kfs = [shell_kf(k2) for k2, _, _ in problems]
    files = []
    for j, (k2, (_, i1, i2)) in enumerate(zip(kfs, problems)):
        files.append(str(tmp_path / ("p%d.bin" % j)))
        TC.write_pairs(files[-1], k1, k2, i1, i2, ratio)
    r = subprocess.run([shell, "batch", str(minimum), str(mono), str(stop), str(tmp_path / "out.bin"), repr(float(k1["mb"]))] + files,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tri shell ok" in r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())
    with open(str(tmp_path / "out.bin"), "rb") as f:
        count = int(np.fromfile(f, np.int32, 1)[0])
        recs = [(np.fromfile(f, np.int32, 3), np.fromfile(f, np.float32, 3)) for _ in range(count)]
    assert count >= (10 if stop == 1 or n < 100 else 40)
    seen1 = set()
    for (j, a, b), x in recs:
        assert 0 <= j < (neighbours if stop < 0 else stop) and a == b and a not in seen1   # the true partner; a KF1 feature gets one point
        seen1.add(int(a))
        want = TC.tri_pair(k1, kfs[j], int(a), int(b), ratio)
        assert want.status == TC.ACCEPTED and np.array_equal(want.x3d.view(np.uint32), x.view(np.uint32))
    if stop < 0 and neighbours > 1:
        assert len({int(j) for (j, _, _), _ in recs}) > 1   # later neighbours create what the earlier ones rejected
