"""GPU tests of SearchByBoW(KeyFrame, KeyFrame) on the device -- ygzf_search_by_bow_kf, k_bow_kf_nodes / k_bow_kf_finish -- against the numpy
restatement of tests/bow_kf_cases.py, bit for bit, on the seeded scenes (whose quality and whose pin to the reference's code
tests/test_bow_kf_cases.py checks on the CPU) and on every constructed case; a batch against single calls; two passes on one context; empty
inputs; argument errors; the context's batch state across a call; the host shells (ORBmatcher::SearchByBoW(KF, KF, ..) and
ygz::SearchByBoWBatch in ORBmatcherLoop.cc) end to end."""
import os
import subprocess

import numpy as np
import pytest

from orb_ygz_slam_amd.capi import KP_DTYPE, Extractor, YgzfError, make_camera
from tests import bow_kf_cases as K
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = K.cases()
PARAMS = ((0.75, True), (0.9, False), (0.6, True))
_scenes = {}


def scene(seed):
    """-> (kf1, candidates as the device takes them, kf2s, joined lists); built once per seed and left unchanged"""
    if seed not in _scenes:
        kf1, cands = K.bow_kf_scene(seed)
        joined = [K.join(kf1["fv"], c["fv"]) for c in cands]
        _scenes[seed] = (kf1, [K.candidate(c, j) for c, j in zip(cands, joined)], cands, joined)
    return _scenes[seed]


_refs = {}


def ref(seed, k, ratio, ori):
    if (seed, k, ratio, ori) not in _refs:
        kf1, _, cands, joined = scene(seed)
        _refs[(seed, k, ratio, ori)] = K.ref_search_by_bow_kf(kf1, cands[k], joined[k], ratio, ori)[:2]
    return _refs[(seed, k, ratio, ori)]


@pytest.fixture(scope="module")
def ex():
    e = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.parametrize("ratio,ori", PARAMS)
@pytest.mark.parametrize("seed", K.SCENE_SEEDS)
def test_scene_matches_restatement(ex, seed, ratio, ori):
    kf1, dc, _, _ = scene(seed)
    m, n = ex.search_by_bow_kf(kf1, dc, ratio, ori)
    assert m.shape == (len(dc), len(kf1["keys"])) and n.shape == (len(dc),)
    for k in range(len(dc)):
        rm, rn = ref(seed, k, ratio, ori)
        bad = np.flatnonzero(m[k] != rm)
        assert not len(bad) and n[k] == rn, (seed, ratio, ori, k, bad[:10], m[k][bad[:10]], rm[bad[:10]], n[k], rn)


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_constructed_case(ex, case):
    m, n = ex.search_by_bow_kf(case.kf1, [K.candidate(case.kf2, case.joined)], case.nnratio, case.check_ori)
    rm, rn, _ = case.ref()
    assert np.array_equal(rm, case.expect)
    assert np.array_equal(m[0], case.expect) and n[0] == rn, (m[0], case.expect, n[0], rn)


def test_batch_equals_single_calls(ex):
    kf1, dc, cands, _ = scene(K.SCENE_SEEDS[1])
    no_common = dict(dc[1], off1=np.zeros(1, np.int32), idx1=np.zeros(0, np.int32), off2=np.zeros(1, np.int32), idx2=np.zeros(0, np.int32))
    no_keys = dict(keys=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8), valid=np.zeros(0, np.uint8), off1=dc[2]["off1"], idx1=dc[2]["idx1"],
                   off2=np.zeros_like(dc[2]["off2"]), idx2=np.zeros(0, np.int32))
    batch = [dc[0], no_common, dc[3], dc[0], no_keys, dc[2]]
    m, n = ex.search_by_bow_kf(kf1, batch)
    for k, c in enumerate(batch):
        sm, sn = ex.search_by_bow_kf(kf1, [c])
        assert np.array_equal(m[k], sm[0]) and n[k] == sn[0], k
    assert np.array_equal(m[0], m[3]) and n[0] == n[3] > 20
    assert (m[1] == -1).all() and n[1] == 0 and (m[4] == -1).all() and n[4] == 0
    assert np.array_equal(m[5], ref(K.SCENE_SEEDS[1], 2, 0.75, True)[0])


def test_two_passes_on_one_context(ex):
    kf1, dc, _, _ = scene(K.SCENE_SEEDS[0])
    a = ex.search_by_bow_kf(kf1, dc)
    ex.search_by_bow_kf(CASES[0].kf1, [K.candidate(CASES[0].kf2, CASES[0].joined)])
    b = ex.search_by_bow_kf(kf1, dc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_empty_inputs_give_presets(ex):
    kf1, dc, _, _ = scene(K.SCENE_SEEDS[2])
    m, n = ex.search_by_bow_kf(kf1, [])
    assert m.shape == (0, len(kf1["keys"])) and n.shape == (0,)
    empty = dict(keys=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8), valid=np.zeros(0, np.uint8))
    m, n = ex.search_by_bow_kf(empty, [dict(dc[0], off1=np.zeros(1, np.int32), off2=np.zeros(1, np.int32))])
    assert m.shape == (1, 0) and n[0] == 0
    m, n = ex.search_by_bow_kf(kf1, [dict(dc[0], n=0), dict(dc[1], n_nodes=0)])
    assert (m == -1).all() and (n == 0).all()


def test_argument_errors_leave_the_context_usable(ex):
    kf1, dc, _, _ = scene(K.SCENE_SEEDS[2])
    c = dc[0]
    n1, n2 = len(kf1["keys"]), len(c["keys"])
    bad = [(dict(kf1, desc=None), [c], "null"), (dict(kf1, valid=None), [c], "null")]
    full = dict(c, n=n2, n_nodes=len(c["off1"]) - 1)       # (the wrapper takes the counts from keys / off1 unless they are given)
    bad += [(kf1, [dc[1], dict(full, **{name: None})], "null") for name in ("keys", "desc", "valid", "off1", "idx1", "off2", "idx2")]
    i1, i2 = c["idx1"].copy(), c["idx2"].copy()
    i1[3], i2[5] = n1, -1
    bad += [(kf1, [dict(c, idx1=i1)], "out of range"), (kf1, [dict(c, idx2=i2)], "out of range")]
    o1, o2 = c["off1"].copy(), c["off2"].copy()
    o1[2], o2[1] = o1[3] + 1, o2[2] + 1
    bad += [(kf1, [dict(c, off1=o1)], "ascending"), (kf1, [dict(c, off2=o2)], "ascending")]
    wide = dict(c, off1=np.array([0, 1], np.int32), idx1=np.zeros(1, np.int32), off2=np.array([0, 4097], np.int32), idx2=np.arange(4097, dtype=np.int32) % n2)
    bad += [(kf1, [wide], "4096")]
    bad += [(dict(kf1, n=-1), [c], "negative"), (kf1, [dict(c, n=-1)], "negative"), (kf1, [dict(c, n_nodes=-2)], "negative")]
    for a, cs, word in bad:
        with pytest.raises(YgzfError) as e:
            ex.search_by_bow_kf(a, cs)
        assert word in str(e.value), (word, str(e.value))
    ok = dict(wide, off2=np.array([0, 4096], np.int32), idx2=wide["idx2"][:4096])      # the limit itself is accepted
    ex.search_by_bow_kf(kf1, [ok])
    m, n = ex.search_by_bow_kf(kf1, dc)
    assert np.array_equal(m[0], ref(K.SCENE_SEEDS[2], 0, 0.75, True)[0])


def test_call_keeps_context_batch_state():
    """A search between extract_batch_host and match_batch_prev leaves the match results unchanged."""
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.stack([synth_frame(50 + s, 752, 480) for s in range(4)])
    cam = make_camera(752, 480)
    kf1, dc, _, _ = scene(K.SCENE_SEEDS[1])
    results = []
    for between in (False, True):
        e = Extractor(1000, 1.2, 8, 20, 7, 752, 480, max_batch=4)
        try:
            e.extract_batch_host(frames[:2])
            e.match_batch_prev(cam)
            e.extract_batch_host(frames[2:])
            if between:
                assert (e.search_by_bow_kf(kf1, dc)[1] > 20).all()
            e.match_batch_prev(cam)
            results.append([e.match_fetch(p) for p in range(2)] + [e.match_counts().copy()])
        finally:
            e.close()
    a, b = results
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        else:
            assert np.array_equal(x, y)


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "bow_kf_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "bow_kf_shell.cc")] + [os.path.join(host, f) for f in
                                                                    ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ORBmatcherLoop.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def _write_kf(f, kf):
    n = len(kf["keys"])
    state = np.where(kf["valid"] != 0, 1, np.where(np.arange(n) % 2 == 0, 0, 2)).astype(np.uint8)   # not valid: an empty slot or a bad MapPoint
    f.write(np.int32(n).tobytes() + np.ascontiguousarray(kf["keys"]).tobytes() + np.ascontiguousarray(kf["desc"]).tobytes() + state.tobytes())
    f.write(np.int32(len(kf["fv"])).tobytes())
    for node in sorted(kf["fv"]):
        f.write(np.array([node, len(kf["fv"][node])] + list(kf["fv"][node]), np.int32).tobytes())


def test_bow_kf_shell_end_to_end(tmp_path):
    """ORBmatcher(0.75, true).SearchByBoW(kf1, kf2, v) per candidate and ygz::SearchByBoWBatch over the device, from KeyFrames with mFeatVec maps
    and MapPoints (some bad, some slots NULL), return the MapPoints and counts of the restatement."""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    seed = K.SCENE_SEEDS[1]
    kf1, _, cands, _ = scene(seed)
    path = os.path.join(str(tmp_path), "scene.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(cands)).tobytes())
        _write_kf(f, kf1)
        for c in cands:
            _write_kf(f, c)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bow kf shell ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    rows = {(w[0], int(w[1])): (int(w[2]), np.array(w[3:], np.int32)) for w in (l.split() for l in out.stdout.splitlines()) if w and w[0] in ("single", "batch")}
    enough = 0
    for k in range(len(cands)):
        rm, rn = ref(seed, k, 0.75, True)
        enough += rn >= 20
        for form in ("single", "batch"):
            n, slots = rows[(form, k)]
            assert n == rn and np.array_equal(slots, np.where(rm >= 0, rm, -1)), (form, k, n, rn)
    assert "enough %d\n" % enough in out.stdout and enough > 0
