"""GPU tests of the loop-closing projection searches on the device -- ygzf_fuse_sim3_candidates (ORBmatcher::Fuse(pKF, Scw, ..)),
ygzf_search_by_projection_sim3 (SearchByProjection(pKF, Scw, ..)) and ygzf_search_by_sim3 (SearchBySim3) -- against the numpy restatement of
tests/loop_cases.py, bit for bit, on seeded scenes (orb_ygz_slam_amd/loop_scene.py, whose quality tests/test_loop_cases.py checks on the CPU) and
on the constructed points; batch against single calls; n_best lists; empty inputs, argument errors, the context's batch state across a call; the
host shells (ORBmatcherLoop.cc, ygz::SearchAndFuseBatch over host/LoopApply.h) end to end against the sequential restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from orb_ygz_slam_amd import loop_scene
from orb_ygz_slam_amd.capi import Extractor, YgzfError, make_camera
from tests import loop_cases as LC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def ex():
    e = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuse_sim3_matches_restatement(oracle, ex, seed):
    kfs, pts = loop_scene.loop_scene(seed)
    K, P = len(kfs), len(pts[0])
    skip = (np.random.default_rng(100 + seed).random((K, P)) < 0.1).astype(np.uint8)
    for th, sk in ((4.0, None), (6.0, skip)):
        bi, bd = ex.fuse_sim3_candidates(kfs, *pts, th=th, skip=sk)
        assert bi.shape == (K, P) and bd.shape == (K, P)
        for k in range(K):
            ri, rd = LC.ref_search(oracle, kfs[k], *pts, th, "fuse", skip=None if sk is None else sk[k])
            bad = np.nonzero((bi[k] != ri[:, 0]) | (bd[k] != rd[:, 0]))[0]
            assert not len(bad), (seed, th, k, bad[:10], bi[k][bad[:10]], ri[bad[:10], 0])
        found = bi >= 0
        assert found.sum() > 20 and ((bd <= LC.TH_LOW) & found).any() and ((bd > LC.TH_LOW) & found).any() and (~found).any()
        if sk is not None:
            assert (bi[sk != 0] == -1).all() and (bd[sk != 0] == 256).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_search_by_projection_matches_restatement(oracle, ex, seed):
    kfs, pts = loop_scene.loop_scene(seed)
    P = len(pts[0])
    rng = np.random.default_rng(200 + seed)
    skip = (rng.random(P) < 0.1).astype(np.uint8)
    for k, kf in enumerate(kfs):
        km = (rng.random(len(kf["keys"])) < 0.3).astype(np.uint8)
        for sk, mask, nb, md in ((None, None, 1, 255), (skip, km, 4, LC.TH_LOW), (None, km, 8, 80), (skip, np.zeros_like(km), 2, 0)):
            ci, cd = ex.search_by_projection_sim3(kf, *pts, th=10.0, skip=sk, key_matched=mask, n_best=nb, max_dist=md)
            assert ci.shape == (P, nb)
            ri, rd = LC.ref_search(oracle, kf, *pts, 10.0, "proj", skip=sk, key_matched=mask, n_best=nb, max_dist=md)
            bad = np.nonzero(((ci != ri) | (cd != rd)).any(axis=1))[0]
            assert not len(bad), (seed, k, nb, md, bad[:10], ci[bad[:3]], ri[bad[:3]])
            if mask is not None and md > 0:
                got = ci[ci >= 0]
                assert len(got) and not mask[got].any()                   # no masked key ever comes back
            if sk is not None:
                assert (ci[sk != 0] == -1).all() and (cd[sk != 0] == 256).all()
    # the mask matters in this scene: some point's best key changes with it
    a, _ = ex.search_by_projection_sim3(kfs[0], *pts, th=10.0)
    km = np.zeros(len(kfs[0]["keys"]), np.uint8)
    km[a[a >= 0][::2]] = 1
    b, _ = ex.search_by_projection_sim3(kfs[0], *pts, th=10.0, key_matched=km)
    assert (a != b).any()


def test_n_best_lists(ex):
    """Ascending (distance, then the list order the device walks), -1 / 256 padded at the end, and the head equals the n_best = 1 answer."""
    kfs, pts = loop_scene.loop_scene(5, P=400)
    kf = kfs[0]
    one_i, one_d = ex.search_by_projection_sim3(kf, *pts, th=10.0, n_best=1, max_dist=LC.TH_LOW)
    for nb in (2, 4, 8):
        ci, cd = ex.search_by_projection_sim3(kf, *pts, th=10.0, n_best=nb, max_dist=LC.TH_LOW)
        assert (ci[:, 0] == one_i[:, 0]).all() and (cd[:, 0] == one_d[:, 0]).all()
        assert (np.diff(cd, axis=1) >= 0).all()
        valid = ci >= 0
        assert (valid[:, :-1] | ~valid[:, 1:]).all()                       # padding only at the end
        assert (cd[valid] <= LC.TH_LOW).all() and (cd[~valid] == 256).all()
        for row in ci:                                                     # no key twice in a list
            r = row[row >= 0]
            assert len(set(r.tolist())) == len(r)
        assert valid[:, 1].any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_constructed_points(oracle, ex, seed):
    kf, pts, labels, km = LC.constructed_scw(oracle, seed)
    ci, cd = ex.search_by_projection_sim3(kf, *pts, th=10.0, key_matched=km)
    ri, rd = LC.ref_search(oracle, kf, *pts, 10.0, "proj", key_matched=km)
    assert (ci == ri).all() and (cd == rd).all(), (labels, ci[:, 0], ri[:, 0])
    assert dict(zip(labels, ci[:, 0] >= 0)) == LC.SCW_EXPECT
    for mutation, flips in LC.SCW_FLIPS.items():                           # the wrong form gives another answer on exactly those points
        mi, _ = LC.ref_search(oracle, kf, *pts, 10.0, "proj", key_matched=km, mutation=mutation)
        assert {lab for lab, a, b in zip(labels, mi[:, 0], ci[:, 0]) if a != b} == flips, mutation
    bi, bd = ex.fuse_sim3_candidates([kf], *pts, th=4.0)
    fi, fd = LC.ref_search(oracle, kf, *pts, 4.0, "fuse")
    assert (bi[0] == fi[:, 0]).all() and (bd[0] == fd[:, 0]).all(), (labels, bi[0], fi[:, 0])
    for mutation in ("norm_float", "dot_float"):
        mi, _ = LC.ref_search(oracle, kf, *pts, 4.0, "fuse", mutation=mutation)
        assert {lab for lab, a, b in zip(labels, mi[:, 0], bi[0]) if a != b} == LC.SCW_FLIPS[mutation], mutation
    # Sim3: norm(Pc) in the target camera's frame.  The entry point runs two rows; the constructed row is the first (KF1's points into KF2)
    kf, pts, labels, R2, t2 = LC.constructed_sim3(seed)
    n = len(kf["keys"])
    assert len(pts[0]) <= n
    pad = lambda a: np.concatenate([a, np.repeat(a[:1], n - len(a), axis=0)])
    p1 = tuple(pad(a) for a in (pts[0], pts[2], pts[3], pts[4], pts[5]))
    skip1 = np.ones(n, np.uint8)
    skip1[:len(pts[0])] = 0
    T = dict(R1w=np.eye(3, dtype=f32), t1w=np.zeros(3, f32), sR21=R2, t21=t2, R2w=np.eye(3, dtype=f32), t2w=np.zeros(3, f32),
             sR12=np.eye(3, dtype=f32), t12=np.zeros(3, f32))
    nf, m12, m1, m2 = ex.search_by_sim3(kf, kf, p1, p1, T, th=7.5, th_dist=LC.TH_HIGH, skip1=skip1, skip2=np.ones(n, np.uint8))
    ri, rd = LC.ref_search(oracle, kf, *pts, 7.5, "sim3", R2=R2, t2=t2)
    assert (m1[:len(labels)] == np.where(rd[:, 0] <= LC.TH_HIGH, ri[:, 0], -1)).all()
    assert dict(zip(labels, m1[:len(labels)] >= 0)) == LC.SIM3_EXPECT
    mi, _ = LC.ref_search(oracle, kf, *pts, 7.5, "sim3", R2=R2, t2=t2, mutation="sim3_world_norm")
    assert {lab for lab, a, b in zip(labels, mi[:, 0], m1) if a != b} == set(labels)
    assert nf == 0 and (m2 == -1).all() and (m12 == -1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_search_by_sim3_matches_restatement(oracle, ex, seed):
    kf1, kf2, p1, p2, has1, has2, T = loop_scene.sim3_pair(seed)
    for s1, s2 in ((1 - has1, 1 - has2), (None, None)):
        nf, m12, m1, m2 = ex.search_by_sim3(kf1, kf2, p1, p2, T, th=7.5, th_dist=LC.TH_HIGH, skip1=s1, skip2=s2)
        rn, r12, r1, r2 = LC.ref_sim3(oracle, kf1, kf2, p1, p2, T, 7.5, LC.TH_HIGH, skip1=s1, skip2=s2)
        assert (m1 == r1).all(), np.nonzero(m1 != r1)[0][:10]
        assert (m2 == r2).all(), np.nonzero(m2 != r2)[0][:10]
        assert (m12 == r12).all() and nf == rn
        assert nf > 0 and nf == (m12 >= 0).sum()
        assert ((m1 >= 0) & (m12 < 0)).any() and (m2 >= 0).sum() > nf                # one-sided matches, rejected by the agreement loop
    # another threshold moves the result (distances lie on both sides of TH_HIGH)
    nf2, _, m1b, _ = ex.search_by_sim3(kf1, kf2, p1, p2, T, th=7.5, th_dist=60, skip1=1 - has1, skip2=1 - has2)
    nf1, _, m1a, _ = ex.search_by_sim3(kf1, kf2, p1, p2, T, th=7.5, th_dist=LC.TH_HIGH, skip1=1 - has1, skip2=1 - has2)
    assert (m1a >= 0).sum() > (m1b >= 0).sum() and nf1 >= nf2


def test_batch_equals_single_calls(ex):
    kfs, pts = loop_scene.loop_scene(7, P=600)
    kfs = kfs + [kfs[0], kfs[2]]                                           # duplicated rows
    skip = (np.random.default_rng(7).random((len(kfs), len(pts[0]))) < 0.2).astype(np.uint8)
    bi, bd = ex.fuse_sim3_candidates(kfs, *pts, skip=skip)
    for k, kf in enumerate(kfs):
        si, sd = ex.fuse_sim3_candidates([kf], *pts, skip=skip[k:k + 1])
        assert (si[0] == bi[k]).all() and (sd[0] == bd[k]).all(), k
    ni, _ = ex.fuse_sim3_candidates(kfs, *pts)
    assert (ni[3] == ni[0]).all() and (ni[4] == ni[2]).all() and (ni >= 0).sum() > 50


def test_empty_inputs(ex):
    kfs, pts = loop_scene.loop_scene(4, P=20)
    e = [np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros((0, 32), np.uint8)]
    assert ex.fuse_sim3_candidates([], *pts)[0].shape == (0, len(pts[0]))
    assert ex.fuse_sim3_candidates(kfs, *e)[0].shape == (len(kfs), 0)
    assert ex.search_by_projection_sim3(kfs[0], *e, n_best=4)[0].shape == (0, 4)
    nokeys = dict(kfs[0], keys=kfs[0]["keys"][:0], desc=kfs[0]["desc"][:0])
    bi, bd = ex.fuse_sim3_candidates([nokeys], *pts)
    assert (bi == -1).all() and (bd == 256).all()
    ci, cd = ex.search_by_projection_sim3(nokeys, *pts, n_best=3)
    assert (ci == -1).all() and (cd == 256).all()
    e5 = (e[0], e[2], e[3], e[4], e[5])
    kf1, kf2, p1, p2, has1, has2, T = loop_scene.sim3_pair(1, n_common=20, n_extra=10)
    nf, m12, m1, m2 = ex.search_by_sim3(nokeys, kf2, e5, p2, T)
    assert nf == 0 and len(m12) == 0 and len(m1) == 0 and (m2 == -1).all()
    nf, m12, m1, m2 = ex.search_by_sim3(kf1, kf2, p1, p2, T, skip1=np.ones(len(has1), np.uint8))
    assert nf == 0 and (m1 == -1).all() and (m12 == -1).all()


def test_argument_errors(ex):
    from orb_ygz_slam_amd.capi import FuseKf, FusePoints, _p
    kfs, pts = loop_scene.loop_scene(9, P=50)
    P = len(pts[0])
    L = ex.L
    bad = dict(kfs[0], keys=kfs[0]["keys"].copy())
    bad["keys"]["octave"][5] = 8                                              # outside the keyframe's 8-level tables
    big = dict(kfs[0], keys=np.resize(kfs[0]["keys"], 40000), desc=np.resize(kfs[0]["desc"], (40000, 32)))
    with pytest.raises(YgzfError, match="octave"):
        ex.fuse_sim3_candidates([kfs[1], bad], *pts)
    with pytest.raises(YgzfError, match="octave"):
        ex.search_by_projection_sim3(bad, *pts)
    with pytest.raises(YgzfError, match="keypoints in one grid"):
        ex.fuse_sim3_candidates([big], *pts)
    with pytest.raises(YgzfError, match="keypoints in one grid"):
        ex.search_by_projection_sim3(big, *pts)
    for nb, md in ((0, 50), (9, 50), (4, 256), (4, -1)):
        with pytest.raises(YgzfError, match="n_best|max_dist"):
            ex.search_by_projection_sim3(kfs[0], *pts, n_best=nb, max_dist=md)
    kf1, kf2, p1, p2, has1, has2, T = loop_scene.sim3_pair(2, n_common=20, n_extra=10)
    bad1 = dict(kf1, keys=kf1["keys"].copy())
    bad1["keys"]["octave"][3] = -1
    with pytest.raises(YgzfError, match="octave"):
        ex.search_by_sim3(bad1, kf2, p1, p2, T)
    # NULL arrays through the C ABI directly
    bi, bd = np.zeros(P * 4, np.int32), np.zeros(P * 4, np.int32)
    w = np.ascontiguousarray(pts[0], f32)
    fp = FusePoints(w.ctypes.data, None, None, None, None, None)
    arr = (FuseKf * 1)()
    for rc in (L.ygzf_fuse_sim3_candidates(ex.h, 1, arr, P, C.byref(fp), None, 4.0, _p(bi), _p(bd)),
               L.ygzf_fuse_sim3_candidates(ex.h, 1, None, P, C.byref(fp), None, 4.0, _p(bi), _p(bd)),
               L.ygzf_search_by_projection_sim3(ex.h, arr, P, C.byref(fp), None, None, 10.0, 4, 50, _p(bi), _p(bd)),
               L.ygzf_search_by_projection_sim3(ex.h, arr, P, None, None, None, 10.0, 4, 50, _p(bi), _p(bd)),
               L.ygzf_search_by_sim3(ex.h, arr, arr, None, None, None, None, None, 7.5, 100, _p(bi), _p(bd), _p(bi), None)):
        assert rc < 0 and b"null" in L.ygzf_last_error(ex.h)
    assert L.ygzf_fuse_sim3_candidates(ex.h, -1, arr, P, C.byref(fp), None, 4.0, _p(bi), _p(bd)) < 0
    assert L.ygzf_search_by_projection_sim3(ex.h, arr, -1, C.byref(fp), None, None, 10.0, 4, 50, _p(bi), _p(bd)) < 0
    # the context is still usable
    a, _ = ex.fuse_sim3_candidates(kfs, *pts)
    b, _ = ex.fuse_sim3_candidates(kfs, *pts)
    assert (a == b).all() and (a >= 0).any()


def test_calls_keep_context_batch_state():
    """The three searches between extract_batch_host and match_batch_prev leave the match results unchanged."""
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.stack([synth_frame(50 + s, 752, 480) for s in range(4)])
    cam = make_camera(752, 480)
    kfs, pts = loop_scene.loop_scene(8, P=200)
    kf1, kf2, p1, p2, has1, has2, T = loop_scene.sim3_pair(3, n_common=100, n_extra=50)
    results = []
    for loop in (False, True):
        e = Extractor(1000, 1.2, 8, 20, 7, 752, 480, max_batch=4)
        try:
            e.extract_batch_host(frames[:2])
            e.match_batch_prev(cam)
            e.extract_batch_host(frames[2:])
            if loop:
                assert (e.fuse_sim3_candidates(kfs, *pts)[0] >= 0).any()
                assert (e.search_by_projection_sim3(kfs[0], *pts, n_best=4, max_dist=50)[0] >= 0).any()
                assert e.search_by_sim3(kf1, kf2, p1, p2, T, skip1=1 - has1, skip2=1 - has2)[0] > 0
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
    exe = os.path.join(tmp, "loop_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "loop_shell.cc")] + [os.path.join(host, f) for f in
                                                                  ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ORBmatcherLoop.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_loop_shell_end_to_end(tmp_path):
    """ygz::SearchAndFuseBatch (LoopClosing.cc:546-569), per-keyframe Fuse(.., Scw, ..) + Replace, SearchByProjection(KF, Scw, ..) and SearchBySim3
    over the device give the graph, vpMatched / vpMatches12 and return values of the sequential restatement."""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    for seed in (1, 2, 3):
        out = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "loop shell ok" in out.stdout, out.stdout
