"""GPU tests of the resident keyframes -- ygzf_kf_put / _erase / _clear / _has / _size / _capacity / _grid, k_kf_grid_build, and the two Fuse members
run against the store (ygzf_fuse_candidates_resident, ygzf_fuse_sim3_candidates_resident: k_proj_search<MODE, resident>).

The stored grid is held to the numpy restatement of tests/kf_store_cases.py, which tests/test_kf_store_cases.py holds to the oracle's Frame grid.
The searches are held to the non-resident calls and to test_gpu_fuse's restatement of src/ORBmatcher.cc:764-868, all exactly: both forms run
the same kernel body over the same keys, descriptors, tables and grid order, so nothing may differ."""
import ctypes as C

import numpy as np
import pytest

from orb_ygz_slam_amd.capi import KF_INITIAL_BYTES, Extractor, FusePoints, KfRef, KfStatic, YgzfError, _p, make_camera
from orb_ygz_slam_amd.fuse_scene import _rot, make_kf, make_points
from tests import kf_store_cases as K
from tests.test_gpu_fuse import assemble, ref_candidates, scene

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def ex_module():
    e = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.fixture
def ex(ex_module):
    ex_module.kf_clear()
    return ex_module


def ref(key, kf):
    return (key, kf["Rcw"], kf["tcw"], kf["Ow"])


def put_all(ex, kfs, base=1000):
    keys = [base + 17 * i for i in range(len(kfs))]
    for k, kf in zip(keys, kfs):
        ex.kf_put(k, kf)
    return keys


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------------------
GRID_SETS = dict(K.constructed_sets(), **K.seeded_keyframes())


@pytest.mark.parametrize("name", sorted(GRID_SETS))
def test_stored_grid_equals_restatement(ex, name):
    kf = GRID_SETS[name]
    n = len(kf["keys"])
    ex.kf_put(5, kf)
    cs, lst = ex.kf_grid(5, n)
    rcs, rlst = K.grid_csr(kf["keys"], kf["cam"])
    assert np.array_equal(cs, rcs), (name, np.nonzero(cs != rcs)[0][:10])
    assert np.array_equal(lst, rlst), (name, np.nonzero(lst != rlst)[0][:10])


# ---- 2. resident == non-resident == restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resident_equals_nonresident_equals_restatement(oracle, ex, seed):
    kfs, pts = scene(seed)
    Kn, P = len(kfs), len(pts[0])
    keys = put_all(ex, kfs)
    refs = [ref(k, kf) for k, kf in zip(keys, kfs)]
    rng = np.random.default_rng(100 + seed)
    skip = (rng.random((Kn, P)) < 0.1).astype(np.uint8)
    for th, sk in ((3.0, None), (5.0, skip)):
        got = ex.fuse_candidates_resident(refs, *pts, th=th, skip=sk)
        non = ex.fuse_candidates(kfs, *pts, th=th, skip=sk)
        assert got[0].shape == (Kn, P) and same(got, non), (seed, th)
        for k in range(Kn):
            ri, rd = ref_candidates(oracle, kfs[k], *pts, th, None if sk is None else sk[k])
            assert (got[0][k] == ri).all() and (got[1][k] == rd).all(), (seed, th, k)
        assert (got[0] >= 0).sum() > 20
        got3 = ex.fuse_sim3_candidates_resident(refs, *pts, th=th + 1.0, skip=sk)
        non3 = ex.fuse_sim3_candidates(kfs, *pts, th=th + 1.0, skip=sk)
        assert same(got3, non3) and (got3[0] >= 0).sum() > 20, (seed, th)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_resident_constructed_bounds(oracle, ex, seed):
    kf, pts, labels, _ = assemble(seed)
    ex.kf_put(9, kf)
    bi, bd = ex.fuse_candidates_resident([ref(9, kf)], *pts)
    ri, rd = ref_candidates(oracle, kf, *pts, 3.0)
    assert (bi[0] == ri).all() and (bd[0] == rd).all(), (labels, bi[0], ri)
    assert same((bi, bd), ex.fuse_candidates([kf], *pts))
    got = dict(zip(labels, bi[0] >= 0))
    assert got == {"proj_in": True, "proj_out": False, "gate_7.8": False, "view_eq": True, "view_below": False}, got


# ---- 3. the row table --------------------------------------------------------------------------------------------------------------------------
def test_resident_rows_at_slice_edge_empty_keyframe_and_duplicate(oracle, ex):
    rng = np.random.default_rng(21)
    stereo = make_kf(rng, 752, 480, 300, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.6)
    empty = dict(make_kf(rng, 752, 480, 16, 8, 1.2, _rot(0.01, 0.02, 0.0), [0.05, 0.0, 0.02]))
    empty["keys"], empty["desc"] = empty["keys"][:0], empty["desc"][:0]
    mono = make_kf(rng, 640, 480, 200, 5, 1.5, _rot(-0.03, 0.04, 0.0), [-0.2, 0.05, 0.1])
    P = 65
    pts = make_points(rng, [stereo, mono], P)
    hit = [ref_candidates(oracle, kf, *pts, 3.0)[0] >= 0 for kf in (stereo, mono)]
    a = int(np.nonzero(hit[0])[0][0])
    b = int(np.nonzero(hit[1] & (np.arange(P) != a))[0][0])
    order = [b] + [i for i in range(P) if i not in (a, b)] + [a]
    pts = tuple(x[order] for x in pts)
    kfs = [stereo, empty, mono, stereo]                                 # the stereo one is listed twice
    keys = put_all(ex, kfs[:3])
    refs = [ref(k, kf) for k, kf in zip(keys + [keys[0]], kfs)]
    skip = np.zeros((4, P), np.uint8)
    skip[0, 64] = skip[2, 0] = 1
    bi, bd = ex.fuse_candidates_resident(refs, *pts, skip=skip)
    assert bi.shape == (4, P)
    for k, kf in enumerate(kfs):
        ri, rd = ref_candidates(oracle, kf, *pts, 3.0, skip[k])
        assert (bi[k] == ri).all() and (bd[k] == rd).all(), k
        si, sd = ex.fuse_candidates_resident([refs[k]], *pts, skip=skip[k:k + 1])
        assert (si[0] == bi[k]).all() and (sd[0] == bd[k]).all(), k
    assert (bi[skip != 0] == -1).all() and (bd[skip != 0] == 256).all()
    assert (bi[1] == -1).all() and (bd[1] == 256).all()
    assert (bi[0, :64] >= 0).any() and (bi[2, 1:] >= 0).any()
    assert bi[0, 64] == -1 and bi[3, 64] == ri[64] and (bi[3, :64] == bi[0, :64]).all()   # the second listing is a row of its own


# ---- 4. the pose is per call -------------------------------------------------------------------------------------------------------------------
def test_pose_travels_with_the_call(ex):
    kfs, pts = scene(5, P=300)
    kf = kfs[0]
    ex.kf_put(77, kf)
    moved = dict(kf)
    R = _rot(0.001, -0.002, 0.0015)                                          # a pixel or so: other candidates, not an empty result
    t = np.array([0.005, -0.003, 0.004], f32)
    moved["Rcw"], moved["tcw"] = R, t
    moved["Ow"] = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(f32)
    both = ex.fuse_candidates_resident([ref(77, kf), ref(77, moved)], *pts)
    non_a, non_b = ex.fuse_candidates([kf], *pts), ex.fuse_candidates([moved], *pts)
    assert (both[0][0] == non_a[0][0]).all() and (both[1][0] == non_a[1][0]).all()
    assert (both[0][1] == non_b[0][0]).all() and (both[1][1] == non_b[1][0]).all()
    assert (non_a[0] != non_b[0]).any() and (non_a[0] >= 0).any() and (non_b[0] >= 0).any()   # the second pose does change the answer
    later = ex.fuse_candidates_resident([ref(77, moved)], *pts)
    assert same(later, non_b)
    again = ex.fuse_candidates_resident([ref(77, kf)], *pts)
    assert same(again, non_a)


# ---- 5. lifecycle ------------------------------------------------------------------------------------------------------------------------------
def test_erase_reuses_the_slot_and_neighbours_still_answer(ex):
    kfs, pts = scene(6, P=200)
    rng = np.random.default_rng(60)
    larger = make_kf(rng, 752, 480, 1900, 8, 1.2, _rot(0.0, 0.01, 0.0), [0.02, 0.0, 0.0], mbf=40.0, stereo_frac=0.4)
    assert [ex.kf_put(k, kf) for k, kf in zip((11, 22, 33), kfs)] == [0, 1, 2]
    assert ex.kf_size() == (3, 3) and ex.kf_has(22)
    ex.kf_erase(22)
    ex.kf_erase(22)                                                          # an unknown key: no error
    ex.kf_erase(123456)
    assert ex.kf_size() == (2, 3) and not ex.kf_has(22)
    used = ex.kf_capacity()[1]
    assert ex.kf_put(44, larger) == 1                                        # the freed slot number, a fresh row behind the others
    assert ex.kf_capacity()[1] > used and ex.kf_size() == (3, 3)
    order = [(11, kfs[0]), (44, larger), (33, kfs[2])]
    got = ex.fuse_candidates_resident([ref(k, kf) for k, kf in order], *pts)
    assert same(got, ex.fuse_candidates([kf for _, kf in order], *pts)) and (got[0] >= 0).any()
    with pytest.raises(YgzfError, match="not resident"):
        ex.fuse_candidates_resident([ref(22, kfs[1])], *pts)


def test_growth_repacks_and_every_seventh_still_answers(ex):
    rng = np.random.default_rng(70)
    cap0, used0 = ex.kf_capacity()
    assert cap0 >= KF_INITIAL_BYTES and used0 == 0
    kfs, caps = [], [cap0]
    while len(caps) < 3:
        assert len(kfs) < 200
        kf = make_kf(rng, 752, 480, 6000 + 13 * len(kfs), 8, 1.2, _rot(0.001 * len(kfs), 0.0, 0.0), [0.01, 0.0, 0.0], mbf=40.0, stereo_frac=0.5)
        ex.kf_put(500 + len(kfs), kf)
        kfs.append(kf)
        cap = ex.kf_capacity()[0]
        if cap != caps[-1]:
            caps.append(cap)
    assert caps[1] == 2 * caps[0] and caps[2] == 2 * caps[1]
    assert ex.kf_size() == (len(kfs), len(kfs))
    pts = make_points(rng, kfs[:3], 130)
    picks = list(range(0, len(kfs), 7))
    got = ex.fuse_candidates_resident([ref(500 + i, kfs[i]) for i in picks], *pts)
    assert same(got, ex.fuse_candidates([kfs[i] for i in picks], *pts)) and (got[0] >= 0).any()
    i = picks[1]
    cs, lst = ex.kf_grid(500 + i, len(kfs[i]["keys"]))
    rcs, rlst = K.grid_csr(kfs[i]["keys"], kfs[i]["cam"])
    assert np.array_equal(cs, rcs) and np.array_equal(lst, rlst)
    # clear: no keys, no slots, the memory stays, an old key is unknown
    ex.kf_clear()
    assert ex.kf_size() == (0, 0) and ex.kf_capacity() == (caps[2], 0)
    with pytest.raises(YgzfError, match="not resident") as ei:
        ex.fuse_candidates_resident([ref(500, kfs[0])], *pts)
    assert (ei.value.outputs[0] == -1).all() and (ei.value.outputs[1] == 256).all()


def test_erase_put_rounds_keep_the_capacity():
    ex = Extractor(1000, 1.2, 8, 20, 7, 752, 480)                            # a store of its own: the arena at its initial size
    try:
        _erase_put_rounds(ex)
    finally:
        ex.close()


def _erase_put_rounds(ex):
    rng = np.random.default_rng(80)
    pool = [make_kf(rng, 752, 480, 800, 8, 1.2, _rot(0.0, 0.002 * i, 0.0), [0.0, 0.01, 0.0], mbf=40.0, stereo_frac=0.5) for i in range(4)]
    for i in range(3):
        ex.kf_put(i, pool[i])
    cap = ex.kf_capacity()[0]
    assert cap == KF_INITIAL_BYTES
    live = {i: pool[i] for i in range(3)}
    tops = []
    for r in range(200):                                                     # ~ 70 KB a row: 14 MB appended in all, more than the arena holds
        old = min(live)
        ex.kf_erase(old)
        del live[old]
        ex.kf_put(3 + r, pool[(3 + r) % 4])
        live[3 + r] = pool[(3 + r) % 4]
        tops.append(ex.kf_capacity()[1])
    assert ex.kf_capacity()[0] == cap and ex.kf_size()[0] == 3
    assert (np.diff(tops) < 0).any()                                         # the holes were dropped by a repack of the same size
    pts = make_points(rng, pool[:2], 120)
    order = sorted(live)
    got = ex.fuse_candidates_resident([ref(k, live[k]) for k in order], *pts)
    assert same(got, ex.fuse_candidates([live[k] for k in order], *pts)) and (got[0] >= 0).any()


def test_put_consumes_its_host_arrays(ex):
    kfs, pts = scene(9, P=200)
    kf = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kfs[0].items()}
    want = ex.fuse_candidates([kfs[0]], *pts)
    ex.kf_put(1, kf)
    kf["keys"]["x"] = 3.0
    kf["keys"]["octave"] = 0
    kf["desc"][:] = 0
    kf["u_right"][:] = 1.0
    kf["scale_factors"][:] = 9.0
    kf["inv_level_sigma2"][:] = 0.0
    assert same(ex.fuse_candidates_resident([ref(1, kfs[0])], *pts), want)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_store_and_the_context_usable(ex):
    kfs, pts = scene(9, P=50)
    P = len(pts[0])
    L = ex.L
    ex.kf_put(1, kfs[0])
    want = ex.fuse_candidates([kfs[0]], *pts)
    with pytest.raises(YgzfError, match="error -5"):                         # YGZF_ERR_STATE: a live key
        ex.kf_put(1, kfs[1])
    assert ex.kf_size() == (1, 1) and same(ex.fuse_candidates_resident([ref(1, kfs[0])], *pts), want)
    bad = dict(kfs[0])
    bad["keys"] = kfs[0]["keys"].copy()
    bad["keys"]["octave"][5] = 8
    with pytest.raises(YgzfError, match="octave"):
        ex.kf_put(2, bad)
    big = dict(kfs[0])
    big["keys"] = np.resize(kfs[0]["keys"], 40000)
    big["desc"] = np.resize(kfs[0]["desc"], (40000, 32))
    big["u_right"] = None
    with pytest.raises(YgzfError, match="keypoints in one grid"):
        ex.kf_put(2, big)
    with pytest.raises(YgzfError, match="keypoints in one grid"):             # ... the limit of the non-resident form
        ex.fuse_candidates([big], *pts)
    rec = KfStatic()
    rec.view.n = 5
    rec.cam = kfs[0]["cam"]
    assert L.ygzf_kf_put(ex.h, 2, C.byref(rec), None) < 0 and b"null" in L.ygzf_last_error(ex.h)
    assert L.ygzf_kf_put(ex.h, 2, None, None) < 0 and b"null" in L.ygzf_last_error(ex.h)
    assert ex.kf_size() == (1, 1) and not ex.kf_has(2)
    # searches: an unknown key, a null point array, a keyframe put without mvInvLevelSigma2 -- outputs preset to -1 / 256
    with pytest.raises(YgzfError, match="not resident") as ei:
        ex.fuse_candidates_resident([ref(1, kfs[0]), ref(99, kfs[1])], *pts)
    assert ei.value.outputs[0].shape == (2, P) and (ei.value.outputs[0] == -1).all() and (ei.value.outputs[1] == 256).all()
    w = np.ascontiguousarray(pts[0], f32)
    fp = FusePoints(w.ctypes.data, None, None, None, None, None)
    arr = (KfRef * 1)()
    arr[0].key = 1
    bi, bd = np.full(P, 7, np.int32), np.full(P, 7, np.int32)
    for fn in (L.ygzf_fuse_candidates_resident, L.ygzf_fuse_sim3_candidates_resident):
        bi[:], bd[:] = 7, 7
        assert fn(ex.h, 1, arr, P, C.byref(fp), None, 3.0, _p(bi), _p(bd)) < 0 and b"null" in L.ygzf_last_error(ex.h)
        assert (bi == -1).all() and (bd == 256).all()
        assert fn(ex.h, 1, None, P, C.byref(fp), None, 3.0, _p(bi), _p(bd)) < 0
        assert fn(ex.h, -1, arr, P, C.byref(fp), None, 3.0, _p(bi), _p(bd)) < 0
        assert fn(ex.h, 1, arr, -1, C.byref(fp), None, 3.0, _p(bi), _p(bd)) < 0
        assert fn(ex.h, 0, None, P, None, None, 3.0, None, None) == 0
        assert fn(ex.h, 1, arr, 0, None, None, 3.0, None, None) == 0
    nosig = dict(kfs[2])
    nosig["inv_level_sigma2"] = None
    ex.kf_put(3, nosig)
    with pytest.raises(YgzfError, match="mvInvLevelSigma2") as ei:
        ex.fuse_candidates_resident([ref(3, nosig)], *pts)
    assert (ei.value.outputs[0] == -1).all() and (ei.value.outputs[1] == 256).all()
    assert same(ex.fuse_sim3_candidates_resident([ref(3, nosig)], *pts), ex.fuse_sim3_candidates([kfs[2]], *pts))
    bi0, _ = ex.fuse_candidates_resident([], *pts)
    assert bi0.shape == (0, P)
    e = [np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros((0, 32), np.uint8)]
    bi0, _ = ex.fuse_candidates_resident([ref(1, kfs[0])], *e)
    assert bi0.shape == (1, 0)
    # the context and the store work afterwards
    assert same(ex.fuse_candidates_resident([ref(1, kfs[0])], *pts), want) and (want[0] >= 0).any()
    assert ex.kf_put(2, kfs[1]) == 2
    assert same(ex.fuse_candidates_resident([ref(2, kfs[1])], *pts), ex.fuse_candidates([kfs[1]], *pts))


# ---- 7. neighbours -----------------------------------------------------------------------------------------------------------------------------
def test_resident_search_keeps_context_batch_state():
    """Puts and a resident search between extract_batch_host and match_batch_prev leave the match results unchanged."""
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.stack([synth_frame(50 + s, 752, 480) for s in range(4)])
    cam = make_camera(752, 480)
    kfs, pts = scene(8, P=200)
    results = []
    for resident in (False, True):
        e = Extractor(1000, 1.2, 8, 20, 7, 752, 480, max_batch=4)
        try:
            e.extract_batch_host(frames[:2])
            e.match_batch_prev(cam)
            e.extract_batch_host(frames[2:])
            if resident:
                keys = put_all(e, kfs)
                bi, _ = e.fuse_candidates_resident([ref(k, kf) for k, kf in zip(keys, kfs)], *pts)
                assert (bi >= 0).any()
            e.match_batch_prev(cam)
            results.append([e.match_fetch(p) for p in range(2)] + [e.match_counts().copy()])
        finally:
            e.close()
    a, b = results
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            assert same(x, y)
        else:
            assert np.array_equal(x, y)


def test_kfdb_on_the_same_context_is_untouched(ex):
    rng = np.random.default_rng(90)
    ex.kfdb_clear()
    vecs = []
    for k in range(6):
        ids = np.sort(rng.choice(5000, 300, replace=False)).astype(np.uint32)
        vals = rng.random(300)
        vecs.append((ids, vals / vals.sum()))
        ex.kfdb_add(900 + k, *vecs[-1])
    before = ex.kfdb_query(vecs[:2])
    kf = make_kf(rng, 752, 480, 8000, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.5)
    cap = ex.kf_capacity()[0]
    n = 0
    while ex.kf_capacity()[0] == cap:                                       # until the arena has been repacked into a larger one
        assert n < 200
        ex.kf_put(n, kf)
        n += 1
    after = ex.kfdb_query(vecs[:2])
    assert same(before, after) and (before[0] > 0).any()
    ex.kfdb_clear()
