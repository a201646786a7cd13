"""Long-run hygiene of the library: device memory must not grow while the same calls repeat (contexts grow their scratch buffers once and
keep them), and creating / destroying contexts returns everything."""
import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame
from orb_ygz_slam_amd.scene import two_view_scene

pytestmark = pytest.mark.gpu


def _free_bytes(ex):
    return ex.device_mem_info()[0]      # (the library's own HIP runtime: a second copy loaded through ctypes may not see the device)


def test_repeated_calls_do_not_grow_device_memory():
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    w, h = 752, 480
    cam = make_camera(w, h)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=4)
    imgs = np.stack([synth_frame(60 + i, w, h) for i in range(4)])
    A, B, _, bp = two_view_scene(9, w, h, EUROC)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    inv = ex.tables()["inv_scale"]

    def one_round(i):
        ex.extract_batch_host(imgs)
        ex.match_batch_prev(cam, 15.0, True, True, True)
        ex.align_batch_prev(cam, 7, 1, 10)
        ex.batch_fetch(i % 4)
        k, d = ex.extract(A if i % 2 else B)
        pa, pb = ex.compute_pyramid(A), ex.compute_pyramid(B)
        ex.sia_run(cam, k, bp(k["x"], k["y"]), ident, pa, ident, pb, inv, 7, 1)
        ex.features_in_area(cam, k, np.array([[300, 200, 40]], np.float32))
        ex.descriptor_distance(d[:100], d[100:200])

    for i in range(6):                       # every buffer reaches its working size
        one_round(i)
    before = _free_bytes(ex)
    for i in range(150):
        one_round(i)
    after = _free_bytes(ex)
    assert before - after < (8 << 20), (before, after)      # allocator slack only: no growth with the call count


def test_contexts_give_their_memory_back():
    from orb_ygz_slam_amd import Extractor
    w, h = 752, 480
    img = synth_frame(61, w, h)
    for _ in range(3):                       # the first contexts load code objects and warm the allocator
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=8)
        ex.extract(img)
        ex.close()
    probe = Extractor(100, 1.2, 4, 20, 7, max_width=64, max_height=64, max_batch=1)   # a small context that only reports
    before = _free_bytes(probe)
    for _ in range(40):
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=8)
        ex.extract(img)
        ex.close()
    after = _free_bytes(probe)
    assert before - after < (8 << 20), (before, after)


_STAGE_W, _STAGE_H, _STAGE_NF = 320, 240, 2000
_stage_inputs_cache = []


def _stage_inputs():
    """The inputs of test_every_stage_gives_its_memory_back, built once: 320x240 frames and keys of the generators the other GPU tests use,
    tiled where a stage's buffers are sized by the number of entries it is handed."""
    if _stage_inputs_cache:
        return _stage_inputs_cache[0]
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    from orb_ygz_slam_amd.scene import rotvec_to_quat
    from tests.test_gpu_fuse import scene as fuse_scene
    from tests.tri_cases import geometry
    w, h = _STAGE_W, _STAGE_H
    s = dict(cam=make_camera(w, h), ident=np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
    rot, tr = (0.01, -0.02, 0.03), (0.1, -0.05, 0.2)
    A, B, (R, t), bp = two_view_scene(9, w, h, EUROC, Z=4.0, rotvec=rot, trans=tr)
    q = rotvec_to_quat(rot)
    s.update(A=A, B=B, T7=np.array([q[0], q[1], q[2], q[3], *tr], np.float32), imgs=np.stack([A, B]))
    ex = Extractor(_STAGE_NF, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
    (ka, da), (kb, db) = ex.extract(A), ex.extract(B)
    s["inv_scale"] = ex.tables()["inv_scale"]
    ex.close()
    assert len(ka) > 800 and len(kb) > 800      # (sia_run's patch cache: 209 bytes a key and level, seven levels)
    rng = np.random.default_rng(0)
    world = bp(ka["x"], ka["y"])
    s.update(ka=ka, da=da, kb=kb, db=db, world=world)

    def tiled(a, n):
        return a[np.arange(n) % len(a)]
    s["many_keys"] = tiled(kb, 40000)                                   # describe list: 20 bytes an entry (+ 32 of shared scratch)
    s["stereo"] = (tiled(ka, 9000), tiled(da, 9000), tiled(kb, 9000), tiled(db, 9000))   # 60 bytes a key + 12 a right key + 12 a left key
    n = 6000                                                            # direct projection: 185 bytes a candidate with its patch
    idx = rng.integers(0, len(ka), n)
    Xc = (R @ world[idx].T.astype(np.float64)).T + t
    px0 = np.stack([EUROC["fx"] * Xc[:, 0] / Xc[:, 2] + EUROC["cx"], EUROC["fy"] * Xc[:, 1] / Xc[:, 2] + EUROC["cy"]], -1) + rng.uniform(-1.5, 1.5, (n, 2))
    s["direct"] = (np.zeros(n, np.int32), np.tile(s["ident"], (n, 1)), ka[idx], world[idx], px0.astype(np.float32))
    sizes = [10 ** l for l in range(6)]                                 # a k = 10, L = 5 vocabulary: 111 111 nodes, 3.5 MB of centroids
    parent = np.full(sum(sizes), -1, np.int32)
    start = np.cumsum([0] + sizes)
    for l in range(1, 6):
        parent[start[l]:start[l + 1]] = start[l - 1] + np.arange(sizes[l]) // 10
    s["voc"] = (parent, rng.integers(0, 256, (len(parent), 32), dtype=np.uint8))
    s["bow_desc"] = tiled(np.concatenate([da, db]), 30000)              # 40 bytes a descriptor
    na, nb = da[:, 0].astype(np.int32) >> 3, db[:, 0].astype(np.int32) >> 3
    ko, fo, ki, fi = [0], [0], [], []
    for node in sorted(set(na.tolist()) & set(nb.tolist())):
        ki.extend(np.nonzero(na == node)[0]); fi.extend(np.nonzero(nb == node)[0])
        ko.append(len(ki)); fo.append(len(fi))
    none = np.zeros(max(len(ka), len(kb)), np.uint8)
    s["tri"] = (ko, ki, fo, fi, dict(keys=ka, desc=da, has_mp=none[:len(ka)], u_right=None), dict(keys=kb, desc=db, has_mp=none[:len(kb)], u_right=None),
                None, None) + tuple(geometry(0.002)) + (False, True)
    nq = 5000                                                           # 5 MB of index lists: beyond the packed transfer, so the shared scratch takes them
    s["area"] = np.stack([tiled(ka["x"], nq), tiled(ka["y"], nq), np.full(nq, 18.0, np.float32)], 1).astype(np.float32)
    P = 5000                                                            # 32 bytes an observation
    s["distinctive"] = (np.arange(P + 1, dtype=np.int32) * 8, tiled(da, P * 8))
    nw = 70000                                                          # one BowVector past the arena's first 65 536 entries: 12 bytes an entry
    s["kfdb"] = (np.arange(nw, dtype=np.uint32) * 3, np.full(nw, 1.0 / nw))
    s["fuse"] = fuse_scene(1)                                           # (the store's arena starts at 8 MiB)
    _stage_inputs_cache.append(s)
    return s


def _every_stage_once(ex, s):
    cam, ident = s["cam"], s["ident"]
    ex.extract_batch_host(s["imgs"])
    ex.match_batch_prev(cam, 15.0, True, True, True)
    ex.align_batch_prev(cam, 7, 1, 10)
    ex.stereo_batch(0.11, 47.9)
    ex.describe_keys(s["many_keys"], frame=1, recompute_angle=True)
    ex.compute_stereo_matches(s["A"], s["B"], *s["stereo"], 0.11, 47.9)
    ex.fast10(s["A"], 20)
    ex.extract_dso(s["B"], existing=s["many_keys"])
    ex.extract_fast_keypoint(s["A"])
    ex.extract_dso_multilevel(s["A"])
    ex.image_cache_reserve(2, _STAGE_W, _STAGE_H)
    ex.image_cache_put(0, s["A"])
    ex.image_cache_put(1, s["B"])
    ex.find_direct_projection_batch(cam, 1, s["T7"], *s["direct"], want_patches=True)
    pa, pb = ex.compute_pyramid(s["A"]), ex.compute_pyramid(s["B"])
    ex.sia_run(cam, s["ka"], s["world"], ident, pa, ident, pb, s["inv_scale"], 7, 1)
    ex.vocabulary_set(*s["voc"], 5)
    ex.bow_transform(s["bow_desc"], 4)
    ex.search_for_triangulation(*s["tri"])
    ex.features_in_area(cam, s["kb"], s["area"], cap=256)
    ex.distinctive_descriptors_batch(*s["distinctive"])
    ex.kfdb_add(1, *s["kfdb"])
    ex.kfdb_query([(s["kfdb"][0][:500], np.full(500, 1.0 / 500))])
    kfs, pts = s["fuse"]
    ex.kf_put(7, kfs[0])
    ex.fuse_candidates_resident([(7, kfs[0]["Rcw"], kfs[0]["tcw"], kfs[0]["Ow"])], *pts)


def test_every_stage_gives_its_memory_back():
    """A context that has called one entry point of every buffer group returns all of it when it is closed: the extractor with the batch matcher
    and aligner, ComputeStereoMatches (batch and one pair), FAST-10, the three grid detectors, describe_keys, FindDirectProjection with
    patches over the image cache, sia_run, the vocabulary and the BoW transform, SearchForTriangulation, features_in_area and
    distinctive_descriptors (the shared scratch), the keyframe database and the resident keyframes with a Fuse against them.  The inputs are
    sized so that every group holds at least 1 MiB in each of the 16 contexts: a group that were not freed would cost 16 MiB against the 8 MiB
    of allocator slack allowed.  Below that whatever the input, and so guaranteed by Buf's destructor and not by this measurement: the stereo bin
    table (16 KB a pair), what ygzf_stereo_batch alone sizes at two frames (24 bytes a keypoint slot; the record reaches its size through the
    one-pair entry), SearchForTriangulation's one buffer (a byte a keypoint), and the counters (dMatchStat, dSplitCnt, dFastStats, dFastCtr)."""
    from orb_ygz_slam_amd import Extractor
    s = _stage_inputs()

    def one_context():
        ex = Extractor(_STAGE_NF, 1.2, 8, 20, 7, max_width=_STAGE_W, max_height=_STAGE_H, max_batch=2)
        _every_stage_once(ex, s)
        ex.close()

    for _ in range(3):                       # the first contexts load code objects and warm the allocator
        one_context()
    probe = Extractor(100, 1.2, 4, 20, 7, max_width=64, max_height=64, max_batch=1)   # a small context that only reports
    before = _free_bytes(probe)
    for _ in range(16):
        one_context()
    after = _free_bytes(probe)
    probe.close()
    assert before - after < (8 << 20), (before, after)


def test_awkward_widths_do_not_fall_off_the_copy_fast_path(oracle):
    """Pitched host<->device copies whose width is not a multiple of 4 are executed row by row by the copy engine (3 ms per 1241x376 frame,
    13 ms per pyramid read-back); the library re-pitches on the device instead.  Latency of such sizes must stay in the family of the
    752x480 case, and the results must still be the oracle's."""
    import time
    from orb_ygz_slam_amd import Extractor

    def med(f, n=30):
        for _ in range(5):
            f()
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        return float(np.median(t))

    lat = {}
    for (w, h) in ((752, 480), (1241, 376), (641, 479), (1242, 375)):
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1)
        img = synth_frame(5, w, h)
        lat[(w, h)] = (med(lambda: ex.extract(img)), med(lambda: ex.compute_pyramid(img)))
        k, d = ex.extract(img)
        ok, od = oracle.Extractor(1000, 1.2, 8, 20, 7).extract(img)
        assert np.array_equal(k["x"], ok["x"]) and np.array_equal(k["y"], ok["y"]) and np.array_equal(d, od), (w, h)
        strided = np.zeros((h, w + 13), np.uint8)                      # a host image with a row pitch that is not its width
        strided[:, :w] = img
        k2, d2 = ex.extract(strided[:, :w])
        assert np.array_equal(k2, k) and np.array_equal(d2, d), (w, h)
    base_e, base_p = lat[(752, 480)]
    for key, (e, p) in lat.items():
        assert e < 3 * base_e + 2e-4 and p < 3 * base_p + 2e-4, (key, lat)
    print({k: (round(1e6 * a), round(1e6 * b)) for k, (a, b) in lat.items()})
