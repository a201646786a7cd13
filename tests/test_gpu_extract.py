"""GPU parity tests of the extractor hot path: libygzf (HIP, through the C ABI) vs the CPU oracle, stage by stage and
end to end.  Bit-exact: pyramid pixels, FAST candidates (x, y, score, order), octree selection + order (bucket ids),
keypoint fields, 256-bit descriptors; orientation angles are compared exactly as well (tolerance 1e-5 per north_star,
the implementation is in fact bit-identical)."""
import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame

pytestmark = pytest.mark.gpu


def _cmp_frame(oracle, ex, oex, img, frame=0):
    w, h = img.shape[1], img.shape[0]
    pyr = oex.pyramid(img)
    for l in range(oex.nlevels):
        got = ex.batch_fetch_level(frame, l)
        assert got.shape == pyr[l].shape
        assert (got == pyr[l]).all(), "pyramid level %d differs" % l
    for l in range(oex.nlevels):
        xs, ys, sc = oex.cell_candidates(l)
        gx, gy, gs = ex.batch_fetch_candidates(frame, l)
        assert len(gx) == len(xs), "level %d: %d candidates vs oracle %d" % (l, len(gx), len(xs))
        assert (gx == xs).all() and (gy == ys).all() and (gs == sc).all(), "level %d candidates differ" % l
    ok, od = oex.extract(img)
    for l in range(oex.nlevels):
        kl = oex.level_keypoints(l)
        gx, gy, gs = ex.batch_fetch_level_keypoints(frame, l)
        assert len(gx) == len(kl), "level %d: octree kept %d vs oracle %d" % (l, len(gx), len(kl))
        assert (gx == kl["x"].astype(np.int32)).all() and (gy == kl["y"].astype(np.int32)).all(), "octree order/selection differs at level %d" % l
        assert (gs == kl["response"].astype(np.int32)).all()
    k, d = ex.batch_fetch(frame)
    assert len(k) == len(ok)
    for fld in ("x", "y", "size", "response", "octave", "class_id"):
        assert (k[fld] == ok[fld]).all(), fld
    assert len(k) == 0 or np.abs(k["angle"] - ok["angle"]).max() <= 1e-5
    assert (k["angle"] == ok["angle"]).all()
    assert (d == od).all(), "descriptors differ in %d rows" % int((d != od).any(axis=1).sum())
    return len(k)


@pytest.mark.parametrize("wh,seed", [((640, 480), 0), ((640, 480), 1), ((752, 480), 2), ((333, 517), 3), ((200, 150), 4)])
def test_extract_stages_bit_exact(oracle, wh, seed):
    from orb_ygz_slam_amd import Extractor
    w, h = wh
    img = synth_frame(seed, w, h)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1)
    oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
    ex.extract_batch_host(img[None])
    n = _cmp_frame(oracle, ex, oex, img)
    assert n > 100
    k, d = ex.extract(img)   # single-frame host entry point gives the same answer
    ok, od = oex.extract(img)
    assert (k == ok).all() and (d == od).all()


def test_extract_batch_and_degenerate(oracle):
    from orb_ygz_slam_amd import Extractor
    w, h = 640, 480
    imgs = np.stack([synth_frame(10, w, h), np.full((h, w), 93, np.uint8),
                     np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8), synth_frame(11, w, h),
                     np.zeros((h, w), np.uint8)])
    imgs[4, 100:140, 200:260] = 255  # fewer corners than nfeatures
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=len(imgs))
    oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
    ex.extract_batch_host(imgs)
    counts = ex.batch_counts()
    for f in range(len(imgs)):
        n = _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
        assert n == counts[f]
    assert counts[1] == 0            # constant image: no keypoints (reference: descriptors.release())
    assert 0 < counts[4] < 200


def test_other_configs(oracle):
    from orb_ygz_slam_amd import Extractor
    # shipped EuRoC mono config: 4 levels x 2.0 (exercises the exact-2x area path of cv::resize) and a tiny quota
    for (nf, sf, nl, w, h) in ((1000, 2.0, 4, 752, 480), (300, 1.2, 8, 640, 480), (2000, 1.2, 8, 960, 540), (1000, 1.2, 12, 800, 600)):
        img = synth_frame(20 + nl, w, h)
        ex = Extractor(nf, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=1)
        oex = oracle.Extractor(nf, sf, nl, 20, 7)
        ex.extract_batch_host(img[None])
        _cmp_frame(oracle, ex, oex, img)


def test_descriptor_distance(oracle):
    from orb_ygz_slam_amd import Extractor
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    b[:10] = a[:10]
    b[10:20] = ~a[10:20]
    ex = Extractor(max_width=64, max_height=64)
    got = ex.descriptor_distance(a, b)
    exp = np.array([oracle.hamming(a[i], b[i]) for i in range(len(a))])
    assert (got == exp).all() and (got[:10] == 0).all() and (got[10:20] == 256).all()


@pytest.mark.parametrize("w,h,nl,nf", [(1920, 1080, 8, 4000), (3840, 2160, 12, 8000)])
def test_baseline_large_configs(oracle, w, h, nl, nf):
    """BASELINE.json configs[3] / configs[4] shapes (one frame, one eye): full-size parity vs the oracle + matcher chain."""
    from orb_ygz_slam_amd import Extractor, make_camera
    img = synth_frame(70 + nl, w, h)
    ex = Extractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=2)
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    imgs = np.stack([img, np.roll(img, 2, axis=1)])
    ex.extract_batch_host(imgs)
    n = _cmp_frame(oracle, ex, oex, imgs[0], frame=0)
    assert n > 0.9 * nf
    ok, od = oex.extract(imgs[1])
    k, d = ex.batch_fetch(1)
    assert (k == ok).all() and (d == od).all()
    # the matcher chain works at this keypoint count (descriptors no longer fit in LDS) and agrees with the oracle
    from orb_ygz_slam_amd import EUROC
    cam = make_camera(w, h)
    ex.match_batch_prev(cam, 15.0, True, True, True)
    k0, d0 = ex.batch_fetch(0)
    world = np.stack([(k0["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]), (k0["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]),
                      np.ones(len(k0), np.float32)], -1)
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    e_n, e_m, e_o = oracle.search_by_projection_last(k, d, oex.tables()["scale"], w, h, EUROC, k0, world, d0, I, z, I, z, 15.0)
    m, o = ex.match_fetch(1)
    assert ex.match_counts()[1] == e_n and (m[:len(k)] == e_m).all() and e_n > 0.3 * nf


def test_bench_clip_parity(oracle):
    """The clip bench.py times, through the HOST entry (ygzf_extract_batch_host: level 0 in the context's own buffer): every frame of a 64-frame
    run (extract + match against the predecessor, carried across two batches) equals the oracle.  The device entry bench.py itself launches
    (ygzf_extract_batch_device on the caller's frames) is covered by tests/test_gpu_device_frames.py."""
    from bench import make_frames
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    w, h = 752, 480
    frames = make_frames(64, w, h)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=32)
    oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
    cam = make_camera(w, h)
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    prev = None
    for half in range(2):
        ex.extract_batch_host(frames[32 * half:32 * half + 32])
        ex.match_batch_prev(cam, 15.0, True, True, True)
        counts = ex.match_counts()
        for f in range(32):
            k, d = ex.batch_fetch(f)
            ok, od = oex.extract(frames[32 * half + f])
            assert len(k) == len(ok) and (k == ok).all() and (d == od).all()
            m, o = ex.match_fetch(f)
            if prev is not None:
                pk, pd = prev
                world = np.stack([(pk["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]),
                                  (pk["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]), np.ones(len(pk), np.float32)], -1).astype(np.float32)
                e_n, e_m, e_o = oracle.search_by_projection_last(k, d, oex.tables()["scale"], w, h, EUROC, pk, world, pd, I, z, I, z, 15.0)
                assert counts[f] == e_n and (m[:len(k)] == e_m).all() and (o[:len(k)] == e_o).all()
            prev = (k, d)


def test_real_image_clip_parity(oracle):
    """The clip bench.py cuts from the one real image the reference ships (Thirdparty/fast/test/data/test1.png: mirror-padded, zoomed, shifted
    crops -- `other_workloads.euroc752x480_test1png`): every stage of three frames of different zoom levels, and keypoints / descriptors / matches of
    a 24-frame run, equal the oracle.  Real content is less corner-dense than the generator (the FAST plan statistics differ)."""
    from bench import make_frames_test1png
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    w, h = 752, 480
    frames = make_frames_test1png(24, w, h)
    assert frames.std() > 20 and (frames[0] != frames[8]).mean() > 0.5          # a real image, and the zoom levels differ
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=24)
    oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
    ex.extract_batch_host(frames)
    cam = make_camera(w, h)
    ex.match_batch_prev(cam, 15.0, True, True, True)
    counts = ex.match_counts()
    for f in (0, 9, 23):
        assert _cmp_frame(oracle, ex, oex, frames[f], f) > 500
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    prev = None
    for f in range(24):
        k, d = ex.batch_fetch(f)
        ok, od = oex.extract(frames[f])
        assert len(k) == len(ok) and (k == ok).all() and (d == od).all()
        m, o = ex.match_fetch(f)
        if prev is not None:
            pk, pd = prev
            world = np.stack([(pk["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]),
                              (pk["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]), np.ones(len(pk), np.float32)], -1).astype(np.float32)
            e_n, e_m, e_o = oracle.search_by_projection_last(k, d, oex.tables()["scale"], w, h, EUROC, pk, world, pd, I, z, I, z, 15.0)
            assert counts[f] == e_n and (m[:len(k)] == e_m).all() and (o[:len(k)] == e_o).all()
        prev = (k, d)


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("YGZF_FUZZ_SEEDS", "10"))))
def test_extract_fuzz_sizes_and_configs(oracle, seed):
    """Random image sizes / pyramid depths / scale factors / feature budgets / thresholds."""
    from orb_ygz_slam_amd import Extractor
    rng = np.random.default_rng(100 + seed)
    w, h = int(rng.integers(120, 900)), int(rng.integers(100, 700))
    nl = int(rng.integers(1, 10))
    sf = float(rng.choice([1.1, 1.2, 1.25, 1.5, 2.0]))
    nf = int(rng.integers(50, 3000))
    ini = int(rng.integers(8, 40))
    mn = int(rng.integers(2, ini + 1))
    ex = Extractor(nf, sf, nl, ini, mn, max_width=w, max_height=h, max_batch=2)
    oex = oracle.Extractor(nf, sf, nl, ini, mn)
    imgs = np.stack([synth_frame(200 + seed, w, h), rng.integers(0, 256, (h, w), dtype=np.uint8)])
    ex.extract_batch_host(imgs)
    for f in range(2):
        k, d = ex.batch_fetch(f)
        ok, od = oex.extract(imgs[f])
        assert len(k) == len(ok) and (k == ok).all() and (d == od).all(), (w, h, nl, sf, nf, ini, mn, f)


def test_two_host_threads_two_contexts(oracle):
    """The reference extracts the two eyes on two std::threads with one extractor each (src/Frame.cc:728-731) and keeps a third, larger
    extractor for initialisation: contexts are independent (own stream, own buffers, no shared mutable state), also when their
    configurations -- and therefore their kernels' LDS plans -- differ.  Concurrent use from host threads gives the same bytes."""
    import threading
    from orb_ygz_slam_amd import Extractor, make_camera, EUROC
    cfgs = [(752, 480, 1000, 8), (752, 480, 2500, 8), (640, 360, 400, 5)]
    imgs = [synth_frame(300 + i, c[0], c[1]) for i, c in enumerate(cfgs)]
    want = [oracle.Extractor(c[2], 1.2, c[3], 20, 7).extract(im) for c, im in zip(cfgs, imgs)]
    errors = []

    def worker(i):
        try:
            w, h, nf, nl = cfgs[i]
            ex = Extractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=1)     # created inside the thread, like the eyes' extractors
            cam = make_camera(w, h)
            k0, d0 = want[i]
            world = np.stack([(k0["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]), (k0["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]),
                              np.ones(len(k0), np.float32)], -1).astype(np.float32)
            I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
            first = None
            for _ in range(25):
                k, d = ex.extract(imgs[i])
                if not ((k == k0).all() and (d == d0).all()):
                    errors.append("thread %d: extraction mismatch" % i)
                    return
                m = ex.search_by_projection_last(cam, k, d, k, world, d, I, z, I, z, 15.0)     # a frame against itself: every key finds itself
                first = first if first is not None else m
                if m[0] != first[0] or (m[1] != first[1]).any() or m[0] < 0.9 * len(k):
                    errors.append("thread %d: matcher mismatch" % i)
                    return
        except Exception as e:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, e))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(cfgs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_extract_on_the_resident_pyramid(oracle):
    """ygzf_extract_resident: the extractor on the image whose pyramid the previous ygzf_compute_pyramid left on the device (what Frame's
    constructors do: ComputePyramid, then the extractor on the same image) == ygzf_extract of that image; refused once another image
    operation has used the buffers."""
    from orb_ygz_slam_amd import Extractor, YgzfError
    for (w, h) in ((752, 480), (641, 479)):
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1)
        a, b = synth_frame(70, w, h), synth_frame(71, w, h)
        ka, da = ex.extract(a)
        pyr = ex.compute_pyramid(a)
        kr, dr = ex.extract_resident(w, h)
        assert np.array_equal(kr, ka) and np.array_equal(dr, da)
        assert all(np.array_equal(p, q) for p, q in zip(pyr, oracle.Extractor(1000, 1.2, 8, 20, 7).pyramid(a)))
        with pytest.raises(YgzfError):
            ex.extract_resident(w, h)              # the extraction itself consumed the resident state
        ex.compute_pyramid(b)
        ex.extract(a)                              # another image came in between
        with pytest.raises(YgzfError):
            ex.extract_resident(w, h)
        ex.compute_pyramid(b)
        kb, db = ex.extract_resident(w, h)
        kb2, db2 = ex.extract(b)
        assert np.array_equal(kb, kb2) and np.array_equal(db, db2)


@pytest.mark.gpu
def test_extract_ahead_of_the_request(oracle):
    """ygzf_set_extract_ahead: compute_pyramid queues the extraction behind the pyramid and returns the levels through a second stream;
    extract_resident collects the same keypoints / descriptors as ygzf_extract (and as the oracle), the levels are the oracle's, the resident
    state is consumed exactly as without the setting, and an image operation in between discards the queued result."""
    from orb_ygz_slam_amd import Extractor, YgzfError
    for (w, h) in ((752, 480), (641, 479)):
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1)
        oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
        a, b = synth_frame(72, w, h), synth_frame(73, w, h)
        ka, da = ex.extract(a)
        ex.set_extract_ahead(True)
        for rep in range(3):
            pyr = ex.compute_pyramid(a)
            assert all(np.array_equal(p, q) for p, q in zip(pyr, oex.pyramid(a)))
            kr, dr = ex.extract_resident(w, h)
            assert np.array_equal(kr, ka) and np.array_equal(dr, da)
            with pytest.raises(YgzfError):
                ex.extract_resident(w, h)
        ok, od = oex.extract(a)
        assert np.array_equal(ka["x"], ok["x"]) and np.array_equal(da, od)
        ex.compute_pyramid(a)
        kb2, db2 = ex.extract(b)                   # another image: the queued extraction of `a` is dropped
        with pytest.raises(YgzfError):
            ex.extract_resident(w, h)
        pyr = ex.compute_pyramid(b)                # pyramid only: the next pyramid simply replaces it
        pyr = ex.compute_pyramid(b)
        kb, db = ex.extract_resident(w, h)
        assert np.array_equal(kb, kb2) and np.array_equal(db, db2)
        assert all(np.array_equal(p, q) for p, q in zip(pyr, oex.pyramid(b)))
        ex.set_extract_ahead(False)
        ex.compute_pyramid(a)
        kr, dr = ex.extract_resident(w, h)
        assert np.array_equal(kr, ka) and np.array_equal(dr, da)


@pytest.mark.parametrize("w,h,nl,sf", [(752, 480, 8, 1.2), (641, 479, 8, 1.2), (1241, 376, 8, 1.2), (333, 517, 6, 1.25), (200, 150, 3, 1.2),
                                       (1920, 1080, 8, 1.2), (752, 480, 12, 1.1), (130, 110, 8, 1.2)])
def test_pyramid_one_launch_and_level_by_level(oracle, monkeypatch, w, h, nl, sf):
    """ComputePyramid (src/ORBextractor.cc:1130-1150) two ways: the whole chain of a frame in one launch (k_pyr_strips: strips of the
    last level with recomputed halo rows, what a context takes for a few frames at a time) and one launch per level (batches): every
    level byte for byte the oracle's, for widths that are no multiple of four, short pyramids, narrow scale steps, and batches that put
    several frames into one launch."""
    from orb_ygz_slam_amd import Extractor
    imgs = np.stack([synth_frame(60 + i, w, h) for i in range(3)])
    oex = oracle.Extractor(500, sf, nl, 20, 7)
    want = [oex.pyramid(imgs[i]) for i in range(3)]
    from orb_ygz_slam_amd.capi import force_env
    for strip_frames in ("8", "0"):
        for strips in ("0", "32"):
            monkeypatch.setenv("YGZF_FORCE", force_env(pyr_strip_frames=strip_frames, pyr_strips=strips))
            ex = Extractor(500, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
            for batch in (imgs[:1], imgs):
                ex.extract_batch_host(batch)
                for f in range(len(batch)):
                    for l in range(nl):
                        got = ex.batch_fetch_level(f, l)
                        assert got.shape == want[f][l].shape and (got == want[f][l]).all(), (strip_frames, strips, f, l)
            del ex


@pytest.mark.parametrize("sf", [1.2, 1.1, 1.27])
def test_pyramid_tiles_of_every_fold(oracle, monkeypatch, sf):
    """k_pyr_resize_tiled cuts a level into 256-column tiles and what is left into 128- / 64- / 32-column tiles whose waves fold 2 / 4 / 8 rows into one
    pass (csrc/extract_kernels.hip, host tables in ygzf_api.hip): level widths with every kind of remainder -- none, 1 .. 31 columns, each binary
    piece alone and together, just below and above a 256-column tile -- and heights that end inside a tile, inside a wave and inside a pass, one
    frame (the graph path) and three per launch; every level byte for byte the oracle's cv::resize."""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    monkeypatch.setenv("YGZF_FORCE", force_env(pyr_strip_frames="0"))
    rng = np.random.default_rng(int(sf * 100))
    level1 = [31, 32, 33, 64, 95, 128, 129, 160, 223, 224, 225, 255, 256, 257, 266, 288, 320, 383, 448, 479, 512, 522, 544, 767, 1000]
    for i, w1 in enumerate(level1):
        w = int(round(w1 * sf)) + 1
        h = [64, 97, 130, 301][i % 4]
        imgs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        oex = oracle.Extractor(200, sf, 3, 20, 7)
        ex = Extractor(200, sf, 3, 20, 7, max_width=w, max_height=h, max_batch=3)
        for batch in (imgs[:1], imgs):
            ex.extract_batch_host(batch)
            for f in range(len(batch)):
                want = oex.pyramid(batch[f])
                for l in range(3):
                    got = ex.batch_fetch_level(f, l)
                    assert got.shape == want[l].shape and (got == want[l]).all(), (w, h, f, l)
        ex.close()


def test_pyramid_contexts_of_different_sizes_on_one_device(oracle):
    """The one-launch pyramid chain asks the runtime for a large LDS allotment per workgroup (123 KB for 1920x1080, 44 KB for 320x240); the
    allotment belongs to the kernel on the device, not to a context: a context of small images prepared AFTER one of large images must not
    take the large one's away (it once did: the large context's next launch was refused)."""
    from orb_ygz_slam_amd import Extractor
    sizes = [(1920, 1080), (320, 240)]
    imgs = [synth_frame(70 + i, w, h) for i, (w, h) in enumerate(sizes)]
    oex = oracle.Extractor(500, 1.2, 8, 20, 7)
    want = [oex.pyramid(im) for im in imgs]
    exs = []
    for k in (0, 1, 0, 1):
        if k >= len(exs):
            exs.append(Extractor(500, 1.2, 8, 20, 7, max_width=sizes[k][0], max_height=sizes[k][1], max_batch=1))
        exs[k].extract_batch_host(imgs[k][None])
        for l in range(8):
            got = exs[k].batch_fetch_level(0, l)
            assert (got == want[k][l]).all(), (k, l)


def test_frames_from_a_pointer_list(oracle):
    """ygzf_extract_batch_host_frames: frames anywhere in host memory -- out of order, row-strided views (crops of a larger image), a regular round-robin
    share of a clip (one two-dimensional copy), frames in page-locked memory -- give the bytes of the same frames handed over as one tight block."""
    import ctypes as C
    from orb_ygz_slam_amd import Extractor
    w, h, n = 320, 240, 12
    big = np.stack([synth_frame(300 + i // 3, w + 24, h + 16) for i in range(n)])
    views = [big[i, (i % 3):(i % 3) + h, 2 * (i % 4):2 * (i % 4) + w] for i in range(n)]           # crops: row pitch w + 24, arbitrary column offset
    tight = np.ascontiguousarray(np.stack(views))
    ex = Extractor(400, 1.2, 5, 20, 7, max_width=w, max_height=h, max_batch=n)
    ex.extract_batch_host(tight)
    want = [ex.batch_fetch(f) for f in range(n)]
    oex = oracle.Extractor(400, 1.2, 5, 20, 7)
    ok, od = oex.extract(tight[5])
    assert (want[5][0] == ok).all() and (want[5][1] == od).all()

    def check(frames, order=None):
        ex.extract_batch_host_frames(frames)
        for j in range(len(frames)):
            k, d = ex.batch_fetch(j)
            f = order[j] if order is not None else j
            assert np.array_equal(k, want[f][0]) and np.array_equal(d, want[f][1]), (j, f)
    check(views)                                                        # strided crops, one copy per frame
    order = [7, 2, 11, 0, 5, 9, 1]
    check([tight[f] for f in order], order)                             # tight frames out of order
    order = [0, 1, 4, 5, 8, 9]
    check([tight[f] for f in order], order)                             # runs of two at one distance: the two-dimensional copy
    L = ex.L
    L.ygzf_alloc_host.restype = C.c_void_p
    L.ygzf_alloc_host.argtypes = [C.c_int, C.c_size_t]
    L.ygzf_free_host.argtypes = [C.c_void_p]
    ptr = C.c_void_p(L.ygzf_alloc_host(0, tight.nbytes))
    assert ptr.value
    pinned = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(tight.nbytes,)).reshape(tight.shape)
    pinned[:] = tight
    order = [3, 10, 4, 6]
    check([pinned[f] for f in order], order)                            # page-locked, irregular
    check([pinned[f] for f in range(n)])                                # page-locked, one block
    ex.sync()
    del pinned
    L.ygzf_free_host(ptr)


def test_packed_fetch_equals_fetch_all():
    """ygzf_batch_fetch_packed (counts / keypoint rows / descriptor rows gathered by a kernel, ONE device-to-host copy: the result path of one-frame
    and one-pair calls) returns the bytes of ygzf_batch_fetch_all, for full and partial batches and for images smaller than the context's maximum."""
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=4)
    for (w, h, n) in ((752, 480, 4), (752, 480, 1), (640, 400, 3), (752, 480, 2)):
        imgs = np.stack([synth_frame(300 + i, w, h) for i in range(n)])
        ex.extract_batch_host(imgs)
        cnt, kps, desc = ex.batch_fetch_packed()
        assert len(cnt) == n and (cnt > 300).all()
        for f in range(n):
            k, d = ex.batch_fetch(f)
            assert cnt[f] == len(k) and np.array_equal(kps[f, :cnt[f]], k) and np.array_equal(desc[f, :cnt[f]], d), (w, h, n, f)
    ex.close()


def test_carry_previous_switch(oracle):
    """ygzf_set_carry_previous (include/ygzf.h): off, a batch extraction returns the same bytes and leaves slot 0 alone -- the batch matcher then
    refuses (there is no Last frame for pair 0, src/Tracking.cc:1262); on again, the next extraction carries the then-last frame and the matcher's
    pair 0 is what an uninterrupted context computes."""
    from orb_ygz_slam_amd import Extractor, make_camera
    from orb_ygz_slam_amd.capi import YgzfError
    w, h = 752, 480
    imgs = np.stack([synth_frame(300 + i, w, h) for i in range(4)])
    cam = make_camera(w, h)
    ref = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
    ref.extract_batch_host(imgs[:2])
    ex.extract_batch_host(imgs[:2])
    ex.set_carry_previous(False)
    ref.extract_batch_host(imgs[:2])
    ex.extract_batch_host(imgs[:2])
    for f in range(2):
        (ka, da), (kb, db) = ref.batch_fetch(f), ex.batch_fetch(f)
        assert np.array_equal(ka, kb) and np.array_equal(da, db)
    with pytest.raises(YgzfError):
        ex.match_batch_prev(cam, 15.0, True, True, True)
    ex.set_carry_previous(True)
    ref.extract_batch_host(imgs[2:])
    ex.extract_batch_host(imgs[2:])
    ref.match_batch_prev(cam, 15.0, True, True, True)
    ex.match_batch_prev(cam, 15.0, True, True, True)
    assert np.array_equal(ref.match_counts(), ex.match_counts()) and ref.match_counts()[0] > 50
    for f in range(2):
        (ma, oa), (mb, ob) = ref.match_fetch(f), ex.match_fetch(f)
        assert np.array_equal(ma, mb) and np.array_equal(oa, ob)
    ref.close(); ex.close()


def test_link_kernels_and_copy_engine_agree(oracle, monkeypatch):
    """Small blocks of a one-frame call cross the link by kernel (a page-locked frame read where it lies, the result rows / the pyramid levels written into
    the page-locked staging area); YGZF_FORCE=upload_kernel_frames=0,fetch_kernel=0,pyr_link=0 brings the copy engine back: same keypoints, descriptors
    and levels either way, from pageable and from page-locked frames."""
    import ctypes as C
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env, load_library
    w, h = 640, 480
    img = synth_frame(411, w, h)
    L = load_library()
    L.ygzf_alloc_host.restype = C.c_void_p
    L.ygzf_alloc_host.argtypes = [C.c_int, C.c_size_t]
    L.ygzf_free_host.argtypes = [C.c_void_p]
    ptr = L.ygzf_alloc_host(0, w * h)                       # page-locked, device-visible (include/ygzf.h)
    assert ptr
    pinned = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(h, w))
    pinned[:] = img
    oex = oracle.Extractor(1000, 1.2, 8, 20, 7)
    want_k, want_d = oex.extract(img)
    want_pyr = oex.pyramid(img)
    for force in ({}, {"upload_kernel_frames": 0, "fetch_kernel": 0, "pyr_link": 0}):
        monkeypatch.setenv("YGZF_FORCE", force_env(**force))
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
        for frame in (img, pinned):
            k, d = ex.extract(frame)
            assert all((k[f] == want_k[f]).all() for f in ("x", "y", "angle", "response", "octave")) and (d == want_d).all()
            pyr = ex.compute_pyramid(frame)
            assert all(np.array_equal(p, q) for p, q in zip(pyr, want_pyr))
            ex.extract_batch_host(np.stack([frame, frame]))
            kb, db = ex.batch_fetch(1)
            assert np.array_equal(kb, k) and np.array_equal(db, d)
        ex.close()
    L.ygzf_free_host(ptr)
