"""Error conventions of the C ABI on a live device: every misuse returns a negative status with an explanation (no exception crosses
the ABI, nothing is silently clamped), and the context stays usable afterwards."""
import ctypes as C

import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame

pytestmark = pytest.mark.gpu


def test_misuse_is_reported_not_absorbed(oracle):
    from orb_ygz_slam_amd import Extractor, make_camera
    from orb_ygz_slam_amd.capi import KP_DTYPE, ExtractorCfg, YgzfError, load_library
    L = load_library()
    # bad configurations are rejected at create time
    for cfg in ((1000, 1.0, 8, 20, 7), (1000, 1.2, 0, 20, 7), (1000, 1.2, 17, 20, 7), (-1, 1.2, 8, 20, 7), (1000, 1.2, 8, 7, 20), (1000, 1.2, 8, 300, 7)):
        h = C.c_void_p()
        c = ExtractorCfg(*cfg)
        assert L.ygzf_create(0, C.byref(c), 640, 480, 1, C.byref(h)) < 0 and not h.value
        assert len(L.ygzf_last_error(None)) > 0
    h = C.c_void_p()
    assert L.ygzf_create(99, C.byref(ExtractorCfg(1000, 1.2, 8, 20, 7)), 640, 480, 1, C.byref(h)) < 0      # no such device
    # one past the last visible device: YGZF_ERR_NO_DEVICE (-2), never a silent fall-back to device 0; the last device itself works
    import torch
    nd = torch.cuda.device_count()
    assert L.ygzf_create(nd, C.byref(ExtractorCfg(1000, 1.2, 8, 20, 7)), 640, 480, 1, C.byref(h)) == -2 and not h.value
    assert L.ygzf_create(-1, C.byref(ExtractorCfg(1000, 1.2, 8, 20, 7)), 640, 480, 1, C.byref(h)) == -2 and not h.value
    assert b"out of range" in L.ygzf_last_error(None)
    last = Extractor(300, 1.2, 4, 20, 7, max_width=320, max_height=240, device=nd - 1)
    k_last, _ = last.extract(synth_frame(2, 320, 240))
    assert len(k_last) > 0
    last.close()
    assert L.ygzf_create(0, C.byref(ExtractorCfg(1000, 1.2, 8, 20, 7, 3)), 640, 480, 1, C.byref(h)) == -1   # cv_mode out of range
    w, hh = 640, 480
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=hh, max_batch=2)
    img = synth_frame(0, w, hh)
    # state errors: nothing extracted yet
    with pytest.raises(YgzfError):
        ex.batch_fetch(0)
    with pytest.raises(YgzfError):
        ex.match_counts()
    with pytest.raises(YgzfError):
        ex.stereo_fetch(0)
    # a batch larger than the context was created for, an image larger than planned
    with pytest.raises(YgzfError):
        ex.extract_batch_host(np.stack([img] * 3))
    with pytest.raises(YgzfError):
        ex.extract(synth_frame(1, 800, 600))
    # capacity too small: the count is reported, nothing is written past the buffer
    k = np.zeros(10, KP_DTYPE)
    d = np.zeros((10, 32), np.uint8)
    n = C.c_int()
    rc = L.ygzf_extract(ex.h, img.ctypes.data_as(C.c_void_p), w, hh, w, k.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), 10, C.byref(n))
    assert rc < 0 and n.value > 10 and (k["x"] == 0).all()
    # stereo needs (left, right) pairs; frame index out of range
    ex.extract_batch_host(img[None])
    with pytest.raises(YgzfError):
        ex.stereo_batch(0.11, 47.9)
    with pytest.raises(YgzfError):
        ex.batch_fetch(1)
    # unaligned device frames are refused (4-byte alignment contract of the resident-batch entry)
    with pytest.raises(YgzfError):
        ex.extract_batch_device(0x7F0000001001, 1, w, hh)      # rejected on the address alone, never dereferenced
    # existing keys outside their level / bad octave in the DSO path
    bad = np.zeros(1, KP_DTYPE)
    bad["x"], bad["y"], bad["octave"] = 3.0, 3.0, 0
    with pytest.raises(YgzfError):
        ex.extract_dso(img, existing=bad)
    bad["x"], bad["y"], bad["octave"] = 100.0, 100.0, 9
    with pytest.raises(YgzfError):
        ex.extract_dso(img, existing=bad)
    # direct projection without a cache / with an empty slot
    cam = make_camera(w, hh)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    with pytest.raises(YgzfError):
        ex.find_direct_projection_batch(cam, 0, ident, [0], ident[None], bad, np.zeros((1, 3), np.float32), np.zeros((1, 2), np.float32))
    ex.image_cache_reserve(2, w, hh)
    ex.image_cache_put(0, img)
    with pytest.raises(YgzfError):
        ex.find_direct_projection_batch(cam, 1, ident, [0], ident[None], bad, np.zeros((1, 3), np.float32), np.zeros((1, 2), np.float32))
    # after all that the context still produces correct results
    kk, dd = ex.extract(img)
    ok, od = oracle.Extractor(1000, 1.2, 8, 20, 7).extract(img)
    assert (kk == ok).all() and (dd == od).all()


def test_extract_resident_needs_the_pyramid_it_was_promised(oracle):
    """ygzf_extract_resident runs on what ygzf_compute_pyramid left on the device: any image operation in between (another extraction, a batch
    that makes the image / pyramid buffers grow, another geometry) must turn it into YGZF_ERR_STATE, never into an extraction of overwritten data"""
    from orb_ygz_slam_amd import Extractor, YgzfError
    from orb_ygz_slam_amd.synth import synth_frame
    w, h = 320, 240
    a, b = synth_frame(61, w, h), synth_frame(62, w, h)
    oex = oracle.Extractor(500, 1.2, 4, 20, 7)
    ex = Extractor(500, 1.2, 4, 20, 7, max_width=2 * w, max_height=2 * h, max_batch=8)
    ex.compute_pyramid(a)
    k, d = ex.extract_resident(w, h)                      # the promised case
    ok, od = oex.extract(a)
    assert (k == ok).all() and (d == od).all()
    for spoil in (lambda: ex.extract(b), lambda: ex.extract_batch_host(np.stack([b] * 8)), lambda: ex.extract_dso(b),
                  lambda: ex.extract_batch_host(np.stack([synth_frame(63, 2 * w, 2 * h)] * 8))):      # (the last one makes the buffers grow)
        ex.compute_pyramid(a)
        spoil()
        try:
            k2, d2 = ex.extract_resident(w, h)
        except YgzfError:
            continue
        raise AssertionError("extract_resident succeeded after an intervening image operation")


def test_round6_entry_points_report_misuse():
    """ygzf_batch_fetch_packed, ygzf_stereo_pair_host, ygzf_host_stream_probe, ygzf_phase_clocks: bad arguments come back as a negative status with a
    message, the contexts stay usable."""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import YgzfError, load_library, host_stream_probe
    L = load_library()
    w, h = 320, 240
    a = Extractor(300, 1.2, 4, 20, 7, max_width=w, max_height=h, max_batch=2)
    b = Extractor(300, 1.2, 4, 20, 7, max_width=w, max_height=h, max_batch=2)
    img = synth_frame(5, w, h)
    host = np.zeros(1 << 20, np.uint8)
    ok, od, by = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    row = C.c_int(0)
    L.ygzf_batch_fetch_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # nothing extracted yet; then a buffer that is too small
    assert L.ygzf_batch_fetch_packed(a.h, host.ctypes.data_as(C.c_void_p), host.nbytes, C.byref(ok), C.byref(od), C.byref(row), C.byref(by)) < 0
    a.extract_batch_host(img[None])
    assert L.ygzf_batch_fetch_packed(a.h, host.ctypes.data_as(C.c_void_p), 1000, C.byref(ok), C.byref(od), C.byref(row), C.byref(by)) < 0
    assert b"packed results need" in L.ygzf_last_error(a.h)
    assert L.ygzf_batch_fetch_packed(a.h, host.ctypes.data_as(C.c_void_p), host.nbytes, C.byref(ok), C.byref(od), C.byref(row), C.byref(by)) == 0 and by.value > 0
    # the carry switch: no context
    L.ygzf_set_carry_previous.argtypes = [C.c_void_p, C.c_int]
    assert L.ygzf_set_carry_previous(None, 0) < 0
    # the pair entry point: the same context twice, a null eye, a pitch below the width
    L.ygzf_stereo_pair_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    hl, hr = np.zeros(1 << 20, np.uint8), np.zeros(1 << 20, np.uint8)
    ur, dp = np.zeros(4096, np.float32), np.zeros(4096, np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    args = lambda l, r, le, ri, pitch: (l, r, le, ri, w, h, pitch, 0.11, 47.9, p(hl), p(hr), hl.nbytes, C.byref(ok), C.byref(od), C.byref(row), p(ur), p(dp))
    assert L.ygzf_stereo_pair_host(*args(a.h, a.h, p(img), p(img), w)) < 0
    assert L.ygzf_stereo_pair_host(*args(a.h, b.h, p(img), None, w)) < 0
    assert L.ygzf_stereo_pair_host(*args(a.h, b.h, p(img), p(img), w - 8)) < 0
    right = np.zeros_like(img)
    right[:, :w - 9] = img[:, 9:]                                                      # the left image seen 9 px to the side
    assert L.ygzf_stereo_pair_host(*args(a.h, b.h, p(img), p(right), w)) == 0         # and the well-formed call works
    n = int(hl[:4].view(np.int32)[0])
    assert n > 50 and (ur[:n] >= 0).sum() > n // 4
    k0, d0 = a.batch_fetch(0)
    assert len(k0) == n
    # two eyes of one size from extractors that differ: another scale factor (the pairing reads both with the left eye's scale tables), another
    # blur generation (the same level layout and keypoint stride: only the extractors' settings tell them apart)
    for other in (Extractor(300, 1.3, 4, 20, 7, max_width=w, max_height=h, max_batch=2),
                  Extractor(300, 1.2, 4, 20, 7, max_width=w, max_height=h, max_batch=2, cv_mode=2)):
        assert L.ygzf_stereo_pair_host(*args(a.h, other.h, p(img), p(right), w)) == -5  # YGZF_ERR_STATE
        assert b"differ" in L.ygzf_last_error(a.h)
        other.close()
    assert b"extractors differ" in L.ygzf_last_error(a.h)                            # (the blur generation: nothing but the settings differs)
    assert L.ygzf_stereo_pair_host(*args(a.h, b.h, p(img), p(right), w)) == 0         # the pair of equal extractors still works
    assert int(hl[:4].view(np.int32)[0]) == n
    # the probe and the phase clocks
    with pytest.raises(YgzfError):
        host_stream_probe(0, 0, 1 << 26, 0.1)
    with pytest.raises(YgzfError):
        host_stream_probe(0, 2, 1000, 0.1)
    assert host_stream_probe(0, 2, 8 << 20, 0.05) > 0.1
    with pytest.raises(YgzfError):
        a.phase_clocks(0)                                                              # the product library carries no stamps
    a.close(); b.close()


def test_stereo_right_keypoint_count_limit():
    """ygzf_compute_stereo_matches packs the right index into 16 bits of its key: 65536 right keypoints are refused with YGZF_ERR_INVALID (-1)
    and a message, nothing is launched, and 65535 are accepted on the same context afterwards"""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import KP_DTYPE, load_library
    L = load_library()
    w, h = 320, 240
    ex = Extractor(300, 1.2, 4, 20, 7, max_width=w, max_height=h, max_batch=2)
    img = np.ascontiguousarray(synth_frame(9, w, h))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    kl = np.zeros(1, KP_DTYPE)
    kl["x"], kl["y"] = 200.0, 100.0
    dl = np.zeros((1, 32), np.uint8)
    kr = np.zeros(65536, KP_DTYPE)
    kr["x"], kr["y"] = 180.0, 100.0
    dr = np.full((65536, 32), 255, np.uint8)
    dr[65534] = 0                                                        # the one right keypoint within the descriptor threshold: the last index
    ur, dp = np.full(1, 7, np.float32), np.full(1, 7, np.float32)
    call = lambda n: L.ygzf_compute_stereo_matches(ex.h, p(img), p(img), w, h, w, 1, p(kl), p(dl), n, p(kr), p(dr), 0.5, 32.0, p(ur), p(dp))
    assert call(65536) == -1 and b"keypoint counts" in L.ygzf_last_error(ex.h)
    assert ur[0] == 7 and dp[0] == 7                                     # refused before anything was written
    assert call(65535) == 0
    assert ur[0] != 7 and dp[0] != 7
    ex.close()
