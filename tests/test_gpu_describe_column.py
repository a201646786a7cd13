"""describe_window's two-phase column pass on the device (sample the pattern's 375 distinct points once, in the point table's order; compare the
pairs' two bytes): keypoints, angles and descriptors equal the oracle's byte for byte, over every keypoint, through both kernels that share it.

  * k_describe: the synthetic 160 x 120 frame and its three 90-degree rotations (orientations in all four quadrants; interior windows and the
    REFLECT_101 byte path of keys 19 and 20 px from a border) in the three cv modes, and three differing frames in one batch call, one of them
    with an odd keypoint count (a workgroup holds two keypoints: the last one then has a single live wave);
  * k_describe_list: an odd number of existing keys on the same image, with preset angles and with computed ones;
  * YGZF_CV_LEGACY_SSE2's tie rule on a tie image (tests/blur_cases.py) 163 columns wide: a seventh of the body's columns tie and round to even,
    the last column ties inside the scalar tail [160, 163) and rounds half up, and keys 19 px from the right border sample both."""
import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame
from tests.blur_cases import blur_model, tie_image

pytestmark = pytest.mark.gpu

W, H, NLEVELS, NFEATURES, INI_TH, MIN_TH = 160, 120, 3, 200, 20, 7
CFG = (NFEATURES, 1.2, NLEVELS, INI_TH, MIN_TH)
MODES = (0, 1, 2)
SEED = 31


def frames():
    base = synth_frame(SEED, W, H)
    return [np.ascontiguousarray(np.rot90(base, k)) for k in range(4)]


def extractor(w, h, mode, batch=1):
    from orb_ygz_slam_amd import Extractor
    return Extractor(*CFG, max_width=w, max_height=h, max_batch=batch, cv_mode=mode)


@pytest.fixture(scope="module")
def expected(oracle):
    """{(mode, rotation): (keys, descriptors)} of the oracle, once"""
    oex = oracle.Extractor(*CFG)
    out = {}
    for mode in MODES:
        with oracle.cv_mode(mode):
            for k, img in enumerate(frames()):
                out[mode, k] = oex.extract(img)
    return out


def test_the_frames_cover_all_quadrants_and_both_staging_paths(expected):
    ang = np.concatenate([expected[1, k][0]["angle"] for k in range(4)])
    assert all(((ang >= 90 * q) & (ang < 90 * q + 90)).sum() >= 20 for q in range(4))
    keys = expected[1, 0][0]
    lvl0 = keys[keys["octave"] == 0]
    border = (lvl0["x"] < 21) | (lvl0["x"] > W - 22) | (lvl0["y"] < 21) | (lvl0["y"] > H - 23)
    assert border.any() and (~border).sum() >= 20
    assert all(len(expected[m, k][0]) > 100 for m in MODES for k in range(4))


@pytest.mark.parametrize("mode", MODES)
def test_rotated_frames_in_each_mode(expected, mode):
    for k, img in enumerate(frames()):
        h, w = img.shape
        ex = extractor(w, h, mode)
        keys, desc = ex.extract(img)
        ok, od = expected[mode, k]
        assert len(keys) == len(ok) and (keys == ok).all(), (mode, k)
        assert (desc == od).all(), "mode %d, rotation %d: %d of %d descriptors differ" % (mode, k, int((desc != od).any(axis=1).sum()), len(od))
        ex.close()


def test_three_frames_in_one_batch_with_an_odd_count(oracle):
    imgs = np.stack([synth_frame(SEED, W, H), synth_frame(SEED + 6, W, H), np.random.default_rng(SEED).integers(0, 256, (H, W), dtype=np.uint8)])
    oex = oracle.Extractor(*CFG)
    want = [oex.extract(im) for im in imgs]
    assert any(len(k) % 2 == 1 for k, _ in want) and len({len(k) for k, _ in want}) > 1
    ex = extractor(W, H, 1, batch=3)
    ex.extract_batch_host(imgs)
    assert list(ex.batch_counts()) == [len(k) for k, _ in want]
    for f, (ok, od) in enumerate(want):
        keys, desc = ex.batch_fetch(f)
        assert len(keys) == len(ok) and (keys == ok).all() and (desc == od).all(), f
    ex.close()


@pytest.mark.parametrize("mode", MODES)
def test_explicit_key_list(oracle, expected, mode):
    img = frames()[0]
    keys = expected[mode, 0][0]
    keys = keys[:len(keys) - 1 + len(keys) % 2].copy()      # an odd number: the last workgroup of k_describe_list has one live wave
    assert len(keys) % 2 == 1 and len(set(keys["octave"])) == NLEVELS
    preset = keys.copy()
    preset["angle"] = np.float32(360.0) - keys["angle"]      # angles that are NOT the keys' own
    oex = oracle.Extractor(*CFG)
    ex = extractor(W, H, mode)
    ex.extract_batch_host(img[None])
    with oracle.cv_mode(mode):
        for given, recompute in ((keys, True), (preset, False)):
            ek, ed = oex.describe_keys(img, given, recompute_angle=recompute)
            ang, d = ex.describe_keys(given, frame=0, recompute_angle=recompute)
            assert (ang.view(np.uint32) == ek["angle"].view(np.uint32)).all(), (mode, recompute)
            assert (d == ed).all(), "mode %d, recompute %s: %d of %d descriptors differ" % (mode, recompute, int((d != ed).any(axis=1).sum()), len(ed))
            if not recompute:
                assert (ang == preset["angle"]).all() and (ed != expected[mode, 0][1][:len(keys)]).any()
    ex.close()


def test_legacy_sse2_ties_in_the_body_and_in_the_tail(oracle):
    from orb_ygz_slam_amd.capi import KP_DTYPE
    w, h = 163, 120
    assert w & 3
    img = tie_image(7 + w, w, h, tail_tie=True)
    xy = [(x, y) for x in (19, 24, 61, 83, w - 41, w - 23, w - 19) for y in (19, 33, 60, h - 19)]
    angles = [0.0, 12.5, 33.0, 54.0, 90.0, 140.0, 181.0, 227.0, 300.25, 359.5]      # at 54, 140 and 227 a point of the keys at w - 19 lands on the last column
    keys = np.zeros(len(xy) * len(angles), KP_DTYPE)
    keys["size"], keys["class_id"] = 31.0, -1
    keys["x"], keys["y"] = np.repeat(np.array(xy, np.float32), len(angles), axis=0).T
    keys["angle"] = np.tile(np.array(angles, np.float32), len(xy))
    got, want = {}, {}
    for mode in (0, 1):
        ex = extractor(w, h, mode)
        ex.extract_batch_host(img[None])
        _, got[mode] = ex.describe_keys(keys, frame=0, recompute_angle=False)
        ex.close()
        oex = oracle.Extractor(*CFG)
        with oracle.cv_mode(mode):
            b = oracle.blur(img)
        want[mode] = np.stack([oex.descriptor(b, float(k["x"]), float(k["y"]), float(k["angle"])) for k in keys])
        assert (got[mode] == want[mode]).all(), "mode %d: %d of %d rows differ" % (mode, int((got[mode] != want[mode]).any(axis=1).sum()), len(keys))
    assert (want[0] != want[1]).any()      # the body's ties separate the two rules ...
    # ... and the tail's tie is sampled: rounding it to even as well would give other descriptors at the right border
    b0, s = blur_model(img, 0)
    tail_even = np.where((s & 0xFFFF) == 0x8000, ((s + 32768) >> 16) & ~1, (s + 32768) >> 16).astype(np.uint8)
    right = np.flatnonzero((keys["x"] == w - 19) & np.isin(keys["angle"], (54.0, 140.0, 227.0)))
    assert len(right) == 12
    assert all((oex.descriptor(tail_even, float(k["x"]), float(k["y"]), float(k["angle"])) != want[0][i]).any() for i, k in zip(right, keys[right]))
