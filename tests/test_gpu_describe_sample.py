"""describe_window's column pass with its sample arithmetic in float (orb_ygz_slam_amd/csrc/describe_sample.h: the rotated pattern point rounded on
the float adder, the hb address by two float multiply-adds, the taps as a multiply-add chain), on the device, against the oracle byte for byte, in
the three cv modes, through both kernels that share describe_window.  One 160 x 120 frame, 2 levels.

  * k_describe: the frame's own keypoints (computed angles; interior windows and the byte path of keys less than 21 px from a border), an odd
    number of them on one level at least;
  * k_describe_list: 41 keys (an odd count: the last workgroup has one live wave) with preset angles that put rotated coordinates on or next to
    ties -- 0, 90, 180, 270 (cos, sin = +-1 and a float's rounding error of 0: every coordinate an integer, or a hair off one) and the eight angles
    with cos or sin = +-0.5 (odd coordinates land on, or a hair off, .5) --, on both levels, interior and on the border path.

tests/test_describe_sample_cpu.py runs the same header text over every pattern point and angle on the CPU."""
import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame
from tests.device_frame_cases import KP_FIELDS, level_size

pytestmark = pytest.mark.gpu

W, H, NLEVELS, NFEATURES, INI_TH, MIN_TH = 160, 120, 2, 200, 20, 7
CFG = (NFEATURES, 1.2, NLEVELS, INI_TH, MIN_TH)
MODES = (0, 1, 2)
SEED = 31
TIE_ANGLES = (0.0, 90.0, 180.0, 270.0, 60.0, 120.0, 240.0, 300.0, 30.0, 150.0, 210.0, 330.0)


def frame():
    return synth_frame(SEED, W, H)


def tie_keys():
    """41 keys, at least 19 px from every border of their level: level 0 interior (29), level 0 on the border path (8), level 1 (4: two interior, two
    border), every one of TIE_ANGLES at least three times, all of them on interior keys."""
    interior = [(x, y) for y in (21, 40, 60, 80, 97) for x in (21, 47, 75, 101, 127, 138)][:29]
    border = [(19, 19), (20, 60), (W - 20, 30), (W - 21, 90), (60, 19), (90, H - 20), (30, H - 22), (W - 20, H - 20)]
    w1, h1 = level_size(W, H, 1)
    lvl1 = [(21, 21), (w1 // 2, h1 // 2), (19, h1 - 20), (w1 - 20, 40)]
    assert all(21 <= x <= W - 22 and 21 <= y <= H - 23 for x, y in interior)
    assert all(19 <= x <= W - 20 and 19 <= y <= H - 20 and not (21 <= x <= W - 22 and 21 <= y <= H - 23) for x, y in border)
    assert all(19 <= x <= w1 - 20 and 19 <= y <= h1 - 20 for x, y in lvl1)
    k = np.zeros(len(interior) + len(border) + len(lvl1), np.dtype(KP_FIELDS))
    k["size"], k["class_id"] = 31.0, -1
    n0 = len(interior) + len(border)
    k["x"][:n0], k["y"][:n0] = np.array(interior + border, np.float32).T
    s1 = np.float32(1.2)
    for i, (x, y) in enumerate(lvl1):                                  # stored in level-0 coordinates, as cv::KeyPoint::pt is
        k[n0 + i] = (np.float32(x) * s1, np.float32(y) * s1, np.float32(31.0) * s1, 0.0, 0.0, 1, -1)
    k["angle"] = np.resize(np.array(TIE_ANGLES, np.float32), len(k))
    assert len(k) == 41
    return k


@pytest.fixture(scope="module")
def expected(oracle):
    """{mode: ((keys, descriptors) of the frame, descriptors of tie_keys())} of the oracle, once"""
    img, given = frame(), tie_keys()
    oex = oracle.Extractor(*CFG)
    out = {}
    for mode in MODES:
        with oracle.cv_mode(mode):
            ek, ed = oex.describe_keys(img, given, recompute_angle=False)
            assert (ek["angle"] == given["angle"]).all()
            out[mode] = (oex.extract(img), ed)
    return out


def test_the_cases_are_what_they_claim(expected):
    keys = expected[1][0][0]
    assert len(keys) > 60 and set(keys["octave"]) == {0, 1}
    assert any((keys["octave"] == l).sum() % 2 == 1 for l in (0, 1)) or len(keys) % 2 == 1
    lvl0 = keys[keys["octave"] == 0]
    border = (lvl0["x"] < 21) | (lvl0["x"] > W - 22) | (lvl0["y"] < 21) | (lvl0["y"] > H - 23)
    assert border.any() and (~border).sum() >= 20
    given = tie_keys()
    assert len(given) % 2 == 1 and all((given["angle"] == a).sum() >= 3 for a in TIE_ANGLES)
    # the preset angles and the cv modes matter: the tie keys' descriptors differ between two angles of one position and between the tap sets
    assert (expected[1][1] != expected[2][1]).any()
    assert len({bytes(d) for d in expected[1][1]}) == len(given)


@pytest.mark.parametrize("mode", MODES)
def test_k_describe_and_k_describe_list_against_the_oracle(expected, mode):
    from orb_ygz_slam_amd import Extractor
    img, given = frame(), tie_keys()
    (ok, od), ed = expected[mode]
    ex = Extractor(*CFG, max_width=W, max_height=H, max_batch=1, cv_mode=mode)
    keys, desc = ex.extract(img)
    assert len(keys) == len(ok) and (keys == ok).all(), mode
    assert (desc == od).all(), "k_describe, mode %d: %d of %d descriptors differ" % (mode, int((desc != od).any(axis=1).sum()), len(od))
    ex.extract_batch_host(img[None])
    ang, d = ex.describe_keys(given, frame=0, recompute_angle=False)
    assert (ang == given["angle"]).all()
    assert (d == ed).all(), "k_describe_list, mode %d: %d of %d descriptors differ" % (mode, int((d != ed).any(axis=1).sum()), len(ed))
    ex.close()
