"""fast9_arc_score computes the corner score on f16 pairs (a byte b as the f16 number 1024 + b, margins by one packed add, three-input
packed minimum / maximum over the arcs): candidates (x, y, score, order), keypoints, angles and descriptors must stay EQUAL to the
oracle's through every caller -- the register path, the listed path, the dense fallback and k_fast_quads -- on the smallest shapes that
reach each of them:
  210x134, one level    cells of 36 x 34: nine quads per row and a fifth pass-1 round (the flagship's level 7)
  82x82, one level      one 50-px cell: k_fast_quads with a run-time window pitch
  160x120, two levels   two levels and a clipped last column
on both kernels, both threshold plans, two threshold pairs, and on contents that reach the dense fallback (noise), saturation of c + t and
c - t (values drawn from {0, 3, 252, 255}: margins up to 255), the extreme score 254 in both polarities (isolated pixels) and equal scores
everywhere (ties)."""
import functools

import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

SHAPES = [(210, 134, 1), (82, 82, 1), (160, 120, 2)]
THRESHOLDS = [(20, 7), (40, 5)]
CONTENTS = ("synthetic", "noise", "extremes", "isolated", "ties")


@functools.lru_cache(maxsize=None)
def _image(name, w, h):
    rng = np.random.default_rng(1000 * w + h)
    if name == "synthetic":
        img = synth_frame(5, w, h)
    elif name == "noise":                                     # > 512 corners per cell: fast9_test + score on every pixel
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif name == "extremes":                                  # c + t > 255 and c - t < 0 both occur, margins up to 255
        img = np.array([0, 3, 252, 255], np.uint8)[rng.integers(0, 4, (h, w))]
    elif name == "isolated":                                  # 255 on 0 (dark ring, score 254) and 0 on 255 (bright ring, score 254)
        img = np.zeros((h, w), np.uint8)
        img[:, w // 2:] = 255
        img[5::9, 5:w // 2 - 8:7] = 255
        img[7::9, w // 2 + 8::7] = 0
    else:                                                     # the `ties` pattern of test_gpu_fast_plans.py
        img = np.zeros((h, w), np.uint8)
        img[::2, ::2] = 200
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


_oracle_cache = {}


def _expected(oracle, name, w, h, nl, ini, mn, mode=0):
    """(candidates per level, keypoints, descriptors) of the oracle, computed once per input and shared"""
    key = (name, w, h, nl, ini, mn, mode)
    if key not in _oracle_cache:
        with oracle.cv_mode(mode):
            oex = oracle.Extractor(1000, 1.2, nl, ini, mn)
            k, d = oex.extract(_image(name, w, h))
            cands = [oex.cell_candidates(l) for l in range(nl)]
        _oracle_cache[key] = (cands, k, d)
    return _oracle_cache[key]


def _check(ex, want, nl, what):
    cands, ok, od = want
    for l in range(nl):
        xs, ys, sc = cands[l]
        gx, gy, gs = ex.batch_fetch_candidates(0, l)
        assert len(gx) == len(xs), (what, l, len(gx), len(xs))
        assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc), (what, l)
    k, d = ex.batch_fetch(0)
    assert len(k) == len(ok), (what, len(k), len(ok))
    for f in ("x", "y", "response", "angle", "octave", "size"):
        assert np.array_equal(k[f], ok[f]), (what, f)
    assert np.array_equal(d, od), what


@pytest.mark.parametrize("plan", [1, 2])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("ini,mn", THRESHOLDS)
@pytest.mark.parametrize("w,h,nl", SHAPES)
def test_candidates_keypoints_descriptors_equal_the_oracle(oracle, w, h, nl, ini, mn, kernel, plan):
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(1000, 1.2, nl, ini, mn, max_width=w, max_height=h, max_batch=1)
    ex.set_fast_kernel(kernel)
    ex.set_fast_plan(plan)
    for name in CONTENTS:
        ex.extract_batch_host(_image(name, w, h)[None])
        _check(ex, _expected(oracle, name, w, h, nl, ini, mn), nl, (name, w, h, kernel, plan, ini, mn))
    ex.close()


def test_the_inputs_reach_the_cases_they_are_named_for(oracle):
    """What the comparison above rests on, asserted on the oracle's own output (no GPU result is looked at)."""
    w, h, nl = 210, 134, 1
    for ini, mn in THRESHOLDS:
        sc = _expected(oracle, "isolated", w, h, nl, ini, mn)[0][0][2]
        assert len(sc) > 20 and (sc == 254).all()                       # the largest score there is, from both halves of the image
        xs = _expected(oracle, "isolated", w, h, nl, ini, mn)[0][0][0]
        assert (xs < w // 2).any() and (xs > w // 2).any()              # ... i.e. both polarities
        sc = _expected(oracle, "extremes", w, h, nl, ini, mn)[0][0][2]
        assert len(sc) > 100 and sc.min() >= 248 and sc.max() <= 254    # margins of 249 .. 255: c + t and c - t saturate at either threshold
        assert len(_expected(oracle, "noise", w, h, nl, ini, mn)[0][0][0]) > 1000
    assert len(_expected(oracle, "ties", w, h, nl, 20, 7)[0][0][0]) == 0   # equal scores everywhere: the NMS keeps nothing
