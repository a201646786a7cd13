"""fast9_quad decides "nine contiguous of the circular sixteen" with 32 operations per polarity and takes its thresholds in the high byte of each
16-bit half (orb_ygz_slam_amd/csrc/fast9_quad.h).  Here the decision is put on constructed rings: candidates (x, y, score), keypoints and
descriptors must be EQUAL to the oracle's on
  210x134, one level    cells of 36 x 34: nine quads per row and a fifth pass-1 round
  82x82, one level      one 50-px cell: k_fast_quads with a run-time window pitch
on both kernels, both threshold plans and the threshold pairs (20, 7) and (40, 5).

An image is tiles of 9 x 9 pixels, one image per (centre value c, threshold t of the pair, polarity).  A tile's centre pixel is c; on its ring an
arc of length 8, 9, 10 or 16 that starts at ring position s sits at exactly c +- (t + 1) and the other ring pixels at exactly c +- t, one below
the threshold; everything else in the image is c +- t as well, so nothing but a tile's centre can be a corner.  c is one of {0, 7, 20, 128, 235,
248, 255}: c + t + 1 and c - t - 1 reach and pass 255 and 0, and a polarity that a centre value cannot have at a threshold (c + t + 1 > 255,
c - t - 1 < 0) is left out.  The tested area of 210x134 (x in 19..190, y in 19..114) holds 19 x 10 tiles: tile n of an image has length
(8, 9, 10, 16)[n % 4] and start (n / 4 + an offset per image) % 16, so every image holds every length at every start, about three times, at changing
positions inside a quad; four neighbours in a row have the four lengths, so every cell holds a corner at the image's threshold and the arcs of 8
are never reached by the cell's FAST(minTh) retry.  82x82 holds 4 x 4 tiles per image: every length at four starts, and every start over the images.
What the comparison rests on -- a tile's centre is among the oracle's candidates exactly when its arc is 9 or longer, with score t -- is asserted
on the oracle alone (no GPU result is looked at)."""
import functools

import numpy as np
import pytest

SHAPES = [(210, 134), (82, 82)]
THRESHOLDS = [(20, 7), (40, 5)]
CENTRES = (0, 7, 20, 128, 235, 248, 255)
LENGTHS = (8, 9, 10, 16)
TILE = 9
# ring position k of a centre at (0, 0): (dx, dy), in the order of the circle
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
BORDER = 16
FIRST = BORDER + 3   # first tested pixel of a level: the image border and the 3-px margin of a cell's window


def _contents(ini, mn):
    """(c, t, sign) of every image of a threshold pair: sign +1 = bright arcs, -1 = dark arcs"""
    out = []
    for c in CENTRES:
        for t in (ini, mn):
            for sign in (1, -1):
                if 0 <= c + sign * (t + 1) <= 255:
                    out.append((c, t, sign))
    return out


def _tiles(w, h, c, t, sign):
    """[(centre x, centre y, arc length, arc start)] of the image (c, t, sign) at w x h"""
    nx, ny = (w - 2 * FIRST) // TILE, (h - 2 * FIRST) // TILE
    off = 4 * CENTRES.index(c) + (2 if sign < 0 else 0) + (1 if t > 10 else 0)   # 82x82: four centre values in a row cover the 16 starts
    return [(FIRST + TILE * (n % nx) + 4, FIRST + TILE * (n // nx) + 4, LENGTHS[n % 4], (n // 4 + off) % 16) for n in range(nx * ny)]


@functools.lru_cache(maxsize=None)
def _image(w, h, c, t, sign):
    img = np.full((h, w), c + sign * t, np.int32)
    for x, y, length, start in _tiles(w, h, c, t, sign):
        img[y, x] = c
        for j in range(length):
            dx, dy = RING[(start + j) % 16]
            img[y + dy, x + dx] = c + sign * (t + 1)
    assert img.min() >= 0 and img.max() <= 255
    img = np.ascontiguousarray(img.astype(np.uint8))
    img.setflags(write=False)
    return img


_oracle_cache = {}


def _expected(oracle, w, h, ini, mn, content):
    """(candidates, keypoints, descriptors) of the oracle, computed once per input and shared"""
    key = (w, h, ini, mn, content)
    if key not in _oracle_cache:
        oex = oracle.Extractor(1000, 1.2, 1, ini, mn)
        k, d = oex.extract(_image(w, h, *content))
        _oracle_cache[key] = (oex.cell_candidates(0), k, d)
    return _oracle_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [1, 2])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("ini,mn", THRESHOLDS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_candidates_keypoints_descriptors_equal_the_oracle(oracle, w, h, ini, mn, kernel, plan):
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(1000, 1.2, 1, ini, mn, max_width=w, max_height=h, max_batch=1)
    ex.set_fast_kernel(kernel)
    ex.set_fast_plan(plan)
    for content in _contents(ini, mn):
        what = (content, w, h, kernel, plan, ini, mn)
        (xs, ys, sc), ok, od = _expected(oracle, w, h, ini, mn, content)
        ex.extract_batch_host(_image(w, h, *content)[None])
        gx, gy, gs = ex.batch_fetch_candidates(0, 0)
        assert len(gx) == len(xs), (what, len(gx), len(xs))
        assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc), what
        k, d = ex.batch_fetch(0)
        assert len(k) == len(ok), (what, len(k), len(ok))
        for f in ("x", "y", "response", "angle", "octave", "size"):
            assert np.array_equal(k[f], ok[f]), (what, f)
        assert np.array_equal(d, od), what
    ex.close()


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_the_tiles_are_corners_exactly_when_their_arc_is_nine_or_longer(oracle, w, h, ini, mn):
    """Asserted on the oracle's own output: the candidates of every image are the centres of its tiles with an arc of 9, 10 or 16, each with
    score t, and nothing else -- no centre of an arc of 8, no other pixel."""
    contents = _contents(ini, mn)
    seen = set()
    for content in contents:
        c, t, sign = content
        xs, ys, sc = _expected(oracle, w, h, ini, mn, content)[0]
        tiles = _tiles(w, h, c, t, sign)
        want = sorted((x - BORDER, y - BORDER) for x, y, length, _ in tiles if length >= 9)   # candidates count from the border
        assert len(want) == len(tiles) * 3 // 4 and len(tiles) == ((w - 38) // 9) * ((h - 38) // 9)
        assert sorted(zip(xs.tolist(), ys.tolist())) == want, content
        assert (sc == t).all(), content
        seen.update((c, t, sign, length, start) for _, _, length, start in tiles)
    if w == 210:   # every image holds every length at every start
        assert seen == {(c, t, sign, length, start) for c, t, sign in contents for length in LENGTHS for start in range(16)}
    else:          # 16 tiles per image: every length at every start in both polarities over the images
        assert {(sign, length, start) for _, _, sign, length, start in seen} == {(sign, length, start) for sign in (1, -1) for length in LENGTHS for start in range(16)}
    # both polarities where the centre value allows them, one where it does not
    pols = {(c, t, sign) for c, t, sign in contents}
    assert {(128, ini, 1), (128, ini, -1), (128, mn, 1), (128, mn, -1), (0, ini, 1), (255, mn, -1), (235, mn, 1), (20, mn, -1)} <= pols
    assert not {(0, ini, -1), (0, mn, -1), (255, ini, 1), (255, mn, 1), (235, ini, 1), (20, ini, -1)} & pols
