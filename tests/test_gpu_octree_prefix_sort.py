"""k_octree's sort plan orders a level's path keys on their top 14 bits and starts the level over with the full sort when a tree pass would read
a digit below them (YGZF_FORCE=oct_sort=prefix, the default; oct_sort=full is the sort on every bit), copies its key tables from a buffer
written once per geometry, and orders its keypoints for k_describe by a compact tile key (csrc/extract_kernels.hip).  Both pins against the
oracle and against each other: octree list order per level, keypoints, descriptors (_cmp_frame).  Which levels start over is not left to the
device: tools/octree_proto.py, the executable specification, says for the oracle's candidates of every (level, frame) whether the tree
consults a digit below the sorted prefix, and the YGZF_DEBUG=oct report must show exactly those restarts -- none under oct_sort=full.

Launches carry five frames or more: from five frames on a launch sorts its keypoints into k_describe's processing order."""
import os
import re
import sys

import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame
from tests.test_gpu_extract import _cmp_frame

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import octree_proto as P  # noqa: E402

pytestmark = pytest.mark.gpu

_ORDER = re.compile(r"\[ygzf octree key order: (prefix|full); workgroups of (\d+) frames that started over with the full sort, per level:((?: \d+)+)\]")
_SMALL = re.compile(r"\[ygzf octree small plan")
_SORT = re.compile(r"\[ygzf octree (sort plan|single launch)")


class _env:
    """YGZF_FORCE with the given keys (None: absent) and YGZF_DEBUG=oct while a context is created"""
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from orb_ygz_slam_amd.capi import force_env
        self.old = {k: os.environ.get(k) for k in ("YGZF_FORCE", "YGZF_DEBUG")}
        os.environ["YGZF_FORCE"] = force_env(base="", **self.kv)
        os.environ["YGZF_DEBUG"] = "oct"

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _two_spots(seed, w, h):
    """test_gpu_octree_plans.py's clustered image: two 80x80 noise spots in an empty frame.  (Each spot falls into one child of its root, the
    list does not grow and the reference stops after the first pass, :696 -- two keypoints per level, no digit below the prefix is read.)"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 120, np.uint8)
    for (cx, cy) in ((w // 5, h // 4), (w - 90, h - 80)):
        img[cy - 40:cy + 40, cx - 40:cx + 40] = rng.integers(0, 256, (80, 80), dtype=np.uint8)
    return img


def _dots_and_spots(seed, w, h, half=12, ndots=100):
    """isolated bright pixels (a FAST corner each) spread over an empty frame, and two small noise spots: the dots keep the list growing through
    the full passes, then the expand phase takes the biggest nodes -- the spots -- first, again and again, down to cells of a pixel or two"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 120, np.uint8)
    img[rng.integers(20, h - 20, ndots), rng.integers(20, w - 20, ndots)] = 250
    for (cx, cy) in ((w // 5, h // 4), (w - 90, h - 80)):
        img[cy - half:cy + half, cx - half:cx + half] = rng.integers(0, 256, (2 * half, 2 * half), dtype=np.uint8)
    return img


def _frames(img):
    """five frames, three distinct"""
    a, b, c = img, np.ascontiguousarray(img[::-1]), np.ascontiguousarray(img[:, ::-1])
    return np.stack([a, b, c, a, b]), (2, 2, 1)


_expected = {}


def _expected_restarts(key, distinct, times, nf, nl):
    """per level: the (level, frame) pairs of the launch whose tree consults a digit below the sorted prefix, by the specification; and the key layout"""
    if key not in _expected:
        tot, lay = [0] * nl, [None] * nl
        for img, k in zip(distinct, times):
            r, p, d, one = P.restart_share([img], nf, 1.2, nl)
            tot = [t + k * int(x) for t, x in zip(tot, r)]
            lay = [a or b for a, b in zip(lay, one)]
        _expected[key] = (tot, lay)
    return _expected[key]


def _extract(capfd, imgs, nf, nl, max_wh=None, ex=None, **force):
    """one extraction under the pins -> (extractor, key order reported, restarts per level reported, stderr)"""
    from orb_ygz_slam_amd import Extractor
    h, w = imgs.shape[1:]
    if ex is None:
        with _env(**force):
            ex = Extractor(nf, 1.2, nl, 20, 7, max_width=(max_wh or (w, h))[0], max_height=(max_wh or (w, h))[1], max_batch=max(len(imgs), 5))
    capfd.readouterr()
    ex.extract_batch_host(imgs)
    err = capfd.readouterr().err
    lines = _ORDER.findall(err)
    if not lines:
        return ex, None, None, err
    assert len(lines) == 1, "the key-order line is printed once per extraction"
    order, frames, counts = lines[0]
    assert int(frames) == len(imgs)
    return ex, order, [int(x) for x in counts.split()][:nl], err


def _check_both_orders(oracle, capfd, img, nf, nl, key):
    imgs, times = _frames(img)
    want, lay = _expected_restarts(key, imgs[:3], times, nf, nl)
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    res = {}
    for sort in ("prefix", "full"):
        ex, order, got, err = _extract(capfd, imgs, nf, nl, oct_plan="sort", oct_sort=sort)
        assert order == sort and not _SMALL.search(err) and _SORT.search(err), "the sort plan under oct_sort=%s did not run" % sort
        print("%s oct_sort=%s: restarts per level %r (specification %r), key layout (D, keyBits, lowBit) %r" % (key, sort, got, want, lay))
        assert got == (want if sort == "prefix" else [0] * nl)
        for f in range(3):
            _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
        res[sort] = [ex.batch_fetch(f) for f in range(len(imgs))] + [[ex.batch_fetch_level_keypoints(f, l) for l in range(nl)] for f in range(len(imgs))]
        ex.close()
    n = len(imgs)
    for f in range(n):
        assert np.array_equal(res["prefix"][f][0], res["full"][f][0]) and np.array_equal(res["prefix"][f][1], res["full"][f][1])
        for l in range(nl):
            assert all(np.array_equal(a, b) for a, b in zip(res["prefix"][n + f][l], res["full"][n + f][l])), "list order differs at level %d" % l
    for f, g in ((0, 3), (1, 4)):   # the same image in two slots of the launch
        assert np.array_equal(res["prefix"][f][0], res["prefix"][g][0]) and np.array_equal(res["prefix"][f][1], res["prefix"][g][1])
    return want, lay


def test_no_restart_on_a_normal_small_frame(oracle, capfd):
    want, lay = _check_both_orders(oracle, capfd, synth_frame(44, 320, 240), 500, 4, "320x240/4/500")
    assert want == [0, 0, 0, 0]
    assert all(x[2] > 0 for x in lay), "every level's key is longer than the prefix"


def test_quota_above_the_corner_count(oracle, capfd):
    """320x240 / 4 levels / 3000 features: the tree divides until nothing divides.  Levels 0 and 1 of every frame end below the sorted prefix and
    start over; the candidates of levels 2 and 3 are all apart by depth 7, the last depth the prefix of their 18-bit keys orders, and must NOT
    start over (a restart the tree did not ask for would be a wasted attempt)."""
    want, lay = _check_both_orders(oracle, capfd, synth_frame(44, 320, 240), 3000, 4, "320x240/4/3000")
    assert want[0] == 5 and want[1] == 5, "every frame's levels 0 and 1 restart"


def test_two_spot_image_of_the_plan_tests(oracle, capfd):
    want, lay = _check_both_orders(oracle, capfd, _two_spots(7, 752, 480), 1000, 8, "752x480/8/1000 two spots")
    assert [x[1] for x in lay] == [21, 21, 21, 19, 19, 19, 19, 17]


def test_deep_trees_restart_on_some_levels(oracle, capfd):
    """752x480 / 8 / 1000 with trees that go down to cells of a pixel or two on the large levels only: restarts and first-attempt levels in one launch"""
    want, lay = _check_both_orders(oracle, capfd, _dots_and_spots(7, 752, 480), 1000, 8, "752x480/8/1000 dots and spots")
    assert any(want) and not all(want), want


@pytest.mark.parametrize("w,h,nl,nf,seed,roots", [(333, 517, 8, 1500, 42, 1), (1280, 360, 6, 1200, 43, 4)], ids=["tall_one_root", "wide_four_roots"])
def test_one_root_and_four_roots(oracle, capfd, w, h, nl, nf, seed, roots):
    want, lay = _check_both_orders(oracle, capfd, synth_frame(seed, w, h), nf, nl, "%dx%d" % (w, h))
    assert P.key_layout(16, w - 16, 16, h - 16)[0] == roots
    assert lay[0][2] == (6 if roots == 1 else 8), "lowBit = keyBits - 14 of level 0: root bits 0 / 2"


def test_deep_trees_with_one_and_four_roots(oracle, capfd):
    """the same two geometries with trees that do go below the prefix (an odd and an even number of key bits above it is not the point here: lowBit is
    even in both; the odd ones are the 752x480 levels above)"""
    for (w, h, nl, nf) in ((333, 517, 4, 1500), (1280, 360, 4, 1200)):
        want, lay = _check_both_orders(oracle, capfd, _dots_and_spots(9, w, h), nf, nl, "%dx%d dots and spots" % (w, h))
        assert any(want), (w, h, want)


def test_short_keys_take_the_unchanged_path(oracle, capfd):
    """100x100 / 3 levels: level 0's key has 16 bits, the two smaller levels' 14 -- the prefix is the whole key, nothing can restart there"""
    img = np.random.default_rng(11).integers(0, 256, (100, 100), dtype=np.uint8)
    want, lay = _check_both_orders(oracle, capfd, img, 300, 3, "100x100/3/300")
    assert lay[0][1] > 14 and all(x is not None and x[1] <= 14 and x[2] == 0 for x in lay[1:]), lay
    assert want[1:] == [0, 0]


@pytest.mark.parametrize("n", [1, 3, 17])
def test_batches_of_1_3_17_frames(oracle, capfd, n):
    """the library's own plan choice: one and three frames of eight levels are the small (histogram) plan's launch, seventeen the sort plan's grouped
    launches with the prefix sort"""
    w, h, nl, nf = 320, 240, 8, 1000
    base = [synth_frame(60 + k, w, h) for k in range(3)] + [_dots_and_spots(5, w, h, half=8, ndots=40)]
    imgs = np.stack([base[k % 4] for k in range(n)])
    ex, order, got, err = _extract(capfd, imgs, nf, nl)
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    if n * nl <= 128:
        assert _SMALL.search(err) and order is None
    else:
        assert order == "prefix" and _SORT.search(err) and not _SMALL.search(err)
        want, _ = _expected_restarts("batch17", base, (5, 4, 4, 4), nf, nl)
        print("17 frames: restarts per level %r (specification %r)" % (got, want))
        assert got == want
    for f in sorted({0, n // 2, n - 1, min(3, n - 1)}):
        _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
    ex.close()


def test_one_context_through_two_image_sizes(oracle, capfd):
    """the key tables belong to the geometry: 320x240, then 752x480, then 320x240 again on one context"""
    nf, nl = 1000, 8
    small, _ = _frames(synth_frame(61, 320, 240))
    large, times = _frames(_dots_and_spots(7, 752, 480))
    oex = oracle.Extractor(nf, 1.2, nl, 20, 7)
    ex = None
    for imgs, key in ((small, None), (large, "752x480/8/1000 dots and spots"), (small, None), (large, "752x480/8/1000 dots and spots")):
        ex, order, got, err = _extract(capfd, imgs, nf, nl, max_wh=(752, 480), ex=ex, oct_plan="sort", oct_sort="prefix")
        assert order == "prefix"
        if key:
            assert got == _expected_restarts(key, imgs[:3], times, nf, nl)[0]
        for f in (0, 2):
            _cmp_frame(oracle, ex, oex, imgs[f], frame=f)
    ex.close()
