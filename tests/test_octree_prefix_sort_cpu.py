"""k_octree's sort plan orders a level's path keys on their top 14 bits first and starts the level over with the full sort when a tree pass would
read a digit below them (csrc/extract_kernels.hip: oct_order, oct_bounds); it orders the level's keypoints for k_describe by a compact tile
key.  Checked here on tools/octree_proto.py, the executable specification, without a device:

  - the tree over keys ordered stably on the top 14 bits equals the tree over fully sorted keys whenever no consulted digit lies below lowBit,
  - the overflow predicate fires exactly in the other cases (and the restarting form then returns the full sort's result),
  - the compact tile key orders every (kx, ky) of a level as the 12-bit key does, with the bits the kernel hands its radix sort."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import octree_proto as P  # noqa: E402


def _unique_points(rng, n, W, H, xs=None, ys=None):
    """n distinct integer positions of a W x H region (FAST candidates are distinct pixels), from the given coordinates or uniform ones"""
    if xs is None:
        xs, ys = rng.integers(0, W, 4 * n), rng.integers(0, H, 4 * n)
    xy = np.unique(np.stack([np.clip(xs, 0, W - 1), np.clip(ys, 0, H - 1)], 1), axis=0)
    xy = xy[rng.permutation(len(xy))[:n]]
    return xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32), rng.integers(7, 200, len(xy)).astype(np.int32)


def _clustered(rng, n, W, H):
    """two tight spots over a thin uniform background: the background keeps the list growing through the full passes (spots alone end the tree at
    once: a node whose points all fall into one child does not grow the list, :696), then the expand phase takes the biggest nodes -- the spots --
    first, again and again, far below the sorted prefix"""
    c = np.array([[W // 5, H // 4], [W - 30, H - 25]])[rng.integers(0, 2, 4 * n)]
    sx, sy = c[:, 0] + rng.integers(-6, 7, 4 * n), c[:, 1] + rng.integers(-6, 7, 4 * n)
    bg = rng.random(4 * n) < 0.3
    return _unique_points(rng, n, W, H, np.where(bg, rng.integers(0, W, 4 * n), sx), np.where(bg, rng.integers(0, H, 4 * n), sy))


# (name, region W x H, candidates, N wanted, generator): W / H decides the roots -- 720 x 448 two, 301 x 485 one (tall), 1248 x 328 four (wide)
SETS = [
    ("random", 720, 448, 2500, 220, _unique_points),
    ("random_few_wanted", 720, 448, 2500, 40, _unique_points),
    ("clustered", 720, 448, 300, 220, _clustered),
    ("tall_one_root", 301, 485, 1500, 300, _unique_points),
    ("tall_clustered", 301, 485, 300, 250, _clustered),
    ("wide_four_roots", 1248, 328, 2000, 250, _unique_points),
    ("wide_clustered", 1248, 328, 300, 250, _clustered),
    ("quota_above_corners", 288, 208, 400, 3000, _unique_points),
    ("short_key", 60, 50, 200, 60, _unique_points),           # one root of at most 64 px: D = 7, keyBits = 14: the prefix IS the key
]


@pytest.mark.parametrize("case", SETS, ids=[s[0] for s in SETS])
@pytest.mark.parametrize("seed", [0, 1])
def test_prefix_sorted_tree_is_the_full_tree_or_overflows(case, seed):
    name, W, H, n, N, gen = case
    xs, ys, sc = gen(np.random.default_rng(seed), n, W, H)
    full, pre, both = {}, {}, {}
    a = P.distribute(xs, ys, sc, 16, 16 + W, 16, 16 + H, N, info=full)
    b = P.distribute(xs, ys, sc, 16, 16 + W, 16, 16 + H, N, prefix_bits=P.PREFIX_BITS, info=pre)
    c = P.distribute_restarting(xs, ys, sc, 16, 16 + W, 16, 16 + H, N, info=both)
    assert full["lowBit"] == 0 and not full["overflow"]
    assert pre["lowBit"] == P.low_bit(full["keyBits"]) == max(0, full["keyBits"] - 14)
    # the predicate: the deepest digit the full tree consults, at shift 2 * (D - (dep + 1)), lies below the sorted bits
    below = 2 * (full["D"] - full["deepest"]) < pre["lowBit"]
    print("%s seed %d: D %d keyBits %d lowBit %d deepest dep + 1 %d -> %s" % (name, seed, full["D"], full["keyBits"], pre["lowBit"], full["deepest"],
                                                                             "restart" if below else "prefix is enough"))
    assert pre["overflow"] == below
    assert both["restarted"] == below
    if not below:
        assert pre["nodes"] == full["nodes"], "the node ranges differ"
        assert np.array_equal(a, b)
    assert np.array_equal(a, c), "the restarting form must always give the full sort's result"
    if name == "short_key":
        assert pre["lowBit"] == 0 and not below
    if name == "quota_above_corners" or name.endswith("clustered"):
        assert below, "this set is meant to drive the tree below the sorted prefix"
    if name in ("random", "random_few_wanted"):
        assert not below, "a normal level stops well above lowBit"


def test_both_parities_of_low_bit_are_covered():
    """lowBit = root bits + 2 D - 14 is odd or even with the root bits while a digit's shift is always even: an odd lowBit cuts a digit in two, and
    `shift < lowBit` has to refuse that digit.  The sets above have to contain both parities."""
    par = set()
    for name, W, H, n, N, gen in SETS:
        keyBits = P.key_layout(16, 16 + W, 16, 16 + H)[3]
        if keyBits > 14:
            par.add((keyBits - 14) & 1)
    assert par == {0, 1}


def _level_sizes(w, h, nlevels=8, sf=1.2):
    out, scale = [], np.float32(1.0)
    for l in range(nlevels):
        if l:
            scale = np.float32(scale * np.float32(sf))
        inv = np.float32(1.0) / scale
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


@pytest.mark.parametrize("wh", [(752, 480), (640, 480), (1920, 1080)])
def test_compact_tile_key_orders_as_the_12_bit_key(wh):
    for (w, h) in _level_sizes(*wh):
        ky, kx = np.mgrid[0:h, 0:w]
        old, new = P.tile_keys(kx.ravel(), ky.ravel(), w)
        bits = P.tile_key_bits(w, h)
        assert int(new.max()) < (1 << bits) and (bits == 0 or int(new.max()) >= (1 << (bits - 1))), "the radix sort gets exactly the bits the largest key needs"
        assert bits <= 12
        # the same order: a stable sort by either key is the same permutation (equal old <=> equal new, and old < old' <=> new < new')
        assert np.array_equal(np.argsort(old, kind="stable"), np.argsort(new, kind="stable"))
        uo, io = np.unique(old, return_index=True)
        assert np.all(np.diff(new[io]) > 0) and len(np.unique(new)) == len(uo)
    if wh != (1920, 1080):
        assert all(P.tile_key_bits(w, h) <= 7 for (w, h) in _level_sizes(*wh)), "one radix pass for every level of this geometry"
