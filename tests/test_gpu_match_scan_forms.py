"""The two forms of k_match_last's speculative scan in launches with one workgroup per pair (YGZF_FORCE=match_scan=filtered|predicated,
match_split=1): `predicated` reads the descriptor of every keypoint of a query's cell window, `filtered` walks each lane over the
cheap filters (level, box, owner, uRight), queues the keypoints that pass and reads only their descriptors, a wave at a time.  Both must
give the oracle's matches, owners and counts, and each other's, element for element.

The inputs are built with tests/matcher_cases.py (frame 512 x 384, grid cells of 8 x 8 px: column c holds x in [8c - 4, 8c + 4)):
  rejections    windows whose keypoints are all rejected by level / by the box alone / by ownership alone, and one where the only keypoint
                that passes is the last one visited
  tie_order     equal distances in one window, separated in the visiting order by rejected keypoints (which still advance `ord`), with
                the index order reversed against the visiting order
  uneven        grid columns of 0, 1, 7, 40 and 3 entries in one window (lanes run out at different steps), and a window of > 256 keypoints
  random_*      4 queries (64 lanes each), 100 queries, 1000 keypoints against 1000 (one lane per query), owners, levels and uRight mixed
run as SearchByProjection(Cur, Last) (mode 0) and SearchByProjection(F, MapPoints) (mode 1: runner-up kept beyond maxDist, lists of eight),
with and without check_level, with uRight present, with match_lanes=fixed, and once through the one-wave in-order pass (match_serial=1)."""
import numpy as np
import pytest

from tests import matcher_cases as MC

pytestmark = pytest.mark.gpu

FORMS = ("filtered", "predicated")


def _rejections(rng):
    s = MC.Scene()
    Q = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(4)]
    # A: query on level 4 (radius 6 * 1.2^4 = 12.4), identical descriptors within 3 px of it, all on level 0 or 7
    for k in range(9):
        s.cand((80.0 + (k % 3) - 1, 80.0 + (k // 3) - 1), Q[0], 0 if k & 1 else 7)
    s.query((80.0, 80.0), Q[0], 4)
    # B: level-0 query at u = 200, box (194, 206), window columns 24..26 = x in [188, 212): keypoints in the window, outside the box
    for k, x in enumerate((189.0, 190.5, 192.0, 193.75, 206.0, 207.5, 209.0, 211.0)):
        s.cand((x, 80.0 + (k % 3)), Q[1])
    for k, y in enumerate((68.5, 70.0, 73.75, 86.0, 88.0, 91.5)):
        s.cand((200.0 + (k % 3), y), Q[1])
    s.query((200.0, 80.0), Q[1])
    # C: in the box, same level, owned by a MapPoint with observations
    for k in range(6):
        s.cand((320.0 + (k % 3) - 1, 80.0 + (k // 3)), Q[2], owner=2)
    s.query((320.0, 80.0), Q[2])
    # D: window columns 9..11, rows 24..26; rejected for all three reasons, then the one that passes in the last cell, highest index
    for k in range(12):
        s.cand((70.0 + k, 196.0 + k), Q[3], 5)                                     # level
    for k in range(6):
        s.cand((68.5 + 0.25 * k, 200.0), Q[3])                                     # left of the box
        s.cand((80.0, 206.0 + 0.25 * k), Q[3])                                     # below the box (|dy| >= 6)
        s.cand((78.0 + k, 198.0 + k), Q[3], owner=2)                               # owner
    last = s.cand((85.75, 205.75), MC.flip(Q[3], range(30)))                       # cell (11, 26)
    s.query((80.0, 200.0), Q[3])

    def check(res):
        m = np.asarray(res[1])
        assert res[0] == 1 and m[last] == 3 and (np.delete(m, last) < 0).all()
    return s, 6.0, check


def _tie_order(rng):
    s = MC.Scene()
    Q = rng.integers(0, 256, 32, dtype=np.uint8)
    T = MC.flip(Q, rng.permutation(256)[:10])
    # level-3 queries at (100, 100): radius 10.37, box (89.63, 110.37), window columns 11..14 (x in [84, 116)), rows likewise.  Six tied
    # keypoints in cells (11, 12) (12, 12) (12, 13) (13, 12) (13, 13) (14, 12), entered in the REVERSE of that visiting order, levels
    # alternating 2 / 3 (the MapPoint search's ratio test compares equals of one level only)
    tied_xy = [(90.5, 100.0), (94.0, 93.0), (97.0, 106.0), (102.0, 98.0), (105.0, 101.0), (109.0, 100.0)]
    tied = [None] * 6
    for k in range(5, -1, -1):
        tied[k] = s.cand(tied_xy[k], T, 2 + (k & 1))
        # ... and all over the window keypoints that are closer but rejected: by level, by the box, by ownership
        for j in range(4):
            s.cand((86.0 + 7.0 * j + 0.5 * k, 88.0 + 4.0 * k), Q, 6)
            s.cand((84.5 + 0.25 * k + j, 90.0 + 3.0 * k), Q, 3)
            s.cand((92.0 + 5.0 * j, 91.0 + 3.0 * k), Q, 3, owner=2)
    for i in range(6):
        s.query((100.0, 100.0), Q, 3)

    def check(res):
        m = np.asarray(res[1])
        assert res[0] == 6 and [int(m[t]) for t in tied] == [0, 1, 2, 3, 4, 5]      # blocking queries take the equals in visiting order
    return s, 6.0, check


def _fillers(s, rng, n):
    """n more queries, each with a keypoint of its own, away from the constructed windows: they set how many lanes a query gets"""
    pts = [p for p in MC.lattice(16) if p[1] < 150 or p[0] > 330]
    for k in range(n):
        Qk = rng.integers(0, 256, 32, dtype=np.uint8)
        s.cand(pts[k], MC.flip(Qk, rng.permutation(256)[:k % 50]), k % 3)
        s.query(pts[k], Qk, k % 3, obs=k & 1)


def _uneven(rng, fill):
    s = MC.Scene()
    Q = rng.integers(0, 256, 32, dtype=np.uint8)

    def some(xy, q, level):     # one in three passes the filters (its distance may still be beyond TH_HIGH); the others: owned, or on a far level
        kind = int(rng.integers(0, 3))
        s.cand(xy, MC.flip(q, rng.permutation(256)[:int(rng.integers(0, 130))]), level if kind < 2 else (level + 4) % 8, owner=2 if kind == 1 else 0)
    # level-3 queries at (200, 250): radius 10.4, window columns 23..27 (x in [180, 220)), rows 29..33 (y in [228, 268)): 0, 1, 7, 40, 3 entries
    for col, n in ((24, 1), (25, 7), (26, 40), (27, 3)):
        for k in range(n):
            some((8.0 * col - 4 + float(rng.integers(0, 32)) / 4, 228.0 + float(rng.integers(0, 160)) / 4), Q, 3)
    for i in range(5):
        s.query((200.0, 250.0), Q, 3)
    # level-7 queries at (100, 300): radius 21.5, window columns 9..16, rows 34..41: 300 keypoints
    Q2 = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in range(300):
        some((68.0 + float(rng.integers(0, 256)) / 4, 268.0 + float(rng.integers(0, 256)) / 4), Q2, 7)
    for i in range(5):
        s.query((100.0, 300.0), Q2, 7)
    _fillers(s, rng, fill)

    def check(res):
        k = s.arrays()["cur_keys"]
        px, py = MC._cell(k["x"]), MC._cell(k["y"])
        assert [int(((px == c) & (py >= 29) & (py <= 33)).sum()) for c in (23, 24, 25, 26, 27)] == [0, 1, 7, 40, 3]
        assert int(((px >= 9) & (px <= 16) & (py >= 34) & (py <= 41)).sum()) > 256
        assert res[0] >= fill + 2      # every filler finds its own keypoint; each of the two windows holds acceptable ones
    return s, 6.0, check


def _random(rng, nq, nc):
    s = MC.Scene()
    xy = np.stack([rng.integers(20 * 4, 492 * 4, nc) / 4.0, rng.integers(20 * 4, 364 * 4, nc) / 4.0], -1)
    octs = rng.integers(0, 8, nc)
    descs = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    for j in range(nc):
        own = int(rng.integers(0, 20))
        ur = -1.0 if rng.integers(0, 2) else float(xy[j, 0]) - 32.0 + float(rng.integers(-80, 81)) / 4
        s.cand(tuple(xy[j]), descs[j], int(octs[j]), owner=2 if own < 2 else 1 if own == 2 else 0, u_right=ur)
    for i in np.argsort(octs[np.arange(nq) % nc], kind="stable"):      # queries by level, as an extractor's keypoints come
        j = int(i) % nc
        s.query((float(xy[j, 0]) + float(rng.integers(-8, 9)) / 4, float(xy[j, 1]) + float(rng.integers(-8, 9)) / 4),
                MC.flip(descs[j], rng.permutation(256)[:int(rng.integers(0, 70))]), min(max(int(octs[j]) + int(rng.integers(-1, 2)), 0), 7),
                obs=int(rng.integers(0, 2)))

    def check(res):
        assert res[0] >= nq // 8
    return s, 15.0, check


SCENES = {"rejections": _rejections, "tie_order": _tie_order, "uneven": lambda r: _uneven(r, 0), "uneven_100q": lambda r: _uneven(r, 90),
          "random_4q": lambda r: _random(r, 4, 300), "random_100q": lambda r: _random(r, 100, 400), "random_1000": lambda r: _random(r, 1000, 1000)}
# how a scene is posed: (tag, matcher_cases function, projected_case arguments)
POSES = [("last", "last", dict(check_level=True)), ("last_anylevel", "last", dict(check_level=False)),
         ("last_uright", "last", dict(check_level=True, mono=False, mb=0.125, mbf=32.0, stereo=True)),
         ("mappoints", "mappoints", dict(check_level=True)), ("mappoints_anylevel", "mappoints", dict(check_level=False)),
         ("mappoints_uright", "mappoints", dict(check_level=True, mb=0.125, mbf=32.0, stereo=True))]
_built = {}


def _case(scene, pose):
    """-> (Case, check of the constructed property or None), built once; the oracle's answer is cached beside it by _expected"""
    if (scene, pose) not in _built:
        if scene not in _built:
            _built[scene] = SCENES[scene](np.random.default_rng(20250 + sorted(SCENES).index(scene)))
        s, radius, check = _built[scene]
        tag, fn, kw = next(p for p in POSES if p[0] == pose)
        c = MC.projected_case("%s_%s" % (scene, tag), 0, fn, s, radius, None, **kw)
        _built[(scene, pose)] = [c, check if pose == "last" else None, None]
    return _built[(scene, pose)]


def _expected(oracle, scene, pose):
    rec = _case(scene, pose)
    if rec[2] is None:
        rec[2] = MC.run_oracle(oracle, rec[0])
    return rec[2]


@pytest.fixture(scope="module")
def ctx():
    """(form, extra plan) -> context with match_split=1 (YGZF_FORCE is read when a context is created), closed when the file is done"""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    made = {}

    def get(form, extra=None):
        if (form, extra) not in made:
            kv = dict(match_split=1, match_scan=form, match_lanes=None, match_serial=None)
            if extra:
                kv.update([extra.split("=")])
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("YGZF_FORCE", force_env(**kv))
                made[(form, extra)] = Extractor(1000, 1.2, 8, 20, 7, max_width=MC.W, max_height=MC.H, max_batch=1)
        return made[(form, extra)]
    yield get
    for ex in made.values():
        ex.close()


def _both_forms(oracle, ctx, scene, pose, extra=None):
    case, check, _ = _case(scene, pose)
    exp = _expected(oracle, scene, pose)
    if check:
        check(exp)
    got = {form: MC.run_device(ctx(form, extra), case, exp) for form in FORMS}
    for form in FORMS:
        assert MC.same(got[form], exp, case) is None, (form, MC.same(got[form], exp, case))
    f, p = got["filtered"], got["predicated"]
    assert len(f) == len(p)
    for a, b in zip(f, p):
        assert np.array_equal(np.asarray(a), np.asarray(b))


RUNS = [(s, p[0]) for s in SCENES for p in POSES]


@pytest.mark.parametrize("scene,pose", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_forms_equal_oracle_and_each_other(oracle, ctx, scene, pose):
    _both_forms(oracle, ctx, scene, pose)


FIXED = [(s, p) for s in ("tie_order", "uneven_100q", "random_1000") for p in ("last", "mappoints_uright")]


@pytest.mark.parametrize("scene,pose", FIXED, ids=["%s-%s" % r for r in FIXED])
def test_forms_with_fixed_lanes(oracle, ctx, scene, pose):
    """match_lanes=fixed: with one workgroup per pair, one lane per query whatever its level"""
    _both_forms(oracle, ctx, scene, pose, "match_lanes=fixed")


def test_forms_feed_the_in_order_pass(oracle, ctx):
    """match_serial=1: the one-wave in-order pass reads the same speculative lists"""
    _both_forms(oracle, ctx, "uneven_100q", "last", "match_serial=1")
    _both_forms(oracle, ctx, "random_1000", "mappoints", "match_serial=1")
