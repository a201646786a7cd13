"""CPU tier of the undistortion (cv::remap, src/Frame.cc:775-805): the constructed cases of tests/remap_cases.py reach what they claim, every wrong
form of the restatement moves exactly the cases that list it, and the host plan (ygzf_remap_plan_host: tiles, boxes, classes, packed records)
agrees with the taps of every case.  No case is excluded from any comparison."""
import numpy as np
import pytest

from tests import remap_cases as R

NAMES = [c.name for c in R.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_claims(name):
    c = R.case_by_name(name)
    assert c.src.shape[1] <= 96 and c.src.shape[0] <= 64 or name.endswith("752x480")
    assert c.reach(c, R.expected(c))


@pytest.mark.parametrize("form", R.WRONG_FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(form):
    moved = [c.name for c in R.CASES if not np.array_equal(R.remap_ref(c.src, c.map_xy, c.map_tab, form), R.expected(c))]
    listed = [c.name for c in R.CASES if form in c.moved_by]
    assert moved == listed
    if form == "tab0_32767":
        # the saturated table entry gives the same byte with or without OpenCV's correction: the formula holds at tab = 0
        assert not listed and any((c.map_tab == 0).any() for c in R.CASES)
    else:
        assert listed, "no case would notice this form"


def test_shift_identity_over_every_sum():
    """(32 S + 2^14) >> 15 == (S + 512) >> 10 for every possible sum S = sum b_j a_k p_jk (0 .. 32 * 32 * 255)"""
    S = np.arange(32 * 32 * 255 + 1, dtype=np.int64)
    assert np.array_equal((32 * S + (1 << 14)) >> 15, (S + 512) >> 10)
    p = np.arange(256, dtype=np.int64)
    assert np.array_equal((32767 * p[:, None] + p[None, :] + (1 << 14)) >> 15, np.broadcast_to(p[:, None], (256, 256)))


# ---- the host plan -------------------------------------------------------------------------------------------------------------------------------
def _plan(c):
    from orb_ygz_slam_amd.capi import remap_plan_host
    return remap_plan_host(c.src.shape[1], c.src.shape[0], c.map_xy, c.map_tab)


def _tile_slices(P, shape):
    (tw, th), (nx, ny) = P["tile"], P["tiles"]
    h, w = shape
    assert nx == -(-w // tw) and ny == -(-h // th)
    for t in range(nx * ny):
        yield t, slice((t // nx) * th, min((t // nx + 1) * th, h)), slice((t % nx) * tw, min((t % nx + 1) * tw, w))


@pytest.mark.parametrize("name", NAMES)
def test_plan_boxes_classes_and_records(name):
    from orb_ygz_slam_amd.capi import REMAP_EMPTY, REMAP_GATHER, REMAP_INSIDE, REMAP_LDS
    c = R.case_by_name(name)
    P = _plan(c)
    inside = R.taps_inside(c)
    sx, sy = c.map_xy[..., 0].astype(np.int64), c.map_xy[..., 1].astype(np.int64)
    fx, fy = c.map_tab.astype(np.int64) & 31, c.map_tab.astype(np.int64) >> 5
    count = [0, 0, 0, 0]
    for t, ys, xs in _tile_slices(P, c.map_tab.shape):
        bx0, by0, bx1, by1 = (int(v) for v in P["boxes"][t])
        # the box is the bounding box of all the tile's taps, unclipped: every tap -- in the source or not -- lies inside it, and it is tight
        assert (bx0, by0, bx1, by1) == (sx[ys, xs].min(), sy[ys, xs].min(), sx[ys, xs].max() + 1, sy[ys, xs].max() + 1)
        x0, pitch, rows = (int(v) for v in P["staged"][t])
        fits = ((bx1 - (bx0 & ~3) + 1 + 3) & ~3) * (by1 - by0 + 1) <= P["lds_bytes"]
        ins = inside[ys, xs]
        want = REMAP_EMPTY if not ins.any() else REMAP_GATHER if not fits else REMAP_INSIDE if ins.all() else REMAP_LDS
        cls = int(P["classes"][t])
        assert cls == want
        count[cls] += 1
        rec = P["records"][ys, xs].astype(np.int64)
        assert np.array_equal(rec & 31, fx[ys, xs]) and np.array_equal((rec >> 5) & 31, fy[ys, xs])
        if cls in (REMAP_INSIDE, REMAP_LDS):
            assert x0 == (bx0 & ~3) and x0 % 4 == 0 and pitch % 4 == 0 and pitch >= bx1 - x0 + 1 and rows == by1 - by0 + 1 and pitch * rows <= P["lds_bytes"]
            off = rec >> 10
            assert np.array_equal(off, (sy[ys, xs] - by0) * pitch + (sx[ys, xs] - x0))
            assert off.min() >= 0 and off.max() + pitch + 1 < pitch * rows       # all four taps of every pixel inside the staged box
        else:
            assert pitch == 0 and rows == 0 and not (rec >> 10).any()
    assert count == P["count"]


def test_plan_classes_of_the_named_cases():
    from orb_ygz_slam_amd.capi import REMAP_EMPTY, REMAP_GATHER, REMAP_INSIDE, REMAP_LDS
    mixed = _plan(R.case_by_name("mixed_classes"))
    assert list(mixed["classes"]) == [REMAP_INSIDE, REMAP_LDS, REMAP_GATHER, REMAP_EMPTY]
    assert set(_plan(R.case_by_name("scatter"))["classes"]) == {REMAP_GATHER}
    # identity: the last column's and the last row's second taps lie one pixel outside (with weight 0): the tiles along those edges are LDS
    ident = _plan(R.case_by_name("identity"))
    nx, ny = ident["tiles"]
    edge = np.array([t % nx == nx - 1 or t // nx == ny - 1 for t in range(nx * ny)])
    assert np.array_equal(ident["classes"], np.where(edge, REMAP_LDS, REMAP_INSIDE))
    assert set(_plan(R.case_by_name("shift_x_plusall"))["classes"]) == {REMAP_EMPTY}
    tr = _plan(R.case_by_name("transpose"))
    assert set(tr["classes"]) == {REMAP_LDS} and (tr["staged"][:, 2] > 3 * tr["staged"][:, 1]).all()      # a tall box: 65 rows of 20 bytes
    assert REMAP_GATHER in _plan(R.case_by_name("extreme_coordinates"))["classes"]


def test_euroc_map_stages_every_tile():
    """a real calibration (752 x 480, k1 -0.283, k2 0.074): no tile needs the gather kernel, and the worst box takes less than half the budget"""
    from orb_ygz_slam_amd.capi import REMAP_GATHER
    P = _plan(R.case_by_name("euroc_752x480"))
    assert P["count"][REMAP_GATHER] == 0 and P["count"][3] == 0
    assert (P["staged"][:, 1] * P["staged"][:, 2]).max() <= P["lds_bytes"] // 2


def test_plan_refuses_what_the_table_does_not_hold():
    import ctypes as C
    from orb_ygz_slam_amd.capi import load_library
    L = load_library()
    c = R.case_by_name("identity")
    h, w = c.map_tab.shape
    xy, tab = np.ascontiguousarray(c.map_xy), np.ascontiguousarray(c.map_tab).copy()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (None, None, None, None, None)
    assert L.ygzf_remap_plan_host(96, 64, w, h, vp(xy), vp(tab), *args) == 0
    tab[h // 2, w // 2] = 1024
    assert L.ygzf_remap_plan_host(96, 64, w, h, vp(xy), vp(tab), *args) == -1
    tab[h // 2, w // 2] = 1023
    assert L.ygzf_remap_plan_host(96, 64, w, h, vp(xy), vp(tab), *args) == 0
    assert L.ygzf_remap_plan_host(96, 64, w, h, None, vp(tab), *args) == -1 and L.ygzf_remap_plan_host(96, 64, w, h, vp(xy), None, *args) == -1
    assert L.ygzf_remap_plan_host(0, 64, w, h, vp(xy), vp(tab), *args) == -1 and L.ygzf_remap_plan_host(96, 64, w, 0, vp(xy), vp(tab), *args) == -1
