"""GPU tier of the constructed direct-projection and frustum cases (tests/direct_cases.py; tests/test_direct_cases.py holds the oracle to a numpy
restatement and to the reference's own code on every one of them and proves that each case is the edge it claims).

k_direct_projection through Extractor.find_direct_projection_batch: one context per configuration with its image cache reserved once; the
configuration's cases run one after another on it -- a one-candidate batch first, then a nine, a one and an eight, so that the buffers grow and a
small batch follows a large one -- and then every case runs a second time.  Both passes equal the oracle: patches, search level and success flag
equal, pixels bit-identical where the oracle's are not NaN and NaN where they are; the run without want_patches agrees with the run with them.
k_frustum through Extractor.is_in_frustum_batch: in_view equal everywhere and the five outputs bit-identical where the point is in view (the
outputs of the other points are unspecified), every case twice on one context with other cases in between.  The fused case goes through
Extractor.search_local_points with projections exactly on maxX and maxY.  No comparison carries a tolerance."""
import numpy as np
import pytest

from tests import direct_cases as DC

pytestmark = pytest.mark.gpu

CASES = DC.direct_cases()
DIRECT_CFGS = ("L8", "P4", "L2", "L1")
FRUSTUM_CFGS = ("L8", "L12", "P4", "L1")


def _extractor(cfg):
    from orb_ygz_slam_amd import Extractor
    sf, nl, w, h = DC.CONFIGS[cfg]
    return Extractor(1000, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=1)


def _ordered(cases):
    """a one-candidate batch first, then n = 9, 1, 8 next to each other, then the rest in the order of the list"""
    by = {c.name: c for c in cases}
    head = [by[n] for n in ("n_1", "n_9", "n_1", "n_8") if n in by]
    return head + [c for c in cases if c.name not in ("n_1", "n_9", "n_8")]


def _same_without_patches(a, b):
    return DC.same_direct(a[:3], b[:3]) and DC.same_direct(b[:3], a[:3])


@pytest.mark.parametrize("cfg", DIRECT_CFGS)
def test_direct_device_equals_oracle_on_two_passes(oracle, cfg):
    mine = _ordered([c for c in CASES if c.cfg == cfg])
    assert mine
    _, _, w, h = DC.CONFIGS[cfg]
    expected = {repr(c): DC.run_oracle(oracle, c) for c in mine}
    ex = _extractor(cfg)
    try:
        ex.image_cache_reserve(max(len(c.images) for c in mine), w, h)
        for run in (1, 2):
            for c in mine:
                e = expected[repr(c)]
                g = DC.run_device(ex, c, want_patches=True)
                assert len(g) == 4 and DC.same_direct(g, e) and DC.same_direct(e, g), (run, c, DC.moved_labels(c, g, e))
                bare = DC.run_device(ex, c, want_patches=False)
                assert len(bare) == 3 and _same_without_patches(bare, g), (run, c)
                groups = {}
                for label, want in c.expect.items():          # (and where the case names the outcome, the device says so)
                    i = c.labels[label]
                    if "sl" in want:
                        assert g[1][i] == want["sl"], (c, label)
                    if "ok" in want:
                        assert g[2][i] == want["ok"], (c, label)
                    if want.get("px") == "nan":
                        assert np.isnan(g[0][i]).all(), (c, label)
                    if want.get("px") == "unchanged":
                        assert np.array_equal(g[0][i].view(np.uint32), c.px0[i].view(np.uint32)), (c, label)
                    if "same" in want:
                        groups.setdefault(want["same"], []).append(i)
                for idx in groups.values():                   # a candidate's answer does not depend on its neighbours in the workgroup
                    for i in idx[1:]:
                        assert DC.same_direct(tuple(x[i:i + 1] for x in g), tuple(x[idx[0]:idx[0] + 1] for x in g)), (c, i)
    finally:
        ex.close()


@pytest.mark.parametrize("cfg", FRUSTUM_CFGS)
def test_frustum_device_equals_oracle_twice(oracle, cfg):
    cases = DC.frustum_cases(oracle)
    mine = [c for c in cases if c.cfg == cfg]
    other = next(c for c in cases if c.name == "n_257")        # runs in between where a configuration has one case only; its answer is not read
    assert mine
    ex = _extractor(cfg)
    try:
        for run in (1, 2):
            for c in mine:
                e = DC.run_frustum_oracle(oracle, c)
                g = DC.run_frustum_device(ex, c)
                assert DC.same_frustum(g, e) and DC.same_frustum(e, g), (run, c, DC.moved_frustum_labels(c, g, e))
                for label, want in c.expect.items():
                    if "in_view" in want:
                        assert g[0][c.labels[label]] == want["in_view"], (c, label)
                    if "level" in want:
                        assert g[4][c.labels[label]] == want["level"], (c, label)
                if len(mine) == 1:
                    DC.run_frustum_device(ex, other)
    finally:
        ex.close()


def test_fused_search_local_points_on_the_image_edges(oracle):
    from orb_ygz_slam_amd import make_camera
    f = DC.fused_case()
    c = f["case"]
    w, h = c.frame
    iv, px, py, pxr, lv, vc = DC.run_frustum_oracle(oracle, c)
    e_n, e_m, e_o = oracle.search_by_projection_mappoints(f["keys"], f["desc"], c.scale, w, h, c.cam, iv, px, py, vc, lv, f["mp_desc"], f["th"], False, 0.8)
    assert e_n == 4
    cam = make_camera(w, h, fx=c.cam["fx"], fy=c.cam["fy"], cx=c.cam["cx"], cy=c.cam["cy"])
    ex = _extractor("L8")
    try:
        for run in (1, 2):
            g_n, g_m, g_o, g_iv = ex.search_local_points(cam, f["keys"], f["desc"], *DC.frustum_args(c)[:9], f["mp_desc"], f["th"], False, 0.8, c.limit,
                                                         scale_factors=c.scale)
            assert (g_iv == iv).all(), run
            assert g_n == e_n and (g_m == e_m).all() and (g_o == e_o).all(), (run, g_m, e_m)
    finally:
        ex.close()
