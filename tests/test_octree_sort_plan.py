"""The launches of the octree's sort plan (csrc/ygzf_api.hip, plan_oct_sort) are host arithmetic: checked here without a device.  Every level is in
exactly one launch, in order; a launch's workgroup size follows its largest list; its LDS holds the list capacity of every level it carries and a
candidate budget at 16 bytes per candidate, the second sort buffer over the cell table and the node arrays (k_octree)."""
import pytest

from orb_ygz_slam_amd.capi import octree_sort_plan_host
from tests import lds_layout_prog

SORTED = [(1000, 1.2, 8, 752, 480), (1000, 1.2, 8, 640, 480), (1500, 1.2, 8, 333, 517), (1200, 1.2, 6, 1280, 360), (500, 1.2, 8, 1241, 376),
          (2000, 1.2, 8, 1024, 768), (300, 1.3, 5, 320, 240), (1000, 1.2, 12, 752, 480), (150, 1.2, 3, 200, 150)]


@pytest.mark.parametrize("nf,sf,nl,w,h", SORTED)
def test_groups_cover_the_levels_and_fit_the_cu(nf, sf, nl, w, h):
    plan = octree_sort_plan_host(nf, sf, nl, w, h)
    assert plan, "this geometry takes the sort plan"
    nxt = 0
    for g in plan:
        assert g["l0"] == nxt and g["n"] >= 1
        nxt += g["n"]
        assert g["block"] in (256, 512, 1024)
        assert g["block"] == (1024 if g["cap"] > 256 else 512 if g["cap"] > 128 else 256)
        assert g["cap"] % 4 == 0 and g["lds_cand"] % 4 == 0 and g["lds_cand"] >= 256
        budget = {1024: 71, 512: 44, 256: 36}[g["block"]] * 1024
        assert g["lds_bytes"] <= budget
        # no less than the layout takes for this list capacity and candidate budget when the launch's levels have no cells (csrc/lds_layout.h)
        assert g["lds_bytes"] >= lds_layout_prog.oct_sort_bytes(0, g["cap"], g["lds_cand"])
    assert nxt == nl
    caps = [g["cap"] for g in plan]
    assert caps == sorted(caps, reverse=True)


def test_the_bench_geometry():
    """752x480 / 8 / 1000: levels 0-3 in 512 threads and 44 KB, 4-7 in 256 threads and 36 KB -- room for the ~2700 candidates the largest levels hold"""
    plan = octree_sort_plan_host(1000, 1.2, 8, 752, 480)
    assert [(g["l0"], g["n"], g["block"]) for g in plan] == [(0, 4, 512), (4, 4, 256)]
    assert [g["lds_bytes"] for g in plan] == [44 * 1024, 36 * 1024]
    assert [g["lds_cand"] for g in plan] == [2816, 2304]


@pytest.mark.parametrize("nf,sf,nl,w,h", [(4000, 1.2, 8, 1920, 1080), (8000, 1.2, 8, 3840, 2160), (3000, 1.2, 4, 320, 240)])
def test_large_budgets_take_the_histogram_plan(nf, sf, nl, w, h):
    assert octree_sort_plan_host(nf, sf, nl, w, h) == []
