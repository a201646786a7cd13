"""The dynamic LDS of k_match_last, k_octree, the FAST cell loop, the grid kernels and k_sia_run is stated once, in
orb_ygz_slam_amd/csrc/lds_layout.h: the kernels carve with it and the host sizes its launches with it.  tests/cpp/lds_layout_cpu.hip walks every
layout over a sweep on the CPU, built here with AddressSanitizer and UBSan (a stand-alone host program, a fresh process): alignment of every
array, no overlap among arrays that are live together, every declared overlay against the phase it is idle in, every array inside the byte
count of the launch -- the program exits non-zero otherwise.  Its byte counts are compared with tests/golden/lds_layout_parent.json, the same
table recorded from the functions this header replaced (match_lds_bytes, octree_lds_bytes, octree_lds_cand, octree_hist_lds_bytes,
fast_quads_lds_bytes, fast_tab_lds_bytes at 1, 2 and 4 waves, fia_lds_bytes, sia_lds_bytes, sia_jac_in_lds, sia_stage_bytes at the commit
before it): every number must be equal."""
import pytest

from tests import lds_layout_prog


@pytest.fixture(scope="module")
def tab():
    return lds_layout_prog.table(sanitize=True)   # (every check of the walk has passed when this returns)


@pytest.fixture(scope="module")
def gold():
    return lds_layout_prog.golden()


def test_matcher_bytes_and_spill_bytes_are_the_parents(tab, gold):
    assert len(gold["matcher"]) == 13 * 2 * 4
    assert tab["matcher"] == gold["matcher"]


def test_octree_bytes_of_every_launch_of_the_sweep_are_the_parents(tab, gold):
    assert len(gold["octree"]) == 13 + 75 and all(gold["octree"].values())
    assert tab["octree"] == gold["octree"]
    assert tab["octree_cand"] == gold["octree_cand"] and gold["octree_cand"]


def test_fast_bytes_at_one_two_and_four_waves_are_the_parents(tab, gold):
    assert len(gold["fast"]) == 13 + 75
    assert tab["fast"] == gold["fast"]
    for pitch, win_rows, smap_rows, quad_cap, quads, tab1, tab2, tab4 in gold["fast"].values():
        assert (tab2 - 64) == 2 * (tab1 - 64) and (tab4 - 64) == 4 * (tab1 - 64)      # a wave's region times the waves of the kernel that is launched


def test_grid_bytes_and_the_keypoint_limit_are_the_parents(tab, gold):
    assert tab["grid"] == gold["grid"] and tab["grid_max_n"] == gold["grid_max_n"]
    assert [n for n, _ in gold["grid"]] == [0, 1, 1000, 30000, gold["grid_max_n"], gold["grid_max_n"] + 1]


def test_aligner_records_are_the_parents(tab, gold):
    assert len(gold["aligner"]["rows"]) == 2 * 10
    assert tab["aligner"] == gold["aligner"]


def test_matcher_plan_switches_lie_where_the_budget_puts_them(tab):
    """what tests/test_gpu_match.py runs: the last keypoint count each plan admits (both frames equal)"""
    sw = {(deep, k): c for deep, k, c in tab["matcher_switch"]}
    assert set(sw) == {(d, k) for d in (0, 1) for k in (0, 1, 2)}
    for deep in (0, 1):
        assert 0 < sw[deep, 0] < sw[deep, 1] < sw[deep, 2] < 65535
