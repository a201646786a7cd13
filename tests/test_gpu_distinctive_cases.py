"""GPU tier of the constructed ComputeDistinctiveDescriptors cases (tests/distinctive_cases.py; tests/test_distinctive_cases.py holds the
restatement to the oracle and to the reference's own compiled MapPoint.cc and proves that each case is the median index, tie, tail, hand-over or
batch layout it claims): k_distinctive and k_distinctive_large through Extractor.distinctive_descriptors_batch equal the restatement exactly on
every case and every seeded scene; the whole list runs twice on one context, largest batch first; one context alternates a large, an empty and
a one-point batch; bad offsets are refused and the context answers the next call; and, where oracle/_ref/boundary/libboundary_mappoint.so
travelled, the reference's own body, the product's per-point member and ygz::ComputeDistinctiveDescriptorsBatch agree on every case."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import distinctive_cases as DC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = DC.cases()
SCENES = DC.scenes()
RUNS = [(c.name, c.off, c.desc) for c in CASES] + SCENES
MAPPOINT_LIB = os.path.join(ROOT, "oracle", "_ref", "boundary", "libboundary_mappoint.so")


@pytest.fixture(scope="module")
def expected():
    """name -> the restatement's answer, computed once and left unchanged"""
    out = {name: DC.restate(off, desc) for name, off, desc in RUNS}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ctx():
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(max_width=64, max_height=64)
    yield ex
    ex.close()


@pytest.mark.parametrize("name,off,desc", RUNS, ids=[r[0] for r in RUNS])
def test_device_equals_restatement(ctx, expected, name, off, desc):
    g = ctx.distinctive_descriptors_batch(off, desc)
    assert np.array_equal(g, expected[name]), (name, np.nonzero(g != expected[name])[0][:8], g[:8], expected[name][:8])


def test_list_twice_on_one_context_largest_first(expected):
    """a fresh context meets its largest batch first (every later one fits the buffers that one sized) and then the list in its own order"""
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(max_width=64, max_height=64)
    by_size = sorted(RUNS, key=lambda r: -int(r[1][-1]))
    assert int(by_size[0][1][-1]) > int(by_size[-1][1][-1]) == 0
    for name, off, desc in by_size + RUNS:
        assert np.array_equal(ex.distinctive_descriptors_batch(off, desc), expected[name]), name
    ex.close()


def test_large_empty_and_one_point_batches_alternate(expected):
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(max_width=64, max_height=64)
    by = {c.name: c for c in CASES}
    large, single = by["batch_interleaved"], by["tie_700_rows_100_613"]
    one = (np.array([0, 5], np.int32), DC.thermo([(40 + 3 * i * i, 9) for i in range(5)]))
    assert DC.restate(*one).tolist() == [1]
    for _ in range(3):
        assert np.array_equal(ex.distinctive_descriptors_batch(large.off, large.desc), expected[large.name])
        assert ex.distinctive_descriptors_batch(np.zeros(1, np.int32), np.zeros((0, 32), np.uint8)).shape == (0,)          # n_points = 0
        assert ex.distinctive_descriptors_batch(*one).tolist() == [1]
        assert np.array_equal(ex.distinctive_descriptors_batch(single.off, single.desc), expected[single.name])
    ex.close()


def test_bad_offsets_are_refused_and_the_context_goes_on(expected):
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import YgzfError
    ex = Extractor(max_width=64, max_height=64)
    c = {c.name: c for c in CASES}["handover_256_257"]
    desc = np.repeat(DC.thermo([(3, 3)]), 16, axis=0)
    for off in ([0, 5, 3, 8], [0, 8, 8, 7], [-1, 2, 5], [-4, -2, 6]):    # descending; a negative first offset
        with pytest.raises(YgzfError, match="libygzf error -1:"):       # YGZF_ERR_INVALID
            ex.distinctive_descriptors_batch(np.array(off, np.int32), desc)
        assert np.array_equal(ex.distinctive_descriptors_batch(c.off, c.desc), expected[c.name])
    ex.close()


def test_reference_body_member_and_batch_agree_on_every_case(expected):
    """bm_distinctive of the boundary library: column 0 the reference's own body of MapPoint::ComputeDistinctiveDescriptors, column 1 the product's
    strong member called per point, column 2 ygz::ComputeDistinctiveDescriptorsBatch, each as the first observation that carries the descriptor the
    MapPoint ends up with."""
    if not os.path.exists(MAPPOINT_LIB):
        pytest.skip("oracle/_ref/boundary/libboundary_mappoint.so did not travel (build() makes it where the reference checkout exists)")
    from orb_ygz_slam_amd import load_library
    load_library()
    B = C.CDLL(MAPPOINT_LIB)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for c in CASES:
        n = len(c.counts)
        desc = np.ascontiguousarray(c.desc) if c.total else np.zeros((1, 32), np.uint8)
        bad = np.zeros(max(c.total, 1), np.uint8)
        out = np.full((n, 3), -9, np.int32)
        assert B.bm_distinctive(n, p(c.off), p(desc), p(bad), p(out)) == 0, c
        want = expected[c.name].copy()
        for q in range(n):                                               # identical observations: the first one that carries the winning descriptor
            if want[q] >= 0:
                rows = c.desc[c.off[q]:c.off[q + 1]]
                want[q] = int(np.nonzero((rows == rows[want[q]]).all(1))[0][0])
        assert np.array_equal(want, expected[c.name]), c                # (no case's answer is ambiguous in the first place)
        for col in range(3):
            assert np.array_equal(out[:, col], want), (c, col, out[:, col], want)
