"""CPU tier of the constructed ComputeDistinctiveDescriptors cases (tests/distinctive_cases.py): every case is what its label says (its reach
predicate over the restatement's medians), every wrong form changes the answer of exactly the cases that list it and is listed somewhere, the
restatement equals the oracle on every case and scene, and -- where oracle/_ref/libref_mappoint.so was built -- the reference's own compiled
src/MapPoint.cc: indices, and the winning descriptors, which is what the reference keeps.  Integer work: every comparison is exact."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import distinctive_cases as DC

CASES = DC.cases()
IDS = [repr(c) for c in CASES]
SCENES = DC.scenes()


@pytest.fixture(scope="module")
def answers():
    out = {}
    for c in CASES:
        trace = []
        out[repr(c)] = (DC.restate(c.off, c.desc, trace=trace), trace)
    return out


def test_ids_are_unique_and_sizes_are_covered():
    assert len(set(IDS)) == len(IDS)
    sizes = {n for c in CASES for n in c.counts}
    assert sizes >= {0, 1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 258, 300, 320, 321, 700} and max(sizes) == 700
    by = {c.name: c for c in CASES}
    assert by["batch_interleaved"].counts == [0, 1, 5, 300, 0, 700, 2]
    assert [sum(n > 256 for n in by["batch_%d_large" % k].counts) for k in (1, 4, 5)] == [1, 4, 5]
    assert [(len(by["batch_n%d" % n].counts) + 1) % 4 for n in (3, 4, 5, 6)] == [0, 1, 2, 3] and all(max(by["batch_n%d" % n].counts) > 256 for n in (3, 4, 5, 6))
    assert by["batch_all_empty"].total == 0


def test_thermometer_distances_are_plane_geometry():
    pts = [(0, 0), (128, 128), (128, 0), (0, 128), (20, 63), (22, 64), (77, 31)]
    D = DC.hamming_matrix(DC.thermo(pts))
    for i, a in enumerate(pts):
        for j, b in enumerate(pts):
            assert D[i, j] == abs(a[0] - b[0]) + abs(a[1] - b[1])
    assert D[0, 1] == 256 and (D == D.T).all()
    # and the matrix product behind hamming_matrix against a popcount of the xor
    rng = np.random.default_rng(0)
    d = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    assert np.array_equal(DC.hamming_matrix(d), np.unpackbits(d[:, None, :] ^ d[None, :, :], axis=2).sum(2))


def test_the_two_small_examples_answer_as_worked_by_hand():
    off, d = np.array([0, 4], np.int32), DC.thermo([(0, 0), (1, 0), (10, 0), (12, 0)])
    assert [int(DC.restate(off, d, f)[0]) for f in (None, "upper_median", "last_minimum")] == [0, 1, 1]
    off, d = np.array([0, 3], np.int32), DC.thermo([(0, 0), (128, 128), (128, 128)])
    assert [int(DC.restate(off, d, f)[0]) for f in (None, "padding_counts")] == [1, 0]
    assert DC.restate(np.array([0, 0, 1], np.int32), d[:1]).tolist() == [-1, 0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_what_it_claims(answers, case):
    a, trace = answers[repr(case)]
    assert len(a) == len(case.counts) == len(trace)
    assert case.reach(a, trace)
    for p, n in enumerate(case.counts):
        assert (a[p] == -1) if n == 0 else (0 <= a[p] < n)


@pytest.mark.parametrize("form", DC.FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(answers, form):
    listed = [c.name for c in CASES if form in c.wrong]
    assert listed, "no case decides %s" % form
    moved = [c.name for c in CASES if not np.array_equal(DC.restate(c.off, c.desc, form), answers[repr(c)][0])]
    assert moved == listed


def test_the_issue_sets_of_cases_move_as_it_asks():
    by = {c.name: c for c in CASES}
    for N in (4, 64, 128, 192, 256, 258, 320):
        assert "upper_median" in by["even_%d" % N].wrong
    for N in (3, 63, 65, 129, 193, 255, 257, 321):
        assert "upper_median" not in by["odd_%d" % N].wrong
    for N in (65, 129, 193, 257, 321):
        assert {"padding_counts", "tail_dropped"} <= set(by["tail_%d" % N].wrong)
    assert "large_as_small" in by["handover_256_257"].wrong
    assert all("last_minimum" in c.wrong for c in CASES if c.name.startswith(("tie_", "identical_")))
    assert all("large_list_shifted" in c.wrong for c in CASES if max(c.counts) > 256)


def test_restatement_equals_oracle(oracle, answers):
    for c in CASES:
        assert np.array_equal(oracle.distinctive_descriptors(c.off, c.desc), answers[repr(c)][0]), c
    for name, off, desc in SCENES:
        assert np.array_equal(oracle.distinctive_descriptors(off, desc), DC.restate(off, desc)), name


def test_restatement_equals_reference_mappoint(answers):
    if O.ref_mappoint_lib() is None:
        pytest.skip("oracle/_ref/libref_mappoint.so not built (reference checkout absent)")
    for name, off, desc, mine in [(c.name, c.off, c.desc, answers[repr(c)][0]) for c in CASES] + [(n, o, d, DC.restate(o, d)) for n, o, d in SCENES]:
        with O.reference_mappoint():
            r = O.distinctive_descriptors(off, desc)
        assert np.array_equal(r, mine), name
        for p in range(len(off) - 1):                                    # the reference keeps the winning DESCRIPTOR
            if mine[p] >= 0:
                assert (desc[off[p] + r[p]] == desc[off[p] + mine[p]]).all(), (name, p)
