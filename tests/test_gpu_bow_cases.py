"""GPU tier of the constructed vocabulary-descent cases (tests/bow_cases.py; tests/test_bow_cases.py holds the restatement to the oracle and to the
reference's own DBoW2 and proves that each case is the tie, chunk edge, interleaved id, key level or ragged leaf it claims): ygzf_vocabulary_set
followed by ygzf_bow_transform (k_bow_descend) equals the restatement exactly on every case, in leaf and in key node, and the BowVector /
FeatureVector assembled from the device's descent equal the ones assembled from the restatement's.  One context serves the whole list, so
vocabularies of 1 to 16 771 nodes replace each other in the list's order; one more context sets the 16 771-node tree, the 7-node interleaved
one, the root alone and the 129-ary tree again: a smaller tree after a larger one must not read the larger one's tables."""
import numpy as np
import pytest

from tests import bow_cases as BC

pytestmark = pytest.mark.gpu

CASES = BC.cases()


@pytest.fixture(scope="module")
def expected():
    out = {c.name: BC.restate(c.voc, c.desc, c.levelsup) for c in CASES}
    for leaf, nid in out.values():
        leaf.setflags(write=False); nid.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ctx():
    from orb_ygz_slam_amd import Extractor
    ex = Extractor(max_width=64, max_height=64)
    yield ex
    ex.close()


def _same_vectors(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and sorted(a[2]) == sorted(b[2]) and
            all(np.array_equal(a[2][key], b[2][key]) for key in a[2]))


def _check(oracle, ex, case, expected):
    ex.vocabulary_set(case.voc["parent"], case.voc["desc"], case.voc["L"])
    leaf, nid = ex.bow_transform(case.desc, case.levelsup)
    e_leaf, e_nid = expected[case.name]
    bad = np.nonzero((leaf != e_leaf) | (nid != e_nid))[0]
    assert len(bad) == 0, (case, bad[:8], leaf[bad[:8]], e_leaf[bad[:8]], nid[bad[:8]], e_nid[bad[:8]])
    assert _same_vectors(oracle.bow_vectors(case.voc, leaf, nid), oracle.bow_vectors(case.voc, e_leaf, e_nid)), case


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_device_equals_restatement(oracle, ctx, expected, case):
    _check(oracle, ctx, case, expected)


def test_smaller_vocabulary_after_larger_on_one_context(oracle, expected):
    from orb_ygz_slam_amd import Extractor
    by = {c.name: c for c in CASES}
    order = [by["branch_129"], by["interleaved_7"], by["root_alone_levelsup_0"], by["root_alone_levelsup_4"], by["tie_63_64_128_k129"], by["branch_129"]]
    assert [len(c.voc["parent"]) for c in order] == [16771, 7, 1, 1, 16771, 16771]
    ex = Extractor(max_width=64, max_height=64)
    for c in order:
        _check(oracle, ex, c, expected)
    # and every query of the large tree on the small ones: whatever the device finds must be a node of the tree that is set
    big = by["branch_129"].desc
    for c in (by["interleaved_7"], by["root_alone_levelsup_0"]):
        ex.vocabulary_set(c.voc["parent"], c.voc["desc"], c.voc["L"])
        leaf, nid = ex.bow_transform(big, c.levelsup)
        e_leaf, e_nid = BC.restate(c.voc, big, c.levelsup)
        assert np.array_equal(leaf, e_leaf) and np.array_equal(nid, e_nid), c
    ex.close()
