"""CPU tier of the constructed vocabulary-descent cases (tests/bow_cases.py): every case is what its label says, every wrong form changes the
answer of exactly the cases that list it and is listed somewhere, the restatement equals oracle.bow_descend on every case, and -- where
oracle/_ref/libref_dbow2.so was built and the reference's text loader takes the tree (k <= 20, L >= 1) -- the BowVector and FeatureVector
assembled from the restatement's descent equal what the reference's own DBoW2 returns for the tree read back by its own loader: word ids, values
bit for bit as doubles, the FeatureVector.  The ties of the k > 20 trees have twins with k = 20 for that.  Every comparison is exact."""
import numpy as np
import pytest

from tests import bow_cases as BC

CASES = BC.cases()
IDS = [repr(c) for c in CASES]


@pytest.fixture(scope="module")
def answers():
    out = {}
    for c in CASES:
        trace = []
        out[repr(c)] = BC.restate(c.voc, c.desc, c.levelsup, trace=trace) + (trace,)
    return out


def test_ids_are_unique_and_shapes_are_covered():
    assert len(set(IDS)) == len(IDS)
    by = {c.name: c for c in CASES}
    assert {c.voc["k"] for c in CASES if c.name.startswith("branch_")} == {1, 2, 63, 64, 65, 128, 129}
    assert max(len(c.voc["parent"]) for c in CASES) == 129 + 129 * 129 + 1 and all(c.voc["L"] <= 2 for c in CASES if c.voc["k"] > 20)
    assert by["interleaved_7"].voc["parent"].tolist() == [-1, 0, 0, 1, 2, 1, 2]
    assert [len(by["batch_%d" % n].desc) for n in (1, 3, 4, 5, 257)] == [1, 3, 4, 5, 257]
    for tree in ("full", "ragged"):
        L = by[tree + "_levelsup_0"].voc["L"]
        assert [by["%s_levelsup_%d" % (tree, s)].levelsup for s in (0, 1, L - 1, L, L + 1)] == [0, 1, L - 1, L, L + 1]
    _, level = BC.positions(by["ragged_levelsup_0"].voc["parent"])
    assert set(level[by["ragged_levelsup_0"].voc["is_leaf"] > 0].tolist()) == {1, 2, 3}
    assert len(by["root_alone_levelsup_0"].voc["parent"]) == 1
    shared = {}
    for c in CASES:                                                      # cases of one `tree` share one vocabulary
        v = shared.setdefault(c.tree, c.voc)
        assert np.array_equal(v["parent"], c.voc["parent"]) and np.array_equal(v["desc"], c.voc["desc"]) and v["L"] == c.voc["L"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_what_it_claims(answers, case):
    leaf, nid, trace = answers[repr(case)]
    assert len(leaf) == len(nid) == len(case.desc) == len(trace)
    assert case.reach(leaf, nid, trace)
    assert case.voc["is_leaf"][leaf].all()


@pytest.mark.parametrize("form", BC.FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(answers, form):
    listed = [c.name for c in CASES if form in c.wrong]
    assert listed, "no case decides %s" % form
    moved = []
    for c in CASES:
        leaf, nid = BC.restate(c.voc, c.desc, c.levelsup, form)
        if not (np.array_equal(leaf, answers[repr(c)][0]) and np.array_equal(nid, answers[repr(c)][1])):
            moved.append(c.name)
    assert moved == listed


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_oracle(oracle, answers, case):
    leaf, nid, _ = answers[repr(case)]
    o_leaf, o_nid = oracle.bow_descend(case.voc, case.desc, case.levelsup)
    assert np.array_equal(o_leaf, leaf) and np.array_equal(o_nid, nid)


def test_every_small_tree_goes_to_the_reference():
    """the rules of the k > 20 trees have a twin the loader takes, and every other tree but the root alone is loadable itself"""
    not_loadable = {c.tree for c in CASES if not BC.reference_loadable(c.voc)}
    assert not_loadable == {"tie_5_69_k70", "tie_63_64_k65", "tie_63_64_128_k129", "branch_63", "branch_64", "branch_65", "branch_128", "branch_129", "root_alone"}
    assert {"twin_5_19_k20", "twin_9_10_k20", "twin_3_4_19_k20"} <= {c.name for c in CASES if BC.reference_loadable(c.voc)}


@pytest.mark.parametrize("case", [c for c in CASES if BC.reference_loadable(c.voc)], ids=[repr(c) for c in CASES if BC.reference_loadable(c.voc)])
def test_restatement_equals_reference_dbow2(oracle, answers, tmp_path, case):
    if oracle.ref_dbow2_lib() is None:
        pytest.skip("oracle/_ref/libref_dbow2.so not built (no reference checkout)")
    leaf, nid, _ = answers[repr(case)]
    voc = dict(case.voc, k=max(case.voc["k"], 2))                        # the header's k only sizes the loader's reserve(), which divides by k - 1
    path = str(tmp_path / "voc.txt")
    oracle.write_vocabulary_text(voc, path)
    ref = oracle.RefVocabulary(path)
    assert ref.size() == int(voc["is_leaf"].sum())
    r_ids, r_vals, r_fv = ref.transform(case.desc, case.levelsup)
    ids, vals, fv = oracle.bow_vectors(case.voc, leaf, nid)
    assert len(ids) > 0 and np.array_equal(ids, r_ids)
    assert np.array_equal(vals.view(np.uint64), r_vals.view(np.uint64))
    defined = BC.key_defined(case.voc, leaf, case.levelsup)
    if defined.all():
        assert sorted(fv) == sorted(r_fv) and all(np.array_equal(fv[key], r_fv[key]) for key in fv)
    else:                                                                # the reference leaves *nid unassigned for a leaf above the key level
        assert case.tree == "ragged"
        for key, feats in fv.items():
            for i in feats:
                if defined[i]:
                    assert key in r_fv and i in r_fv[key].tolist(), (key, i)
