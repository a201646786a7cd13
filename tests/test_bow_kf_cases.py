"""CPU tier of the SearchByBoW(KeyFrame, KeyFrame) tests: the constructed cases of tests/bow_kf_cases.py do what their labels say, its wrong forms
change exactly the cases listed for them, the seeded scenes exercise every rejection, and the restatement is pinned to reference code.

The pin.  Feature for feature, src/ORBmatcher.cc:480-595 on (KF1, KF2) is :155-263 on (KF1, the KF2 features that carry a good MapPoint) with the
result inverted -- the same walk, the same strict `<` scan, the same chain through "slot already matched", the same histogram arithmetic --
unless some attempt reaches the ratio test with bestDist1 == 50, where :216 accepts and :548 does not.  So every scene is first shown to hold
no such attempt and then compared with oracle_py.search_by_bow on the filtered lists: once with the oracle's restatement of :155-263 and once
more with the reference's own compiled :155-263 where oracle/_ref holds it.  The == 50 case is the one thing this reduction cannot see; it is
pinned by the constructed case and by reading :548."""
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import bow_kf_cases as K

CASES = K.cases()
PARAMS = ((0.75, True), (0.9, False), (0.6, True))
_scenes = {}


def scene(seed):
    if seed not in _scenes:
        kf1, cands = K.bow_kf_scene(seed)
        _scenes[seed] = (kf1, cands, [K.join(kf1["fv"], c["fv"]) for c in cands])
    return _scenes[seed]


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_case_does_what_its_label_says(case):
    r = case.ref()
    assert case.reach(case, r), "the case does not reach what its label names: %r" % (r[2],)
    assert np.array_equal(r[0], case.expect), (r[0], case.expect)
    assert r[1] == int((case.expect >= 0).sum())


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_wrong_form_changes_exactly_its_cases(mutation):
    changed = set()
    for case in CASES:
        a, b = case.ref(), case.ref(mutation)
        if not (np.array_equal(a[0], b[0]) and a[1] == b[1]):
            changed.add(case.label)
    listed = set(c.label for c in CASES if mutation in c.wrong)
    assert listed, "no case is listed for %s" % mutation
    assert changed == listed, (sorted(changed - listed), sorted(listed - changed))


def test_labels_are_unique():
    assert len(set(c.label for c in CASES)) == len(CASES)


@pytest.mark.parametrize("seed", K.SCENE_SEEDS)
def test_scene_quality(seed):
    kf1, cands, joined = scene(seed)
    assert 550 <= len(kf1["keys"]) <= 650 and len(cands) == 4
    assert 0.08 < 1 - kf1["valid"].mean() < 0.22
    rounds = 0
    for kf2, j in zip(cands, joined):
        assert 300 <= len(kf2["keys"]) <= 800 and 0.08 < 1 - kf2["valid"].mean() < 0.22
        rounds = max(rounds, int(np.diff(j["off2"]).max()))
        m, n, ev = K.ref_search_by_bow_kf(kf1, kf2, j, 0.75, True)
        assert n > 20 and n == (m >= 0).sum()
        assert any(e[1] >= K.TH_LOW and e[1] < 256 for e in ev), "no rejection by the threshold"
        assert any(e[1] < K.TH_LOW and not e[3] for e in ev), "no rejection by the ratio"
        assert (m == -2).any(), "nothing culled by the rotation check"
        m2, n2, _ = K.ref_search_by_bow_kf(kf1, kf2, j, 0.75, True, "no_chain")
        assert not np.array_equal(m, m2), "the vbMatched2 chain never bites"
    if K.NODE_BITS[seed] == 1:
        assert rounds > 128, "the 1-bit node ids give no node of more than two rounds"


def _by_frame_form(kf1, kf2, j, ratio, ori):
    """:155-263 on (KF1, KF2's features with a good MapPoint), inverted -> (match12, nmatches)"""
    keep = kf2["valid"][j["idx2"]] != 0
    f_idx = j["idx2"][keep]
    f_off = np.concatenate([[0], np.cumsum(keep)])[j["off2"]].astype(np.int32)
    n, m = O.search_by_bow(j["off1"], j["idx1"], f_off, f_idx, kf1["valid"], kf1["keys"], kf1["desc"], kf2["keys"], kf2["desc"], ratio, ori)
    m = np.asarray(m)
    match12 = np.full(len(kf1["keys"]), -1, np.int32)
    f = np.flatnonzero(m >= 0)
    match12[m[f]] = f
    return match12, int(n)


@pytest.mark.parametrize("leg", ["oracle", "reference"])
@pytest.mark.parametrize("seed", K.SCENE_SEEDS)
def test_restatement_equals_frame_form_on_filtered_lists(seed, leg):
    if leg == "reference" and O.ref_matcher_lib() is None:
        pytest.skip("oracle/_ref/libref_orbmatcher.so is not built")
    kf1, cands, joined = scene(seed)
    for ratio, ori in PARAMS:
        for kf2, j in zip(cands, joined):
            m, n, ev = K.ref_search_by_bow_kf(kf1, kf2, j, ratio, ori)
            assert not any(e[1] == K.TH_LOW for e in ev), "an attempt with bestDist1 == 50: the reduction does not hold for this scene"
            if leg == "reference":
                with O.reference_matcher():
                    fm, fn = _by_frame_form(kf1, kf2, j, ratio, ori)
            else:
                fm, fn = _by_frame_form(kf1, kf2, j, ratio, ori)
            # a culled match leaves -2 in the FRAME slot of :155-263's restatement and nothing in the reference's own answer: in either
            # case the inverse has no entry for it
            assert np.array_equal(np.where(m == -2, -1, m), fm) and n == fn
