"""CPU tier of the KeyFrameDatabase tests: the constructed cases of tests/kfdb_cases.py do what their labels say, its wrong forms change exactly
the cases listed for them, the form the device path takes (per-slot common / first / score, the list sorted by (first, order of add)) equals the
walk over the inverted file everywhere, the seeded scenes have the sizes and the bite they are meant to have, and the restatement equals
tests/golden/kfdb_ref.npz -- what the reference's own src/KeyFrameDatabase.cc and DBoW2 returned on the same worlds
(tools/make_golden_kfdb_ref.py), minimum scores, candidate lists, all six fields after every query and the fp64 scores, bit for bit."""
import hashlib
import os

import numpy as np
import pytest

from tests import kfdb_cases as K
from tests.conftest import ROOT

CASES = K.cases()
WORLDS = K.worlds()
_answers = {}


def answers(name):
    if name not in _answers:
        _answers[name] = K.run(WORLDS[name])
    return _answers[name]


def same(a, b):
    return len(a) == len(b) and all(x.same(y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_case_does_what_its_label_says(case):
    a = answers("case/" + case.label)
    assert case.reach(a), "the case does not reach what its label names: %r" % ([(x.cands, x.trace) for x in a],)


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_wrong_form_changes_exactly_its_cases(mutation):
    changed = set(c.label for c in CASES if not same(answers("case/" + c.label), K.run(c.world, mutation)))
    listed = set(c.label for c in CASES if mutation in c.wrong)
    assert listed, "no case is listed for %s" % mutation
    assert changed == listed, (sorted(changed - listed), sorted(listed - changed))


def test_labels_are_unique_and_mutations_known():
    assert len(set(c.label for c in CASES)) == len(CASES)
    assert all(m in K.MUTATIONS for c in CASES for m in c.wrong)


@pytest.mark.parametrize("name", list(WORLDS))
def test_device_form_equals_inverted_file_walk(name):
    assert same(answers(name), K.run(WORLDS[name], form="arrays"))


def test_scene_quality():
    sizes, bites = [], set()
    for seed in K.SCENE_SEEDS:
        w, a = WORLDS["scene/%d" % seed], answers("scene/%d" % seed)
        n = len(w.kfs) - 3
        sizes.append(n)
        assert 3 <= n <= 300 and all(1 <= len(k.ids) <= 400 for k in w.kfs)
        assert len(a) == 8 and a[5].cands == [] and sum(len(x.cands) for x in a) >= 4          # (a[5] repeats a[4]'s query)
        pw = K.run(w, "pairwise_l1")
        assert any((x.raw[~np.isnan(x.raw)].view(np.uint64) != y.raw[~np.isnan(y.raw)].view(np.uint64)).any() for x, y in zip(a, pw)), \
            "pairwise summation changes no score of scene %d in its bits" % seed
        bites |= set(m for m in K.MUTATIONS if m != "pairwise_l1" and not same(a, K.run(w, m)))
    assert min(sizes) <= 5 and max(sizes) >= 250
    assert bites >= {"ge_word_gate", "slot_order", "keep_connected", "loop_rule_for_reloc", "last_duplicate"}, bites


@pytest.mark.parametrize("name", list(WORLDS))
def test_restatement_equals_reference_golden(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz"))
    w = WORLDS[name]
    assert bytes(g[name + "/sha"]) == hashlib.sha256(K.world_bytes(w)).digest(), "the golden file was recorded for another world: rerun tools/make_golden_kfdb_ref.py"
    mine = K.golden_arrays(name, w, answers(name))
    assert len(mine[name + "/op"]) > 0
    for key, v in mine.items():
        ref = g[key]
        if key.endswith("/raw"):                       # (NaN marks a keyframe that is not stored: any NaN)
            assert np.array_equal(np.isnan(v.view(np.float64)), np.isnan(ref.view(np.float64))), key
            keep = ~np.isnan(ref.view(np.float64))
            v, ref = v[keep], ref[keep]
        assert v.shape == ref.shape and np.array_equal(v, ref), (key, np.argwhere(v != ref)[:5])
