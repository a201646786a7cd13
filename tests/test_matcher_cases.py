"""CPU tier of the constructed matcher cases (tests/matcher_cases.py): for every case the oracle equals THE REFERENCE'S OWN src/ORBmatcher.cc
(oracle/_ref/libref_orbmatcher.so; skipped where it was never built, as tests/test_ref_matcher.py) in count, every assignment, ownership and
updated prev_matched; and the case's reach predicate holds on the oracle's answer: the inputs really are the crowding / tie / edge they claim."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import matcher_cases as MC

CASES = MC.cases()
needs_reference = pytest.mark.skipif(O.ref_matcher_lib() is None, reason="oracle/_ref/libref_orbmatcher.so not built (reference checkout absent)")


def test_scale_table_is_the_extractors():
    assert (MC.SF == O.Extractor(1000, 1.2, 8, 20, 7).tables()["scale"]).all()


def test_every_family_and_function_is_present():
    fams = {(c.family, c.fn) for c in CASES}
    for fam in (1, 2, 3, 5, 6, 9, 10):
        for fn in MC.PROJ:
            assert (fam, fn) in fams, (fam, fn)
    for need in ((4, "last"), (4, "kf"), (5, "init"), (7, "last"), (7, "mappoints"), (7, "kf"), (7, "init"), (7, "bow"), (8, "last"), (8, "kf"), (11, "bow"),
                 (12, "init"), (10, "init"), (6, "tri")):
        assert need in fams, need


@pytest.mark.parametrize("case", CASES, ids=MC.case_ids())
def test_case_reaches_what_it_claims(case):
    res = MC.run_oracle(O, case)
    assert (res[0] == 0) == case.none, "%d matches" % res[0]
    case.reach(case, res)


@needs_reference
@pytest.mark.parametrize("case", CASES, ids=MC.case_ids())
def test_oracle_equals_reference(case):
    exp = MC.run_oracle(O, case)
    with O.reference_matcher():
        ref = MC.run_oracle(O, MC.for_reference(case))      # (all of the case but for ORBdist = 256, where the reference is undefined)
    assert MC.same(ref, exp, case, culled_as_null=True) is None, MC.same(ref, exp, case, culled_as_null=True)
