"""GPU tier of the constructed stereo cases (tests/stereo_cases.py; tests/test_stereo_cases.py holds the oracle to a numpy restatement and to the
reference's own Frame.cc on every one of them and proves that each case is the tie / edge / threshold it claims): k_stereo_prep, k_stereo_match
and k_stereo_cut through Extractor.compute_stereo_matches equal the oracle bit for bit in mvuRight and mvDepth -- tolerance zero, as the README
states for stereo depths -- and a second run on the same context equals the first: k_stereo_prep orders the records inside a bin by atomics,
and the answer must not depend on that order.  One context per configuration (8 levels, 12 levels) serves every case of that
configuration in the order of the list, so that every case also follows another one's buffers, and the frame size changes between the n_left
cases (512 x 384 / 416 x 312) through the context's geometry path."""
import numpy as np
import pytest

from tests import stereo_cases as SC

pytestmark = pytest.mark.gpu

CASES = SC.cases()


@pytest.fixture(scope="module")
def ctx():
    from orb_ygz_slam_amd import Extractor
    made = {}

    def get(cfg):
        nlevels = SC.CONFIGS[cfg][0]
        if nlevels not in made:
            w = max(c[1] for c in SC.CONFIGS.values() if c[0] == nlevels)
            h = max(c[2] for c in SC.CONFIGS.values() if c[0] == nlevels)
            made[nlevels] = Extractor(1000, 1.2, nlevels, 20, 7, max_width=w, max_height=h, max_batch=2)
        return made[nlevels]
    yield get
    for ex in made.values():
        ex.close()


@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_device_equals_oracle_twice(oracle, ctx, case):
    ex = ctx(case.cfg)
    exp = SC.run_oracle(oracle, case)
    first = tuple(a.copy() for a in SC.run_device(ex, case))
    second = SC.run_device(ex, case)
    diff = [(i, first[0][i], exp[0][i], first[1][i], exp[1][i]) for i in range(len(exp[0])) if first[0][i] != exp[0][i] or first[1][i] != exp[1][i]]
    assert SC.same(first, exp), (case, diff[:5])
    assert SC.same(second, first), case
    for label, want in case.expect.items():          # (and where the case says a match is accepted / is not, the device says so)
        if "code" in want:
            assert (first[0][case.labels[label]] >= 0) == (want["code"] in ("ACCEPT", "ACCEPT_ZERO_DISP")), label
