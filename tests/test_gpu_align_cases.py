"""GPU tier of the constructed aligner cases (tests/align_cases.py; tests/test_align_cases.py holds the oracle to the reference's own code on every
one of them and proves that each case reaches the gate, the stale patch or the kernel form it claims; tests/test_sia_host_progs.py proves which
LDS plan each takes).  For every case, with the reference patches of all levels built by k_sia_precompute (sia_precompute=1) and inside
k_sia_run (sia_precompute=0), twice on the same context: return value, SE3, linearisations, chi2 and Hessian equal the oracle's device-order
mode bit for bit; the count equals the predicted integer where the case predicts one; the SE3 lies within 1e-5 of the oracle's reference-order
mode and of the file recorded from the reference's own code.  And a stale case followed by its twin on one context: nothing of the first is
left in the patch caches.

On the stale cases the kernel followed the reference all along (zero gradients under the kept patch); it was the oracle's device-order mode that
kept the coarser level's gradients (oracle/oracle_align.cpp)."""
import os

import numpy as np
import pytest

from tests import align_cases as AC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-5          # on the 7 SE3 parameters, as tests/test_gpu_align.py

CASES = AC.cases()
PLANS = [1, 0]


@pytest.fixture(scope="module")
def ctx():
    """sia_precompute -> context (YGZF_FORCE is read when a context is created), closed when the file is done"""
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    made = {}

    def get(pre):
        if pre not in made:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("YGZF_FORCE", force_env(sia_precompute=pre))
                made[pre] = Extractor(600, 1.2, 8, 20, 7, max_width=64, max_height=64, max_batch=1)
        return made[pre]
    yield get
    for ex in made.values():
        ex.close()


@pytest.fixture(scope="module")
def answers(oracle):
    """case name -> (device-order answer, reference-order answer, recorded reference answer), computed once"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "align_cases_ref.npz"))
    return {c["name"]: (AC.run_oracle(oracle, c, device_order=True), AC.run_oracle(oracle, c), g["T_" + c["name"]]) for c in CASES}


def _check(case, got, answers, what):
    dev, ref, gold = answers[case["name"]]
    assert got[0] == dev[0], (what, got[0], dev[0])
    assert np.array_equal(AC.bits(got[3]), AC.bits(dev[3])), (what, "H")
    assert np.array_equal(AC.bits(got[2]), AC.bits(dev[2])), (what, "linearisations / chi2", got[2], dev[2])
    assert np.array_equal(AC.bits(got[1]), AC.bits(dev[1])), (what, "SE3", got[1], dev[1])
    if case["expect_ret"] is not None:
        assert got[0] == case["expect_ret"], (what, got[0], case["expect_ret"])
    assert float(np.abs(got[1] - ref[1]).max()) <= TOL and float(np.abs(got[1] - gold).max()) <= TOL, (what, got[1], ref[1], gold)


RUNS = [(c, p) for p in PLANS for c in CASES]


@pytest.mark.parametrize("case,pre", RUNS, ids=["precompute%d-%s" % (p, c["name"]) for c, p in RUNS])
def test_device_equals_oracle_twice(ctx, answers, case, pre):
    ex = ctx(pre)
    for step in range(2):
        _check(case, AC.run_device(ex, case), answers, (case["name"], pre, step))


@pytest.mark.parametrize("pre", PLANS)
def test_stale_case_then_its_twin_on_one_context(ctx, answers, pre):
    ex = ctx(pre)
    by = AC.by_name()
    for name in ("stale_a", "stale_c", "stale_d", "count_1025"):
        first, second = by[name], by[by[name]["twin"] or "stale_a_twin"]
        _check(first, AC.run_device(ex, first), answers, (name, pre))
        _check(second, AC.run_device(ex, second), answers, (second["name"], pre, "after", name))
