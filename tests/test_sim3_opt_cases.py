"""tests/sim3_opt_cases.py held to its own claims, on the CPU: every constructed case reaches what it is listed for in both summation modes,
with a decision margin >= MARGIN_MIN on every chi2 gate, rho sign and stop rule and pivots >= PIVOT_MARGIN_MIN; both modes decide alike and
round every projection quotient to the same float (the admission rule of the dithered Jacobian); EPS_ORDER is what the cases measure; every
wrong form moves exactly the cases listed for it; the header's sin / cos / exp against libm within the recorded figure."""
import math

import numpy as np
import pytest

from tests import sim3_opt_cases as SC


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_reaches_its_claim(name):
    c = SC.case_by_name(name)
    a, b = SC.expected(c, "reference"), SC.expected(c, "device")
    print("%s: margin %.3e at %s / %.3e at %s, pivots %.3e / %.3e, nBad %d ret %d iterations %s trials %s stop %s" % (
        name, a.margin, a.where, b.margin, b.where, a.pivot_margin, b.pivot_margin, a.n_bad, a.ret, a.iters, a.trials, a.stop))
    assert c.reach(a) and c.reach(b), "the case does not reach its claim"
    assert a.margin >= SC.MARGIN_MIN and b.margin >= SC.MARGIN_MIN
    assert a.pivot_margin >= SC.PIVOT_MARGIN_MIN and b.pivot_margin >= SC.PIVOT_MARGIN_MIN
    assert a.qhash == b.qhash, "the two modes round a projection quotient to different floats: the case does not qualify"
    assert SC.same_decisions(a, b), "the two modes decide differently"


def test_the_list_covers_what_the_issue_names():
    stops = {s for c in SC.CASES for s in SC.expected(c, "reference").stop}
    assert stops == {SC.STOP_MAX_ITER, SC.STOP_TRIALS, SC.STOP_RHO_ZERO, SC.STOP_NBAD, SC.STOP_NOT_RUN}
    sizes = {len(c.problem.P1c) for c in SC.CASES}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 600} <= sizes
    left = {len(r.removed) - r.n_bad for r in (SC.expected(c, "reference") for c in SC.CASES if c.name.startswith("survive_"))}
    assert left == {0, 1, 9, 10, 11}
    assert {bool(c.problem.fix_scale) for c in SC.CASES} == {True, False}
    assert any(c.problem.K1 != c.problem.K2 for c in SC.CASES)
    assert any(len(set(np.asarray(c.problem.is1).tolist())) > 1 for c in SC.CASES)
    assert len(SC.WRONG_FORMS) >= 11 and set(SC.MOVED) == set(SC.WRONG_FORMS)


def test_eps_order_is_what_the_cases_measure():
    worst, at = 0.0, None
    for c in SC.CASES:
        a, b = SC.expected(c, "reference"), SC.expected(c, "device")
        with np.errstate(all="ignore"):
            d = np.abs(a.S12 - b.S12)
        d = d[~np.isnan(d)]
        if len(d) and d.max() > worst:
            worst, at = float(d.max()), c.name
    print("largest Sim3 difference between the modes: %.3e at %s (EPS_ORDER %.3e)" % (worst, at, SC.EPS_ORDER))
    assert worst <= SC.EPS_ORDER and worst >= SC.EPS_ORDER / 4


@pytest.mark.parametrize("wrong", SC.WRONG_FORMS)
def test_wrong_form_moves_exactly_its_cases(wrong):
    for mode in ("reference", "device"):
        moved = [c.name for c in SC.CASES if not SC.same(SC.optimize_sim3(c.problem, mode, wrong), SC.expected(c, mode))]
        assert moved == SC.MOVED[wrong], mode


def test_last_trial_errors_equal_the_accepted_ones():
    """the finding behind MOVED['classify_accepted'] == []: the three routes on which a round ends with a rejected trial are reached, and on
    each the gate says the same at the last trial and at the accepted estimate"""
    for name, stop in (("stop_trials", SC.STOP_TRIALS), ("stop_rho_zero", SC.STOP_RHO_ZERO), ("nan_point", SC.STOP_MAX_ITER)):
        r = SC.expected(SC.case_by_name(name), "reference")
        rounds = [rt for rt, s in zip(r.trace, r.stop) if s == stop and not rt["trials"][-1]["good"]]
        assert rounds, name
        for rt in rounds:
            assert np.array_equal(rt["bad"], rt["bad_accepted"]), name


def test_transcendentals_against_libm():
    x = np.linspace(-math.pi, math.pi, 20001)
    sc = np.array([SC.so_sincos(v) for v in x])
    ds, dc = float(np.max(np.abs(sc[:, 0] - np.sin(x)))), float(np.max(np.abs(sc[:, 1] - np.cos(x))))
    s = np.linspace(-1.0, 1.0, 20001)
    de = float(np.max(np.abs(np.array([SC.so_exp(v) for v in s]) / np.exp(s) - 1.0)))
    print("largest distance from libm: sin %.3e cos %.3e (absolute, |theta| <= pi), exp %.3e (relative, |sigma| <= 1); bound %.1e" % (ds, dc, de, SC.LIBM_EPS))
    assert ds <= SC.LIBM_EPS and dc <= SC.LIBM_EPS and de <= SC.LIBM_EPS
    assert SC.so_exp(0.0) == 1.0 and SC.so_sincos(0.0) == (0.0, 1.0)
    assert abs(SC.so_exp(1e-9) / math.exp(1e-9) - 1.0) <= SC.LIBM_EPS and abs(SC.so_exp(-1e-9) / math.exp(-1e-9) - 1.0) <= SC.LIBM_EPS


def test_transcendentals_are_defined_everywhere():
    for v in (np.inf, -np.inf, np.nan):
        sn, cs = SC.so_sincos(v)
        assert np.isnan(sn) and np.isnan(cs)
    for v in (1e300, -1e300, 1048577.0):
        assert SC.so_sincos(v) == (0.0, 1.0)
    sn, cs = SC.so_sincos(1048576.0)
    assert abs(sn - math.sin(1048576.0)) < 1e-9 and abs(cs - math.cos(1048576.0)) < 1e-9   # (the edge of the reduction: ~k eps)
    assert SC.so_exp(np.inf) == np.inf and SC.so_exp(1e300) == np.inf and SC.so_exp(710.0) == np.inf
    assert SC.so_exp(-np.inf) == 0.0 and SC.so_exp(-1e300) == 0.0 and SC.so_exp(-746.0) == 0.0
    assert np.isnan(SC.so_exp(np.nan))
    assert abs(SC.so_exp(700.0) / math.exp(700.0) - 1.0) < 1e-13 and abs(SC.so_exp(-700.0) / math.exp(-700.0) - 1.0) < 1e-13
