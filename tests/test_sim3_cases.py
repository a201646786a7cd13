"""CPU tier: the cases of tests/sim3_cases.py are held to their claims on the numpy restatement of Sim3Solver -- no device, no library.

Every constructed case reaches what its label says and keeps the decision margin MARGIN_MIN in both modes (reference: eigenvector -> atan2 ->
angle-axis -> Rodrigues; device: the rotation straight from the quaternion); both modes take the same decisions on every constructed case; the
largest difference of their hypotheses -- EPS_MODE -- is measured here and held against the recorded constant from which MARGIN_MIN is derived;
each wrong form moves exactly the cases that list it.  The seeded scenes reach their claim in both modes but are not compared across modes and
keep no margin: their 300 random triples include near-degenerate ones, which amplify a last-bit difference without bound -- no defect of either
mode.  (The device is compared with mode "device" bit for bit, so it needs no margin there.)"""
import numpy as np
import pytest

from tests import sim3_cases as SC


def test_the_case_list_covers_what_it_must():
    sizes = {len(c.problem.X1) for c in SC.constructed() if c.name.startswith("all_n")}
    assert sizes == {3, 20, 63, 64, 65, 128, 129}
    names = SC.NAMES + SC.SCENE_NAMES
    assert len(names) == len(set(names)) and set(SC.MOVED_BY) == set(names)
    for must in ("gate13_inside", "gate13_between", "gate_exact", "count_min", "count_min_plus1", "tie", "return_then_beat", "ends_on_max", "returns_on_max",
                 "n_below_min", "min_equals_n", "collinear", "coincident", "identity", "behind_camera2", "z_zero", "fix_scale_17", "nonfinite"):
        assert must in SC.NAMES
    for name, cands, _ in SC._SCENES:
        got = SC.scene(name)
        assert len(got) == cands and 3 <= cands <= 10
        for c in got:
            assert 20 <= len(c.problem.X1) <= 500 and c.problem.samples.shape == (300, 3)
    assert SC.JACOBI_SWEEPS >= 6


def test_the_gate_pair_differs_in_the_gate_only():
    a, b = SC.case_by_name("gate13_inside").problem, SC.case_by_name("gate13_between").problem
    assert np.array_equal(a.X2, b.X2) and np.array_equal(a.samples, b.samples) and np.array_equal(a.sigma2_1, b.sigma2_1)
    assert int((a.X1 != b.X1).sum()) == 1
    assert float(SC.gates(a.sigma2_1)[7]) == 13.0 and abs(float(SC.gates(a.sigma2_1, "float_gates")[7]) - 13.2624) < 1e-4
    assert list(SC.gates(SC.SIGMA2[:2])) == [9.0, 13.0]
    e = float(SC.expected(SC.case_by_name("gate13_between")).hyps.err1[0, 7])
    assert 13.0 < e < 13.26


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_reaches_its_claim_with_margin(name):
    c = SC.case_by_name(name)
    ref, dev = SC.expected(c, "reference"), SC.expected(c, "device")
    print("%s: margin %.3e (reference) %.3e (device), counts %s, calls %s" % (
        name, ref.hyps.margin, dev.hyps.margin, list(map(int, dev.hyps.count[:12])), [(x.returned, x.hyp_index, x.no_more) for x in dev.calls]))
    assert c.reach(c.problem, ref), "the case does not get where its label says"
    assert c.reach(c.problem, dev)
    assert ref.hyps.margin >= SC.MARGIN_MIN and dev.hyps.margin >= SC.MARGIN_MIN


@pytest.mark.parametrize("name", SC.SCENE_NAMES)
def test_seeded_scene_reaches_its_claim(name):
    c = SC.case_by_name(name)
    for mode in ("reference", "device"):
        r = SC.expected(c, mode)
        assert c.reach(c.problem, r)
        tail = len(c.problem.X1) % 64
        if tail:
            assert not (r.hyps.bits[:, -1] >> np.uint64(tail)).any()


@pytest.mark.parametrize("name", SC.NAMES)
def test_both_modes_decide_alike(name):
    c = SC.case_by_name(name)
    assert SC.same_decisions(SC.expected(c, "reference"), SC.expected(c, "device"))


def test_eps_mode_is_what_the_constant_says():
    worst, at = 0.0, None
    for c in SC.constructed():
        a, b = SC.expected(c, "reference").hyps.hyp, SC.expected(c, "device").hyps.hyp
        assert np.array_equal(np.isnan(a), np.isnan(b)), c.name
        fin = np.isfinite(a) & np.isfinite(b)
        d = float(np.max(np.abs(a[fin].astype(np.float64) - b[fin]))) if fin.any() else 0.0
        if d > worst:
            worst, at = d, c.name
    print("eps_mode measured %.3e (at %s), recorded %.3e" % (worst, at, SC.EPS_MODE))
    assert worst <= SC.EPS_MODE, "the recorded EPS_MODE understates the difference between the modes"
    assert SC.EPS_MODE <= 2 * worst, "the recorded EPS_MODE is looser than the measurement supports"
    assert SC.MARGIN_MIN >= 10 * 520 * SC.EPS_MODE   # the derivation in the module


@pytest.mark.parametrize("wrong", SC.WRONG_FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(wrong):
    moved = [c.name for c in SC.cases() if not SC.same_result(SC.expected(c, "reference"), SC.expected(c, "reference", wrong))]
    listed = [c.name for c in SC.cases() if wrong in c.moved_by]
    assert moved == listed
    if wrong != "niter_no_n_rule":   # (SC.MOVED_BY says why that one cannot move a case)
        assert any(n in SC.NAMES or wrong == "sample_replace" for n in moved), "no constructed case tells this wrong form from the restatement"


def test_max_its_table():
    """SetRansacParameters' arithmetic on the table the host program is held to as well"""
    for N, m, p, mx, want in SC.MAX_ITS_TABLE:
        assert SC.ransac_max_its(N, p, m, mx) == want, (N, m, p, mx)
    assert SC.ransac_max_its(12, 0.99, 12, 300, "niter_no_n_rule") == 1


def test_draws_are_without_replacement_and_in_the_reference_order():
    g = SC.Lcg(7)
    tri = SC.draw_triples(5, 200, g.random_int)
    assert all(len(set(t)) == 3 for t in tri.tolist()) and tri.min() == 0 and tri.max() == 4
    assert any(len(set(t)) < 3 for t in SC.draw_triples(5, 200, SC.Lcg(7).random_int, "sample_replace").tolist())
    # the swap-with-back: a scripted RandomInt that always answers 0 draws index 0, then the former back, then the new back
    assert SC.draw_triples(6, 1, lambda lo, hi: 0).tolist() == [[0, 5, 4]]
    assert SC.draw_triples(6, 1, lambda lo, hi: hi).tolist() == [[5, 4, 3]]
