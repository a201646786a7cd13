"""CPU tier: the constructed cases of tests/pose_opt_cases.py are held to their claims on the numpy restatement of
Optimizer::PoseOptimization(Frame *) -- no device, no library.

Every case reaches what its label says and keeps its decision margin in both summation modes; each wrong form moves exactly the cases that list
it; the reference-order and the device-order sums take the same decisions everywhere; and the largest difference between the two modes' double
poses -- EPS_ORDER, what reordering alone does to the reference's algorithm -- is measured here and held against the recorded constant that the
GPU test's tolerance is built from.

The decision margin of a run is the smallest distance of any branch operand from its branch point, relative to the operand's own scale: raw chi2
against the gate (|chi2 - gate| / gate), the LDLT pivots against 0 (|d| / the largest diagonal entry), the two sides of the stop rule against
each other, and rho against 0 -- rho is a ratio already (the decrease over the predicted decrease + 1e-3; 1 for a step that does what the model
says), so its distance from 0 is |rho|.  Exact ties that every summation order reproduces are not decisions and are left out: an all-zero
system, an update that leaves the pose bit for bit where it was (rho == 0), non-finite operands."""
import numpy as np
import pytest

from tests import pose_opt_cases as PC

NAMES = [s[0] for s in PC.SPECS]


def test_the_case_list_covers_what_it_must():
    counts = {PC._count(c.problem) for c in PC.cases()}
    assert {2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 2049} <= counts
    assert len(NAMES) == len(set(NAMES)) and set(PC.MOVED_BY) == set(NAMES)
    assert sum(n.startswith("scene") for n in NAMES) >= 12
    for must in ("mono_only", "stereo_only", "interleaved", "round0_rejects", "readmitted", "side_change_23", "empty_round", "reject_then_accept", "nbad_stop",
                 "rho_zero", "behind_camera", "in_camera_plane", "octave0", "octave7", "far_pose"):
        assert must in NAMES


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_claim_with_margin(name):
    c = PC.case_by_name(name)
    ref, dev = PC.expected(c, "reference"), PC.expected(c, "device")
    print("%s: margin %.3e (reference order) %.3e (device order), ret %d of %d, iterations %s trials %s stop %s" % (
        name, ref.margin, dev.margin, ref.ret, PC._count(c.problem), ref.iters, ref.trials, ref.stop))
    assert c.reach(c.problem, ref), "the case does not get where its label says"
    assert c.reach(c.problem, dev)
    assert ref.margin >= PC.MARGIN_MIN and dev.margin >= PC.MARGIN_MIN


@pytest.mark.parametrize("name", NAMES)
def test_both_summation_orders_take_the_same_decisions(name):
    c = PC.case_by_name(name)
    ref, dev = PC.expected(c, "reference"), PC.expected(c, "device")
    assert np.array_equal(ref.outlier, dev.outlier) and ref.ret == dev.ret
    assert (ref.iters, ref.trials, ref.stop) == (dev.iters, dev.trials, dev.stop)
    assert np.max(np.abs(ref.Tcw.view(np.int32).astype(np.int64) - dev.Tcw.view(np.int32).astype(np.int64))) <= 1


def test_eps_order_is_what_the_constant_says():
    """the tolerance measurement: max over all cases of the two modes' double-pose difference"""
    worst, at = 0.0, None
    for c in PC.cases():
        d = PC.pose_diff(PC.expected(c, "reference").Tcw64, PC.expected(c, "device").Tcw64)
        if d > worst:
            worst, at = d, c.name
    print("eps_order measured %.3e (at %s), recorded %.3e" % (worst, at, PC.EPS_ORDER))
    assert worst <= PC.EPS_ORDER, "the recorded EPS_ORDER understates the reordering error"
    assert worst >= PC.EPS_ORDER / 4, "the recorded EPS_ORDER is looser than the measurement supports"


@pytest.mark.parametrize("wrong", PC.WRONG_FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(wrong):
    moved = []
    for c in PC.cases():
        if not PC.same_result(PC.expected(c, "reference"), PC.pose_opt(c.problem, "reference", wrong)):
            moved.append(c.name)
    listed = [c.name for c in PC.cases() if wrong in c.moved_by]
    assert moved == listed
    if wrong != "gate_robust":   # (PC.MOVED_BY says why that one cannot move a case that keeps its margin)
        assert moved, "no case tells this wrong form from the restatement"


def test_non_correspondences_and_early_return_leave_their_marks():
    c = PC.case_by_name("n2")
    r = PC.expected(c)
    P = c.problem
    valid = np.asarray(P.mp_valid).astype(bool)
    assert r.ret == 0 and not r.outlier[valid].any() and np.array_equal(r.outlier[~valid], np.asarray(P.outlier_in)[~valid])
    assert np.array_equal(r.Tcw, np.asarray(P.Tcw, np.float32)) and abs(float(np.linalg.norm(r.Tcw[:4])) - 1) > 5e-4   # verbatim: not normalised


def test_ldlt_solves_and_refuses():
    rs = np.random.RandomState(3)
    for _ in range(20):
        A = rs.normal(size=(6, 6))
        H = A @ A.T + np.diag(rs.uniform(0, 3, 6))
        b = rs.normal(size=6)
        ok, m, tr, piv = PC.ldlt(H)
        assert ok and np.allclose(PC.ldlt_solve(m, tr, b), np.linalg.solve(H, b), rtol=1e-9, atol=1e-12)
        assert sorted(piv, reverse=True)[0] == piv[0] == np.max(np.diag(H))
    with np.errstate(all="ignore"):
        assert not PC.ldlt(np.zeros((6, 6)))[0]
        assert not PC.ldlt(np.diag([1.0, 2.0, -1.0, 3.0, 1.0, 1.0]))[0]


def test_se3_exp_agrees_with_the_oracles_float_exp(oracle):
    """a sanity check, not a pin: the restatement's fp64 SE3d::exp against the oracle's float exp, to float precision"""
    rs = np.random.RandomState(11)
    for k in range(50):
        a = np.concatenate([rs.uniform(-2, 2, 3), rs.uniform(-1, 1, 3) * (1e-7 if k % 10 == 0 else 1.0)])
        q, t = PC.se3_exp(a)
        f = oracle.se3_exp(a.astype(np.float32))
        assert PC.pose_diff(np.concatenate([q, t]), f.astype(np.float64)) < 2e-6
