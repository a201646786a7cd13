"""tests/triangulate_cases.py held to its own claims, on the CPU: every constructed case reaches the exit and the source of x3D it names, with
the margin recorded there; every wrong form moves exactly the cases that list it; the fixed JacobiSVD is an SVD; the sweep cap is far away."""
import numpy as np
import pytest

from tests import triangulate_cases as TC

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_reaches_what_it_claims(name):
    c = TC.case_by_name(name)
    p = TC.expected(c)
    assert (p.status, p.source) == (c.spec.status, c.spec.source)
    for gate in c.spec.exact:
        assert gate in p.margins, "the case names gate %s as met exactly and never gets there" % gate
    assert TC.margin(c) >= TC.MARGIN_MIN, p.margins


def test_every_exit_and_every_source_is_reached():
    got = {(TC.expected(c).status, TC.expected(c).source) for c in TC.cases()}
    assert {s for s, _ in got} == set(range(TC.SWEEP_CAP))   # the cap is a deviation no input of the suite reaches: see test_sweep_cap_*
    assert {f for _, f in got} == {TC.FROM_NONE, TC.FROM_SVD, TC.FROM_KF1, TC.FROM_KF2}
    for s in (TC.ACCEPTED, TC.Z1, TC.Z2, TC.REPROJ1, TC.REPROJ2, TC.ZERO_DIST, TC.SCALE_RATIO):   # the exits behind the triangulation, from an unprojection too
        assert any(st == s and f in (TC.FROM_KF1, TC.FROM_KF2) for st, f in got), s


def test_the_gates_met_with_equality_are_met_with_equality():
    """the cases whose names end in _equal / _zero sit on their gate exactly, and their partners one float outside it"""
    for name, gate in (("chi2_mono1_equal", "chi2_mono1"), ("chi2_stereo1_equal", "chi2_stereo1"), ("chi2_mono2_equal", "chi2_mono2"),
                       ("chi2_stereo2_equal", "chi2_stereo2"), ("z1_zero", "z1"), ("z2_zero", "z2"), ("zero_dist1", "dist"), ("zero_dist2", "dist"),
                       ("cos_zero", "cos_positive"), ("ratio_low_equal", "ratio_low"), ("ratio_high_equal", "ratio_high")):
        assert TC.expected(TC.case_by_name(name)).margins[gate] == 0, name
    for name, gate in (("chi2_mono1_outside", "chi2_mono1"), ("chi2_stereo1_outside", "chi2_stereo1"), ("chi2_mono2_outside", "chi2_mono2"),
                       ("chi2_stereo2_outside", "chi2_stereo2"), ("z1_one_float", "z1"), ("z2_one_float", "z2"), ("ratio_low_outside", "ratio_low"),
                       ("ratio_high_outside", "ratio_high"), ("cos_one_float_above_zero", "cos_positive")):
        assert 0 < TC.expected(TC.case_by_name(name)).margins[gate] < 1e-6, name
    lo, hi = (TC.expected(TC.case_by_name(n)).cos_rays for n in ("mono_cos_below_9998", "mono_cos_above_9998"))
    assert f64(lo) < 0.9998 < f64(hi) and np.nextafter(lo, f32(2)) == hi   # the two floats around the double 0.9998


@pytest.mark.parametrize("wrong", TC.WRONG_FORMS)
def test_wrong_form_moves_exactly_the_cases_that_list_it(wrong):
    moved = [c.name for c in TC.cases() if not TC.same_pair(TC.expected(c), TC.expected(c, wrong))]
    assert moved == [c.name for c in TC.cases() if wrong in c.spec.moved_by]
    assert moved, "no case shows this rule"


def test_every_listed_form_exists():
    for c in TC.cases():
        assert set(c.spec.moved_by) <= set(TC.WRONG_FORMS), c.name
    for s in TC.SVD_SPECS:
        assert set(s.moved_by) <= set(TC.WRONG_FORMS), s.name


def _same_svd(a, b):
    return a.sweeps == b.sweeps and np.array_equal(a.V.view(np.uint32), b.V.view(np.uint32)) and np.array_equal(a.sv.view(np.uint32), b.sv.view(np.uint32))


@pytest.mark.parametrize("name", TC.SVD_NAMES)
def test_svd_case(name):
    s = TC.svd_case(name)
    A = s.make()
    r = TC.jacobi_svd4(A)
    if s.sweeps is not None:
        assert r.sweeps == s.sweeps
    moved = tuple(w for w in TC.WRONG_FORMS if not _same_svd(r, TC.jacobi_svd4(A, w)))
    assert sorted(moved) == sorted(s.moved_by)


def _svd_matrices():
    out = [(s.name, s.make()) for s in TC.SVD_SPECS]
    out += [(c.name, np.array(TC.expected(c).A, f32)) for c in TC.cases() if TC.expected(c).A is not None]
    for sc in TC.SCENE_NAMES:
        out += [("%s[%d]" % (sc, i), np.array(p.A, f32)) for i, p in enumerate(TC.scene_expected(sc)) if p.A is not None]
    return out


def test_the_restatement_is_an_svd():
    """V is orthogonal, the values descend and are those of numpy's fp64 SVD, and A v is minimal for the last column.  The tolerance is not
    tuned: a sweep is 6 plane rotations, each a handful of fp32 operations per entry, so one rotation perturbs the matrix by at most about
    4 eps ||A|| and the orthogonality of V by 4 eps; the suite's matrices take at most 4 sweeps = 24 rotations (test_sweep_cap_is_far_away),
    the scaling by the largest entry adds one rounding: 128 eps leaves the bound of 24 * 4 + 1 a third to spare."""
    eps = f64(np.finfo(f32).eps)
    for name, A in _svd_matrices():
        r = TC.jacobi_svd4(A)
        A64, V = A.astype(f64), r.V.astype(f64)
        norm = np.linalg.norm(A64)
        assert np.abs(V.T @ V - np.eye(4)).max() <= 128 * eps, name
        assert (np.diff(r.sv) <= 0).all(), name
        ref = np.linalg.svd(A64, compute_uv=False)
        assert np.abs(r.sv.astype(f64) - ref).max() <= 128 * eps * max(norm, np.finfo(f32).tiny), name
        assert np.linalg.norm(A64 @ V[:, 3]) <= ref[3] + 128 * eps * norm, name


def test_sweep_cap_is_far_away():
    """the largest sweep count over every constructed case, svd case and seeded scene (DESIGN.md records it) stays below half the cap"""
    met = TC.max_sweeps_met()
    assert met == 4                      # the figure DESIGN.md states
    assert 2 * met < TC.MAX_SWEEPS


def test_sweep_cap_gets_its_own_status():
    """with the cap lowered to a count the suite's matrices need, the restatement reports exactly the cap and no more"""
    A = TC.most_sweeps_matrix()
    full = TC.jacobi_svd4(A)
    assert full.sweeps == TC.max_sweeps_met()
    assert TC.jacobi_svd4(A, max_sweeps=full.sweeps - 1).sweeps == full.sweeps - 1   # == its cap: the caller rejects the pair
    assert TC.jacobi_svd4(A, max_sweeps=full.sweeps).sweeps == full.sweeps


@pytest.mark.parametrize("name", TC.SCENE_NAMES)
def test_scene_is_a_scene(name):
    """a seeded scene accepts a good part of its pairs, rejects its mismatches, and takes every path worth the name"""
    ps = TC.scene_expected(name)
    assert len(ps) == TC.SCENE_PAIRS
    st = np.array([p.status for p in ps])
    assert (st == TC.ACCEPTED).sum() >= 100
    assert set(st) >= {TC.ACCEPTED, TC.LOW_PARALLAX, TC.Z1, TC.REPROJ1, TC.REPROJ2, TC.SCALE_RATIO}
    acc = np.array([p.x3d for p in ps if p.status == TC.ACCEPTED])
    assert np.isfinite(acc).all() and (acc[:, 2] > 0.5).all()
