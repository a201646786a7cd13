"""tests/pnp_cases.py against itself (CPU): every constructed case reaches what it claims; each wrong form moves exactly the cases MOVES lists
for it, and every case is moved by the forms it was built for; the fixed linear algebra against numpy's (as a decomposition, not bit for
bit); EPnP recovers a known pose; the draws; SetRansacParameters on values worked out by hand."""
import math

import numpy as np
import pytest

from tests import pnp_cases as PC


@pytest.mark.parametrize("name", PC.NAMES)
def test_case_reaches_its_claim(name):
    c = PC.case_by_name(name)
    assert c.reach(), name
    want = PC.expected(c)
    assert len(want.calls) == len(c.problem.calls)
    assert len(c.problem.samples) >= max([k.iterations for k in want.calls] + [0]), "the case needs a sample set for every iteration its calls reach"


def test_names_are_the_cases():
    assert [c.name for c in PC.constructed()] == PC.NAMES and set(PC.MOVES) == set(PC.WRONG)


@pytest.mark.parametrize("form", PC.WRONG)
def test_wrong_form_moves_exactly_its_cases(form):
    got = tuple(c.name for c in PC.constructed() if PC.moved(c, form))
    assert got == PC.MOVES[form]
    for c in PC.constructed():
        assert form not in c.moved_by or c.name in got, "%s was built for %s" % (c.name, form)


def test_every_order_dependent_form_has_a_case():
    for form in PC.WRONG:
        if form not in ("draw_replace", "reperr_le"):   # (see the finding above MOVES)
            assert PC.MOVES[form], form


def test_scenes_have_records_and_outliers():
    for name in PC.SCENE_NAMES:
        c = PC.scene(name)
        h = PC.pnp_hypotheses(c.problem)
        n = len(c.problem.P3D)
        assert 60 <= n <= 150 and (h.refined_n >= 0).sum() >= 2, name
        assert 0.45 * n <= h.refined_n.max() <= 0.75 * n, "30 - 50 % of the correspondences are outliers"
        assert PC.same_calls(PC.pnp_iterate(c.problem), PC.expected(c).calls)


def test_jacobi_svd_is_a_decomposition():
    rng = np.random.default_rng(1)
    for m, n in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        A = rng.normal(size=(m, n))
        if m == 12:
            A = A[:8].T @ A[:8]   # rank 8, as MtM of four correspondences
        At, W, Vt = PC.jacobi_svd([list(r) for r in A.T])
        U, W, Vt = np.array(At).T, np.array(W), np.array(Vt)
        assert np.all(np.diff(W) <= 0) and np.allclose(W, np.linalg.svd(A, compute_uv=False), atol=1e-12 * W[0])
        assert np.allclose(Vt @ Vt.T, np.eye(n), atol=1e-13)
        live = W > 1e-10 * W[0]
        assert np.allclose((U[:, live] * W[live]) @ Vt[live], A, atol=1e-12 * W[0])
        assert np.allclose(U.T @ U, np.eye(n), atol=1e-6)   # the null rows are normalised rounding residue: orthogonal to the rest, coarsely
        if m == 12:
            assert np.abs(A @ U[:, ~live]).max() < 1e-12 * W[0], "rows 8 .. 11 span the null space"


def test_solve_invert_multiply_and_qr():
    rng = np.random.default_rng(2)
    A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
    ls = np.linalg.lstsq(A, b, rcond=None)[0]
    assert np.allclose(PC.solve_svd([list(r) for r in A], list(b)), ls, atol=1e-12)
    x = [0.0] * 4
    assert PC.qr_solve([list(r) for r in A], list(b), x) and np.allclose(x, ls, atol=1e-12)
    B = rng.normal(size=(3, 3))
    assert np.allclose(PC.invert_svd([list(r) for r in B]), np.linalg.inv(B), atol=1e-11)
    assert np.allclose(PC.mul_transposed([list(r) for r in A]), A.T @ A, atol=1e-13)
    # a singular column: x stays what it was; a rank-deficient solve passes over the small singular value
    A0 = A.copy()
    A0[:, 0] = 0
    x = [7.0] * 4
    assert not PC.qr_solve([list(r) for r in A0], list(b), x) and x == [7.0] * 4
    A1 = A.copy()
    A1[:, 3] = A1[:, 2]
    assert np.allclose(PC.solve_svd([list(r) for r in A1], list(b)), np.linalg.pinv(A1) @ b, atol=1e-10)
    # the pivot search of qr_solve never reads the last row
    A2 = np.zeros((6, 4))
    A2[5, 0] = 1.0
    assert not PC.qr_solve([list(r) for r in A2], list(b), [0.0] * 4)


def test_epnp_recovers_a_pose():
    rng = np.random.default_rng(3)
    X, uv, (R, t) = PC._scene(rng, 30, 0, noise=0.0)
    P = PC._problem("recover", X, uv, PC._gates(rng, 30), PC._sets_from(rng, 30, 1), 10, 1, (1,))
    hyp, info = PC.compute_pose(P, tuple(range(30)))
    assert np.allclose(hyp[:9].reshape(3, 3), R, atol=1e-4) and np.allclose(hyp[9:], t, atol=1e-3)
    assert PC.check_inliers(P, hyp).all()
    assert np.allclose(np.linalg.det(hyp[:9].reshape(3, 3)), 1, atol=1e-9)


def test_draws():
    script = iter([2, 0, 1, 0, 4, 3, 0, 0])
    got = PC.draw_quads(5, 4, 2, lambda lo, hi: next(script))
    # [0 1 2 3 4] -> 2, back 4 into its place: [0 1 4 3] -> 0: [3 1 4] -> 1: [3 4] -> 3;  then 4: [0 1 2 3] -> 3: [0 1 2] -> 0: [2 1] -> 2
    assert got.tolist() == [[2, 0, 1, 3], [4, 3, 0, 2]]
    for n, ms, seed in ((4, 4, 1), (5, 5, 2), (20, 4, 3), (150, 4, 4), (9, 8, 5)):
        a = PC.draw_quads(n, ms, 50, PC.Lcg(seed).random_int)
        assert a.shape == (50, ms) and all(len(set(r)) == ms for r in a.tolist()) and a.min() >= 0 and a.max() < n
        b = PC.draw_quads(n, ms, 50, PC.Lcg(seed).random_int, frozenset(["draw_replace"]))
        assert not np.array_equal(a, b) or n == ms == 1
    assert any(len(set(r)) < 4 for r in PC.draw_quads(5, 4, 50, PC.Lcg(6).random_int, frozenset(["draw_replace"])).tolist())
    assert PC.draw_quads(3, 4, 5, PC.Lcg(1).random_int).shape == (0, 4)


def test_ransac_parameters():
    # the tracker's call: N = 500 -> nMinInliers = 250, epsilon 0.5, ceil(log(0.01) / log(1 - 0.125)) = 35
    assert PC.ransac_parameters(500, 0.99, 10, 300, 4, 0.5) == (250, math.ceil(math.log(0.01) / math.log(0.875)))
    assert PC.ransac_parameters(500, 0.99, 10, 300, 4, 0.5)[1] == 35
    assert PC.ransac_parameters(10, 0.99, 10, 300, 4, 0.5) == (10, 1)      # minInliers == N: one iteration
    assert PC.ransac_parameters(3, 0.99, 10, 300, 4, 0.5) == (10, 300)      # N < minInliers: the logarithm of a negative number
    assert PC.ransac_parameters(50, 0.99, 2, 300, 4, 0.01) == (4, 300)      # raised to minSet; epsilon 0.08: thousands of iterations, capped
    assert PC.ransac_parameters(11, 0.99, 10, 300, 4, 0.5)[0] == 10
