"""tests/pnp_cases.py against tests/golden/pnp_ref.npz, the record of what the REFERENCE's own compiled src/PnPsolver.cc returns from every
iterate / find call of every case (tools/make_golden_pnp_ref.py): whether a matrix came back, the matrix bit for bit, nInliers, bNoMore,
vbInliers with its size, mnIterations and mnBestInliers.  The reference ran over this project's fixed cvSVD / cvSolve / cvInvert /
cvMulTransposed (csrc/pnp_math.h), so this pins the reference's EPnP and RANSAC logic and roundings over that linear algebra -- the order of
every sum in fill_M, compute_L_6x10, gauss_newton, qr_solve, estimate_R_and_t, the mixed widths of CheckInliers, the `||` loop, Refine on the
best set, the gates -- and not the linear algebra itself, which is pinned to nothing but its restatement."""
import os

import numpy as np
import pytest

from tests import pnp_cases as PC
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "pnp_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_record_covers_the_cases(golden):
    assert list(golden["names"]) == PC.NAMES + PC.SCENE_NAMES
    assert os.path.getsize(GOLDEN) < 270 * 1024


@pytest.mark.parametrize("name", PC.NAMES + PC.SCENE_NAMES)
def test_restatement_equals_the_reference(golden, name):
    c = PC.case_by_name(name)
    want = PC.expected(c).calls
    meta, T, sizes = golden[name + "/meta"], golden[name + "/T"], golden[name + "/sizes"]
    inl = np.unpackbits(golden[name + "/inliers"])[:int(sizes.sum())]
    assert len(meta) == len(want)
    pos = 0
    for j, (w, m) in enumerate(zip(want, meta)):
        returned, n_inl, no_more, size, iterations, best = (int(v) for v in m)
        got = inl[pos:pos + size]
        pos += size
        assert (bool(returned), n_inl, size) == (w.kind != PC.EMPTY, w.n_inliers, len(w.inliers)), (name, j)
        assert c.problem.calls[j] < 0 or bool(no_more) == bool(w.no_more), (name, j)
        assert (iterations, best) == (w.iterations, w.best_inliers), (name, j)
        assert np.array_equal(got, w.inliers), (name, j)
        if returned:
            nan = np.isnan(w.T).reshape(-1)
            assert np.array_equal(np.isnan(T[j]), nan) and np.array_equal(T[j].view(np.uint32)[~nan], w.T.reshape(-1).view(np.uint32)[~nan]), (name, j)
