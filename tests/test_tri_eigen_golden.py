"""The fixed JacobiSVD of csrc/tri_math.h (restated in tests/triangulate_cases.py) against a compiled Eigen: tests/golden/tri_eigen.npz holds A, V and
x3D of every matrix of the suite as Eigen::JacobiSVD<Matrix4f> gives them, written by tools/make_golden_triangulate_eigen.cc on a machine that has
Eigen.  Skipped until that fixture exists (parity unpinned).  Equality is asked bit for bit: the text claims to be Eigen
3.3's algorithm operation by operation, and a build whose Eigen vectorises or contracts the rotations is a finding to write down, not to absorb
in a tolerance."""
import os

import numpy as np
import pytest

from tests import triangulate_cases as TC
from tests.conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "tri_eigen.npz")


@pytest.mark.skipif(not os.path.exists(FIXTURE), reason="tests/golden/tri_eigen.npz not recorded yet (tools/make_golden_triangulate_eigen.cc needs Eigen)")
def test_restatement_equals_compiled_eigen():
    z = np.load(FIXTURE)
    A = TC.svd_inputs()
    assert z["A"].shape == A.shape and np.array_equal(z["A"].view(np.uint32), A.view(np.uint32)), "the fixture was recorded for other matrices"
    print("Eigen %d.%d.%d, %d matrices" % (tuple(z["version"]) + (len(A),)))
    for k in range(len(A)):
        r = TC.jacobi_svd4(A[k])
        assert r.sweeps < TC.MAX_SWEEPS
        assert np.array_equal(r.V.view(np.uint32), z["V"][k].view(np.uint32)), "V of matrix %d differs from Eigen's" % k
        with np.errstate(all="ignore"):
            x = np.array([r.V[0][3] / r.V[3][3], r.V[1][3] / r.V[3][3], r.V[2][3] / r.V[3][3]], np.float32)
        nan = np.isnan(x)
        assert np.array_equal(np.isnan(z["x3D"][k]), nan) and np.array_equal(x.view(np.uint32)[~nan], z["x3D"][k].view(np.uint32)[~nan]), "x3D of matrix %d" % k
