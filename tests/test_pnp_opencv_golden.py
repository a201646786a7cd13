"""The fixed linear algebra of PnPsolver (csrc/pnp_math.h as tests/pnp_cases.py restates it: cvMulTransposed, cvSVD, cvSolve and
cvInvert(CV_SVD)) against OpenCV itself, through the fixture tools/make_golden_pnp_opencv.py writes on a machine that has cv2.  Until that
fixture exists the four routines are pinned to nothing but their restatement and this test skips.

The comparison is not bit for bit: another hypot, another summation order or a contracted product moves the last bits, and on the rank-8
MtM of four correspondences the whole basis of the null space.  The tool records, per kind of result, the largest deviation it found over
the well-conditioned matrices; the bound here is BOUND_FACTOR times that, for the well-conditioned matrices only, and the null space of MtM
is compared as a subspace."""
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "pnp_opencv.npz")
BOUND_FACTOR = 4.0   # (a small multiple of the recorded deviation: the cases may grow by a hypothesis without the fixture being recorded again)

pytestmark = pytest.mark.skipif(not os.path.exists(FIXTURE), reason="tests/golden/pnp_opencv.npz has not been produced yet (needs cv2: tools/make_golden_pnp_opencv.py)")


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_pnp_opencv", os.path.join(ROOT, "tools", "make_golden_pnp_opencv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixed_linear_algebra_within_the_recorded_deviation():
    mk = _tool()
    g = np.load(FIXTURE)
    bound = {str(k): BOUND_FACTOR * float(v) for k, v in zip(g["kinds"], g["max_deviation"])}
    assert bound and max(bound.values()) < 1e-6, "the recorded deviations are those of two double-precision SVDs of the same matrix"
    seen = 0
    for name, h, P, sub, m in mk.subsets():
        key = "%s/%d" % (name, h)
        assert key + "/mtm_w" in g.files, "the fixture is older than the case list: run tools/make_golden_pnp_opencv.py again"
        a = mk.ours(m)
        b = dict(mtm_w=g[key + "/mtm_w"], mtm_null=g[key + "/mtm_null"], pw0_w=g[key + "/pw0_w"], cc_inv=g[key + "/cc_inv"], rot=g[key + "/rot"],
                 betas=[g[key + "/betas%d" % j] for j in range(3)], mtm=np.diag(g[key + "/mtm_diag"]))
        a["mtm"] = np.diag(np.diag(a["mtm"]))
        for kind, v in mk.deviations(m, a, b).items():
            assert v <= bound[kind], (key, kind, v, bound[kind])
        seen += 1
    assert seen > 50
