"""The restatement of cv::remap (tests/remap_cases.py) against cv2.remap itself, through the fixture tools/make_golden_remap_opencv.py writes on
a machine that has OpenCV.  Until that fixture exists the primitive is unpinned and this test skips."""
import os
import zlib

import numpy as np
import pytest

from tests import remap_cases as R
from tests.conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "remap_opencv.npz")


@pytest.mark.skipif(not os.path.exists(FIXTURE), reason="tests/golden/remap_opencv.npz has not been produced yet (needs cv2: tools/make_golden_remap_opencv.py)")
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_restatement_equals_opencv(name):
    g = np.load(FIXTURE)
    assert name in g.files, "the fixture is older than the case list: run tools/make_golden_remap_opencv.py again"
    e = R.expected(R.case_by_name(name))
    want = g[name]
    if want.ndim == 2:
        assert np.array_equal(e, want)
    else:
        got = np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in e], np.uint32)
        assert np.array_equal(got, want), "rows %s differ" % np.flatnonzero(got != want)[:10]
