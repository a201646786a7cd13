#!/usr/bin/env python3
"""Pins the restatement of cv::remap's fixed-point bilinear path (tests/remap_cases.py; src/Frame.cc:775-805) to a real OpenCV.

Run on a machine that has cv2:  python tools/make_golden_remap_opencv.py  ->  tests/golden/remap_opencv.npz
For every constructed case: cv2.remap(src, map_xy, map_tab, cv2.INTER_LINEAR) (BORDER_CONSTANT, value 0: the defaults) -- the image itself for the
small cases, the CRC-32 of every row for the two 752 x 480 ones (the fixture stays far below the size limit for committed files).
tests/test_remap_opencv_golden.py holds the restatement to it and skips while the fixture is absent."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import remap_cases as R  # noqa: E402

FULL_IMAGE_MAX = 96 * 96


def row_crcs(img):
    return np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in img], np.uint32)


def main():
    import cv2                                      # (no fallback: without OpenCV there is nothing to pin against)
    out = {"opencv_version": np.array(cv2.__version__)}
    for c in R.CASES:
        dst = cv2.remap(c.src, c.map_xy, c.map_tab, cv2.INTER_LINEAR)
        assert dst.dtype == np.uint8 and dst.shape == c.map_tab.shape
        out[c.name] = dst if dst.size <= FULL_IMAGE_MAX else row_crcs(dst)
        print("%-28s %s" % (c.name, "equal to the restatement" if np.array_equal(dst, R.expected(c)) else "DIFFERS from the restatement"))
    path = os.path.join(ROOT, "tests", "golden", "remap_opencv.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, OpenCV %s)" % (path, os.path.getsize(path), cv2.__version__))


if __name__ == "__main__":
    main()
