"""host/FrameUndistort.cc -- ygz::Frame::ComputeImagePyramid (src/Frame.cc:773-814) with its undistortion on the device -- is a strong definition
for the reference tree: no reference binary is built from it here, so it gets a compile check against the reference's own headers over the
stand-in OpenCV (oracle/ref_shim), with the flags of oracle/build_boundary.sh.  Skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

REF = os.environ.get("REF", "/root/reference")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "Frame.cc")), reason="reference checkout absent")
@pytest.mark.parametrize("src", ["FrameUndistort.cc", "ORBextractor.cc"])
def test_compiles_against_the_reference_headers(src):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = "-O2 -std=c++14 -msse4.2 -pthread -w -ffp-contract=off -DYGZ_REF_TRACKING -DYGZ_REF_MATCHER -DYGZ_REF_FRAME -DYGZ_BOUNDARY_BUILD -DYGZ_REAL_DBOW2 -DYGZF_WITH_REFERENCE_HEADERS".split()
    inc = ["-I" + os.path.join(shim, "tracking"), "-I" + shim, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(REF, "include"), "-I" + REF, "-I" + host,
           "-include", os.path.join(shim, "dbow2_stubs.h"), "-include", os.path.join(host, "ORBextractor.h"), "-include", os.path.join(shim, "tracking", "tracking_stubs.h")]
    r = subprocess.run(["g++"] + flags + inc + ["-fsyntax-only", os.path.join(host, src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
