"""host/OptimizerSim3.{h,cc} -- ygz::OptimizeSim3Device / OptimizeSim3Batch, what a user forwards Optimizer::OptimizeSim3 to
(src/Optimizer.cc:2409-2594) -- reads members of the reference's own KeyFrame and MapPoint: no reference binary is built from it here, so it
gets a compile check against the reference's headers -- the real include/KeyFrame.h and include/MapPoint.h -- over the stand-in OpenCV
(oracle/ref_shim), with the flags of tests/test_optimizer_pose_compiles.py, and one against the stand-alone classes and the stand-in Sim3 type
the GPU test builds it with.  The first is skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

REF = os.environ.get("REF", "/root/reference")
HOST = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "Optimizer.cc")), reason="reference checkout absent")
def test_compiles_against_the_reference_headers():
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = "-O2 -std=c++14 -msse4.2 -pthread -w -ffp-contract=off -DYGZ_REF_TRACKING -DYGZ_REF_MATCHER -DYGZ_REF_MAPPOINT -DYGZ_REF_FRAME -DYGZ_BOUNDARY_BUILD -DYGZ_REAL_DBOW2 -DYGZF_WITH_REFERENCE_HEADERS".split()
    inc = ["-I" + os.path.join(shim, "tracking"), "-I" + shim, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(REF, "include"), "-I" + REF, "-I" + HOST,
           "-include", os.path.join(shim, "dbow2_stubs.h"), "-include", os.path.join(HOST, "ORBextractor.h"), "-include", os.path.join(shim, "tracking", "tracking_stubs.h")]
    r = subprocess.run(["g++"] + flags + inc + ["-fsyntax-only", os.path.join(HOST, "OptimizerSim3.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_compiles_against_the_standalone_classes():
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I", HOST, "-I", os.path.join(HOST, "standalone"), "-fsyntax-only",
                        os.path.join(HOST, "OptimizerSim3.cc"), os.path.join(ROOT, "tests", "cpp", "sim3_opt_shell.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
