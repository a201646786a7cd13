"""host/PnPsolver.cc -- ygz::PnPsolver and ygz::PnPsolverBatch, what takes the place of src/PnPsolver.cc -- reads members of the reference's
own Frame and MapPoint: no reference binary is built from it here, so it gets a compile check against the reference's headers -- the real
include/Frame.h and include/MapPoint.h, with host/standalone/PnPsolver.h in the place of include/PnPsolver.h as INTEGRATION.md prescribes --
over the stand-in OpenCV (oracle/ref_shim), with the flags of oracle/build_boundary.sh, and one against the stand-alone classes the GPU test
builds it with.  The first is skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

REF = os.environ.get("REF", "/root/reference")
HOST = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "PnPsolver.cc")), reason="reference checkout absent")
def test_compiles_against_the_reference_headers():
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = "-O2 -std=c++14 -msse4.2 -pthread -w -ffp-contract=off -DYGZ_REF_TRACKING -DYGZ_REF_MATCHER -DYGZ_REF_MAPPOINT -DYGZ_REF_FRAME -DYGZ_BOUNDARY_BUILD -DYGZ_REAL_DBOW2 -DYGZF_WITH_REFERENCE_HEADERS".split()
    inc = ["-I" + os.path.join(shim, "tracking"), "-I" + shim, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(REF, "include"), "-I" + REF,
           "-I" + HOST, "-include", os.path.join(shim, "dbow2_stubs.h"), "-include", os.path.join(HOST, "ORBextractor.h"), "-include", os.path.join(ROOT, "tests", "cpp", "pnp_compile_prefix.h"),
           "-include", os.path.join(HOST, "standalone", "PnPsolver.h")]   # in the place of include/PnPsolver.h: the same include guard
    r = subprocess.run(["g++"] + flags + inc + ["-fsyntax-only", os.path.join(HOST, "PnPsolver.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_compiles_against_the_standalone_classes():
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I", HOST, "-I", os.path.join(HOST, "standalone"), "-fsyntax-only",
                        os.path.join(HOST, "PnPsolver.cc"), os.path.join(ROOT, "tests", "cpp", "pnp_shell.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_include_guard_is_the_reference_s():
    text = open(os.path.join(HOST, "standalone", "PnPsolver.h")).read()
    assert "#ifndef YGZ_PNPSOLVER_H_" in text and "#define YGZ_PNPSOLVER_H_" in text
