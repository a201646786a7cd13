"""host/LocalMappingTriangulate.{h,cc} -- ygz::TriangulatePairsDevice and ygz::CreateNewMapPointsBatch, what a user forwards the neighbour loop of
LocalMapping::CreateNewMapPoints to -- reads members of the reference's own KeyFrame, MapPoint and Map: no reference binary is built from it here,
so it gets a compile check against the reference's headers -- the real include/MapPoint.h and the stand-in KeyFrame / Map of oracle/ref_shim, with
the four members that stand-in lacks declared by tests/cpp/tri_compile_prefix.h; the flags are those of tests/test_optimizer_sim3_compiles.py --
and one against the stand-alone classes the GPU test builds it with.  The first is skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

REF = os.environ.get("REF", "/root/reference")
HOST = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "LocalMapping.cc")), reason="reference checkout absent")
def test_compiles_against_the_reference_headers():
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    flags = "-O2 -std=c++14 -msse4.2 -pthread -w -ffp-contract=off -DYGZ_REF_TRACKING -DYGZ_REF_MATCHER -DYGZ_REF_MAPPOINT -DYGZ_REF_FRAME -DYGZ_BOUNDARY_BUILD -DYGZ_REAL_DBOW2 -DYGZF_WITH_REFERENCE_HEADERS".split()
    inc = ["-I" + os.path.join(shim, "tracking"), "-I" + shim, "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(REF, "include"), "-I" + REF, "-I" + HOST,
           "-include", os.path.join(ROOT, "tests", "cpp", "tri_compile_prefix.h"),   # first: it reads the stand-in KeyFrame's header once, widened
           "-include", os.path.join(shim, "dbow2_stubs.h"), "-include", os.path.join(HOST, "ORBextractor.h"), "-include", os.path.join(shim, "tracking", "tracking_stubs.h")]
    r = subprocess.run(["g++"] + flags + inc + ["-fsyntax-only", os.path.join(HOST, "LocalMappingTriangulate.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_compiles_against_the_standalone_classes():
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I", HOST, "-I", os.path.join(HOST, "standalone"),
                        "-I", os.path.join(ROOT, "tests", "cpp"), "-fsyntax-only", os.path.join(HOST, "LocalMappingTriangulate.cc"),
                        os.path.join(ROOT, "tests", "cpp", "tri_shell.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_threshold_default_is_the_measured_crossover():
    """the default of YGZF_TRI_DEVICE_MIN is the 64 that profiles/triangulate_rate.txt arrives at, and the source cites the file"""
    src = open(os.path.join(HOST, "LocalMappingTriangulate.cc")).read()
    prof = open(os.path.join(ROOT, "profiles", "triangulate_rate.txt")).read()
    assert "return 64;   // profiles/triangulate_rate.txt" in src
    assert "below 64 pairs per call (YGZF_TRI_DEVICE_MIN)" in prof
