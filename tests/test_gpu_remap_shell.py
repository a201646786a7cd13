"""GPU test of the undistortion behind the extractor shell (csrc/host/ORBextractor.h: SetUndistortMaps, ComputePyramidUndistorted, Undistort;
src/Frame.cc:775-813): tests/cpp/remap_shell.cc, built with g++ over the stand-alone classes as kf_store_shell.cc is, on two synthetic scenes seen
through the EuRoC map -- twice on one extractor."""
import os
import subprocess

import pytest

from tests import remap_cases as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "remap_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "remap_shell.cc")] + [os.path.join(host, f) for f in ("ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_remap_shell_end_to_end(tmp_path):
    """ComputePyramidUndistorted + operator()(Frame *, ...) == the plain shell on the restated image: levels, keypoints, descriptors"""
    from orb_ygz_slam_amd import load_library
    from orb_ygz_slam_amd.synth import synth_frame
    load_library()
    exe = _build_shell(str(tmp_path))
    case = R.case_by_name("euroc_752x480")
    d = tmp_path / "data"
    d.mkdir()
    (d / "meta.txt").write_text("752 480 752 480 2\n")
    case.map_xy.tofile(str(d / "map_xy.bin"))
    case.map_tab.tofile(str(d / "map_tab.bin"))
    for k in range(2):
        raw = synth_frame(90 + k, 752, 480)
        raw.tofile(str(d / ("raw_%d.bin" % k)))
        R.remap_ref(raw, case.map_xy, case.map_tab).tofile(str(d / ("want_%d.bin" % k)))
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "remap shell ok" in out.stdout, out.stdout + out.stderr
