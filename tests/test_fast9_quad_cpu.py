"""The arithmetic of fast9_quad -- saturated thresholds in the high byte of each 16-bit half, the v_lerp_u8 comparison and the 32-operation arc
network per polarity (orb_ygz_slam_amd/csrc/fast9_quad.h) -- is written over four primitives that are the gfx950 builtins on the device and plain
C++ restatements of those instructions on the host.  The host form is compiled here with AddressSanitizer and UBSan into a stand-alone program
(tests/cpp/fast9_quad_cpu.hip) that checks
  the arc network   on every 16-bit ring mask, both polarities, in every byte lane, with random don't-care bits, against "nine contiguous of the
                    circular sixteen";
  the thresholds    on every centre x every ring value x t in {0, 1, 5, 7, 20, 40, 127, 128, 130, 254, 255} x every byte position:
                    bright <=> ring > c + t, not dark <=> ring >= c - t;
  the whole         on 10^5 random quads of full-range values and 10^5 of values from {0, 3, 252, 255} against the scalar FAST 9/16 rule.
A fresh process, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    out = str(tmp_path_factory.mktemp("fast9_quad") / "fast9_quad_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "orb_ygz_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fast9_quad_cpu.hip"),
                           "-L", rocm_lib, "-lamdhip64", "-o", out])
    return out


def test_thresholds_arcs_and_whole_quads_agree_with_the_definitions(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fast9 quad ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
