"""The arithmetic of one sample of describe_window's column pass (orb_ygz_slam_amd/csrc/describe_sample.h, included by the kernel and by the host
program tests/cpp/describe_sample_cpu.hip): the rotated pattern point rounded on the float adder ((v + M) - M, M = 1.5 * 2^23), its hb byte address
formed by two float multiply-adds with the integer taken out of the mantissa, and the 7-tap column sum as a chain of 24-bit multiply-adds.  The
program runs that text on the CPU, built without contraction as the library is (and with AddressSanitizer and UBSan, a fresh process), against the
form it replaces -- rintf, the integer address 2 * ((18 + r) * kHbP + 18 + q), the sum written out with four multiplications:

  * all 375 pattern points under sincos_deg of every multiple of 1/64 degree and of 10^5 random angles;
  * integer points of [-13, 13]^2 under (a, b) of multiples of 1/8 (and so of 1/2) inside the unit disc: exact .5 ties of both signs, both
    rounding directions -- points with |x| = 13 at a = +-0.5 among them;
  * (v + M) - M == rintf(v) on 10^6 random floats of (-2^22, 2^22) and on every half-integer of [-64, 64];
  * the tap chain on all-0, all-65535 and 10^5 random u16 septets in the three cv modes' constants.

Zero mismatches are required; the counts say that the cases were really met."""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    out = str(tmp_path_factory.mktemp("describe_sample") / "describe_sample_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-g", "-std=c++17", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "orb_ygz_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "describe_sample_cpu.hip"),
                           "-L", rocm_lib, "-lamdhip64", "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout)
    res["stderr"] = r.stderr[-2000:]
    print(res)
    return res


def test_the_float_form_equals_rintf_and_integer_arithmetic_everywhere(got):
    assert got["mismatches"] == 0, got["stderr"]


def test_the_cases_were_met(got):
    assert got["points"] == 375
    assert got["grid_angles"] == 360 * 64 + 1 and got["grid_samples"] == 375 * (360 * 64 + 1)
    assert got["random_samples"] == 375 * 100000
    assert got["rounds"] == 1000000 and got["halves"] == 257 and got["septets"] == 100002
    # ties: thousands among the hand-made rotations, of both signs, rounded both ways (to even is up for some, down for others), |x| = 13 at a = +-0.5
    assert got["hand_ties"] > 1000 and got["x13_half_ties"] > 0
    assert got["ties_negative"] > 1000 and got["ties_positive"] > 1000
    assert got["ties_rounded_up"] > 1000 and got["ties_rounded_down"] > 1000
    # the rotated pattern stays inside hb's 37 columns and the rows its seven taps need: offsets of at most 18 from the centre
    assert -18 <= got["r_range"][0] < 0 < got["r_range"][1] <= 18
    assert -18 <= got["q_range"][0] < 0 < got["q_range"][1] <= 18
