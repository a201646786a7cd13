"""The extractor's planning unit (orb_ygz_slam_amd/csrc/ygzf_plan.hip: geometry tables, pyramid strips, octree launches, FAST kernel choice) is
host arithmetic without a kernel: it is compiled here with AddressSanitizer and UBSan into a stand-alone program (tests/cpp/extract_plan_cpu.hip)
that walks the geometries and pins of the octree and pyramid tests and checks every stored index against its table, every octree plan's
cover of the levels and its LDS, and choose_fast's rules.  A fresh process, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    csrc = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")
    tmp = tmp_path_factory.mktemp("extract_plan")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    objs = []
    for src in (os.path.join(csrc, "ygzf_plan.hip"), os.path.join(ROOT, "tests", "cpp", "extract_plan_cpu.hip")):
        obj = str(tmp / (os.path.basename(src) + ".o"))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-D_GLIBCXX_ASSERTIONS"] + san +
                              ["-I", csrc, "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj])
        objs.append(obj)
    out = str(tmp / "extract_plan_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only"] + san + objs + ["-L", rocm_lib, "-lamdhip64", "-o", out])
    return out


def test_plans_of_the_sweep_under_the_sanitizers(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("YGZF_FORCE", "YGZF_DEBUG")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "extract plan ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
