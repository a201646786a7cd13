"""Builds and runs the aligner's two stand-alone host programs (no test in here): tests/cpp/sia_gate_cpu.hip (csrc/sia_gate.h against the
reference's form of the border test) and tests/cpp/sia_plan_cpu.hip (what csrc/lds_layout.h decides for a one-pair SparseImgAlign launch).  Host
code only, built with AddressSanitizer and UBSan, each run a fresh process; never for a test that runs on the GPU machine."""
import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile

from tests.conftest import ROOT


@functools.lru_cache(maxsize=None)
def exe(name):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    csrc = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix=name + "_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".hip"), "-o", out])
    return out


def run(name, args=()):
    env = {k: v for k, v in os.environ.items() if k not in ("YGZF_FORCE", "YGZF_DEBUG")}
    r = subprocess.run([exe(name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def plans(launches, static_lds=0):
    """launches: [(features, [bytes of each current level the run visits])] -> the program's records"""
    return json.loads(run("sia_plan_cpu", [static_lds] + ["%d:%s" % (n, ",".join(str(b) for b in lv)) for n, lv in launches]))
