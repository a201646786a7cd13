"""Builds and runs tests/cpp/lds_layout_cpu.hip, the stand-alone host program that walks orb_ygz_slam_amd/csrc/lds_layout.h (no test in here: the
tests that want its table or one of its numbers import this).  One build per process and flavour."""
import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile

from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "lds_layout_parent.json")


@functools.lru_cache(maxsize=None)
def exe(sanitize=False):
    """sanitize: AddressSanitizer and UBSan on the host code (a fresh process of its own; never for a test that runs on the GPU machine)"""
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    csrc = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="lds_layout_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    objs = []
    for src in (os.path.join(csrc, "ygzf_plan.hip"), os.path.join(ROOT, "tests", "cpp", "lds_layout_cpu.hip")):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-D_GLIBCXX_ASSERTIONS"] + san +
                              ["-I", csrc, "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj])
        objs.append(obj)
    out = os.path.join(tmp, "lds_layout_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only"] + san + objs + ["-L", rocm_lib, "-lamdhip64", "-o", out])
    return out


def run(args, sanitize=False):
    env = {k: v for k, v in os.environ.items() if k not in ("YGZF_FORCE", "YGZF_DEBUG")}
    r = subprocess.run([exe(sanitize)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def table(sanitize=False):
    """the program's JSON, at the static LDS of k_sia_run that the golden file records (the aligner's ceiling follows from it)"""
    return json.loads(run([golden()["aligner"]["static_lds"]], sanitize))


def oct_sort_bytes(n_cells, cap, lds_cand):
    return int(run(["oct_sort", n_cells, cap, lds_cand]))
